"""The bf16 entry points of libgq_mxr.so held to include/gq_mxr.h (TENSOR-SIDE TYPE), bit for bit: the bodies of
tests/test_gpu_z_mx_bf16_contract.py over the rotated launches -- what gets narrowed is the inverse transform's float32 output, the
wire is the float32 twin's byte for byte, and under error feedback the residual comes from the unrounded w."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mxr_contract as mxr  # noqa: E402
import test_gpu_z_mx_bf16_contract as base  # noqa: E402

pytestmark = pytest.mark.gpu

SIGNS = mxr.SEEDED


@pytest.fixture(autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available()
    yield


@pytest.mark.parametrize("off", base.OFFSETS)
@pytest.mark.parametrize("mode", base.MODES)
@pytest.mark.parametrize("fmt", base.FMTS)
def test_seams_views_and_wire_equivalence(fmt, mode, off):
    base.body_seams(fmt, mode, off, SIGNS)


@pytest.mark.parametrize("mode", base.MODES)
@pytest.mark.parametrize("fmt", base.FMTS)
def test_seventy_tensors_and_the_dense_copy(fmt, mode):
    base.body_seventy(fmt, mode, SIGNS)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("mode", base.MODES)
@pytest.mark.parametrize("fmt", base.FMTS)
def test_error_feedback_three_records(fmt, mode, off):
    base.body_error_feedback(fmt, mode, off, SIGNS)


@pytest.mark.parametrize("fmt", base.FMTS)
def test_decode_mean(fmt):
    base.body_decode(fmt, SIGNS)


def test_refusals():
    from gq_amd import native
    base.body_refusals(native.mxr_lib, "gq_mxr_", SIGNS)
