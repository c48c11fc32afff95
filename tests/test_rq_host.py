"""The residual compressor on its two-section wire, host side (no GPU): codec routing, wire layout and size, grouping, the draw
plan, the library's ABI, the driver's switch, and the quantizers' host logic on the CPU oracle against the reference's fixtures."""
import ctypes
import json
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)

FCN_SHAPES = [(256, 784), (256,), (10, 256), (10,)]


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=1, ef=False, two_phase=False, scale="exp",
                num_users=1, mode="ps", cr=256, gq_rng="reference")
    base.update(kw)
    return Namespace(**base)


def _params(shapes):
    return [torch.nn.Parameter(torch.zeros(s)) for s in shapes]


def _resnet50_shapes():
    with open(os.path.join(GOLDEN, "resnet50_cifar_shapes.json")) as f:
        return json.load(f)["parameter_shapes"]


def _up(x, a=16):
    return (x + a - 1) // a * a


def test_quantizers_choose_the_residual_codec():
    """The codec the quantizers give a ResidualCompressor tensor: the two-section wire, in ps and ring mode; shapes libgq_rq.so
    does not serve keep GenericCodec."""
    from gq_amd.codecs import BatchedResidual, GenericCodec, ResidualCodec, quantizer_codec_factory
    from gq_amd.compressors import NearestNeighborCompressor, ResidualCompressor
    from gq_amd.quantizers import PSQuantizer, RingQuantizer
    for cls, mode in ((PSQuantizer, "ps"), (RingQuantizer, "ring")):
        q = cls(ResidualCompressor, _params(FCN_SHAPES), make_args(mode=mode))
        assert [type(c).__name__ for c in q.codecs] == ["ResidualCodec", "DenseCodec", "ResidualCodec", "DenseCodec"], mode
        assert [g[0] for g in q._groups] == [BatchedResidual] and q._groups[0][1] == [0, 2]
    n = 96 * 64
    np.random.seed(0)
    for kw, want in ((dict(c_dim=16, k_bit=8), ResidualCodec), (dict(c_dim=8, k_bit=8), ResidualCodec), (dict(c_dim=32, k_bit=8), ResidualCodec),
                     (dict(c_dim=12, k_bit=8), GenericCodec), (dict(c_dim=24, k_bit=8), GenericCodec),
                     (dict(c_dim=16, k_bit=4), GenericCodec)):
        cd = quantizer_codec_factory(ResidualCompressor(n, torch.Size([n]), make_args(**kw)), n, torch.Size([n]))
        assert type(cd) is want, kw
    # K == d (a random orthogonal codebook per tensor) takes the codec, not the group
    cd = quantizer_codec_factory(ResidualCompressor(n, torch.Size([n]), make_args(c_dim=32, k_bit=5)), n, torch.Size([n]))
    assert type(cd) is ResidualCodec and not BatchedResidual.eligible(cd)
    hs = quantizer_codec_factory(NearestNeighborCompressor(n, torch.Size([n]), make_args()), n, torch.Size([n]))
    assert not BatchedResidual.eligible(hs)


@pytest.mark.parametrize("kw", [dict(), dict(n_bit=32), dict(n_bit=8), dict(random=0, n_bit=8)], ids=["n6", "n32", "n8_int16", "n8_det"])
def test_wire_is_two_hsq_sections_back_to_back(kw):
    """The layout arithmetic: stage 1's HSQ section at the tensor's offset, stage 2's at the next 16-byte boundary, each with
    HSQCodec's own offsets; one user's ResNet-50 wire is the sum of the sections and far from dense f32."""
    from gq_amd.codecs import HSQCodec, ResidualCodec
    from gq_amd.compressors import NearestNeighborCompressor, ResidualCompressor
    from gq_amd.quantizers import PSQuantizer
    shapes = _resnet50_shapes()
    q = PSQuantizer(ResidualCompressor, _params(shapes), make_args(**kw))
    total = 0
    for i, cd in enumerate(q.codecs):
        if type(cd) is not ResidualCodec:
            continue
        n = cd.numel
        h = HSQCodec(NearestNeighborCompressor(n, torch.Size([n]), make_args(**kw)), n, torch.Size([n]))
        for st in (cd.s1, cd.s2):
            assert (st.codes_off, st.levels_off, st.lbub_off, st.nbytes, st.level_dtype) == (h.codes_off, h.levels_off, h.lbub_off, h.nbytes, h.level_dtype)
        M = n // 16
        lvl = M * (4 if kw.get("n_bit") == 32 else (2 if (kw.get("n_bit") == 8 and kw.get("random", 1)) else 1))
        assert h.nbytes == _up(M) + _up(lvl) + 16
        assert cd.stage2_off == _up(h.nbytes) and cd.nbytes == cd.stage2_off + h.nbytes
        assert q.offsets[i] % 16 == 0
        total += _up(cd.nbytes)
    assert sum(1 for c in q.codecs if type(c) is ResidualCodec) == 76
    assert q.wire_bytes_per_user() == _up(total + q.dense_bytes)
    if not kw:
        qh = PSQuantizer(NearestNeighborCompressor, _params(shapes), make_args())
        assert q.dense_off == 2 * qh.dense_off == total      # (dense_off: where the compressed sections end)
        assert q.wire_bytes_per_user() == 5_966_704
    assert q.wire_bytes_per_user() < 94_083_376 // 4      # the decoded dense f32 of the generic path


def test_draw_plan_three_runs_in_the_reference_order():
    from gq_amd.compressors import ResidualCompressor
    from gq_amd.quantizers import PSQuantizer
    q = PSQuantizer(ResidualCompressor, _params(FCN_SHAPES), make_args())
    Ms = [256 * 784 // 16, 10 * 256 // 16]
    assert q._draw_off == {0: 0, 2: 3 * Ms[0]} and q._draw_total == 3 * sum(Ms)
    assert q.codecs[0].draw_count() == 3 * Ms[0] and q.codecs[0].draw_runs() == (0, 1, 2)      # levels 1, codewords 2, levels 2
    for kw in (dict(random=0), dict(n_bit=32)):      # only stage 2's sampler draws
        q1 = PSQuantizer(ResidualCompressor, _params(FCN_SHAPES), make_args(**kw))
        assert q1._draw_off == {0: 0, 2: Ms[0]} and q1._draw_total == sum(Ms), kw
        assert q1.codecs[0].draw_runs() == (None, 0, None)
    assert PSQuantizer(ResidualCompressor, _params(FCN_SHAPES), make_args(gq_rng="device"))._draw_total == 0


def test_rq_library_abi_and_driver_switch():
    from gq_amd import driver, native
    from gq_amd.compressors import ResidualCompressor
    L = native.rq_lib()
    assert L.gq_rq_abi_version() == native.RQ_ABI_VERSION == 1
    for d, K, cb, want in ((16, 256, 1, 1), (8, 32, 1, 1), (32, 64, 1, 1), (12, 256, 1, 0), (16, 16, 1, 0), (16, 512, 4, 0), (16, 48, 1, 0),
                           (64, 256, 1, 0)):
        assert L.gq_rq_batched_serves(d, K, cb) == want
        assert native.rq_batched_serves(d, K, torch.uint8 if cb == 1 else torch.int32) is bool(want)
    assert ctypes.sizeof(native._RQBatchStruct) == 40
    assert native.lib().gq_abi_version() == 5 and native.pvq_lib().gq_pvq_abi_version() == 1      # the other libraries are as they were
    assert driver.quantizer_choices["rq"] is ResidualCompressor
    assert driver.build_parser().parse_args(["--quantizer", "rq"]).quantizer == "rq"


import rq_fixture_util as fxu  # noqa: E402


@pytest.mark.parametrize("name", fxu.FCN_FIXTURES)
def test_host_logic_reproduces_the_reference_fixtures(name):
    """The reference's own PSQuantizer / RingQuantizer over its ResidualCompressor (tests/golden/make_golden_rq.py) against this
    project's quantizers on the CPU oracle codec, gq_rng = "reference": both stages' codes, levels and (lb, ub) of every user,
    every step's aggregate, the residuals and server residuals -- identical.  Pins the draw order (stage 1's levels, stage 2's
    codewords, stage 2's levels, per tensor in parameter order, the second phase included), the (0 + d1) + d2 decode and the
    error-feedback / two-phase sequence to the reference, not to this code."""
    from oracle_codec_rq import oracle_rq_codec_factory
    diffs, q = fxu.run_fixture(name, torch.device("cpu"), oracle_rq_codec_factory)
    assert not diffs, diffs[:8]
    assert q._draw_total > 0
