"""The host layers of the threshold compressor without a GPU: the compressor's arguments and refusals, the driver flags, group keys,
the three quantizer refusals, kept_counts' shape, and the ctypes struct and export list against include/gq_thr.h and the built library."""
import ctypes
import os
import re
import sys
from argparse import Namespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import thr_contract as tc  # noqa: E402
from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedThr, ThrCodec, default_codec_factory, thr_section_bytes  # noqa: E402
from gq_amd.compressors import ThresholdSparsificationCompressor as Thr  # noqa: E402
from gq_amd.driver import build_parser, quantizer_choices  # noqa: E402
from gq_amd.quantizers import Quantizer  # noqa: E402


def args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=2, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


def test_arguments_and_refusals():
    c = Thr(200704, (256, 784), args())
    assert (c.stages, c.percent, c.fit_stride, c.k) == (3, 150, 1, 784)
    assert Thr(5000, (5000,), args(thr_stages=0, thr_value=0.0)).eta == 0.0
    for bad in (dict(thr_stages=9), dict(thr_stages=-1), dict(thr_stages=True), dict(thr_stages=0), dict(thr_stages=0, thr_value=-1.0),
                dict(thr_stages=0, thr_value=-0.0), dict(thr_stages=0, thr_value=float("inf")), dict(thr_stages=0, thr_value=float("nan")),
                dict(thr_stages=0, thr_value=1e39), dict(thr_cap_percent=0), dict(thr_fit_stride=0), dict(cr=0)):
        with pytest.raises(ValueError):
            Thr(5000, (5000,), args(**bad))
    with pytest.raises(TypeError, match="float32"):
        c.compress(torch.zeros(5000))
    with pytest.raises(ValueError, match="at least 1"):
        ThrCodec(Thr(100, (100,), args()), 100, (100,))
    for n, M in ((4096 * 16, 8), (4096 * 64, 8), (4096 * 33, 2), (4096 * 30, 2), (1001, 8), (4096 * 64, 3)):
        assert Thr.stride_for(n, M) == tc.stride_for(n, M)
    assert Thr.stride_for(4096 * 64, 8) == 4 and Thr.stride_for(4096 * 30, 2) == 1 and Thr.stride_for(4096 * 64, 3) == 2
    assert Thr.capacity(1001, 3, 150) == tc.capacity(1001, 3) == 5


def test_codec_group_key_and_factory():
    a = default_codec_factory(Thr(8193, (8193,), args(cr=64)), 8193, (8193,))
    b = default_codec_factory(Thr(200704, (200704,), args(cr=64, thr_fit_stride=2)), 200704, (200704,))
    c = default_codec_factory(Thr(8193, (8193,), args(cr=64, thr_stages=0, thr_value=1e-3)), 8193, (8193,))
    assert type(a) is ThrCodec and a.GROUP is BatchedThr and BatchedThr.eligible(a)
    assert (a.k, a.cap, a.stride, a.nbytes) == (128, 192, 1, tc.section_bytes(8193, 64)) and b.stride == 2
    assert BatchedThr.group_key(a) == BatchedThr.group_key(b) != BatchedThr.group_key(c)
    assert thr_section_bytes(8193, 64) == 16 + 8 * 192


def test_driver_flags():
    assert quantizer_choices["threshold"] is Thr
    p = build_parser()
    base = ["--quantizer", "threshold"]
    a = p.parse_args(base)
    assert (a.thr_stages, a.thr_value, a.thr_cap_percent, a.thr_fit_stride, a.cr) == (3, None, 150, 1, 256)
    a = p.parse_args(base + ["--thr-stages", "0", "--thr-value", "0.01", "--thr-cap-percent", "200", "--thr-fit-stride", "8", "--cr", "64"])
    assert (a.thr_stages, a.thr_value, a.thr_cap_percent, a.thr_fit_stride, a.cr) == (0, 0.01, 200, 8, 64)
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--thr-stages", "9"])
    from gq_amd import driver
    with pytest.raises(SystemExit):
        driver.main(base + ["--thr-stages", "0"])


def test_quantizer_refusals_and_kept_counts_shape():
    params = [torch.nn.Parameter(torch.zeros(256, 784)), torch.nn.Parameter(torch.zeros(256))]
    with pytest.raises(ValueError, match="ring mode"):
        Quantizer(Thr, params, args(mode="ring"))
    with pytest.raises(ValueError, match="momentum_correction"):
        Quantizer(Thr, params, args(momentum_correction=0.9))
    with pytest.raises(ValueError, match="float32"):
        Quantizer(Thr, [torch.nn.Parameter(torch.zeros(256, 784, dtype=torch.bfloat16))], args())
    q = Quantizer(Thr, params, args(ef=True, two_phase=True))
    assert [type(c).__name__ for c in q.codecs] == ["ThrCodec", "DenseCodec"] and q.kept_counts() == []
    q._wire = torch.zeros((2, q.user_bytes), dtype=torch.uint8)
    q._wire[1, :12] = torch.tensor(list((5).to_bytes(4, "little") + (9).to_bytes(4, "little") + (0x3f800000).to_bytes(4, "little")), dtype=torch.uint8)
    assert q.kept_counts(1) == [(5, 9, 1.0)] and q.kept_counts(0) == [(0, 0, 0.0)] and q.kept_counts(2) == []


def test_struct_and_exports_against_the_header_and_the_library():
    h = open(os.path.join(ROOT, "include", "gq_thr.h")).read()
    body = re.search(r"typedef struct gq_thr_batch \{(.*?)\} gq_thr_batch;", h, re.S).group(1)
    names = [re.search(r"(\w+);", ln).group(1) for ln in body.splitlines() if ";" in ln]
    assert names == [f[0] for f in native._ThrBatchStruct._fields_] and ctypes.sizeof(native._ThrBatchStruct) == 88
    assert sorted(set(re.findall(r"\b(gq_thr_\w+)\(", h))) == sorted(native.THR_EXPORTS)
    assert int(re.search(r"#define GQ_THR_ABI_VERSION (\d+)", h).group(1)) == native.THR_ABI_VERSION
    L = native.thr_lib()
    assert L.gq_thr_abi_version() == native.THR_ABI_VERSION and all(hasattr(L, n) for n in native.THR_EXPORTS)


def test_the_shared_code_is_the_sparse_header_s():
    from test_topk_host import shared_header_checks
    text = shared_header_checks("thr.hip")
    assert "thr_reduce_kernel" in text and "thr_pick_kernel" in text      # the fit is its own
