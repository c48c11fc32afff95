"""The item-table batches' ctypes calls against the prototypes of include/gq_*.h, without a GPU: a recording stand-in takes the
place of every loaded library, and each compress / decode / record must name the entry point the header declares and hand it
arguments of the declared kinds, in the declared order, through one _check per entry point."""
import ctypes
import os
import re

import pytest
import torch

import item_host_stubs as stubs
from gq_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
BYREF = type(ctypes.byref(ctypes.c_int(0)))


def _prototypes():
    """{entry point: [ctypes kind per parameter, "ptr" for any pointer]} of every int gq_*(...) the headers declare."""
    protos = {}
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        with open(os.path.join(ROOT, "include", header)) as f:
            code = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
        for name, params in re.findall(r"\bint\s+(gq_\w+)\s*\(([^)]*)\)\s*;", code):
            kinds = []
            for p in (q.strip() for q in params.split(",")):
                if p == "void":
                    continue
                ctype = " ".join(w for w in p.split()[:-1] if w != "const")
                kinds.append("ptr" if "*" in p else KINDS.get(ctype, ctype))      # (a type no item-table entry point takes: by name)
            protos[name] = kinds
    return protos


PROTOTYPES = _prototypes()


def _kind(arg):
    return "ptr" if isinstance(arg, (ctypes.c_void_p, BYREF)) else type(arg)


def _expect(rec, names):
    """The calls recorded since the last look: these entry points, each with its prototype's kinds."""
    calls, rec.calls = rec.calls, []
    assert [n for n, _ in calls] == names
    for name, args in calls:
        assert [_kind(a) for a in args] == PROTOTYPES[name], name


def _call(rec, names, fn, *args, **kw):
    before = native.CALLS[0]
    fn(*args, **kw)
    _expect(rec, names)
    assert native.CALLS[0] - before == len(names)


NSEG, NITEMS, NDRAWS = 2, 3, 5


def _tables():
    return torch.zeros(NSEG * 8, dtype=torch.int64), torch.tensor([0, 1, 1], dtype=torch.int32)


def _i32(n):
    return torch.zeros(n, dtype=torch.int32)


def _f64(n):
    return torch.zeros(n, dtype=torch.float64)


def _f32(n):
    return torch.zeros(n, dtype=torch.float32)


def _topk(cls=native.TopKBatch, *more):
    return cls(*_tables(), NSEG, NITEMS, _i32(NSEG * native.TOPK_HIST_BINS), _i32(NSEG * 4), _i32(NITEMS * 2), *more)


def _psgd():
    b = native.PSGDBatch(*_tables(), NSEG, NITEMS, rank=2, seed=7, lay=torch.zeros(NSEG * 4, dtype=torch.int64), aitem_seg=_i32(2), naitems=2,
                         pwork=_f32(8), cpart=_f32(8), flags=_i32(NSEG * 4))
    b.set_state(torch.zeros(NSEG * 2, dtype=torch.int64))
    return b


def _maurey():
    return native.MaureyBatch(*_tables(), NSEG, NITEMS, NDRAWS, _f64(NITEMS * 4), _f64(NSEG), _i32(NITEMS * 3), _i32(NDRAWS), _f32(NDRAWS))


PLAIN = [      # (id, prefix, constructor): compress(wire, out, ef_scale)
    ("topk", "gq_topk_", _topk),
    ("sign", "gq_sign_", lambda: native.SignBatch(*_tables(), NSEG, NITEMS)),
    ("stc", "gq_stc_", lambda: _topk(native.STCBatch, _f64(NITEMS))),
    ("psgd", "gq_psgd_", _psgd),
]
DRAWN = [      # (id, prefix, suffix, dtype of out, constructor): compress(wire, random_mode, seed, r, out, ef_scale)
    ("maurey", "gq_maurey_", "", torch.float32, _maurey),
    ("mx-f32", "gq_mx_", "", torch.float32, lambda: native.MXBatch(*_tables(), NSEG, NITEMS, native.MX_FP4)),
    ("mx-bf16", "gq_mx_", "_bf16", torch.bfloat16, lambda: native.MXBatch(*_tables(), NSEG, NITEMS, native.MX_FP8, torch.bfloat16)),
    ("mxr-f32", "gq_mxr_", "", torch.float32, lambda: native.MXRBatch(*_tables(), NSEG, NITEMS, native.MX_FP4, (1, 2, 3, 4))),
    ("mxr-bf16", "gq_mxr_", "_bf16", torch.bfloat16,
     lambda: native.MXRBatch(*_tables(), NSEG, NITEMS, native.MX_FP6_E2M3, (1, 2, 3, 4), torch.bfloat16)),
]
ROTATED = [    # (id, prefix, constructor): compress(wire, out, ef_scale, rotation, stream)
    ("drive", "gq_drive_", lambda: native.DriveBatch(*_tables(), NSEG, NITEMS, native.DRIVE_MSE, (1, 2, 3, 4))),
    ("eden", "gq_eden_", lambda: native.EdenBatch(*_tables(), NSEG, NITEMS, 3, native.EDEN_MSE, (1, 2, 3, 4))),
]


@pytest.fixture
def rec(monkeypatch):
    return stubs.install(monkeypatch)


def _wire():
    return torch.zeros(64, dtype=torch.uint8), torch.zeros((2, 64), dtype=torch.uint8)


def _decodes(rec, b, name, out):
    _, gathered = _wire()
    _call(rec, [name], b.decode, gathered, 2, out)
    _call(rec, [name], b.decode, gathered[:1], 1, out, True)
    _call(rec, [name], b.decode, gathered[:, :48], 2, out, plain=False)      # (strided rows)


def test_the_headers_declare_what_the_cases_name():
    for lib in stubs.ITEM_LIBRARIES:
        exports = getattr(native, lib + "_EXPORTS")
        assert all(n in PROTOTYPES for n in exports if not n.endswith(("_abi_version", "_last_error"))), lib
    assert PROTOTYPES["gq_topk_compress_batched"] == ["ptr", "ptr", ctypes.c_float, "ptr", "ptr"]
    assert PROTOTYPES["gq_drive_decode_sum_batched_streams"] == ["ptr", "ptr", ctypes.c_int32, "ptr", ctypes.c_int64, ctypes.c_int, "ptr",
                                                                  ctypes.c_int, "ptr"]


@pytest.mark.parametrize("case", PLAIN, ids=[c[0] for c in PLAIN])
def test_plain_batches(rec, case):
    _, prefix, make = case
    b, (wire, _), out = make(), _wire(), _f32(16)
    _call(rec, [prefix + "compress_batched"], b.compress, wire)
    _call(rec, [prefix + "compress_batched"], b.compress, wire, out, 0.5)
    _decodes(rec, b, prefix + "decode_sum_batched", out)
    part = b.part(*_tables(), NSEG, NITEMS)
    _call(rec, [prefix + "decode_sum_batched"], part.decode, _wire()[1], 2, out)


def test_thr_batch(rec):
    b = native.ThrBatch(*_tables(), NSEG, NITEMS, _f64(NITEMS), _i32(NSEG * 4), _i32(NITEMS * 2), 3, 1, 1, 1)
    (wire, _), out = _wire(), _f32(16)
    _call(rec, ["gq_thr_compress_batched"], b.compress, wire)
    _call(rec, ["gq_thr_compress_batched"], b.compress, wire, out, 0.5, 0.25)
    b.compress(wire, out, 0.5, 0.25)
    (_, args), = rec.calls
    rec.calls = []
    assert (args[2].value, args[3].value) == (0.25, 0.5)      # eta stands between the wire and ef_scale (include/gq_thr.h)
    _decodes(rec, b, "gq_thr_decode_sum_batched", out)


@pytest.mark.parametrize("case", DRAWN, ids=[c[0] for c in DRAWN])
def test_drawn_batches(rec, case):
    _, prefix, suffix, dtype, make = case
    b, (wire, _), out = make(), _wire(), torch.zeros(16, dtype=dtype)
    name = prefix + "compress_batched" + suffix
    _call(rec, [name], b.compress, wire, native.RANDOM_DEVICE, 2 ** 64 + 5)
    _call(rec, [name], b.compress, wire, native.RANDOM_GIVEN, 0, _f32(NDRAWS), out, 0.5)
    _call(rec, [name], b.compress, wire, native.RANDOM_DEVICE_COUNTER, 12345, None, out, None)
    b.compress(wire, native.RANDOM_DEVICE, 2 ** 64 + 5)
    (_, args), = rec.calls
    rec.calls = []
    assert (args[2].value, args[3].value, args[4].value) == (native.RANDOM_DEVICE, None, 5)      # mode, r, seed mod 2^64
    _decodes(rec, b, prefix + "decode_sum_batched" + suffix, out)
    with pytest.raises(TypeError):
        b.compress(wire, native.RANDOM_OFF, 0, None, torch.zeros(16, dtype=torch.float16), None)
    assert rec.calls == []


def test_maurey_keeps_its_draw_count_assertion(rec):
    b, (wire, _) = _maurey(), _wire()
    with pytest.raises(AssertionError):
        b.compress(wire, native.RANDOM_GIVEN, 0, _f32(NDRAWS - 1))
    assert rec.calls == []


@pytest.mark.parametrize("case", ROTATED, ids=[c[0] for c in ROTATED])
def test_rotated_batches(rec, case):
    _, prefix, make = case
    b, (wire, gathered), out = make(), _wire(), _f32(16)
    pair = torch.zeros((1, 2), dtype=torch.int64)
    c, d = prefix + "compress_batched", prefix + "decode_sum_batched"
    _call(rec, [c], b.compress, wire)
    _call(rec, [c], b.compress, wire, out, 0.5)
    _call(rec, [c + "_stepped"], b.compress, wire, out, 0.5, pair)
    _call(rec, [c + "_stepped"], b.compress, wire, rotation=pair)
    _call(rec, [c + "_streams"], b.compress, wire, out, 0.5, pair, 3)
    _call(rec, [c + "_streams"], b.compress, wire, None, None, rotation=pair, stream=0)
    _decodes(rec, b, d, out)
    _call(rec, [d + "_stepped"], b.decode, gathered, 2, out, rotation=pair)
    _call(rec, [d + "_stepped"], b.decode, gathered[:1], 1, out, True, pair)
    _call(rec, [d + "_streams"], b.decode, gathered, 2, out, rotation=pair, first_stream=0)
    _call(rec, [d + "_streams"], b.decode, gathered, 2, out, False, pair, 5)
    part = b.part(*_tables(), NSEG, NITEMS)
    assert part.signs == b.signs == (1, 2, 3, 4)
    _call(rec, [d + "_stepped"], part.decode, gathered, 2, out, rotation=pair)
    # what _rotation_ptr and _stream_arg refuse, they refuse in front of the call
    before = native.CALLS[0]
    for kw, error in ((dict(rotation=torch.zeros(2, dtype=torch.int64)), TypeError), (dict(rotation=None, stream=1), TypeError),
                      (dict(rotation=pair, stream=True), TypeError), (dict(rotation=pair, stream=1.0), TypeError),
                      (dict(rotation=pair, stream=2 ** 31), ValueError)):
        with pytest.raises(error):
            b.compress(wire, out, None, **kw)
    with pytest.raises(ValueError, match="stream -2147483649 does not fit int32"):
        b.decode(gathered, 2, out, rotation=pair, first_stream=-2 ** 31 - 1)
    with pytest.raises(TypeError, match=r"rotation must be a device int64 \[1, 2\] tensor"):
        b.decode(gathered, 2, out, rotation=None, first_stream=1)
    assert rec.calls == [] and native.CALLS[0] == before


def test_dgc_record(rec):
    b = _topk(native.DGCBatch)
    b.set_state(torch.zeros(NSEG * 8, dtype=torch.int64))
    (wire, _), out = _wire(), _f32(16)
    _call(rec, ["gq_dgc_accumulate_batched", "gq_topk_compress_batched", "gq_dgc_mask_batched"], b.record, wire, out, 0.9)
    _call(rec, ["gq_topk_compress_batched"], b.compress, wire, out, None)      # (the plain top-k of the two-phase re-compress)
    _decodes(rec, b, "gq_topk_decode_sum_batched", out)
