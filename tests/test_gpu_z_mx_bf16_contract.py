"""The bf16 entry points of libgq_mx.so held to include/gq_mx.h (TENSOR-SIDE TYPE), bit for bit: every comparison is np.array_equal
on uint8 / uint16 / uint32 views against tests/mx_bf16_contract.py (whose own checks are tests/test_mx_bf16_contract.py).  All four
formats, each with nearest rounding, given draws and device draws; canaries round the wire, guarded sources, error buffers and
outputs; sources and outputs 1, 2 and 8 elements past a 16-byte boundary (2-, 4- and 16-byte aligned: the scalar path and the
16-byte path at every seam).  tests/test_gpu_z_mxr_bf16_contract.py runs the same bodies over libgq_mxr.so (`signs`)."""
import ctypes
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx6_contract as m6  # noqa: E402
import mx_bf16_contract as bx  # noqa: E402

pytestmark = pytest.mark.gpu

f32, U16, U32 = np.float32, np.uint16, np.uint32
FMTS = bx.FMTS
MODES = ["off", "given", "device"]
OFFSETS = [1, 2, 8]
SEED = 0x1234567887654321
GUARD = 16                    # elements in front of and behind every guarded buffer
SRC_CANARY, OUT_PRESET = 0x5A5A, 0x40E0      # (0x40E0 = 7.0)
WIRE_CANARY_BYTES = 64


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def to_dev16(bits, dev):
    return torch.from_numpy(np.ascontiguousarray(bits, U16).view(np.int16).copy()).to(dev).view(torch.bfloat16)


def bits16(t):
    return t.view(torch.int16).cpu().numpy().view(U16)


def make_group(sizes, fmt, dtype=torch.bfloat16, random=True, rng="device", dense_sizes=(), signs=None):
    from gq_amd.codecs import BatchedMX, BatchedMXR, MXCodec, MXRCodec
    dev = torch.device("cuda:0")
    comp = SimpleNamespace(format=m6.NAMES[fmt], random=random, _rng=rng, rotate_signs=signs)
    codecs = [(MXRCodec if signs else MXCodec)(comp, n, torch.Size([n]), dtype) for n in sizes]
    offs, dense, ub = m6.layout(sizes, fmt, dense_sizes)
    g = (BatchedMXR if signs else BatchedMX)(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=dense or None)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return SimpleNamespace(g=g, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), fmt=fmt, first=first, signs=signs, dtype=dtype)


def _guarded(values, off, dev, kind):
    """values at GUARD + off elements of a buffer full of canaries -> (view, whole).  kind: 'bf16' (uint16 bits) or 'f32'."""
    n = values.size
    if kind == "bf16":
        whole = torch.full((n + 2 * GUARD + off,), SRC_CANARY, dtype=torch.int16, device=dev).view(torch.bfloat16)
        whole[GUARD + off:GUARD + off + n] = to_dev16(values, dev)
    else:
        whole = torch.full((n + 2 * GUARD + off,), -1.5, dtype=torch.float32, device=dev)
        whole[GUARD + off:GUARD + off + n] = torch.from_numpy(np.asarray(values, f32)).to(dev)
    return whole[GUARD + off:GUARD + off + n], whole


def _guards_intact(whole, off, n, kind):
    w = bits16(whole) if kind == "bf16" else whole.cpu().numpy()
    edge = np.concatenate([w[:GUARD + off], w[GUARD + off + n:]])
    return bool(np.all(edge == (SRC_CANARY if kind == "bf16" else f32(-1.5))))


def compress(G, vs, mode="off", r=None, errs=None, s=None, dense_src=(), v_off=0, e_off=0, o_off=0, want_out=True):
    """One compress launch of the group -> wire, out, the sources and error buffers afterwards (numpy; bf16 as uint16 bits).  Every
    source sits v_off, `out` o_off and every error buffer e_off elements past a 16-byte boundary."""
    dev, g = G.dev, G.g
    kind = "bf16" if G.dtype == torch.bfloat16 else "f32"
    src = [_guarded(v, v_off, dev, kind) for v in vs]
    er = [_guarded(e, e_off, dev, "f32") for e in errs] if errs is not None else None
    ds = [(to_dev16(a, dev) if kind == "bf16" else torch.from_numpy(a).to(dev)) for a in dense_src]
    whole = torch.full((G.ub + 2 * WIRE_CANARY_BYTES,), m6.CANARY, dtype=torch.uint8, device=dev)
    wire = whole[WIRE_CANARY_BYTES:WIRE_CANARY_BYTES + G.ub]
    wire.fill_(0xAB)
    if kind == "bf16":
        obig = torch.full((g.out_floats + 2 * GUARD + o_off,), OUT_PRESET, dtype=torch.int16, device=dev).view(torch.bfloat16)
    else:
        obig = torch.full((g.out_floats + 2 * GUARD + o_off,), 7.0, dtype=torch.float32, device=dev)
    out = obig[GUARD + o_off:GUARD + o_off + g.out_floats] if want_out else None
    kw = {}
    if mode == "given":
        kw["draws"] = (torch.from_numpy(np.asarray(r, f32)).to(dev), {i: int(x) for i, x in enumerate(G.first)})
    elif mode == "device":
        kw["seed"] = SEED
    if er is not None:
        kw.update(errs=[e[0] for e in er], ef_scale=float(s))
    if ds:
        kw.update(dense=ds)
    assert g.encode([t for t, _ in src], wire, 0, 0, out=out, **kw)
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    assert np.all(w[:WIRE_CANARY_BYTES] == m6.CANARY) and np.all(w[WIRE_CANARY_BYTES + G.ub:] == m6.CANARY), "a write outside the wire"
    for (t, big), v in zip(src, vs):
        assert _guards_intact(big, v_off, v.size, kind), "a write outside a source"
    for (t, big), e in zip(er or (), errs or ()):
        assert _guards_intact(big, e_off, e.size, "f32"), "a write outside an error buffer"
    ob = bits16(obig) if kind == "bf16" else obig.cpu().numpy()
    preset = OUT_PRESET if kind == "bf16" else f32(7.0)
    assert np.all(ob[:GUARD + o_off] == preset) and np.all(ob[GUARD + o_off + g.out_floats:] == preset), "a write outside out"
    get = bits16 if kind == "bf16" else (lambda t: t.cpu().numpy())
    return SimpleNamespace(wire=w[WIRE_CANARY_BYTES:WIRE_CANARY_BYTES + G.ub], out=ob[GUARD + o_off:GUARD + o_off + g.out_floats],
                           src=[get(t) for t, _ in src], err=[t.cpu().numpy() for t, _ in er] if er else None)


def draws_of(G, mode, given=None):
    """Per-tensor draws of the reference for a launch made with `mode`."""
    if mode == "off":
        return [None] * len(G.sizes)
    if mode == "given":
        return np.split(np.asarray(given, f32), np.cumsum(G.sizes)[:-1])
    return [m6.draws(m6.DEVICE, n, int(fd), SEED) for n, fd in zip(G.sizes, G.first)]


def check(G, res, vs, rs, errs=None, s=None, out=True):
    """Every tensor's section, `out`, source and residual against the reference.  -> the residuals afterwards."""
    after = []
    for i, v in enumerate(vs):
        n, off, oo = G.sizes[i], G.offs[i], G.g.out_off[i]
        e = errs[i] if errs is not None else None
        sec, D16, w16, ne = bx.compress(v, G.fmt, rs[i], e, s, G.signs)
        assert sec.size == m6.section_bytes(n, G.fmt)
        assert np.array_equal(res.wire[off:off + sec.size], sec), "tensor %d (n = %d): its section of the wire" % (i, n)
        if out:
            assert np.array_equal(res.out[oo:oo + n], D16), "tensor %d (n = %d): the compress's dense decode" % (i, n)
            end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
            assert np.all(res.out[oo + n:end] == OUT_PRESET), "a write behind tensor %d's decode" % i
        if e is not None:
            assert np.array_equal(res.src[i], w16), "tensor %d (n = %d): g <- narrow(w)" % (i, n)
            assert m6.same(res.err[i], ne, nan_as_one=True), "tensor %d (n = %d): err <- w - decoded, from the unrounded w" % (i, n)
        else:
            assert np.array_equal(res.src[i], v), "tensor %d: the source changed without error feedback" % i
        after.append(ne)
    if not G.dense:
        last = G.offs[-1] + m6.section_bytes(G.sizes[-1], G.fmt)
        assert np.all(res.wire[last:] == 0xAB)
    return after


@functools.lru_cache(maxsize=None)
def _seam_inputs():
    vs = [bx.edge_gradient(n, 100 + n) for n in bx.SEAM_SIZES]
    r = np.random.RandomState(7).rand(sum(bx.SEAM_SIZES)).astype(f32)
    r[::7] = 0
    return vs, r


def body_seams(fmt, mode, off, signs=None):
    """Every seam size in one group, with +-0, bf16 subnormals, +-inf and NaNs in the gradients; then the float32 launch on the
    widened tensors: the same wire, byte for byte."""
    vs, r = _seam_inputs()
    G = make_group(bx.SEAM_SIZES, fmt, random=mode != "off", signs=signs)
    assert all(o % 8 == 0 for o in G.g.out_off)
    res = compress(G, vs, mode, r, v_off=off, o_off=off)
    check(G, res, vs, draws_of(G, mode, r))
    F = make_group(bx.SEAM_SIZES, fmt, dtype=torch.float32, random=mode != "off", signs=signs)
    wide = compress(F, [bx.widen(v) for v in vs], mode, r)
    assert np.array_equal(res.wire, wide.wire), "the wire of a bf16 source is not the wire of the widened float32 tensor"


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", FMTS)
def test_seams_views_and_wire_equivalence(fmt, mode, off):
    body_seams(fmt, mode, off)


def body_seventy(fmt, mode, signs=None):
    rs = np.random.RandomState(9)
    sizes = [int(x) for x in rs.randint(1, 3000, 70)]
    sizes[5], sizes[40] = m6.ITEM + 3, 2 * m6.ITEM
    dense_sizes = [10, 256, 1]
    vs = [bx.randn16(n, 400 + i) for i, n in enumerate(sizes)]
    dsrc = [bx.edge_gradient(n, 500 + n, nonfinite=False) for n in dense_sizes]
    dsrc[1][3], dsrc[1][4], dsrc[1][5] = 0x7F80, 0xFFC1, 0x7F81       # (a copy: NaN payloads travel as they are, widened)
    G = make_group(sizes, fmt, random=mode != "off", dense_sizes=dense_sizes, signs=signs)
    r = rs.rand(sum(sizes)).astype(f32)
    res = compress(G, vs, mode, r, dense_src=dsrc)
    check(G, res, vs, draws_of(G, mode, r))
    for (off, n), a in zip(G.dense, dsrc):
        assert np.array_equal(res.wire[off:off + 4 * n].view(U32), a.astype(U32) << U32(16)), "an identity tensor's widened copy"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", FMTS)
def test_seventy_tensors_and_the_dense_copy(fmt, mode):
    body_seventy(fmt, mode)


EF_SIZES = [1, 9, 33, 257, 2049, 4097]


def body_error_feedback(fmt, mode, off, signs=None):
    """Three consecutive records: source, residual and wire after each against the reference stepped the same way; `out` too."""
    cases = [bx.ef_case(n, 900 + n) for n in EF_SIZES]
    errs = [c[1] for c in cases]
    G = make_group(EF_SIZES, fmt, random=mode != "off", signs=signs)
    r = np.random.RandomState(11).rand(sum(EF_SIZES)).astype(f32)
    for t in range(3):
        vs = [c[0][t] for c in cases]
        res = compress(G, vs, mode, r, errs=errs, s=1.0, v_off=off, e_off=(off % 4), o_off=off)
        want = check(G, res, vs, draws_of(G, mode, r), errs, 1.0)
        for got, ne in zip(res.err, want):
            assert m6.same(got, ne, nan_as_one=True)
        errs = [np.ascontiguousarray(e) for e in res.err]      # the carried state is the device's own, bit for bit


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", FMTS)
def test_error_feedback_three_records(fmt, mode, off):
    body_error_feedback(fmt, mode, off)


def decode(G, payloads, R, plain=False, byte_shift=0, stride_pad=0, o_off=0):
    """The group's decode-mean of R payloads -> out (uint16 bits).  byte_shift: the payloads start that many bytes past a 16-byte
    boundary; stride_pad: extra bytes between payloads."""
    dev, g = G.dev, G.g
    stride = G.ub + stride_pad
    buf = np.full(byte_shift + R * stride + 16, 0xAB, np.uint8)
    for r in range(R):
        for off, sec in zip(G.offs, payloads[r]):
            buf[byte_shift + r * stride + off:byte_shift + r * stride + off + sec.size] = sec
    t = torch.from_numpy(buf).to(dev)
    gathered = t[byte_shift:byte_shift + R * stride].view(R, stride)[:, :G.ub]
    obig = torch.full((g.out_floats + 2 * GUARD + o_off,), OUT_PRESET, dtype=torch.int16, device=dev).view(torch.bfloat16)
    out = obig[GUARD + o_off:GUARD + o_off + g.out_floats]
    if not g.ready:
        g.upload_layout()
    g._batch.decode(gathered, R, out, plain=plain)
    torch.cuda.synchronize()
    ob = bits16(obig)
    assert np.all(ob[:GUARD + o_off] == OUT_PRESET) and np.all(ob[GUARD + o_off + g.out_floats:] == OUT_PRESET), "a write outside out"
    return ob[GUARD + o_off:GUARD + o_off + g.out_floats]


def check_decode(G, out, payloads, R, plain=False):
    for i, n in enumerate(G.sizes):
        want = bx.decode_mean([payloads[r][i] for r in range(R)], n, G.fmt, plain, G.signs)
        oo = G.g.out_off[i]
        assert np.array_equal(out[oo:oo + n], want), "tensor %d (n = %d), R = %d%s" % (i, n, R, ", plain" if plain else "")
        end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
        assert np.all(out[oo + n:end] == OUT_PRESET)


def body_decode(fmt, signs=None):
    """The hand-built payloads (ties both ways, the carry, a bf16 subnormal, -0, scale byte 0xFF) at R = 1 plain and not, 2, 3, 8, 16,
    on aligned and misaligned gathered buffers and outputs."""
    if signs is None:
        payloads = bx.decode_payloads(fmt, 16)
    else:
        payloads = [[bx.rotated_payloads(n, fmt, 1, 1000 * r + n)[0] for n in bx.DEC_SIZES] for r in range(16)]
        for r in (0, 1):      # (rotated_payloads builds its tie from payloads 0 and 1 of ONE call)
            for i, n in enumerate(bx.DEC_SIZES):
                payloads[r][i] = bx.rotated_payloads(n, fmt, 2, 55 + n)[r]
    G = make_group(bx.DEC_SIZES, fmt, signs=signs)
    for R, plain, shift, pad, o_off in ((1, True, 0, 0, 0), (1, False, 0, 0, 8), (2, False, 0, 0, 0), (2, False, 1, 3, 1), (3, False, 4, 4, 2),
                                        (8, False, 0, 16, 0), (16, False, 2, 6, 1), (1, True, 3, 0, 1)):
        check_decode(G, decode(G, payloads, R, plain, shift, pad, o_off), payloads, R, plain)


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_mean(fmt):
    body_decode(fmt)


def body_refusals(lib, prefix, signs=None):
    """The twins' refusals, with one difference: `out` may be 2-byte aligned -- an odd address is refused."""
    from gq_amd import native
    G = make_group([100, 4097], m6.FP4, signs=signs)
    g = G.g
    g.upload_layout()
    b = g._batch
    L = lib()
    comp, dec = getattr(L, prefix + "compress_batched_bf16"), getattr(L, prefix + "decode_sum_batched_bf16")
    last = getattr(L, prefix + "last_error")
    wire = torch.zeros(G.ub + 16, dtype=torch.uint8, device=G.dev)
    out = torch.zeros(g.out_floats + 8, dtype=torch.bfloat16, device=G.dev)
    P, nan, st = ctypes.c_void_p, ctypes.c_float(float("nan")), native._stream()

    def c(w, mode=0, r=None, seed=0, o=None, ref=None):
        return comp(ref if ref is not None else b.ref, P(w), ctypes.c_int(mode), P(r), ctypes.c_uint64(seed), nan, P(o), st)

    def d(gath, R, o, stride=0, ref=None):
        return dec(ref if ref is not None else b.ref, P(gath), ctypes.c_int64(stride), ctypes.c_int(R), P(o), ctypes.c_int(0), st)

    wp, op = wire.data_ptr(), out.data_ptr()
    assert c(wp, o=op + 1) == native.ERR_INVALID_ARG and b"2-byte aligned" in last()      # an odd address
    assert c(None) == native.ERR_INVALID_ARG                                                 # a null wire
    assert c(wp + 8) == native.ERR_INVALID_ARG                                               # a wire that is not 16-byte aligned
    assert c(wp, mode=7) == native.ERR_INVALID_ARG                                           # an unknown random mode
    assert c(wp, mode=native.RANDOM_GIVEN) == native.ERR_INVALID_ARG                         # given draws without draws
    assert c(wp, mode=native.RANDOM_GIVEN, r=op + 2) == native.ERR_INVALID_ARG               # draws that are not 4-byte aligned
    assert c(wp, mode=native.RANDOM_DEVICE_COUNTER, seed=0) == native.ERR_INVALID_ARG        # a counter without its pair
    assert c(wp, ref=ctypes.c_void_p(0)) == native.ERR_INVALID_ARG        # no descriptor
    assert d(wp, 1, op + 1) == native.ERR_INVALID_ARG and b"2-byte aligned" in last()
    assert d(None, 1, op) == native.ERR_INVALID_ARG and d(wp, 1, None) == native.ERR_INVALID_ARG
    assert d(wp, 0, op) == native.ERR_INVALID_ARG and d(wp, 2, op, stride=-16) == native.ERR_INVALID_ARG
    bad = type(b.s)()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(b.s), ctypes.sizeof(bad))
    bad.format = 2
    assert c(wp, ref=ctypes.byref(bad)) == native.ERR_INVALID_ARG and d(wp, 1, op, ref=ctypes.byref(bad)) == native.ERR_INVALID_ARG
    bad.format, bad.struct_bytes = 0, 44
    assert c(wp, ref=ctypes.byref(bad)) == native.ERR_INVALID_ARG
    # (nothing was launched: every call above fails its checks first.  That `out` IS taken on a 2-byte boundary is what the other
    # tests' o_off = 1 shows, with real sources behind the table.)


def test_refusals():
    from gq_amd import native
    body_refusals(native.mx_lib, "gq_mx_")
