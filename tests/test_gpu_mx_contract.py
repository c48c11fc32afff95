"""libgq_mx.so held to include/gq_mx.h, bit for bit: every comparison is np.array_equal on bytes or uint32 views against
tests/mx_contract.py (whose own checks are tests/test_mx_contract.py) -- wire, dense out, the gradient and the residual after error
feedback; where an input block is not finite every NaN counts as one pattern.  The wire starts as 0xAB inside canaries, `out` as
7.0, tensors sit inside guarded buffers."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD, CANARY_BYTES = 3.0, 64
FMTS = [mx.FP4, mx.FP8]
NAMES = {mx.FP4: "fp4", mx.FP8: "fp8"}
ITEM = mx.ITEM


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _place(arr, off, dev):
    """arr as a view `off` floats into a buffer of its own (4 * off bytes past a 16-byte boundary) -> (view, buffer)"""
    big = torch.full((arr.size + 8,), GUARD, dtype=torch.float32, device=dev)
    view = big[off:off + arr.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view, big


def _guards_intact(big, off, n):
    b = big.cpu().numpy()
    return np.all(b[:off] == GUARD) and np.all(b[off + n:] == GUARD)


def make_group(sizes, fmt, random=True, rng="device", dense_sizes=()):
    from gq_amd.codecs import BatchedMX, MXCodec
    dev = torch.device("cuda:0")
    comp = SimpleNamespace(format=NAMES[fmt], random=random, _rng=rng)
    codecs = [MXCodec(comp, n, torch.Size([n])) for n in sizes]
    assert [cd.nbytes for cd in codecs] == [mx.section_bytes(n, fmt) for n in sizes]
    offs, dense, ub = mx.layout(sizes, fmt, dense_sizes)
    g = BatchedMX(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=dense or None)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return SimpleNamespace(g=g, codecs=codecs, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), fmt=fmt, first=first)


def compress(G, vs, r=None, seed=None, errs=None, s=None, dense_src=(), v_offs=None, e_offs=None, o_off=0, want_out=True):
    """One compress of the group -> wire, out, the sources and error buffers afterwards (numpy).  r: the group's given draws
    (float32 [sum of sizes]); seed: GQ_RANDOM_DEVICE; neither: the group's own mode (off, or the counter pair)."""
    dev, g = G.dev, G.g
    nt = len(vs)
    v_offs = v_offs or [0] * nt
    e_offs = e_offs or [0] * nt
    src = [_place(v, o, dev) for v, o in zip(vs, v_offs)]
    er = [(_place(e, o, dev) if e is not None else None) for e, o in zip(errs, e_offs)] if errs is not None else None
    ds = [torch.from_numpy(a).to(dev) for a in dense_src]
    whole = torch.full((G.ub + 2 * CANARY_BYTES,), mx.CANARY, dtype=torch.uint8, device=dev)
    wire = whole[CANARY_BYTES:CANARY_BYTES + G.ub]
    wire.fill_(0xAB)
    obig = torch.full((g.out_floats + 8,), 7.0, dtype=torch.float32, device=dev)
    out = obig[o_off:o_off + g.out_floats] if want_out else None
    kw = {}
    if r is not None:
        kw["draws"] = (torch.from_numpy(np.asarray(r, f32)).to(dev), {i: int(x) for i, x in enumerate(G.first)})
    if seed is not None:
        kw["seed"] = seed
    if er is not None:
        if any(e is None for e in er):      # a null row of the error column: the table is written by hand
            kw.update(errs=[(e[0] if e is not None else src[i][0]) for i, e in enumerate(er)], ef_scale=float(s))
        else:
            kw.update(errs=[e[0] for e in er], ef_scale=float(s))
    if ds:
        kw.update(dense=ds)
    if er is not None and any(e is None for e in er):
        assert g._choose_header([t for t, _ in src], 0, g.align, kw["errs"], ds or None, None, False)
        tab = g._dev[:g._table_words].view(-1, 8)
        for i, e in enumerate(er):
            if e is None:
                tab[i, 7] = 0
        from gq_amd import native
        g._batch.compress(wire, native.RANDOM_GIVEN if r is not None else native.RANDOM_OFF, 0,
                          kw["draws"][0] if r is not None else None, out, float(s))
        g._last_ptrs = None
    else:
        assert g.encode([t for t, _ in src], wire, 0, 0, out=out, **kw)
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    assert np.all(w[:CANARY_BYTES] == mx.CANARY) and np.all(w[CANARY_BYTES + G.ub:] == mx.CANARY), "a write outside the wire"
    for (t, big), o, v in zip(src, v_offs, vs):
        assert _guards_intact(big, o, v.size), "a write outside the source"
    for e, o, a in zip(er or (), e_offs, errs or ()):
        if e is not None:
            assert _guards_intact(e[1], o, a.size), "a write outside the error buffer"
    ob = obig.cpu().numpy()
    assert np.all(ob[:o_off] == 7.0) and np.all(ob[o_off + g.out_floats:] == 7.0), "a write outside out"
    return SimpleNamespace(wire=w[CANARY_BYTES:CANARY_BYTES + G.ub], out=ob[o_off:o_off + g.out_floats],
                           src=[t.cpu().numpy() for t, _ in src],
                           err=[(e[0].cpu().numpy() if e is not None else None) for e in er] if er is not None else None)


def check(G, res, vs, rs=None, errs=None, s=None, nonfinite=False, out=True):
    """Every tensor's section, dense decode, gradient and residual against the restatement.  rs: per-tensor draws or None."""
    for i, v in enumerate(vs):
        n, off, oo = G.sizes[i], G.offs[i], G.g.out_off[i]
        e = errs[i] if errs is not None else None
        sec, D, w, ne = mx.compress(v, G.fmt, rs[i] if rs is not None else None, e, s)
        got = res.wire[off:off + sec.size]
        nb = -(-n // 32)
        assert np.array_equal(got[:nb], sec[:nb]), "tensor %d (n = %d): scale bytes" % (i, n)
        assert np.array_equal(got[:mx._up(nb)], sec[:mx._up(nb)]), "tensor %d (n = %d): the scale bytes' pad" % (i, n)
        assert np.array_equal(got, sec), "tensor %d (n = %d): codes" % (i, n)
        if out:
            assert mx.same(res.out[oo:oo + n], D, nonfinite), "tensor %d (n = %d): the compress's dense decode" % (i, n)
            end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
            assert np.all(res.out[oo + n:end] == 7.0), "a write behind tensor %d's decode" % i
        if e is not None:
            assert mx.same(res.src[i], w, nonfinite), "tensor %d: g <- w" % i
            assert mx.same(res.err[i], ne, nonfinite), "tensor %d: err <- w - decoded" % i
        else:
            assert mx.same(res.src[i], v), "tensor %d: the source changed without error feedback" % i
    last = G.offs[-1] + mx.section_bytes(G.sizes[-1], G.fmt)
    if not G.dense:
        assert np.all(res.wire[last:] == 0xAB)


def _split(r, sizes):
    return np.split(np.asarray(r, f32), np.cumsum(sizes)[:-1])


SIZES = [1, 31, 32, 33, ITEM - 1, ITEM, ITEM + 1, 2 * ITEM + 1, 2048 - 8, 2048 + 9]


@pytest.mark.parametrize("mode", ["off", "given"])
@pytest.mark.parametrize("fmt", FMTS)
def test_sizes(fmt, mode):
    """n = 1, 31, 32, 33, one item -+ 1 element, two items + 1, around one workgroup-wide step -- one group, heavy-tailed values."""
    vs = [mx.randn(n, 100 + n) for n in SIZES]
    G = make_group(SIZES, fmt, random=mode != "off")
    r = np.random.RandomState(7).rand(sum(SIZES)).astype(f32) if mode == "given" else None
    res = compress(G, vs, r=r)
    check(G, res, vs, _split(r, SIZES) if r is not None else None)


@pytest.mark.parametrize("fmt", FMTS)
def test_misaligned_views(fmt):
    """Source, error buffer and out each one float past a 16-byte boundary, alone and together: the scalar paths."""
    sizes = [ITEM + 5, 77]
    vs = [mx.randn(n, 200 + n) for n in sizes]
    es = [mx.randn(n, 300 + n) for n in sizes]
    G = make_group(sizes, fmt)
    r = np.random.RandomState(8).rand(sum(sizes)).astype(f32)
    for v_offs, e_offs, o_off in (([1, 0], [0, 0], 0), ([0, 0], [0, 3], 0), ([0, 0], [0, 0], 1), ([1, 2], [3, 1], 1)):
        res = compress(G, vs, r=r, errs=es, s=0.5, v_offs=v_offs, e_offs=e_offs, o_off=o_off)
        check(G, res, vs, _split(r, sizes), es, 0.5)


@pytest.mark.parametrize("fmt", FMTS)
def test_seventy_tensors_with_identity_tensors(fmt):
    rs = np.random.RandomState(9)
    sizes = [int(x) for x in rs.randint(1, 3000, 70)]
    sizes[5], sizes[40] = ITEM + 3, 3 * ITEM
    dense_sizes = [10, 256, 1]
    vs = [mx.randn(n, 400 + i) for i, n in enumerate(sizes)]
    dsrc = [mx.randn(n, 500 + n) for n in dense_sizes]
    G = make_group(sizes, fmt, dense_sizes=dense_sizes)
    r = rs.rand(sum(sizes)).astype(f32)
    res = compress(G, vs, r=r, dense_src=dsrc)
    check(G, res, vs, _split(r, sizes))
    for (off, n), a in zip(G.dense, dsrc):
        assert np.array_equal(res.wire[off:off + 4 * n].view(np.uint32), a.view(np.uint32)), "an identity tensor's copy"


@pytest.mark.parametrize("mode", ["off", "given"])
@pytest.mark.parametrize("fmt", FMTS)
def test_edge_blocks(fmt, mode):
    """Edge blocks 1 ... 7 and 9: zeros and signed zeros, the smallest subnormal, an all-subnormal block, FLT_MAX, the maximum's
    mantissa at MTHR and one ulp above, +-inf and NaNs with payloads next to finite blocks, every grid value and every midpoint
    (both parities of the tie), y subnormal.  Given draws: uniform, with zeros sprinkled in (frac > 0 against r = 0)."""
    w, where = mx.edge_tensor(fmt)
    r = None
    if mode == "given":
        r = np.random.RandomState(10).rand(w.size).astype(f32)
        r[::5] = 0
        at, m = where["subnormal_y"]
        r[at:at + m] = 0
    G = make_group([w.size], fmt, random=mode != "off")
    res = compress(G, [w], r=r)
    check(G, res, [w], [r] if r is not None else None, nonfinite=True)
    # with error feedback the same blocks arrive as g + 1.0 * 0
    res = compress(G, [w], r=r, errs=[np.zeros_like(w)], s=1.0)
    check(G, res, [w], [r] if r is not None else None, [np.zeros_like(w)], 1.0, nonfinite=True)


@pytest.mark.parametrize("fmt", FMTS)
def test_frac_equals_draw(fmt):
    """Edge 8: the comparison is strict -- r = frac stays, r = frac - 2^-24 goes up, r = 0 goes up only where frac > 0."""
    blocks = [mx.frac_equals_draw(fmt, s, seed) for s, seed in ((-5, 3), (0, 4), (-127, 5), (100, 6))]
    w = np.concatenate([b[0] for b in blocks])
    r = np.concatenate([b[1] for b in blocks])
    G = make_group([w.size], fmt)
    res = compress(G, [w], r=r)
    check(G, res, [w], [r])
    _, code = mx.unpack(res.wire[:mx.section_bytes(w.size, fmt)], w.size, fmt)
    F = mx.FORMATS[fmt]
    assert np.all(code.reshape(-1, 32)[:, 1:10] == F.cmax - 1) and np.all(code.reshape(-1, 32)[:, 11:21] == F.cmax)


@pytest.mark.parametrize("fmt", FMTS)
def test_given_draws_outside_the_unit_interval(fmt):
    """A caller's buffer may hold anything: -0, negatives, 1, values above 1, subnormals, inf, NaN -- frac > r as float32."""
    w = mx.randn(256, 21)
    w[:32] = mx.subnormal_y(fmt)
    special = np.array([-0.0, -1.0, 1.0, 2.5, 2.0 ** -149, 2.0 ** -130, np.inf, -np.inf, np.nan, 0.0], np.float64).astype(f32)
    r = special[np.arange(256) % special.size]
    G = make_group([256], fmt)
    res = compress(G, [w], r=r)
    check(G, res, [w], [r])


@pytest.mark.parametrize("counter", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
def test_device_draws_code_for_code(fmt, counter):
    """GQ_RANDOM_DEVICE and GQ_RANDOM_DEVICE_COUNTER through the restated hash, over two consecutive steps; element i of tensor
    s takes draw first draw + i."""
    sizes = [33, ITEM + 1, 500]
    vs = [mx.randn(n, 600 + n) for n in sizes]
    G = make_group(sizes, fmt)
    seed = 0x1234567887654321
    if counter:
        pairs = torch.tensor([[seed - (1 << 64) if seed >= 1 << 63 else seed, 41], [0, 0]], dtype=torch.int64, device=G.dev)
        G.g.rng_pairs = pairs
    seen = []
    for step in (41, 42):
        if counter:
            res = compress(G, vs)
            pairs[0, 1] += 1
            rs = [mx.draws(mx.COUNTER, n, int(fd), seed, step) for n, fd in zip(sizes, G.first)]
        else:
            res = compress(G, vs, seed=seed + step)
            rs = [mx.draws(mx.DEVICE, n, int(fd), seed + step) for n, fd in zip(sizes, G.first)]
        check(G, res, vs, rs)
        seen.append(res.wire.copy())
    assert not np.array_equal(seen[0], seen[1]), "two steps drew the same numbers"


@pytest.mark.parametrize("fmt", FMTS)
def test_error_feedback(fmt):
    """w = g + s * err with the product rounded first (visible against a fused multiply-add), a carried residual holding inf and
    NaN, and a null row in the error column (that tensor is compressed as it is and its source only read)."""
    sizes = [ITEM + 7, 100, 64]
    vs = [mx.randn(n, 700 + n) for n in sizes]
    es = [mx.randn(n, 800 + n) for n in sizes]
    es[1][3], es[1][40], es[1][77] = np.inf, np.nan, -np.inf
    G = make_group(sizes, fmt)
    r = np.random.RandomState(11).rand(sum(sizes)).astype(f32)
    s = 0.3
    w = (vs[0] + (f32(s) * es[0]).astype(f32)).astype(f32)
    fused = (vs[0].astype(np.float64) + np.float64(f32(s)) * es[0].astype(np.float64)).astype(f32)
    assert not np.array_equal(w.view(np.uint32), fused.view(np.uint32)), "the two roundings are visible in this input"
    res = compress(G, vs, r=r, errs=es, s=s)
    check(G, res, vs, _split(r, sizes), es, s, nonfinite=True)
    # without `out`: the same wire, gradient and residual
    res2 = compress(G, vs, r=r, errs=es, s=s, want_out=False)
    check(G, res2, vs, _split(r, sizes), es, s, nonfinite=True, out=False)
    # a null error row
    es2 = [es[0], None, es[2]]
    res3 = compress(G, vs, r=r, errs=es2, s=s)
    check(G, res3, vs, _split(r, sizes), es2, s)


def decode(G, secs_per_payload, R, plain=False, byte_shift=0, stride_pad=0, o_off=0):
    """The group's decode-mean of R payloads laid out at the group's offsets -> out (numpy).  byte_shift: the payloads start that
    many bytes past a 16-byte boundary; stride_pad: extra bytes between payloads."""
    dev, g = G.dev, G.g
    stride = G.ub + stride_pad
    buf = np.full(byte_shift + R * stride + 16, 0xAB, np.uint8)
    for r in range(R):
        for off, sec in zip(G.offs, secs_per_payload[r]):
            buf[byte_shift + r * stride + off:byte_shift + r * stride + off + sec.size] = sec
    t = torch.from_numpy(buf).to(dev)
    gathered = t[byte_shift:byte_shift + R * stride].view(R, stride)[:, :G.ub]
    obig = torch.full((g.out_floats + 8,), 7.0, dtype=torch.float32, device=dev)
    out = obig[o_off:o_off + g.out_floats]
    if not g.ready:
        g.upload_layout()
    g._batch.decode(gathered, R, out, plain=plain)
    torch.cuda.synchronize()
    ob = obig.cpu().numpy()
    assert np.all(ob[:o_off] == 7.0) and np.all(ob[o_off + g.out_floats:] == 7.0), "a write outside out"
    return ob[o_off:o_off + g.out_floats]


def check_decode(G, out, payloads, R, plain=False):
    for i, n in enumerate(G.sizes):
        want = mx.decode_mean([payloads[r][i] for r in range(R)], n, G.fmt, plain)
        oo = G.g.out_off[i]
        assert mx.same(out[oo:oo + n], want, nan_as_one=True), "tensor %d (n = %d), R = %d" % (i, n, R)
        end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
        assert np.all(out[oo + n:end] == 7.0)


DEC_SIZES = [1, 33, 300, ITEM + 1, 2 * ITEM]


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_hand_built_payloads(fmt):
    """Every code value under the scale bytes 0, 1, 126, 127, 253 and 255; R = 1 ... 17; plain with one payload; sums that are
    subnormal (byte 0 and 1) and huge (byte 253: partial sums overflow to inf, inf - inf gives NaN)."""
    G = make_group(DEC_SIZES, fmt)
    payloads = [[mx.payload_set(n, fmt, 1, seed=1000 * r + n)[0] for n in DEC_SIZES] for r in range(17)]
    for R in list(range(1, 17)) + [17]:
        check_decode(G, decode(G, payloads, R), payloads, R)
    check_decode(G, decode(G, payloads, 1, plain=True), payloads, 1, plain=True)
    check_decode(G, decode(G, payloads[3:], 1, plain=True), payloads[3:], 1, plain=True)


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_every_code_under_every_special_scale_byte_alone(fmt):
    """R = 1, plain and as a mean: EVERY (scale byte, code) pair for the scale bytes 0, 1, 126, 127, 253 and 255 and all 2^bits
    codes decoded on its own -- whole blocks of one scale byte, the codes in ascending order."""
    F = mx.FORMATS[fmt]
    ncode = 1 << F.bits
    per = max(ncode, mx.BLOCK) // mx.BLOCK                  # blocks per scale byte: 1 (FP4, the 16 codes twice) or 8 (FP8)
    specials = [0, 1, 126, 127, 253, 255]
    sb = np.repeat(np.array(specials, np.uint8), per)
    code = np.tile(np.arange(per * mx.BLOCK) % ncode, len(specials))
    n = sb.size * mx.BLOCK
    sec = mx.pack(sb, code, fmt)
    assert sec.size == mx.section_bytes(n, fmt)
    pairs = {(int(a), int(c)) for a, c in zip(np.repeat(sb, mx.BLOCK), code)}
    assert pairs == {(a, c) for a in specials for c in range(ncode)}
    G = make_group([n], fmt)
    for plain in (True, False):
        check_decode(G, decode(G, [[sec]], 1, plain=plain), [[sec]], 1, plain=plain)
    got = decode(G, [[sec]], 1, plain=True)
    assert np.array_equal(mx.bits_of(got[:n]), mx.bits_of(mx.decode_values(sb, code, fmt)))      # (no NaN is excused here)


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_misaligned_wires_and_out(fmt):
    G = make_group(DEC_SIZES, fmt)
    payloads = [[mx.payload_set(n, fmt, 1, seed=77 * r + n)[0] for n in DEC_SIZES] for r in range(3)]
    for shift, pad, o_off in ((1, 0, 0), (4, 0, 0), (8, 0, 1), (0, 3, 0), (0, 8, 3), (5, 7, 1)):
        check_decode(G, decode(G, payloads, 3, byte_shift=shift, stride_pad=pad, o_off=o_off), payloads, 3)
    check_decode(G, decode(G, payloads, 1, plain=True, byte_shift=3, o_off=1), payloads, 1, plain=True)


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_of_compressed_payloads(fmt):
    """Eight users' compressed gradients, -0 and non-finite blocks included: the mean, and the plain decode equals the compress's
    own dense decode."""
    w, _ = mx.edge_tensor(fmt)
    sizes = [w.size, 1000]
    G = make_group(sizes, fmt)
    payloads = []
    for r in range(8):
        vs = [np.roll(w, 32 * r), mx.randn(1000, 900 + r)]
        rr = np.random.RandomState(r).rand(sum(sizes)).astype(f32)
        res = compress(G, vs, r=rr)
        payloads.append([res.wire[o:o + mx.section_bytes(n, fmt)].copy() for o, n in zip(G.offs, sizes)])
        if r == 0:
            got = decode(G, payloads, 1, plain=True)
            assert mx.same(got[:w.size], res.out[:w.size], nan_as_one=True)
    check_decode(G, decode(G, payloads, 8), payloads, 8)


def test_refusals():
    """Each refusal comes before any launch and leaves its text in gq_mx_last_error."""
    from gq_amd import native
    L = native.mx_lib()
    L.gq_mx_last_error.restype = ctypes.c_char_p
    dev = torch.device("cuda:0")
    G = make_group([100], mx.FP4)
    v = torch.zeros(100, device=dev)
    wire = torch.full((G.ub + 16,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats,), 7.0, device=dev)
    assert G.g._choose_header([v], 0, 4, None, None, None, False)
    b = G.g._batch

    def refused(call, text):
        with pytest.raises(native.GQNativeError):
            call()
        assert text in L.gq_mx_last_error().decode(), L.gq_mx_last_error()

    refused(lambda: b.compress(wire[:G.ub], 3), "random_mode")
    refused(lambda: b.compress(wire[:G.ub], 7), "random_mode")
    refused(lambda: b.compress(wire[:G.ub], native.RANDOM_GIVEN), "without draws")
    refused(lambda: b.compress(wire[4:4 + G.ub], native.RANDOM_OFF), "16-byte aligned")
    refused(lambda: b.compress(wire[:G.ub], native.RANDOM_DEVICE_COUNTER, seed=0), "pair")
    fmt = b.s.format
    b.s.format = 2
    refused(lambda: b.compress(wire[:G.ub], native.RANDOM_OFF), "format")
    refused(lambda: b.decode(wire[:G.ub].view(1, -1), 1, out), "format")
    b.s.format = fmt
    b.s.struct_bytes += 8
    refused(lambda: b.compress(wire[:G.ub], native.RANDOM_OFF), "another size")
    refused(lambda: b.decode(wire[:G.ub].view(1, -1), 1, out), "another size")
    b.s.struct_bytes -= 8
    table = b.s.seg_table
    b.s.seg_table = None
    refused(lambda: b.compress(wire[:G.ub], native.RANDOM_OFF), "null table")
    refused(lambda: b.decode(wire[:G.ub].view(1, -1), 1, out), "null table")
    b.s.seg_table = table
    torch.cuda.synchronize()
    assert np.all(wire.cpu().numpy() == 0xAB) and np.all(out.cpu().numpy() == 7.0), "a refused call launched something"
    b.compress(wire[:G.ub], native.RANDOM_OFF)      # and the descriptor still works
    torch.cuda.synchronize()
    assert np.array_equal(wire[:G.ub].cpu().numpy()[:mx.section_bytes(100, mx.FP4)], mx.compress(np.zeros(100, f32), mx.FP4)[0])
