"""The two 6-bit formats (FP6 E2M3, FP6 E3M2) of libgq_mx.so held to include/gq_mx.h, bit for bit: every comparison is np.array_equal
on bytes or uint32 views against tests/mx6_contract.py (whose own checks are tests/test_mx6_contract.py) -- every byte of every
section (the 8 zero bytes behind an odd number of blocks included), dense out, the gradient and the residual after error feedback;
only where an input block is not finite does every NaN count as one pattern.  The harness (canaries round the wire, guarded sources
and error buffers, `out` preset to 7.0, the wire preset to 0xAB) is tests/test_gpu_mx_contract.py's.
(The name sorts behind every other GPU test file: tests/test_gpu_z_mx6_api.py says why.)"""
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
import mx6_contract as m6  # noqa: E402
import test_gpu_mx_contract as base  # noqa: E402  (the harness: compress, decode, _split)

pytestmark = pytest.mark.gpu

f32 = np.float32
FMTS = list(m6.FP6)
ITEM = m6.ITEM
SEED = 0x1234567887654321


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def make_group(sizes, fmt, random=True, rng="device", dense_sizes=()):
    from gq_amd.codecs import BatchedMX, MXCodec
    dev = torch.device("cuda:0")
    comp = SimpleNamespace(format=m6.NAMES[fmt], random=random, _rng=rng)
    codecs = [MXCodec(comp, n, torch.Size([n])) for n in sizes]
    assert [cd.nbytes for cd in codecs] == [m6.section_bytes(n, fmt) for n in sizes]
    offs, dense, ub = m6.layout(sizes, fmt, dense_sizes)
    g = BatchedMX(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=dense or None)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return SimpleNamespace(g=g, codecs=codecs, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), fmt=fmt, first=first)


def check(G, res, vs, rs=None, errs=None, s=None, nonfinite=False, out=True):
    """Every tensor's section, dense decode, gradient and residual against the restatement.  rs: per-tensor draws or None."""
    for i, v in enumerate(vs):
        n, off, oo = G.sizes[i], G.offs[i], G.g.out_off[i]
        e = errs[i] if errs is not None else None
        sec, D, w, ne = m6.compress(v, G.fmt, rs[i] if rs is not None else None, e, s)
        assert sec.size == m6.section_bytes(n, G.fmt)
        got = res.wire[off:off + sec.size]
        nb = -(-n // 32)
        assert np.array_equal(got[:nb], sec[:nb]), "tensor %d (n = %d): scale bytes" % (i, n)
        assert np.array_equal(got[:m6._up(nb)], sec[:m6._up(nb)]), "tensor %d (n = %d): the scale bytes' pad" % (i, n)
        assert np.array_equal(got[:m6._up(nb) + 24 * nb], sec[:m6._up(nb) + 24 * nb]), "tensor %d (n = %d): codes" % (i, n)
        assert np.array_equal(got, sec), "tensor %d (n = %d): the zero pad behind the codes" % (i, n)
        if out:
            assert m6.same(res.out[oo:oo + n], D, nonfinite), "tensor %d (n = %d): the compress's dense decode" % (i, n)
            end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
            assert np.all(res.out[oo + n:end] == 7.0), "a write behind tensor %d's decode" % i
        if e is not None:
            assert m6.same(res.src[i], w, nonfinite), "tensor %d: g <- w" % i
            assert m6.same(res.err[i], ne, nonfinite), "tensor %d: err <- w - decoded" % i
        else:
            assert m6.same(res.src[i], v), "tensor %d: the source changed without error feedback" % i
    last = G.offs[-1] + m6.section_bytes(G.sizes[-1], G.fmt)
    if not G.dense:
        assert np.all(res.wire[last:] == 0xAB)


# n = 1, 31, 32, 33 (nb 2), 63 / 64 / 65 (nb 2, 2, 3: an odd nb writes the pad), the step seam, the item seam, two items + 1
SIZES = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, ITEM - 1, ITEM, ITEM + 1, 2 * ITEM + 1]


@pytest.mark.parametrize("mode", ["off", "given"])
@pytest.mark.parametrize("fmt", FMTS)
def test_sizes(fmt, mode):
    assert {(-(-n // 32)) % 2 for n in SIZES} == {0, 1}
    vs = [m6.randn(n, 100 + n) for n in SIZES]
    G = make_group(SIZES, fmt, random=mode != "off")
    r = np.random.RandomState(7).rand(sum(SIZES)).astype(f32) if mode == "given" else None
    res = base.compress(G, vs, r=r)
    check(G, res, vs, base._split(r, SIZES) if r is not None else None)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("n", [1, 33, 65, 2049, ITEM + 1])
def test_one_tensor_alone(fmt, n):
    """A tensor on its own: its section ends the wire, so nothing behind the pad belongs to anyone (the canaries start there)."""
    v = m6.randn(n, 150 + n)
    G = make_group([n], fmt, random=False)
    assert G.ub == m6.section_bytes(n, fmt)
    check(G, base.compress(G, [v]), [v])


@pytest.mark.parametrize("fmt", FMTS)
def test_misaligned_views(fmt):
    """Source, error buffer and out each one float past a 16-byte boundary, alone and together: the scalar paths."""
    sizes = [ITEM + 5, 77]
    vs = [m6.randn(n, 200 + n) for n in sizes]
    es = [m6.randn(n, 300 + n) for n in sizes]
    G = make_group(sizes, fmt)
    r = np.random.RandomState(8).rand(sum(sizes)).astype(f32)
    for v_offs, e_offs, o_off in (([1, 0], [0, 0], 0), ([0, 0], [0, 3], 0), ([0, 0], [0, 0], 1), ([1, 2], [3, 1], 1)):
        res = base.compress(G, vs, r=r, errs=es, s=0.5, v_offs=v_offs, e_offs=e_offs, o_off=o_off)
        check(G, res, vs, base._split(r, sizes), es, 0.5)


@pytest.mark.parametrize("fmt", FMTS)
def test_seventy_tensors_with_identity_tensors(fmt):
    rs = np.random.RandomState(9)
    sizes = [int(x) for x in rs.randint(1, 3000, 70)]
    sizes[5], sizes[40] = ITEM + 3, 3 * ITEM
    nbs = [(-(-n // 32)) % 2 for n in sizes]
    assert 20 < sum(nbs) < 50, "odd and even numbers of blocks mixed"
    dense_sizes = [10, 256]
    vs = [m6.randn(n, 400 + i) for i, n in enumerate(sizes)]
    dsrc = [m6.randn(n, 500 + n) for n in dense_sizes]
    G = make_group(sizes, fmt, dense_sizes=dense_sizes)
    r = rs.rand(sum(sizes)).astype(f32)
    res = base.compress(G, vs, r=r, dense_src=dsrc)
    check(G, res, vs, base._split(r, sizes))
    for (off, n), a in zip(G.dense, dsrc):
        assert np.array_equal(res.wire[off:off + 4 * n].view(np.uint32), a.view(np.uint32)), "an identity tensor's copy"


@pytest.mark.parametrize("mode", ["off", "given"])
@pytest.mark.parametrize("fmt", FMTS)
def test_edge_blocks(fmt, mode):
    """Zeros and signed zeros, the smallest subnormal, an all-subnormal block, FLT_MAX, the maximum's mantissa at this format's MTHR
    and one ulp above, +-inf and NaNs with payloads next to finite blocks, every grid value and every midpoint (both parities of
    the tie), y subnormal."""
    w, where = m6.edge_tensor(fmt)
    r = None
    if mode == "given":
        r = np.random.RandomState(10).rand(w.size).astype(f32)
        r[::5] = 0
        at, m = where["subnormal_y"]
        r[at:at + m] = 0
    G = make_group([w.size], fmt, random=mode != "off")
    res = base.compress(G, [w], r=r)
    check(G, res, [w], [r] if r is not None else None, nonfinite=True)
    res = base.compress(G, [w], r=r, errs=[np.zeros_like(w)], s=1.0)
    check(G, res, [w], [r] if r is not None else None, [np.zeros_like(w)], 1.0, nonfinite=True)


@pytest.mark.parametrize("fmt", FMTS)
def test_frac_equals_draw(fmt):
    """The comparison is strict -- r = frac stays, r = frac - 2^-24 goes up, r = 0 goes up only where frac > 0."""
    blocks = [m6.frac_equals_draw(fmt, s, seed) for s, seed in ((-5, 3), (0, 4), (-127, 5), (100, 6))]
    w = np.concatenate([b[0] for b in blocks])
    r = np.concatenate([b[1] for b in blocks])
    G = make_group([w.size], fmt)
    res = base.compress(G, [w], r=r)
    check(G, res, [w], [r])
    _, code = m6.unpack(res.wire[:m6.section_bytes(w.size, fmt)], w.size, fmt)
    F = m6.FORMATS[fmt]
    assert np.all(code.reshape(-1, 32)[:, 1:10] == F.cmax - 1) and np.all(code.reshape(-1, 32)[:, 11:21] == F.cmax)


@pytest.mark.parametrize("counter", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
def test_device_draws_code_for_code(fmt, counter):
    """GQ_RANDOM_DEVICE and GQ_RANDOM_DEVICE_COUNTER through the restated hash, at two seeds / steps; element i of tensor s takes
    draw first draw + i (three different first draws)."""
    sizes = [33, ITEM + 1, 500]
    vs = [m6.randn(n, 600 + n) for n in sizes]
    G = make_group(sizes, fmt)
    if counter:
        pairs = torch.tensor([[SEED, 41], [0, 0]], dtype=torch.int64, device=G.dev)
        G.g.rng_pairs = pairs
    seen = []
    for step in (41, 42):
        if counter:
            res = base.compress(G, vs)
            pairs[0, 1] += 1
            rs = [m6.draws(m6.COUNTER, n, int(fd), SEED, step) for n, fd in zip(sizes, G.first)]
        else:
            res = base.compress(G, vs, seed=SEED + step)
            rs = [m6.draws(m6.DEVICE, n, int(fd), SEED + step) for n, fd in zip(sizes, G.first)]
        check(G, res, vs, rs)
        seen.append(res.wire.copy())
    assert not np.array_equal(seen[0], seen[1]), "two steps drew the same numbers"


@pytest.mark.parametrize("fmt", FMTS)
def test_counter_draws_replayed_from_a_graph(fmt):
    """Compress + plain decode captured once: a replay writes the same bytes while the step word stands, and draws afresh once it
    has moved -- each time the restatement's bytes."""
    from gq_amd import native
    sizes = [65, ITEM + 1]
    vs = [m6.randn(n, 650 + n) for n in sizes]
    G = make_group(sizes, fmt)
    dev = G.dev
    pairs = torch.tensor([[SEED, 5], [0, 0]], dtype=torch.int64, device=dev)
    src = [torch.from_numpy(v).to(dev) for v in vs]
    wire = torch.full((G.ub,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats,), 7.0, device=dev)
    mean = torch.full((G.g.out_floats,), 7.0, device=dev)
    assert G.g._choose_header(src, 0, G.g.align, None, None, None, False)
    b = G.g._batch

    def launches():
        b.compress(wire, native.RANDOM_DEVICE_COUNTER, pairs.data_ptr(), None, out)
        b.decode(wire.view(1, -1), 1, mean, plain=True)

    launches()      # (eagerly once: nothing is allocated under capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    seen = []
    for step in (5, 5, 6):
        wire.fill_(0xAB)
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        res = SimpleNamespace(wire=wire.cpu().numpy(), out=out.cpu().numpy(), src=[t.cpu().numpy() for t in src], err=None)
        check(G, res, vs, [m6.draws(m6.COUNTER, n, int(fd), SEED, step) for n, fd in zip(sizes, G.first)])
        assert np.array_equal(m6.bits_of(mean.cpu().numpy()), m6.bits_of(res.out))
        seen.append(res.wire.copy())
        if len(seen) == 2:
            pairs[0, 1] += 1
    assert np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


@pytest.mark.parametrize("fmt", FMTS)
def test_error_feedback_over_two_records(fmt):
    """ef_scale 1 and 0.5, two consecutive records each (the second starts from the first one's residual), a tensor of the group
    without an error buffer, the wire full of garbage beforehand and every byte of every section compared."""
    sizes = [ITEM + 7, 100, 65]
    G = make_group(sizes, fmt)
    for s in (1.0, 0.5):
        es = [m6.randn(n, 800 + n) for n in sizes]
        es[1][3], es[1][40], es[1][77] = np.inf, np.nan, -np.inf
        for rec in range(2):
            vs = [m6.randn(n, 700 + 10 * rec + n) for n in sizes]
            r = np.random.RandomState(11 + rec).rand(sum(sizes)).astype(f32)
            res = base.compress(G, vs, r=r, errs=es, s=s)
            check(G, res, vs, base._split(r, sizes), es, s, nonfinite=True)
            es = [e.copy() for e in res.err]
    es = [m6.randn(n, 900 + n) for n in sizes]
    vs = [m6.randn(n, 950 + n) for n in sizes]
    r = np.random.RandomState(13).rand(sum(sizes)).astype(f32)
    w = (vs[0] + (f32(0.3) * es[0]).astype(f32)).astype(f32)
    fused = (vs[0].astype(np.float64) + np.float64(f32(0.3)) * es[0].astype(np.float64)).astype(f32)
    assert not np.array_equal(w.view(np.uint32), fused.view(np.uint32)), "the two roundings are visible in this input"
    res = base.compress(G, vs, r=r, errs=es, s=0.3, want_out=False)
    check(G, res, vs, base._split(r, sizes), es, 0.3, out=False)
    es2 = [es[0], None, es[2]]
    res = base.compress(G, vs, r=r, errs=es2, s=0.3)
    check(G, res, vs, base._split(r, sizes), es2, 0.3)


def check_decode(G, out, payloads, R, plain=False):
    for i, n in enumerate(G.sizes):
        want = m6.decode_mean([payloads[r][i] for r in range(R)], n, G.fmt, plain)
        oo = G.g.out_off[i]
        assert m6.same(out[oo:oo + n], want, nan_as_one=True), "tensor %d (n = %d), R = %d" % (i, n, R)
        end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
        assert np.all(out[oo + n:end] == 7.0)


DEC_SIZES = [1, 33, 65, 300, ITEM + 1, 2 * ITEM]


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_hand_built_payloads(fmt):
    """Every one of the 64 codes under the scale bytes 0, 1, 126, 127, 253 and 255; R = 1 ... 16; plain with one payload."""
    G = make_group(DEC_SIZES, fmt)
    payloads = [[m6.payload_set(n, fmt, 1, seed=1000 * r + n)[0] for n in DEC_SIZES] for r in range(16)]
    for R in range(1, 17):
        check_decode(G, base.decode(G, payloads, R), payloads, R)
    check_decode(G, base.decode(G, payloads, 1, plain=True), payloads, 1, plain=True)
    check_decode(G, base.decode(G, payloads[3:], 1, plain=True), payloads[3:], 1, plain=True)


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_every_code_under_every_special_scale_byte_alone(fmt):
    """R = 1, plain and as a mean: EVERY (scale byte, code) pair for the scale bytes 0, 1, 126, 127, 253, 255 and all 64 codes; a
    -0 (code 32) survives the plain decode and becomes +0 in the mean."""
    specials = [0, 1, 126, 127, 253, 255]
    sb = np.repeat(np.array(specials, np.uint8), 2)
    code = np.tile(np.arange(64), len(specials))
    n = sb.size * 32
    sec = m6.pack(sb, code, fmt)
    assert sec.size == m6.section_bytes(n, fmt)
    G = make_group([n], fmt)
    for plain in (True, False):
        check_decode(G, base.decode(G, [[sec]], 1, plain=plain), [[sec]], 1, plain=plain)
    got = base.decode(G, [[sec]], 1, plain=True)
    assert np.array_equal(m6.bits_of(got[:n]), m6.bits_of(m6.decode_values(sb, code, fmt)))      # (no NaN is excused here)
    at = 6 * 32 + 32      # scale byte 127, code 32
    assert m6.bits_of(got[at:at + 1])[0] == 0x80000000
    assert m6.bits_of(base.decode(G, [[sec]], 1)[at:at + 1])[0] == 0


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_byte_path_equals_word_path(fmt):
    """`gathered` 1, 2, 4 and 8 bytes past a 16-byte boundary, odd and even strides: 4-byte aligned payloads take dword loads, the
    others byte loads; both against the restatement, hence bit-equal to each other.  The last payload ends the buffer's used part."""
    G = make_group(DEC_SIZES, fmt)
    payloads = [[m6.payload_set(n, fmt, 1, seed=77 * r + n)[0] for n in DEC_SIZES] for r in range(3)]
    aligned = base.decode(G, payloads, 3)
    check_decode(G, aligned, payloads, 3)
    for shift, pad, o_off in ((1, 0, 0), (2, 0, 0), (4, 0, 0), (8, 0, 1), (0, 3, 0), (0, 4, 0), (0, 8, 3), (5, 7, 1), (4, 1, 0)):
        got = base.decode(G, payloads, 3, byte_shift=shift, stride_pad=pad, o_off=o_off)
        assert np.array_equal(m6.bits_of(got), m6.bits_of(aligned)), (shift, pad)
    for shift in (0, 1, 2, 3, 4):
        check_decode(G, base.decode(G, payloads, 1, plain=True, byte_shift=shift, o_off=1), payloads, 1, plain=True)


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_of_compressed_payloads(fmt):
    """Eight users' compressed gradients, -0 and non-finite blocks included: the mean, and the plain decode equals the compress's
    own dense decode."""
    w, _ = m6.edge_tensor(fmt)
    sizes = [w.size, 1000]
    G = make_group(sizes, fmt)
    payloads = []
    for r in range(8):
        vs = [np.roll(w, 32 * r), m6.randn(1000, 900 + r)]
        rr = np.random.RandomState(r).rand(sum(sizes)).astype(f32)
        res = base.compress(G, vs, r=rr)
        payloads.append([res.wire[o:o + m6.section_bytes(n, fmt)].copy() for o, n in zip(G.offs, sizes)])
        if r == 0:
            got = base.decode(G, payloads, 1, plain=True)
            assert m6.same(got[:w.size], res.out[:w.size], nan_as_one=True)
    check_decode(G, base.decode(G, payloads, 8), payloads, 8)


def test_refusals():
    """Ids that name no format stay refused by both entry points, before any launch."""
    from gq_amd import native
    L = native.mx_lib()
    L.gq_mx_last_error.restype = ctypes.c_char_p
    dev = torch.device("cuda:0")
    G = make_group([100], m6.FP6_E2M3, random=False)
    v = torch.zeros(100, device=dev)
    wire = torch.full((G.ub + 16,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats,), 7.0, device=dev)
    assert G.g._choose_header([v], 0, 4, None, None, None, False)
    b = G.g._batch
    fmt = b.s.format
    assert fmt == 0x23
    for bad in (2, 0x22, 6, 0x33, -1):
        b.s.format = bad
        for call in (lambda: b.compress(wire[:G.ub], native.RANDOM_OFF), lambda: b.decode(wire[:G.ub].view(1, -1), 1, out)):
            with pytest.raises(native.GQNativeError):
                call()
            assert "format" in L.gq_mx_last_error().decode(), L.gq_mx_last_error()
    b.s.format = fmt
    torch.cuda.synchronize()
    assert np.all(wire.cpu().numpy() == 0xAB) and np.all(out.cpu().numpy() == 7.0), "a refused call launched something"
    b.compress(wire[:G.ub], native.RANDOM_OFF)      # and the descriptor still works
    torch.cuda.synchronize()
    assert np.array_equal(wire[:G.ub].cpu().numpy(), m6.compress(np.zeros(100, f32), m6.FP6_E2M3)[0])
