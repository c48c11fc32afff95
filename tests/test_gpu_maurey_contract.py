"""libgq_maurey.so held to include/gq_maurey.h's order of additions at every level, bit for bit: every comparison is
np.array_equal on bytes or uint32 views against tests/maurey_contract.py (whose own checks are tests/test_maurey_contract.py), with
nothing excused.  Long tensors (the run level with m = 2 and 3), draws exactly on C_i with zero weights behind them across every
kind of edge, u = 0 / -0 / >= 1 / inf / NaN, the order of additions seen through the clamp, draws with replacement, misaligned views,
the error-feedback edges, scratch full of garbage, 70 tensors in one group, and the decode launch on hand-built payloads.  Every
compress hands the draws in (GQ_RANDOM_GIVEN); wire and `out` start as 0xAB / 7.0, tensors sit inside guarded buffers."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import maurey_contract as mc  # noqa: E402

pytestmark = pytest.mark.gpu

HEADER, SIGN, GUARD = mc.HEADER, mc.SIGN, 3.0


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


class _K(object):
    def __init__(self, k):
        self.k = k


def _up(x, a=16):
    return (x + a - 1) // a * a


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _place(arr, off, dev):
    """arr as a view `off` floats into a buffer of its own (4 * off bytes past a 16-byte boundary) -> (view, buffer)"""
    big = torch.full((arr.size + 8,), GUARD, dtype=torch.float32, device=dev)
    view = big[off:off + arr.size]
    view.copy_(torch.from_numpy(arr))
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view, big


def _guards_intact(big, off, n):
    b = big.cpu().numpy()
    return np.all(b[:off] == GUARD) and np.all(b[off + n:] == GUARD)


def make_group(sizes, ks, dense_sizes=()):
    """A BatchedMaurey over tensors of `sizes`, its wire laid out as the quantizer lays it out (identity-compressed tensors behind)."""
    from gq_amd.codecs import BatchedMaurey, MaureyCodec
    dev = torch.device("cuda:0")
    codecs = [MaureyCodec(_K(k), n, torch.Size([n])) for n, k in zip(sizes, ks)]
    offs, off = [], 0
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes)
    dense = []
    for n in dense_sizes:
        dense.append((off, n))
        off += 4 * n
    ub = _up(off)
    g = BatchedMaurey(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=dense or None)
    return SimpleNamespace(g=g, codecs=codecs, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), ks=list(ks))


def compress(G, vs, us, errs=None, s=None, dense_src=(), v_offs=None, e_offs=None):
    """One compress of the group -> the wire, `out`, the sources and the error buffers afterwards (numpy)."""
    dev, g = G.dev, G.g
    nt = len(vs)
    v_offs = v_offs or [0] * nt
    e_offs = e_offs or [0] * nt
    src = [_place(v, o, dev) for v, o in zip(vs, v_offs)]
    er = [_place(e, o, dev) for e, o in zip(errs, e_offs)] if errs is not None else None
    ds = [torch.from_numpy(a).to(dev) for a in dense_src]
    starts = np.concatenate([[0], np.cumsum(G.ks)[:-1]])
    draws = (torch.from_numpy(np.concatenate(us).astype(np.float32)).to(dev), {i: int(x) for i, x in enumerate(starts)})
    wire = torch.full((G.ub,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((g.out_floats,), 7.0, dtype=torch.float32, device=dev)
    kw = {}
    if er is not None:
        kw.update(errs=[t for t, _ in er], ef_scale=float(s))
    if ds:
        kw.update(dense=ds)
    assert g.encode([t for t, _ in src], wire, 0, 0, draws=draws, out=out, **kw)
    torch.cuda.synchronize()
    for (t, big), o, v in zip(src, v_offs, vs):
        assert _guards_intact(big, o, v.size), "a write outside the source"
    for (t, big), o, e in zip(er or (), e_offs, errs or ()):
        assert _guards_intact(big, o, e.size), "a write outside the error buffer"
    return SimpleNamespace(wire=wire.cpu().numpy(), out=out.cpu().numpy(), src=[t.cpu().numpy() for t, _ in src],
                           err=[t.cpu().numpy() for t, _ in er] if er is not None else None)


def check_tensor(G, res, i, w, u):
    """Tensor i's section and dense decode against the restatement of the contract on w."""
    n, k, off, oo = G.sizes[i], G.ks[i], G.offs[i], G.g.out_off[i]
    sec, D = mc.compress(w, u, k)
    got = res.wire[off:off + G.codecs[i].nbytes]
    assert got.size == sec.size == HEADER + _up(4 * k)
    assert np.array_equal(got[:HEADER], sec[:HEADER]), "tensor %d (n = %d): header" % (i, n)
    assert np.array_equal(got[HEADER:HEADER + 4 * k], sec[HEADER:HEADER + 4 * k]), "tensor %d (n = %d): words" % (i, n)
    assert np.array_equal(got, sec), "tensor %d (n = %d): padding" % (i, n)
    assert np.array_equal(_bits(res.out[oo:oo + n]), _bits(D)), "tensor %d (n = %d): the compress's dense decode" % (i, n)
    end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
    assert np.all(res.out[oo + n:end] == 7.0), "a write behind tensor %d's decode" % i
    return mc.split_section(sec, k)


def one(v, u, **kw):
    """A one-tensor group through a compress, checked against the restatement -> (result, scale, words)"""
    G = make_group([v.size], [u.size])
    res = compress(G, [v], [u], **kw)
    scale, words = check_tensor(G, res, 0, v, u)
    assert np.array_equal(_bits(res.src[0]), _bits(v)), "the source changed without error feedback"
    return res, scale, words


# ---- long tensors: the run level ---------------------------------------------------------------------------------------
LONG = [1048576, 1048577, 1310000, 2097153]      # 256 items (m = 1), 257 (m = 2, the last run one item of one element), 320, 513 (m = 3)


@pytest.mark.parametrize("kind", ["heavy_tailed", "islands"])
@pytest.mark.parametrize("n", LONG)
def test_long_tensors(n, kind):
    """k = 4099 (not a multiple of 4: the padding is written).  heavy_tailed: randn * 1e-3 * exp(3 * randn); islands: zero except
    for three islands of items, so that the leading 300 items (160 of the two shapes with fewer than 320), whole runs in the
    middle and the trailing items are zero."""
    k = 4099
    v = mc.heavy_tailed(n, n % 997) if kind == "heavy_tailed" else mc.islands(n, n % 997)
    u = np.random.RandomState(n % 997 + 1).rand(k).astype(np.float32)
    res, scale, words = one(v, u)
    assert np.all(v[(words & ~SIGN).astype(np.int64)] != 0)


# ---- draws exactly on C_i, zero weights behind them ---------------------------------------------------------------------
@pytest.mark.parametrize("long", [False, True], ids=["12289", "1048577"])
def test_ties_and_zero_weights(long):
    """Integer inputs with T = 2^p (p <= 24) and u = C_i / T exactly (tests/test_maurey_contract.py asserts both): t = C_i selects
    the next element of nonzero weight, across a thread, a group and an item edge and a whole zero item (n = 12,289), across a run
    edge, a whole zero run and into a last run of one element (n = 1,048,577); t = 0 in front of leading zeros."""
    v, u, t, p, behind = mc.tie_case(long)
    res, scale, words = one(v, u)
    idx = (words & ~SIGN).astype(np.int64)
    assert np.all(v[idx] != 0), "an element of weight zero was drawn"
    assert np.all(np.isin(behind, idx))
    assert scale == np.float32(2.0 ** p) / np.float32(u.size)


# ---- u at and beyond the ends of [0, 1) ---------------------------------------------------------------------------------
def test_edge_values_of_u():
    """u = [0, -0, 1e-45, nextafter(1, 0), 1, 2, inf, NaN] on tensors whose first and last items are zero, whose last item is
    partial behind trailing zeros, and whose first nonzero element is small enough for 1e-45 to pass it."""
    cases = mc.edge_u_tensors()
    vs = [v for _, v in cases]
    G = make_group([v.size for v in vs], [mc.EDGE_U.size] * len(vs))
    res = compress(G, vs, [mc.EDGE_U] * len(vs))
    for i, v in enumerate(vs):
        scale, words = check_tensor(G, res, i, v, mc.EDGE_U)
        assert np.all(v[(words & ~SIGN).astype(np.int64)] != 0), cases[i][0]


@pytest.mark.parametrize("long", [False, True], ids=["5000", "1048577"])
def test_the_clamp_follows_the_tree_order(long):
    """|v| = [2^100, 2^46 x 4989, 0 x 10], every u = 1: every word is the last element that moved the TREE sum (4989; a
    left-to-right sum gives 0), and the header is float32(T_tree) / float32(k).  n = 1,048,577, |v| = [2^100, 2^35 ...]: the same
    through the run level (the first element of item 255; a sum without runs of two items never moves after item 0)."""
    v = mc.order_case(long)
    pick = mc.ORDER_LONG_PICK if long else mc.ORDER_PICK
    k = 7
    res, scale, words = one(v, np.ones(k, np.float32))
    want = np.uint32(pick) | (SIGN if v[pick] < 0 else np.uint32(0))
    assert np.array_equal(words, np.full(k, want, np.uint32))
    assert scale == np.float32(mc.tree_cdf(v)[1]) / np.float32(k)


@pytest.mark.parametrize("n,k", [(100, 5000), (4096, 10000)])
def test_draws_with_replacement(n, k):
    v = mc.heavy_tailed(n, 120 + n % 7)
    v[::7] = 0
    u = np.random.RandomState(121).rand(k).astype(np.float32)
    res, scale, words = one(v, u)
    assert np.unique(words).size < k and np.all(v[(words & ~SIGN).astype(np.int64)] != 0)


# ---- views that are not 16-byte aligned ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, 20000])
def test_misaligned_views(n):
    """The source `o` floats into its buffer, o = 1, 2, 3 (whole threads read element by element), without and with error feedback;
    under error feedback the error buffer at another offset, one of the two aligned or neither.  Bytes, dense decode, stored-back
    source and residual equal the aligned run's, which equals the restatement."""
    k, s = n // 33, np.float32(0.75)
    rs = np.random.RandomState(130 + n % 5)
    v, e = mc.heavy_tailed(n, 131), (rs.standard_normal(n) * 1e-3).astype(np.float32)
    u = rs.rand(k).astype(np.float32)
    G = make_group([n], [k])
    base = compress(G, [v], [u])
    check_tensor(G, base, 0, v, u)
    for o in (1, 2, 3):
        res = compress(G, [v], [u], v_offs=[o])
        assert np.array_equal(res.wire, base.wire) and np.array_equal(_bits(res.out), _bits(base.out)), o
        assert np.array_equal(_bits(res.src[0]), _bits(v)), o
    w = mc.feedback(v, e, s)
    base = compress(G, [v], [u], errs=[e], s=s)
    scale, words = check_tensor(G, base, 0, w, u)
    D = mc.dense(words, scale, n)
    assert np.array_equal(_bits(base.src[0]), _bits(w)) and np.array_equal(_bits(base.err[0]), _bits(w - D))
    for vo, eo in ((1, 2), (2, 3), (3, 1), (0, 1), (1, 0), (2, 2)):
        res = compress(G, [v], [u], errs=[e], s=s, v_offs=[vo], e_offs=[eo])
        assert np.array_equal(res.wire, base.wire) and np.array_equal(_bits(res.out), _bits(base.out)), (vo, eo)
        assert np.array_equal(_bits(res.src[0]), _bits(w)) and np.array_equal(_bits(res.err[0]), _bits(w - D)), (vo, eo)


# ---- error feedback where the sampler has nothing to do ------------------------------------------------------------------
def _ef_inputs():
    n, rs = 20000, np.random.RandomState(140)
    s = np.float32(0.5)
    # all of w's weight in item 2: items 1, 3, 4 are zero in v and err, item 0 cancels (v = -1, err = 2: w = -1 + 0.5 * 2 = +0)
    v1, e1 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    v1[8192:12288] = mc.heavy_tailed(4096, 141)
    e1[8192:12288] = (rs.standard_normal(4096) * 1e-3).astype(np.float32)
    v1[:4096], e1[:4096] = -1, 2
    # w all zero: +0, -0 and cancelling pairs
    v2, e2 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    v2[1::3] = np.float32(-0.0)
    v2[5000:6000], e2[5000:6000] = 3, -6
    # one inf
    v3, e3 = mc.heavy_tailed(n, 142), (rs.standard_normal(n) * 1e-3).astype(np.float32)
    v3[7] = np.inf
    return s, [("one_item", v1, e1), ("all_zero", v2, e2), ("one_inf", v3, e3)]


@pytest.mark.parametrize("case", [0, 1, 2], ids=["one_item", "all_zero", "one_inf"])
def test_error_feedback_edges(case):
    """The source becomes w = v + s * err (the product rounded, then the sum), err = w - D, out = D, the wire that of w: where four
    of five items receive no draw (one of them holds v and err that cancel: it is still stored back), where w is all zero, and
    where w holds an inf (degenerate: index 0 with a plus sign, scale inf)."""
    s, cases = _ef_inputs()
    name, v, e = cases[case]
    n, k = v.size, 600
    u = np.random.RandomState(143).rand(k).astype(np.float32)
    w = mc.feedback(v, e, s)
    if case == 0:
        assert not w[:8192].any() and not w[12288:].any() and w[8192:12288].any() and np.all(_bits(w[:4096]) == 0)
    if case == 1:
        assert np.all(w == 0)
    G = make_group([n], [k])
    res = compress(G, [v], [u], errs=[e], s=s)
    scale, words = check_tensor(G, res, 0, w, u)
    D = mc.dense(words, scale, n)
    assert np.array_equal(_bits(res.src[0]), _bits(w)), "the source is not v + s * err"
    with np.errstate(invalid="ignore"):
        assert np.array_equal(_bits(res.err[0]), _bits(w - D)), "the residual is not w - D"
    if case == 1:
        assert not res.wire.any()
    if case == 2:
        assert np.isinf(scale) and not words.any() and np.isinf(res.out[0]) and not res.out[1:n].any()


# ---- the scratch may hold anything ----------------------------------------------------------------------------------------
def test_scratch_need_not_be_zero():
    sizes, ks = [1001, 17, 4097, 20000, 1], [27, 5, 124, 600, 3]
    G = make_group(sizes, ks)
    g = G.g
    vs = [mc.heavy_tailed(n, 150 + i) for i, n in enumerate(sizes)]
    for rnd in range(2):
        g._sums.fill_(float("nan"))
        g._totals.fill_(float("nan"))
        g._counts.fill_(-1)
        g._draw_item.fill_(-1)
        g._bucket.fill_(7.0)
        rs = np.random.RandomState(160 + rnd)
        us = [rs.rand(k).astype(np.float32) for k in ks]
        res = compress(G, vs, us)
        for i, (v, u) in enumerate(zip(vs, us)):
            check_tensor(G, res, i, v, u)
    us2 = [np.random.RandomState(170).rand(k).astype(np.float32) for k in ks]      # and on what the last compress left behind
    res = compress(G, vs, us2)
    for i, (v, u) in enumerate(zip(vs, us2)):
        check_tensor(G, res, i, v, u)


# ---- many tensors ------------------------------------------------------------------------------------------------------------
def test_seventy_tensors_in_one_group():
    cyc = [1, 2, 3, 15, 16, 17, 4095, 4096, 4097, 9000]
    sizes = [cyc[i % len(cyc)] for i in range(70)]
    ks = [1 if n <= 17 else n // 33 for n in sizes]
    dense_sizes = [10, 257, 5]
    G = make_group(sizes, ks, dense_sizes)
    assert np.array_equal(G.g._layout[:, 6].numpy(), np.concatenate([[0], np.cumsum(ks)[:-1]])) and G.g.ndraws == sum(ks)
    rs = np.random.RandomState(180)
    vs = [mc.heavy_tailed(n, 181 + i) for i, n in enumerate(sizes)]
    us = [rs.rand(k).astype(np.float32) for k in ks]
    small = [rs.standard_normal(n).astype(np.float32) for n in dense_sizes]
    res = compress(G, vs, us, dense_src=small)
    for i, (v, u) in enumerate(zip(vs, us)):
        check_tensor(G, res, i, v, u)
        assert np.array_equal(_bits(res.src[i]), _bits(v))
    for a, (off, n) in zip(small, G.dense):
        assert np.array_equal(res.wire[off:off + 4 * n], a.view(np.uint8)), "an identity-compressed tensor"
    end = G.dense[-1][0] + 4 * G.dense[-1][1]
    assert np.all(res.wire[end:] == 0xAB)      # (the wire's tail belongs to nobody)


# ---- the decode launch on payloads written by hand ------------------------------------------------------------------------
DEC_SIZES, DEC_KS, DEC_PAYLOADS = [1, 4096, 4097, 12289], [5, 37, 64, 131], 16


def _hand_words(n, k, r, rs):
    """Payload r's k words of an n-element tensor, piled on the chunk edges: r % 4 == 0 -- all k on ONE index; 1 -- the first chunk
    only; 2 -- every hot index and a few others; 3 -- the last chunk only (so chunks go without a word from some payloads).
    The sign of an index alternates from payload to payload."""
    hot = sorted(set(i for i in (0, 4095, 4096, 8191, 8192, n - 1) if i < n))
    last = (n - 1) // mc.CHUNK * mc.CHUNK
    if r % 4 == 0:
        pool = [hot[(r // 4) % len(hot)]]
    elif r % 4 == 1:
        pool = [i for i in hot if i < mc.CHUNK]
    elif r % 4 == 2:
        pool = hot + [int(x) for x in rs.randint(0, n, size=3)]
    else:
        pool = [i for i in hot if i >= last]
    idx = np.sort(np.array(pool, np.int64)[rs.randint(0, len(pool), size=k)])
    return idx.astype(np.uint32) | np.where((idx + r) % 2 == 1, SIGN, np.uint32(0))


@pytest.fixture(scope="module")
def hand_built():
    """16 payloads for tensors of [1, 4096, 4097, 12289] elements (k = 5 > n for the first), sections 48 bytes apart in rows longer
    than they need, scales that differ per payload and are 0.0 in two of them."""
    from gq_amd.codecs import BatchedMaurey, MaureyCodec
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(190)
    codecs = [MaureyCodec(_K(k), n, torch.Size([n])) for n, k in zip(DEC_SIZES, DEC_KS)]
    offs, off = [], 32
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes) + 48
    stride = off + 112
    g = BatchedMaurey(codecs, offs, list(range(len(codecs))), dev, 1, stride)
    scales = (rs.rand(DEC_PAYLOADS, len(codecs)) * np.float32(10.0) ** rs.randint(-3, 3, size=(DEC_PAYLOADS, len(codecs)))).astype(np.float32)
    scales[1], scales[6] = 0.0, 0.0
    rows = np.full((DEC_PAYLOADS, stride), 0xAB, np.uint8)
    payloads = [[] for _ in codecs]
    for r in range(DEC_PAYLOADS):
        for s, (cd, o, n, k) in enumerate(zip(codecs, offs, DEC_SIZES, DEC_KS)):
            words = _hand_words(n, k, r, rs)
            sec = np.zeros(cd.nbytes // 4, np.uint32)
            sec[0] = scales[r, s:s + 1].view(np.uint32)[0]
            sec[4:4 + k] = words
            rows[r, o:o + cd.nbytes] = sec.view(np.uint8)
            payloads[s].append((scales[r, s], words))
    g.upload_layout()
    return SimpleNamespace(g=g, rows=torch.from_numpy(rows).to(dev), payloads=payloads)


@pytest.mark.parametrize("first,R,plain", [(0, 1, True), (1, 1, True), (0, 1, False), (1, 1, False), (0, 2, False), (3, 2, False),
                                           (0, 8, False), (0, 16, False)],
                         ids=["plain", "plain_scale0", "R1", "R1_scale0", "R2", "R2_from3", "R8", "R16"])
def test_decode_of_hand_built_payloads(hand_built, first, R, plain):
    """out = ((+0 + D_first) + ... + D_{first + R - 1}) / float32(R) in f32, or D_first itself (plain: a -0 stays -0), bit for bit;
    +0 where nothing was drawn; nothing written between the tensors' outputs."""
    H = hand_built
    g = H.g
    out = torch.full((g.out_floats,), 7.0, dtype=torch.float32, device=H.rows.device)
    g._batch.decode(H.rows[first:first + R], R, out, plain=plain)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for s, (n, oo) in enumerate(zip(DEC_SIZES, g.out_off)):
        want = mc.decode_mean(H.payloads[s][first:first + R], n, plain=plain)
        assert np.array_equal(_bits(got[oo:oo + n]), _bits(want)), "tensor %d (n = %d)" % (s, n)
        end = g.out_off[s + 1] if s + 1 < len(DEC_SIZES) else g.out_floats
        assert np.all(got[oo + n:end] == 7.0)
    if plain and first == 1:
        assert any((_bits(got[oo:oo + n]) == 1 << 31).any() for n, oo in zip(DEC_SIZES, g.out_off))      # scale 0: -0 was there to keep
