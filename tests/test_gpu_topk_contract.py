"""libgq_topk.so held to include/gq_topk.h bit for bit, through BatchedTopK as the quantizer lays a group out: every comparison is
np.array_equal on bytes or uint32 views against tests/topk_contract.py (whose own checks, and one assertion for every claim made
here about an input, are tests/test_topk_contract.py).  One exception: where float arithmetic made a NaN, any NaN equals any NaN --
`out` (w * 1 or w * 0), and v, err and the wire's values under error feedback (w is a sum there); without error feedback the wire's
values are bit copies, NaN payloads included.

The threshold at both ends and on the seams of every pass's histogram, ties whose last kept one sits on every edge of the write
and scan launches, error feedback against the restatement (two roundings, not a fused multiply-add), garbage in the scratch, two
compresses without a reset, 70 tensors in one group, and the decode launch on payloads written by hand.  The wire starts as 0xAB
and `out` as 7.0, sources and error buffers are views inside guarded buffers, and after EVERY compress the group's histogram is
all zero, the guards are intact and every byte outside the sections and the dense copies still holds its fill.

Not expressible, so not tested: a group where only some tensors carry an error buffer -- BatchedTopK.encode takes `errs` as one
tensor per tensor of the group or not at all."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import topk_contract as tc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, FILL, OUT_FILL, TAIL = 3.0, 0xAB, 7.0, 8


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _dev():
    return torch.device("cuda:0")


class _K(object):
    def __init__(self, k):
        self.k = k


def _up(x, a=16):
    return (x + a - 1) // a * a


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    """Bitwise equal, except that any NaN equals any NaN."""
    a, b = tc.f32(a), tc.f32(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


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


def make_group(sizes, ks, dense_sizes=(), lead=0, gap=0):
    """A BatchedTopK over tensors of `sizes`, its wire laid out as the quantizer lays it out (16-byte aligned sections, the
    identity-compressed tensors behind them); lead / gap: bytes that belong to nobody in front of and between the sections, and 16
    more at the end."""
    from gq_amd.codecs import BatchedTopK, TopKCodec
    dev = _dev()
    codecs = [TopKCodec(_K(k), n, torch.Size([n])) for n, k in zip(sizes, ks)]
    offs, off = [], lead
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes) + gap
    dense = []
    for n in dense_sizes:
        dense.append((off, n))
        off += 4 * n
    ub = _up(off) + 16
    g = BatchedTopK(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=dense or None)
    assert g.out_floats == sum(sizes)
    return SimpleNamespace(g=g, codecs=codecs, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), ks=list(ks))


def compress(G, vs, errs=None, s=None, dense_src=(), v_offs=None, e_offs=None):
    """One compress of the group -> the wire, `out`, the sources and the error buffers afterwards (numpy).  Checks the guards and
    that the histogram is zero again."""
    dev, g = G.dev, G.g
    nt = len(vs)
    v_offs = v_offs or [0] * nt
    e_offs = e_offs or [0] * nt
    src = [_place(v, o, dev) for v, o in zip(vs, v_offs)]
    er = [_place(e, o, dev) for e, o in zip(errs, e_offs)] if errs is not None else None
    ds = [torch.from_numpy(a).to(dev) for a in dense_src]
    wire = torch.full((G.ub,), FILL, dtype=torch.uint8, device=dev)
    out = torch.full((g.out_floats + TAIL,), OUT_FILL, dtype=torch.float32, device=dev)
    kw = {}
    if er is not None:
        kw.update(errs=[t for t, _ in er], ef_scale=float(s))
    if ds:
        kw.update(dense=ds)
    assert g.encode([t for t, _ in src], wire, 0, 0, out=out, **kw)
    torch.cuda.synchronize()
    assert not g._hist.cpu().numpy().any(), "the compress left the histogram non-zero"
    for (t, big), o, v in zip(src, v_offs, vs):
        assert _guards_intact(big, o, v.size), "a write outside the source"
    for (t, big), o, e in zip(er or (), e_offs, errs or ()):
        assert _guards_intact(big, o, e.size), "a write outside the error buffer"
    return SimpleNamespace(wire=wire.cpu().numpy(), out=out.cpu().numpy(), src=[t.cpu().numpy() for t, _ in src],
                           err=[t.cpu().numpy() for t, _ in er] if er is not None else None)


def check(G, res, ws, vs=None, errs=None, s=None, dense_src=(), orders=None):
    """Every section, every dense copy, every gap, `out` and its tail against the restatement.  ws: what the select works on (the
    sources, or with error feedback -- vs, errs, s given -- v + s * err, recomputed here)."""
    ef = errs is not None
    covered = np.zeros(G.ub, bool)
    for i, (n, k, off, oo) in enumerate(zip(G.sizes, G.ks, G.offs, G.g.out_off)):
        order = orders[i] if orders is not None else None
        if ef:
            w, sec, D, e2 = tc.error_feedback(vs[i], errs[i], s, k)
        else:
            w = tc.f32(ws[i])
            sec, D = tc.section_bytes(w, k, order), tc.dense(w, k, order)
        what = "tensor %d (n = %d, k = %d)" % (i, n, k)
        got = res.wire[off:off + 8 * k]
        assert np.array_equal(got[:4 * k], sec[:4 * k]), what + ": indices"
        if ef:
            assert _same(got[4 * k:].view(np.float32), sec[4 * k:].view(np.float32)), what + ": values"
            assert _same(res.src[i], w), what + ": the source is not v + s * err"
            assert _same(res.err[i], e2), what + ": the residual is not w - decoded"
        else:
            assert np.array_equal(got[4 * k:], sec[4 * k:]), what + ": values (bit copies)"
            assert np.array_equal(_bits(res.src[i]), _bits(w)), what + ": the source changed without error feedback"
        assert _same(res.out[oo:oo + n], D), what + ": the dense decode"
        covered[off:off + 8 * k] = True
    for a, (off, n) in zip(dense_src, G.dense):
        assert np.array_equal(res.wire[off:off + 4 * n], a.view(np.uint8)), "an identity-compressed tensor"
        covered[off:off + 4 * n] = True
    assert len(dense_src) == len(G.dense)
    assert np.all(res.wire[~covered] == FILL), "a write outside the sections and the dense copies"
    assert (~covered).sum() >= 16
    assert np.all(res.out[G.g.out_floats:] == OUT_FILL), "a write behind the last tensor's decode"


def alone_and_between(w, k):
    """w as a one-tensor group, then between two ordinary tensors in a group of three (gaps in the wire)."""
    G = make_group([w.size], [k])
    check(G, compress(G, [w]), [w])
    (na, ka, sa), (nb, kb, sb) = tc.NEIGHBOURS
    ws = [tc.ordinary(na, sa), w, tc.ordinary(nb, sb)]
    G = make_group([na, w.size, nb], [ka, k, kb], lead=32, gap=48)
    check(G, compress(G, ws), ws)


# ---- the threshold at the ends and seams of the histograms ----------------------------------------------------------------
@pytest.mark.parametrize("low,more,k", tc.low9_cases(), ids=["low%d%s" % (c[0], "_one_more" if c[1] else "") for c in tc.low9_cases()])
def test_threshold_in_the_last_nine_bits(low, more, k):
    """Keys 0x3f800000 + j, j < 512: passes 0 and 1 see one bin, pass 2 decides.  The threshold's low bits 0, 1 (pick thread 255),
    255 | 256 (threads 128 | 127, two waves), 510, 511 (thread 0); every tie kept, or one more: one tie of the bin below."""
    alone_and_between(tc.low9_input(), k)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["a-1", "a", "a+1"])
@pytest.mark.parametrize("name", sorted(tc.PAIRS))
def test_threshold_on_a_seam_between_two_pick_threads(name, which):
    """Two keys in neighbouring bins that two pick threads own, a = #(the larger one): k = a - 1, a (the pick's interval test
    before < k <= before + sum at its upper end) and a + 1 (at the lower end of the next thread's).  one: 1.0 | nextafter(1, 0), pass-0
    bins 1016 | 1015, threads 128 | 129 (128 the first lane of a wave); two: 2.0 | nextafter(2, 0), bins 1024 | 1023, threads 127 | 128,
    a wave seam; bit9: pass-1 bins 1 | 0; pass1_thread: pass-1 bins 1536 | 1535, threads 63 | 64, a wave seam."""
    alone_and_between(tc.pair_input(name), tc.pair_ks(name)[which])


@pytest.mark.parametrize("name,k", tc.subnormal_cases(), ids=[c[0] for c in tc.subnormal_cases()])
def test_threshold_in_the_lowest_bin(name, k):
    """Signed zeros, subnormals and 7 normals, k above the count of normals: T the smallest subnormal, one in mid-bin, and T = 0 with
    fewer zeros needed than there are -- the kept -0 stays -0 on the wire."""
    alone_and_between(tc.subnormal_input(), k)


@pytest.mark.parametrize("kind,k", tc.TOP_CASES, ids=["more_nans_than_k", "more_infs_than_k", "exactly_k_nonfinite"])
def test_threshold_in_the_top_bins(kind, k):
    """T = 0x7fffffff (NaNs of seven bit patterns, both signs: the lowest indices, their payloads copied), T = 0x7f800000 (pass-0
    bin 2040, the last bin of pick thread 0) with a tie left out and with every tie kept."""
    alone_and_between(tc.top_input(kind), k)


@pytest.mark.parametrize("j", range(6))
def test_k_on_the_end_of_a_pick_threads_bins(j):
    """k = the cumulative count at the end of a pass-0 pick thread's eight bins, and one above it, for three threads."""
    alone_and_between(tc.stair_input(), tc.stair_ks()[j][0])


# ---- ties across every edge of the write and scan launches ------------------------------------------------------------------
@pytest.fixture(scope="module")
def tie_inputs():
    out = {}
    for kind, w, T in (("all_equal", tc.all_equal(tc.TIE_N, 1), 0x3e800000), ("two_level", tc.two_level(tc.TIE_N, 2, tc.TIE_EDGES), tc.ONE)):
        out[kind] = (w, T, tc.ranking(w))
    return out


@pytest.mark.parametrize("pos", tc.TIE_EDGES)
@pytest.mark.parametrize("kind", ["all_equal", "two_level"])
def test_last_kept_tie_on_every_edge(tie_inputs, kind, pos):
    """n = 1,052,673 (258 items).  The last kept tie at 0 (need = 1), 62 | 63 | 64 (lanes, waves), 255 | 256 (steps of an item),
    4095 | 4096 (items), 1,048,575 | 1,048,576 (the scan launch's two rounds of 256 items) and n - 1 (every tie).  all_equal: +-0.25;
    two_level: 2.0 on every sixteenth element of +-1.0, so the count of larger keys in front of a tie is not zero."""
    w, T, order = tie_inputs[kind]
    k = tc.k_for_last_tie(w, T, pos)
    G = make_group([w.size], [k])
    res = compress(G, [w])
    check(G, res, [w], orders=[order])
    assert res.wire[:4 * k].view(np.uint32)[-1] >= pos      # (the last kept index is the tie at pos, or a larger key behind it)


@pytest.mark.parametrize("k", [1048576, 1048577])
def test_half_of_two_million_equal_elements(k):
    w = tc.all_equal(tc.HALF_N, 3)
    G = make_group([w.size], [k])
    res = compress(G, [w])
    check(G, res, [w])
    assert np.array_equal(res.wire[:4 * k].view(np.uint32), np.arange(k, dtype=np.uint32))


@pytest.mark.parametrize("kind", ["all_equal", "two_level"])
def test_tied_tensors_of_every_small_size(kind):
    """n = 1, 255, 256, 257, 4095, 4096, 4097, 8192, each with k = 1 and with k = n, in one group."""
    make = tc.all_equal if kind == "all_equal" else tc.two_level
    sizes = [n for n in tc.TIE_SIZES for _ in range(2)]
    ks = [k for n in tc.TIE_SIZES for k in (1, n)]
    ws = [make(n, 20 + j) for j, n in enumerate(sizes)]
    G = make_group(sizes, ks, gap=16)
    check(G, compress(G, ws), ws)


# ---- error feedback ----------------------------------------------------------------------------------------------------------
EF_CASES = {"reorder_s0.75": (tc.ef_reorder, 0.75), "reorder_s1": (tc.ef_reorder, 1.0), "fma_across_the_threshold": (lambda: tc.ef_fma()[:3], 0.75),
            "ties_on_w_alone": (tc.ef_ties, 1.0), "s0_err_inf": (tc.ef_inf, 0.0), "zeros_s0": (tc.ef_signed_zeros, 0.0),
            "zeros_s-0": (tc.ef_signed_zeros, -0.0)}


@pytest.mark.parametrize("name", sorted(EF_CASES))
def test_error_feedback(name):
    """w = f32(v + f32(s * err)), the select on w, v <- w, err <- w - decoded, out = decoded; wire, out, v and err against the
    restatement.  err that reorders the ranking (s = 0.75 and 1); elements where a fused multiply-add lands one ulp away and swaps
    two elements at the threshold; ties on w that v does not have; s = 0 with err = +-inf (w = NaN, ranked first); s = 0 and -0 on
    signed zeros."""
    make, s = EF_CASES[name]
    v, e, k = make()
    G = make_group([v.size], [k])
    res = compress(G, [v], errs=[e], s=s)
    check(G, res, None, vs=[v], errs=[e], s=s)


def test_error_feedback_with_a_tensor_that_keeps_nothing():
    """k = 0 under error feedback: v becomes w and err becomes w - w * 0, beside a tensor that keeps something."""
    v0, e0, _ = tc.ef_reorder()
    v0, e0 = v0[:4100].copy(), e0[:4100].copy()
    e0[5], v0[6] = np.inf, -np.inf
    v1, e1, k1 = tc.ef_ties()
    G = make_group([v0.size, v1.size], [0, k1], gap=16)
    res = compress(G, [v0, v1], errs=[e0, e1], s=1.0)
    check(G, res, None, vs=[v0, v1], errs=[e0, e1], s=1.0)
    assert np.isnan(res.err[0][[5, 6]]).all() and np.isinf(res.src[0][[5, 6]]).all()


@pytest.mark.parametrize("vo,eo", [(1, 2), (2, 3), (3, 1), (0, 1), (1, 0), (2, 2), (3, 3)])
def test_error_feedback_on_misaligned_views(vo, eo):
    """v and err 4, 8 and 12 bytes past a 16-byte boundary, together and one of them alone, n = 4097 and 5000."""
    v, e, k = tc.ef_reorder()
    vs, es = [v[:4097].copy(), v], [e[:4097].copy(), e]
    G = make_group([4097, v.size], [100, k])
    res = compress(G, vs, errs=es, s=0.75, v_offs=[vo, vo], e_offs=[eo, eo])
    check(G, res, None, vs=vs, errs=es, s=0.75)
    res = compress(G, vs, v_offs=[vo, eo])      # and without error feedback
    check(G, res, vs)


# ---- scratch and replay -------------------------------------------------------------------------------------------------------
def _scratch_group():
    sizes, ks = [1001, 300, 4097, 20000, 1], [27, 0, 124, 600, 1]
    return make_group(sizes, ks, gap=16), sizes, ks


def test_state_and_counts_may_hold_anything():
    """`state` and `counts` are written before they are read: 0x5A5A5A5A in both changes nothing (a k = 0 tensor in the group)."""
    G, sizes, ks = _scratch_group()
    ws = [tc.two_level(n, 30 + i) if i % 2 else tc.ordinary(n, 30 + i) for i, n in enumerate(sizes)]
    for rnd in range(2):
        G.g._state.fill_(0x5A5A5A5A)
        G.g._counts.fill_(0x5A5A5A5A)
        check(G, compress(G, ws), ws)


def test_compresses_follow_one_another_without_a_reset():
    """Three compresses on one group, other inputs each time, the second one with error feedback, nothing reset in between: each is
    right and leaves the histogram zero (compress() asserts it)."""
    G, sizes, ks = _scratch_group()
    a = [tc.heavy_tailed(n, 40 + i) for i, n in enumerate(sizes)]
    check(G, compress(G, a), a)
    v = [tc.two_level(n, 50 + i) for i, n in enumerate(sizes)]
    e = [tc.ordinary(n, 60 + i) for i, n in enumerate(sizes)]
    res = compress(G, v, errs=e, s=0.75)
    check(G, res, None, vs=v, errs=e, s=0.75)
    b = [tc.all_equal(n, 70 + i) for i, n in enumerate(sizes)]
    check(G, compress(G, b), b)


# ---- many tensors ------------------------------------------------------------------------------------------------------------
def test_seventy_tensors_in_one_group():
    """n = 1, k = 0, k = n, ragged sizes, tied and ordinary inputs, two identity-compressed tensors through the dense table: every
    section, every dense copy and every gap."""
    cyc = [1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 9000]
    sizes = [cyc[i % len(cyc)] for i in range(70)]
    ks = [0 if i % 7 == 3 else (n if i % 7 == 5 else max(1, n // 9)) for i, n in enumerate(sizes)]
    assert 0 in ks and any(k == n for k, n in zip(ks, sizes)) and any(n == 1 and k == 1 for k, n in zip(ks, sizes))
    makers = [tc.ordinary, tc.two_level, tc.all_equal, tc.heavy_tailed]
    ws = [makers[i % 4](n, 80 + i) for i, n in enumerate(sizes)]
    small = [tc.ordinary(n, 200 + n) for n in (10, 257)]
    G = make_group(sizes, ks, dense_sizes=[a.size for a in small], gap=16)
    res = compress(G, ws, dense_src=small)
    check(G, res, ws, dense_src=small)


# ---- the decode launch on payloads written by hand ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand_built():
    """tc.hand_payloads() in 16 rows of a buffer wider than a user's wire, every byte outside the sections random."""
    P = tc.hand_payloads()
    G = make_group(tc.DEC_SIZES, tc.DEC_KS, lead=32, gap=48)
    stride = G.ub + 112
    rows = np.random.RandomState(990).randint(0, 256, size=(tc.DEC_PAYLOADS, stride)).astype(np.uint8)
    for r in range(tc.DEC_PAYLOADS):
        for s, (off, k) in enumerate(zip(G.offs, G.ks)):
            idx, val = P[s][r]
            rows[r, off:off + 4 * k] = idx.view(np.uint8)
            rows[r, off + 4 * k:off + 8 * k] = val.view(np.uint8)
    G.g.upload_layout()
    return SimpleNamespace(G=G, rows=torch.from_numpy(rows).to(G.dev), payloads=P)


@pytest.mark.parametrize("first,R,plain", [(f, r, False) for f, r in tc.DEC_WINDOWS] + [(0, 1, True), (1, 1, True)])
def test_decode_of_hand_built_payloads(hand_built, first, R, plain):
    """out = (+0 + c_first + ... + c_{first + R - 1}) / f32(R), payloads in order, a true division, or with plain the one payload
    as it is.  1e8, 1, -1e8 on one index in all six orders (R = 3), sums that a multiplication by f32(1 / 3) gets wrong, indices at
    0, 4095, 4096 and n - 1, payloads whose indices fall into one chunk, a chunk nobody names, k = 0, k = n, NaN and +-inf, -0
    (kept by plain, +0 under the mean), rows 112 bytes and more apart with garbage between them."""
    H = hand_built
    G, g = H.G, H.G.g
    out = torch.full((g.out_floats + TAIL,), OUT_FILL, dtype=torch.float32, device=G.dev)
    g._batch.decode(H.rows[first:first + R, :G.ub], R, out, plain=plain)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for s, (n, k, oo) in enumerate(zip(G.sizes, G.ks, g.out_off)):
        want = tc.decode_mean(H.payloads[s][first:first + R], n, k, R, plain=plain)
        assert _same(got[oo:oo + n], want), "tensor %d (n = %d, k = %d)" % (s, n, k)
    assert np.all(got[g.out_floats:] == OUT_FILL), "a write behind the last tensor's decode"
    s, c = tc.DEC_UNTOUCHED
    oo = g.out_off[s]
    assert not _bits(got[oo + c * tc.CHUNK:oo + (c + 1) * tc.CHUNK]).any()      # +0 where no payload names an index
    if R == 1 and first == 0:
        neg = any((_bits(got[oo:oo + n]) == 1 << 31).any() for n, oo in zip(G.sizes, g.out_off))
        assert neg == plain      # -0 stays -0 under plain; (+0 + -0) / 1 is +0
