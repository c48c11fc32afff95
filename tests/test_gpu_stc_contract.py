"""libgq_stc.so held to include/gq_stc.h at tolerance 0, through BatchedSTC as the quantizer lays a group out: every comparison is
np.array_equal against tests/stc_contract.py (whose own checks, and one assertion for every claim made here about an input, are
tests/test_stc_contract.py).  The wire is compared as bytes everywhere -- mu's NaN is one pattern by contract.  In `out`, the
source and `err`, where float arithmetic made a NaN (w = v + s * err, err = w - decoded), every NaN is mapped to one pattern first.

The wire starts as 0xAB and `out` as 7.0, sources and error buffers are views inside guarded buffers, and after EVERY compress the
group's histogram is all zero, the guards are intact and every byte outside the sections and the dense copies still holds its fill."""
import ctypes
import os
import sys
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import stc_contract as sc  # noqa: E402
import topk_contract as tc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, FILL, OUT_FILL, TAIL = 3.0, 0xAB, 7.0, 8


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _dev():
    return torch.device("cuda:0")


def _one_nan(a):
    """The uint32 view with every NaN as one pattern."""
    a = tc.f32(a)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def _place(arr, off, dev):
    big = torch.full((arr.size + 8,), GUARD, dtype=torch.float32, device=dev)
    view = big[off:off + arr.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view, big


def _guards_intact(big, off, n):
    b = big.cpu().numpy()
    return np.all(b[:off] == GUARD) and np.all(b[off + n:] == GUARD)


def make_group(sizes, ks, dense_sizes=(), lead=0, gap=0):
    """A BatchedSTC over tensors of `sizes`, its wire laid out as the quantizer lays it out (16-byte aligned sections, the
    identity-compressed tensors behind them); lead / gap: canary bytes in front of and between the sections, and 16 more at the end."""
    from gq_amd.codecs import BatchedSTC, STCCodec
    dev = _dev()
    codecs = [STCCodec(None, n, torch.Size([n]), k=k) for n, k in zip(sizes, ks)]
    assert [cd.k for cd in codecs] == list(ks) and all(cd.nbytes == sc.section_size(n, k) for cd, n, k in zip(codecs, sizes, ks))
    offs, off = [], lead
    for cd in codecs:
        offs.append(off)
        off = off + cd.nbytes + gap
    dense = []
    for n in dense_sizes:
        dense.append((off, n))
        off += 4 * n
    ub = sc.up16(off) + 16
    g = BatchedSTC(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=dense or None)
    assert g.out_floats == sum(sizes)
    return SimpleNamespace(g=g, codecs=codecs, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), ks=list(ks))


def garbage(g):
    g._state.fill_(0x5A5A5A5A)
    g._counts.fill_(0x5A5A5A5A)
    g._sums.view(torch.int64).fill_(0x7ff8dead5a5a5a5a)      # sums: a NaN


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
    """Every section, every dense copy, every canary, `out` and its tail against the restatement.  ws: what the select works on (the
    sources, or with error feedback -- vs, errs, s given -- v + s * err, recomputed here)."""
    ef = errs is not None
    covered = np.zeros(G.ub, bool)
    for i, (n, k, off, oo) in enumerate(zip(G.sizes, G.ks, G.offs, G.g.out_off)):
        order = orders[i] if orders is not None else None
        if ef:
            w, sec, D, e2 = sc.error_feedback(vs[i], errs[i], s, k)
        else:
            w = tc.f32(ws[i])
            sec, D = sc.section_bytes(w, k, order), sc.dense(w, k, order)
        what = "tensor %d (n = %d, k = %d)" % (i, n, k)
        got = res.wire[off:off + sec.size]
        assert np.array_equal(got[:16], sec[:16]), what + ": header %r, expected %r" % (got[:16].view(np.uint32), sec[:16].view(np.uint32))
        assert np.array_equal(got, sec), what + ": starts, words or padding"
        if ef:
            assert np.array_equal(_one_nan(res.src[i]), _one_nan(w)), what + ": the source is not v + s * err"
            assert np.array_equal(_one_nan(res.err[i]), _one_nan(e2)), what + ": the residual is not w - decoded"
        else:
            assert np.array_equal(sc.bits(res.src[i]), sc.bits(w)), what + ": the source changed without error feedback"
        assert np.array_equal(sc.bits(res.out[oo:oo + n]), sc.bits(D)), what + ": the dense decode"
        covered[off:off + sec.size] = True
    for a, (off, n) in zip(dense_src, G.dense):
        assert np.array_equal(res.wire[off:off + 4 * n], a.view(np.uint8)), "an identity-compressed tensor"
        covered[off:off + 4 * n] = True
    assert len(dense_src) == len(G.dense)
    assert np.all(res.wire[~covered] == FILL), "a write outside the sections and the dense copies"
    assert (~covered).sum() >= 16
    assert np.all(res.out[G.g.out_floats:] == OUT_FILL), "a write behind the last tensor's decode"


# ---- sizes and selections ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ordinary", "heavy_tailed", "all_equal"])
def test_every_small_size(kind):
    """n = 1,001, 4,096, 4,097, 8,193 and 12,289, each with k = 0, 1, n // 16 and n, in one group with canaries between the sections.
    all_equal: every kept element is a tie (S is need * |T| alone)."""
    make = {"ordinary": tc.ordinary, "heavy_tailed": tc.heavy_tailed, "all_equal": tc.all_equal}[kind]
    sizes = [n for n in sc.SIZES for _ in range(4)]
    ks = [k for n in sc.SIZES for k in (0, 1, n // 16, n)]
    ws = [make(n, 300 + j) for j, n in enumerate(sizes)]
    G = make_group(sizes, ks, lead=32, gap=48)
    check(G, compress(G, ws), ws)


@pytest.fixture(scope="module")
def big_inputs():
    out = {}
    for kind, w in (("heavy_tailed", tc.heavy_tailed(sc.BIG_N, 310)), ("all_equal", tc.all_equal(sc.BIG_N, 311))):
        out[kind] = (w, tc.ranking(w))
    return out


@pytest.mark.parametrize("kind,k", [("heavy_tailed", sc.BIG_N // 256), ("all_equal", sc.BIG_N // 2), ("heavy_tailed", sc.BIG_N)])
def test_two_million_elements(big_inputs, kind, k):
    """513 items: three rounds of the scan launch, the sum tree padded to 1,024 with two halvings inside a thread."""
    w, order = big_inputs[kind]
    G = make_group([w.size], [k])
    check(G, compress(G, [w]), [w], orders=[order])


@pytest.mark.parametrize("j", range(4))
def test_last_kept_tie_on_either_side_of_an_item_seam(j):
    k, pos = sc.seam_ks()[j]
    w = sc.seam_input()
    G = make_group([w.size], [k], lead=16)
    check(G, compress(G, [w]), [w])


def test_items_that_keep_nothing_beside_one_that_keeps_everything():
    w, k = sc.lopsided_input()
    G = make_group([w.size], [k])
    res = compress(G, [w])
    check(G, res, [w])
    assert list(res.wire[16:16 + 24].view(np.uint32)) == [0, 0, 0, 4096, 4096, 4136]


@pytest.mark.parametrize("name", [c[0] for c in sc.special_cases()])
def test_special_values(name):
    """+-0, subnormals, +-inf and NaN, kept and dropped: mu = NaN (one pattern) or inf, a subnormal mu, kept -0 and kept NaN carry
    their sign bit into the word and the decode."""
    _, w, k = [c for c in sc.special_cases() if c[0] == name][0]
    G = make_group([w.size], [k])
    check(G, compress(G, [w]), [w])


# ---- error feedback --------------------------------------------------------------------------------------------------------------
EF_CASES = {"reorder_s0.75": (tc.ef_reorder, 0.75), "reorder_s1": (tc.ef_reorder, 1.0), "fma_across_the_threshold": (lambda: tc.ef_fma()[:3], 0.75),
            "ties_on_w_alone": (tc.ef_ties, 1.0), "s0_err_inf": (tc.ef_inf, 0.0), "zeros_s-0": (tc.ef_signed_zeros, -0.0)}


@pytest.mark.parametrize("name", sorted(EF_CASES))
def test_error_feedback(name):
    """w = f32(v + f32(s * err)) in every pass (two roundings: the fma case swaps two elements at the threshold under a fused load),
    v <- w, err <- w - decoded, out = decoded.  A NaN ef_scale switches it off: the same group without `errs` leaves v alone."""
    make, s = EF_CASES[name]
    v, e, k = make()
    G = make_group([v.size], [k])
    res = compress(G, [v], errs=[e], s=s)
    check(G, res, None, vs=[v], errs=[e], s=s)
    check(G, compress(G, [v]), [v])


@pytest.mark.parametrize("vo,eo", [(1, 2), (3, 1), (2, 0)])
def test_misaligned_views(vo, eo):
    v, e, k = tc.ef_reorder()
    vs, es = [v[:4097].copy(), v], [e[:4097].copy(), e]
    G = make_group([4097, v.size], [128, k])
    res = compress(G, vs, errs=es, s=0.75, v_offs=[vo, vo], e_offs=[eo, eo])
    check(G, res, None, vs=vs, errs=es, s=0.75)
    res = compress(G, vs, v_offs=[vo, eo])
    check(G, res, vs)


# ---- scratch, many tensors, replay ---------------------------------------------------------------------------------------------------
def test_scratch_may_hold_anything_and_compresses_follow_one_another():
    """`state`, `counts` and `sums` are written before they are read; three compresses with no reset, the second with error feedback."""
    sizes, ks = [1001, 300, 4097, 20000, 1], [27, 0, 128, 625, 1]
    G = make_group(sizes, ks, gap=16)
    a = [tc.heavy_tailed(n, 40 + i) for i, n in enumerate(sizes)]
    garbage(G.g)
    check(G, compress(G, a), a)
    v = [tc.two_level(n, 50 + i) for i, n in enumerate(sizes)]
    e = [tc.ordinary(n, 60 + i) for i, n in enumerate(sizes)]
    garbage(G.g)
    check(G, compress(G, v, errs=e, s=0.75), None, vs=v, errs=e, s=0.75)
    b = [tc.all_equal(n, 70 + i) for i, n in enumerate(sizes)]
    check(G, compress(G, b), b)


def test_seventy_tensors_and_dense_tensors_in_one_group():
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


def test_graph_replay_over_changing_inputs():
    """The eight launches captured once and replayed three times over new gradients in the same storage, the scratch scribbled over."""
    sizes, ks = [1001, 4097, 12289], [3, 16, 768]
    G = make_group(sizes, ks)
    dev, g = G.dev, G.g
    src = [torch.zeros(n, dtype=torch.float32, device=dev) for n in sizes]
    wire = torch.zeros(G.ub, dtype=torch.uint8, device=dev)
    out = torch.zeros(g.out_floats + TAIL, dtype=torch.float32, device=dev)
    assert g.encode(src, wire, 0, 0, out=out)      # eager once: the tables are uploaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert g.encode(src, wire, 0, 0, out=out, table_current=True)
    for rep in range(3):
        vs = [tc.heavy_tailed(n, 400 + 10 * rep + i) for i, n in enumerate(sizes)]
        for t, v in zip(src, vs):
            t.copy_(torch.from_numpy(v))
        wire.fill_(FILL)
        out.fill_(OUT_FILL)
        garbage(g)
        graph.replay()
        torch.cuda.synchronize()
        assert not g._hist.cpu().numpy().any()
        res = SimpleNamespace(wire=wire.cpu().numpy(), out=out.cpu().numpy(), src=[t.cpu().numpy() for t in src], err=None)
        check(G, res, vs)


# ---- the decode launch on payloads written by hand ------------------------------------------------------------------------------
DEC_N, DEC_K = [12289, 4097, 1001], [192, 4097, 0]


@pytest.fixture(scope="module")
def hand_built():
    """17 payloads per tensor in rows 4 bytes past a 16-byte boundary and row + 4 bytes apart, 0xEE between them."""
    G = make_group(DEC_N, DEC_K, lead=16, gap=32)
    secs = [sc.hand_sections(n, k, 17, 500 + i)[0] for i, (n, k) in enumerate(zip(DEC_N, DEC_K))]
    stride = G.ub + 4
    buf = np.full(4 + 17 * stride, 0xEE, np.uint8)
    for r in range(17):
        for off, per in zip(G.offs, secs):
            buf[4 + r * stride + off:4 + r * stride + off + per[r].size] = per[r]
    G.g.upload_layout()
    dev_buf = torch.from_numpy(buf).to(G.dev)
    return SimpleNamespace(G=G, secs=secs, rows=torch.as_strided(dev_buf, (17, G.ub), (stride, 1), 4), keep=dev_buf)


@pytest.mark.parametrize("R,plain", [(r, False) for r in range(1, 18)] + [(1, True)])
def test_decode_of_hand_built_payloads(hand_built, R, plain):
    """out = (+0 + c_0 + ... + c_{R-1}) / f32(R), payloads in order, a true division; plain: +-mu as it is.  Payload 1 cancels
    payload 0 (+mu + -mu = +0), every third payload sits in one item, k = n (a full item of words) and k = 0 beside them; `out` a
    misaligned view between canaries."""
    H = hand_built
    G, g = H.G, H.G.g
    obig = torch.full((3 + g.out_floats + TAIL,), OUT_FILL, dtype=torch.float32, device=G.dev)
    g._batch.decode(H.rows[:R], R, obig[3:3 + g.out_floats], plain=plain)
    torch.cuda.synchronize()
    ob = obig.cpu().numpy()
    assert np.all(ob[:3] == OUT_FILL) and np.all(ob[3 + g.out_floats:] == OUT_FILL), "a write outside `out`"
    got = ob[3:3 + g.out_floats]
    for s, (n, k, oo) in enumerate(zip(DEC_N, DEC_K, g.out_off)):
        want = sc.decode_mean(H.secs[s][:R], n, k, R, plain=plain)
        assert np.array_equal(sc.bits(got[oo:oo + n]), sc.bits(want)), "tensor %d (n = %d, k = %d)" % (s, n, k)
    if R == 2:
        assert not sc.bits(got[:DEC_N[0]]).any()      # the two payloads cancel to +0 everywhere
    if R == 1:
        neg = bool((sc.bits(got[:DEC_N[0]]) >> 31).any())
        assert neg      # -mu under both; the mean of one payload divides by 1


def test_decode_of_a_wire_that_lies():
    """Starts above k and out of order, positions past the item's length, k in the header above the table's: nothing outside `out`
    is written and the launch returns."""
    n, k = sc.LIE_N, sc.LIE_K
    G = make_group([n], [k])
    sec = sc.lying_section()
    row = np.full(G.ub, 0xEE, np.uint8)
    row[:sec.size] = sec
    obig = torch.full((n + TAIL,), OUT_FILL, dtype=torch.float32, device=G.dev)
    G.g.upload_layout()
    G.g._batch.decode(torch.from_numpy(row).to(G.dev).view(1, -1), 1, obig[:n])
    torch.cuda.synchronize()
    ob = obig.cpu().numpy()
    assert np.all(ob[n:] == OUT_FILL)
    assert np.array_equal(sc.bits(ob[:n]), sc.bits(sc.decode_mean([sec], n, k, 1)))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from gq_amd import native
    G = make_group([4097, 8193], [16, 32])
    dev, g = G.dev, G.g
    src = [torch.from_numpy(tc.ordinary(n, 1)).to(dev) for n in (4097, 8193)]
    wire = torch.full((G.ub + 16,), FILL, dtype=torch.uint8, device=dev)
    assert g.encode(src, wire[:G.ub], 0, 0)
    torch.cuda.synchronize()
    wire.fill_(FILL)
    out = torch.full((g.out_floats + 1,), OUT_FILL, dtype=torch.float32, device=dev)
    b, L = g._batch, native.stc_lib()
    nan = ctypes.c_float(float("nan"))
    W, O = ctypes.c_void_p(wire.data_ptr()), ctypes.c_void_p(out.data_ptr())

    def refused(rc):
        assert rc != 0 and L.gq_stc_last_error()

    def comp(wp=W, ef=nan, op=O):
        return L.gq_stc_compress_batched(b.ref, wp, ef, op, None)

    def with_field(name, value, call):
        old = getattr(b.s, name)
        setattr(b.s, name, value)
        try:
            refused(call())
        finally:
            setattr(b.s, name, old)

    for name, value in (("struct_bytes", 72), ("nseg", 0), ("nitems", 0), ("seg_table", None), ("item_seg", None), ("hist", None),
                        ("state", None), ("counts", None), ("sums", None)):
        with_field(name, value, comp)
    refused(comp(wp=ctypes.c_void_p(wire.data_ptr() + 2)))
    refused(comp(wp=ctypes.c_void_p(0)))
    refused(comp(ef=ctypes.c_float(1.0), op=ctypes.c_void_p(0)))
    dec = lambda R, gp=W, stride=G.ub: L.gq_stc_decode_sum_batched(b.ref, gp, ctypes.c_int64(stride), R, O, 0, None)
    refused(dec(0))
    refused(dec(2, stride=G.ub + 2))
    refused(dec(1, gp=ctypes.c_void_p(wire.data_ptr() + 2)))
    with_field("struct_bytes", 72, lambda: dec(1))
    torch.cuda.synchronize()
    assert bool((wire == FILL).all()) and bool((out == OUT_FILL).all()), "a refused call wrote something"


def test_quantizer_refusals():
    from gq_amd.compressors import SparseTernaryCompressor
    from gq_amd.quantizers import PSQuantizer, RingQuantizer
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=1, mode="ps", cr=64)
    params = [torch.nn.Parameter(torch.zeros(5000, device=_dev()))]
    with pytest.raises(ValueError, match="ring mode"):
        RingQuantizer(SparseTernaryCompressor, params, Namespace(**dict(base, mode="ring")))
    with pytest.raises(ValueError, match="momentum_correction"):
        PSQuantizer(SparseTernaryCompressor, params, Namespace(**dict(base, momentum_correction=0.9)))
    with pytest.raises(ValueError, match="float32 parameters only"):
        PSQuantizer(SparseTernaryCompressor, [torch.nn.Parameter(torch.zeros(5000, device=_dev(), dtype=torch.bfloat16))], Namespace(**base))
