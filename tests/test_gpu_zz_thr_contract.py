"""libgq_thr.so held to include/gq_thr.h, bit for bit: every comparison is np.array_equal on bytes or uint32 views against
tests/thr_contract.py (whose own checks are tests/test_thr_contract.py) -- the whole wire section with canaries round the wire, the
dense `out`, the gradient and the residual after error feedback, guards round every buffer, garbage in every scratch buffer.
NaNs: w * 0 of an infinity or a NaN, and a sum that takes a NaN in, leave the NaN's sign and payload to the hardware; such elements
(where the INPUT holds an infinity or a NaN -- computed from the input, never from what the kernels return) count as one pattern.
(zz: the file runs behind the other GPU tests, for the reason tests/test_gpu_z_mx6_api.py gives.)"""
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
import thr_contract as tc  # noqa: E402

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
GUARD = f32(-123.25)
CANARY, CANARY_BYTES = 0xC5, 64
SIZES = [1001, 4096, 4097, 8193, 135169]      # 1, 1, 2, 3 and 34 items
CR = 64


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def same(got, want, loose=None):
    """All 32 bits; where `loose`: NaN where the contract has NaN, the bits elsewhere."""
    g, w = np.ascontiguousarray(got, dtype=f32).view(u32), np.ascontiguousarray(want, dtype=f32).view(u32)
    if loose is None:
        return np.array_equal(g, w)
    nan = loose & np.isnan(want)
    return np.array_equal(g[~nan], w[~nan]) and bool(np.all(np.isnan(np.asarray(got)[nan])))


def _place(arr, off, dev):
    big = torch.full((arr.size + 8,), float(GUARD), dtype=torch.float32, device=dev)
    view = big[off:off + arr.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view, big


def _guards_intact(big, off, n):
    b = big.cpu().numpy()
    return np.all(b[:off] == GUARD) and np.all(b[off + n:] == GUARD)


def make_group(sizes, S, eta=None, cr=CR, percent=150, M=1, dense_sizes=()):
    from gq_amd.codecs import BatchedThr, ThrCodec, thr_section_bytes
    from gq_amd.compressors import ThresholdSparsificationCompressor
    dev = torch.device("cuda:0")
    args = SimpleNamespace(cr=cr, thr_stages=S, thr_value=eta, thr_cap_percent=percent, thr_fit_stride=M)
    codecs = [ThrCodec(ThresholdSparsificationCompressor(n, (n,), args), n, torch.Size([n])) for n in sizes]
    assert [cd.nbytes for cd in codecs] == [tc.section_bytes(n, cr, percent) for n in sizes] == [thr_section_bytes(n, cr, percent) for n in sizes]
    assert [cd.stride for cd in codecs] == [tc.stride_for(n, M) for n in sizes]
    offs, dense, ub = tc.layout(sizes, cr, percent, dense_sizes)
    g = BatchedThr(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=dense or None)
    return SimpleNamespace(g=g, codecs=codecs, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), S=S, eta=eta, cr=cr, percent=percent,
                           M=M)


def garbage(g):
    """Garbage in every scratch buffer: the launches write what they read."""
    g._sums.fill_(float("nan"))
    g._state.fill_(0x5A5A5A5A)
    g._counts.fill_(0x7B7B7B7B)


def compress(G, vs, errs=None, s=None, dense_src=(), v_offs=None, e_offs=None, o_off=0, want_out=True):
    dev, g = G.dev, G.g
    nt = len(vs)
    v_offs = v_offs or [0] * nt
    e_offs = e_offs or [0] * nt
    src = [_place(v, o, dev) for v, o in zip(vs, v_offs)]
    er = [_place(e, o, dev) for e, o in zip(errs, e_offs)] if errs is not None else None
    ds = [torch.from_numpy(a).to(dev) for a in dense_src]
    whole = torch.full((G.ub + 2 * CANARY_BYTES,), CANARY, dtype=torch.uint8, device=dev)
    wire = whole[CANARY_BYTES:CANARY_BYTES + G.ub]
    wire.fill_(0xAB)
    obig = torch.full((g.out_floats + 8,), 7.0, dtype=torch.float32, device=dev)
    out = obig[o_off:o_off + g.out_floats] if want_out else None
    kw = {}
    if er is not None:
        kw.update(errs=[e[0] for e in er], ef_scale=float(s))
    if ds:
        kw.update(dense=ds)
    garbage(g)
    assert g.encode([t for t, _ in src], wire, 0, 0, out=out, **kw)
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    assert np.all(w[:CANARY_BYTES] == CANARY) and np.all(w[CANARY_BYTES + G.ub:] == CANARY), "a write outside the wire"
    for (t, big), o, v in zip(src, v_offs, vs):
        assert _guards_intact(big, o, v.size), "a write outside the source"
    for e, o, a in zip(er or (), e_offs, errs or ()):
        assert _guards_intact(e[1], o, a.size), "a write outside the error buffer"
    ob = obig.cpu().numpy()
    assert np.all(ob[:o_off] == 7.0) and np.all(ob[o_off + g.out_floats:] == 7.0), "a write outside out"
    return SimpleNamespace(wire=w[CANARY_BYTES:CANARY_BYTES + G.ub], out=ob[o_off:o_off + g.out_floats],
                           src=[t.cpu().numpy() for t, _ in src], err=[e[0].cpu().numpy() for e in er] if er is not None else None)


def check(G, res, vs, errs=None, s=None, out=True, dense_src=()):
    """Every tensor's section, dense decode, gradient and residual against the restatement -> [(kept, found, eta)]."""
    seen = []
    for i, v in enumerate(vs):
        n, off, oo = G.sizes[i], G.offs[i], G.g.out_off[i]
        e = errs[i] if errs is not None else None
        sec, D, w, ne, eta, found = tc.compress(v, G.cr, G.S, G.eta, G.percent, G.codecs[i].stride, e, s)
        what = "tensor %d (n = %d, S = %d)" % (i, n, G.S)
        got = res.wire[off:off + sec.size]
        assert np.array_equal(got[:16].view(u32), sec[:16].view(u32)), what + ": header %r, want %r" % (got[:16].view(u32), sec[:16].view(u32))
        assert np.array_equal(got, sec), what + ": the section"
        loose = ~np.isfinite(w)
        if out:
            assert same(res.out[oo:oo + n], D, loose), what + ": the compress's dense decode"
        if errs is not None:
            assert same(res.src[i], w, loose), what + ": the gradient after error feedback"
            assert same(res.err[i], ne, loose), what + ": the residual"
        else:
            assert same(res.src[i], v), what + ": the gradient was written"
        seen.append((int(sec[:4].view(u32)[0]), found, eta))
    for (off, n), a in zip(G.dense, dense_src):
        assert np.array_equal(res.wire[off:off + 4 * n].view(u32), a.view(u32)), "a dense copy"
    return seen


def inputs(sizes, seed):
    fams = [tc.specials, tc.laplace, tc.gaussian, tc.student, tc.half_zero]
    return [fams[i % len(fams)](n, seed + i) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("S", [1, 2, 3, 4, 8])
def test_fitted_stages(S):
    """Every size (1, 1, 2, 3, 34 items; fit stride 2 on the last), special values in the first tensor, garbage scratch."""
    G = make_group(SIZES, S, M=2)
    assert G.codecs[-1].stride == 2 and all(cd.stride == 1 for cd in G.codecs[:-1])
    vs = inputs(SIZES, 10 * S)
    seen = check(G, compress(G, vs), vs)
    assert any(found > 0 for _, found, _ in seen)


@pytest.mark.parametrize("eta", [0.0, 1e-3, 2.5e-3, float(tc.FLT_MAX)])
def test_fixed_threshold(eta):
    G = make_group(SIZES, 0, eta=eta)
    vs = inputs(SIZES, 3)
    seen = check(G, compress(G, vs, want_out=False), vs, out=False)
    if eta == 0.0:
        assert all(found > cd.cap for (_, found, _), cd in zip(seen, G.codecs))
    if eta == float(tc.FLT_MAX):
        assert seen[0][1] == 6 and all(found == 0 for _, found, _ in seen[1:])      # the first tensor's infinities and NaNs


@pytest.mark.parametrize("which", ["cap", "cap+1", "far", "none", "sparse", "on_eta"])
def test_outcomes(which):
    """found exactly cap, cap + 1 and far above it, found = 0, fewer non-zeros than k (eta stays 0), elements exactly on eta."""
    case = tc.outcome_case(which)
    G = make_group([case.v.size], case.S, eta=case.eta, cr=case.cr)
    seen = check(G, compress(G, [case.v]), [case.v])
    assert seen[0][1] == case.found and tc.ebits(seen[0][2]) == tc.ebits(case.eta_out)


def test_seventy_tensors_dense_and_misaligned_views():
    rs = np.random.RandomState(5)
    sizes = [int(x) for x in rs.randint(1001, 9000, size=70)]
    dense_sizes = [10, 1000, 3]
    G = make_group(sizes, 3, dense_sizes=dense_sizes)
    vs = inputs(sizes, 100)
    ds = [tc.gaussian(n, 900 + n) for n in dense_sizes]
    offs = [i % 4 for i in range(70)]
    res = compress(G, vs, dense_src=ds, v_offs=offs, o_off=1)
    check(G, res, vs, dense_src=ds)


@pytest.mark.parametrize("S,scale", [(3, 1.0), (2, 0.3), (0, 0.7)])
def test_error_feedback(S, scale):
    """v + s * err with both roundings (s = 0.3 / 0.7: the product is inexact), special values in v and err, misaligned views."""
    G = make_group(SIZES, S, eta=1e-3 if S == 0 else None)
    vs = inputs(SIZES, 40)
    errs = [tc.specials(n, 77 + n) if i % 2 == 0 else tc.laplace(n, 77 + n, 3e-4) for i, n in enumerate(SIZES)]
    res = compress(G, vs, errs=errs, s=scale, v_offs=[1, 0, 2, 3, 0], e_offs=[0, 3, 1, 0, 2])
    check(G, res, vs, errs=errs, s=scale)
    if scale == 1.0:      # (the product is exact: one rounding either way)
        return
    with np.errstate(all="ignore"):
        fused = [np.float64(v) + np.float64(scale) * np.float64(e) for v, e in zip(vs, errs)]
    assert any(np.any(np.float32(f)[np.isfinite(f)] != tc.feedback(v, e, scale)[np.isfinite(f)]) for f, v, e in zip(fused, vs, errs)), \
        "no element on which a fused v + s * err would differ"


def test_graph_replay_over_changing_inputs():
    """The whole sequence captured once and replayed three times over new gradients in the same storage."""
    G = make_group(SIZES, 3, M=2)
    dev, g = G.dev, G.g
    src = [torch.zeros(n, dtype=torch.float32, device=dev) for n in SIZES]
    wire = torch.zeros(G.ub, dtype=torch.uint8, device=dev)
    out = torch.zeros(g.out_floats, dtype=torch.float32, device=dev)
    vs = inputs(SIZES, 60)
    for t, v in zip(src, vs):
        t.copy_(torch.from_numpy(v))
    assert g.encode(src, wire, 0, 0, out=out)      # eager once: the tables are uploaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert g.encode(src, wire, 0, 0, out=out, table_current=True)
    for rep in range(3):
        vs = inputs(SIZES, 61 + rep)
        for t, v in zip(src, vs):
            t.copy_(torch.from_numpy(v))
        wire.fill_(0xAB)
        garbage(g)
        graph.replay()
        torch.cuda.synchronize()
        res = SimpleNamespace(wire=wire.cpu().numpy(), out=out.cpu().numpy(), src=[t.cpu().numpy() for t in src], err=None)
        check(G, res, vs)


@pytest.mark.parametrize("R", [1, 2, 3, 8, 16])
def test_decode_hand_built_payloads(R):
    """kept = 0, = cap and > cap (clamped), an index every payload shares, the last element of a chunk and the first of the next,
    rows at a 4-byte alignment."""
    n, cr = 8193, 64
    G = make_group([n], 0, eta=0.0, cr=cr)
    cap = G.codecs[0].cap
    rs = np.random.RandomState(R)
    pays = []
    for r in range(R):
        kind = r % 3
        if kind == 0:      # full, and a header that claims more than the section holds
            idx = np.sort(np.concatenate([[7, 4095, 4096, 8192], rs.permutation(np.arange(100, 4000))[:cap - 4]]))
            val = (rs.standard_normal(cap) * 3).astype(f32)
            pays.append(tc.hand_payload(n, cap, cap + 1000 if r % 2 else cap, idx, val))
        elif kind == 1:    # nothing
            pays.append(tc.hand_payload(n, cap, 0, [], []))
        else:
            idx = np.array([7, 4095, 4096, 8000])
            pays.append(tc.hand_payload(n, cap, 4, idx, np.array([-0.0, 1.5, -2.25, 1e-40], dtype=f32)))
    _decode_and_compare(G, pays, n, cap, R)


def _decode_and_compare(G, pays, n, cap, R):
    """The decode launch over hand-built payloads (rows at a 4-byte alignment, `out` a misaligned view between canaries) against
    the restatement."""
    row = pays[0].size
    buf = np.full(4 + R * (row + 4), 0xEE, dtype=np.uint8)
    for r, p in enumerate(pays):
        buf[4 + r * (row + 4):4 + r * (row + 4) + row] = p
    dev_buf = torch.from_numpy(buf).to(G.dev)
    gathered = torch.as_strided(dev_buf, (R, row), (row + 4, 1), 4)
    obig = torch.full((n + 8,), 7.0, dtype=torch.float32, device=G.dev)
    for plain in ([False, True] if R == 1 else [False]):
        G.g.decode_into(gathered, R, obig[3:3 + n], plain=plain)
        torch.cuda.synchronize()
        ob = obig.cpu().numpy()
        assert np.all(ob[:3] == 7.0) and np.all(ob[3 + n:] == 7.0)
        assert same(ob[3:3 + n], tc.decode_mean(pays, n, cap, R, plain=plain)), "R = %d, plain = %r" % (R, plain)


@pytest.mark.parametrize("R", [5, 8, 16])
def test_decode_indices_every_payload_carries(R):
    """EVERY one of the R payloads carries indices 7, 4095 (the last element of a chunk), 4096 (the first of the next) and 8192 (the
    last element), at a different slot in each and with values of mixed sign and magnitude: the R-term sum on one slot in payload
    order.  The restatement's sum must depend on that order, or the comparison would not see another one."""
    n, cr = 8193, 64
    G = make_group([n], 0, eta=0.0, cr=cr)
    cap = G.codecs[0].cap
    rs = np.random.RandomState(100 + R)
    shared = np.array([7, 4095, 4096, 8192])
    pays = []
    for r in range(R):
        kept = 4 + (r * 37) % (cap - 3)
        idx = np.sort(np.concatenate([shared, rs.permutation(np.arange(100, 4000))[:kept - 4]]))
        val = (rs.standard_normal(kept) * 10.0 ** rs.randint(-3, 4, size=kept)).astype(f32)
        pays.append(tc.hand_payload(n, cap, kept, idx, val))
    want = tc.decode_mean(pays, n, cap, R)
    assert not same(want[shared], tc.decode_mean(pays[::-1], n, cap, R)[shared]), "no shared slot on which the order of the payloads shows"
    _decode_and_compare(G, pays, n, cap, R)


def test_refusals_launch_nothing():
    from gq_amd import native
    G = make_group([4097, 8193], 3)
    dev, g = G.dev, G.g
    vs = inputs([4097, 8193], 1)
    src = [torch.from_numpy(v).to(dev) for v in vs]
    wire = torch.full((G.ub + 16,), 0xAB, dtype=torch.uint8, device=dev)
    assert g.encode(src, wire[:G.ub], 0, 0)
    torch.cuda.synchronize()
    wire.fill_(0xAB)
    out = torch.full((g.out_floats + 1,), 7.0, dtype=torch.float32, device=dev)
    b, L = g._batch, native.thr_lib()
    nan = ctypes.c_float(float("nan"))
    W = ctypes.c_void_p(wire.data_ptr())
    O = ctypes.c_void_p(out.data_ptr())

    def refused(rc):
        assert rc != 0 and L.gq_thr_last_error()

    def comp(wp=W, eta=0.0, ef=nan, op=O):
        return L.gq_thr_compress_batched(b.ref, wp, ctypes.c_float(eta), ef, op, None)

    def with_field(name, value, call):
        old = getattr(b.s, name)
        setattr(b.s, name, value)
        try:
            refused(call())
        finally:
            setattr(b.s, name, old)

    with_field("struct_bytes", 80, comp)
    with_field("nseg", 0, comp)
    with_field("nitems", 0, comp)
    with_field("seg_table", None, comp)
    with_field("item_seg", None, comp)
    with_field("sums", None, comp)
    with_field("stages", 9, comp)
    with_field("stages", -1, comp)
    with_field("min_k", 0, comp)
    with_field("min_cap", 0, comp)
    with_field("min_stride", 0, comp)
    refused(comp(wp=ctypes.c_void_p(wire.data_ptr() + 4)))
    refused(comp(wp=ctypes.c_void_p(0)))
    refused(comp(op=ctypes.c_void_p(out.data_ptr() + 2)))
    refused(comp(ef=ctypes.c_float(1.0), op=ctypes.c_void_p(0)))
    for eta in (-0.0, -1.0, float("inf"), float("nan")):
        with_field("stages", 0, lambda: comp(eta=eta))
    dec = lambda R, plain, gp=W, stride=G.ub: L.gq_thr_decode_sum_batched(b.ref, gp, ctypes.c_int64(stride), R, O, plain, None)
    refused(dec(2, 1))
    refused(dec(0, 0))
    refused(dec(2, 0, stride=G.ub + 2))
    refused(dec(1, 0, gp=ctypes.c_void_p(wire.data_ptr() + 2)))
    with_field("struct_bytes", 72, lambda: dec(1, 0))
    torch.cuda.synchronize()
    assert bool((wire == 0xAB).all()) and bool((out == 7.0).all()), "a refused call wrote something"
