"""libgq_rq.so's two launches held to include/gq_rq.h bit for bit, through native.RQBatch over hand-built tables and hand-built
stage-1 sections: every comparison is np.array_equal on bytes or uint32 views against tests/rq_contract.py (whose own checks, and
one assertion for every claim made here about an input, are tests/test_rq_contract.py).  One exception: where an input holds inf
or NaN, any NaN equals any NaN.  Every valid slot is compared; the padded slots of u_flat are unspecified and are not.

The wire starts as 0xA5 with garbage in the sections the encode writes, u_flat as garbage, `out` and the error buffers as 7.0, the
gradients sit in one buffer with 3.0 between them: after every launch every byte and float that belongs to nobody still holds
its fill, and the gradients are unchanged.

The multi-tile cases are sized from the device's CU count, so that every wave of the encode runs two tiles or more (the prefetch
across a tile's encode, the hand-over, flush_minmax() where the tensor changes inside a run, waves_with_one_more) and every
workgroup of the decode strides twice or more.  The CPU oracle's share of the six multi-tile encode cases, measured on eight
cores of the build machine with 256 CUs assumed (12,325 / 24,575 tiles at d = 8 with K = 64, 6,181 / 12,287 at d = 16 with K = 256,
4,133 / 8,191 at d = 32 with K = 64): 0.13 s and 0.27 s, 0.46 s and 0.95 s, 0.16 s and 0.33 s; building a case's inputs takes
0.5 to 3 s more."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import rq_contract as rc  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY, OUT_FILL, V_GUARD, V_GAP = 0xA5, 7.0, 3.0, 8
LEVEL_TORCH = {0: torch.float32, 1: torch.uint8, 2: torch.int16, 4: torch.int32}
GIVEN, DEVICE, COUNTER = "given", "device", "counter"


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _cus():
    from gq_amd import native
    return native.device_info(0)[0]


def _place(arrs, fill=V_GUARD):
    """Float arrays in ONE device buffer, V_GAP floats of `fill` round each (16-byte aligned starts) -> (buffer, pointers, offsets)"""
    offs, off = [], V_GAP
    for a in arrs:
        offs.append(off)
        off += (a.size + 3) // 4 * 4 + V_GAP
    host = np.full(off, fill, np.float32)
    for a, o in zip(arrs, offs):
        host[o:o + a.size] = a
    buf = _t(host)
    assert buf.data_ptr() % 16 == 0
    return buf, [buf.data_ptr() + 4 * o for o in offs], offs, host


def _batch(G, cb1, cb2, cdag, grad_ptrs=None, err_ptrs=None, lo=0, hi=None, **kw):
    from gq_amd import native
    t1, t2, tile_seg, nseg, ntiles = G.tables(grad_ptrs, err_ptrs, lo, hi)
    return native.RQBatch(_t(t1.reshape(-1)), _t(t2.reshape(-1)), _t(tile_seg), nseg, ntiles, cb1, cb2, cdag, torch.uint8,
                          LEVEL_TORCH[G.level_bytes], G.n_bit, **kw)


# ---- the encode ---------------------------------------------------------------------------------------------------------------------
def _encode_wire(G, T, seed=3):
    """One user's wire before the launch: 0xA5, stage 1's sections as built, garbage where stage 2's codes go."""
    wire = np.full(G.ub, CANARY, np.uint8)
    m = G.mask(stages=(1,), cols=(3,))
    wire[m] = np.random.RandomState(seed).randint(0, 256, size=int(m.sum())).astype(np.uint8)
    for s, t in enumerate(T):
        G.put(wire, s, 0, t["codes1"], t["raw1"], (t["lb"], t["ub"]))
    return wire


def run_encode(G, T, mode=GIVEN, seed=0, step=0):
    """One gq_rq_encode2_batched launch -> what it left (numpy) and what was there before."""
    from gq_amd import native
    from types import SimpleNamespace
    cb1, cdag, _ = rc.codebooks(G.d, G.K)
    cb1_t, cdag_t = _t(cb1), _t(cdag)
    wire0 = _encode_wire(G, T)
    vbuf, vptrs, _, v0 = _place([t["v"] for t in T])
    rs = np.random.RandomState(9)
    u0 = rs.randint(0, 2 ** 32, size=G.ntiles * 64, dtype=np.uint64).astype(np.uint32)      # garbage, NaN patterns among it
    r_flat = np.full(G.ntiles * 64, np.nan, np.float32)                                     # (padding slots are not read)
    for s, t in enumerate(T):
        r_flat[G.slots(s)] = t["r"]
    u_flat = _t(u0.view(np.int32)).view(torch.float32)
    minmax = torch.tensor([[-1, 0]] * G.nseg, dtype=torch.int32, device=_dev())             # { 0xFFFFFFFF, 0 }, as the header says
    level2 = torch.tensor([0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A5A5A5A5A], dtype=torch.int64, device=_dev())
    words = torch.tensor([seed, step], dtype=torch.int64, device=_dev())
    b = _batch(G, cb1_t, cb1_t, cdag_t, grad_ptrs=vptrs, u_flat2=u_flat, seg_minmax2=minmax, level2_words=level2)
    wire = _t(wire0)
    if mode == GIVEN:
        b.encode2(wire, native.RANDOM_GIVEN, 0, _t(r_flat))
    elif mode == DEVICE:
        b.encode2(wire, native.RANDOM_DEVICE, seed)
    else:
        b.encode2(wire, native.RANDOM_DEVICE_COUNTER, words.data_ptr())
    torch.cuda.synchronize()
    return SimpleNamespace(wire=wire.cpu().numpy(), wire0=wire0, u=u_flat.cpu().numpy(), u0=u0, minmax=minmax.cpu().numpy().view(np.uint32),
                           v=vbuf.cpu().numpy(), v0=v0, level2=[x & rc.M64 for x in level2.cpu().tolist()],
                           words=[x & rc.M64 for x in words.cpu().tolist()])


def check_encode(G, T, res, want=None):
    """Every tensor's codes, u and (min, max) pair against the contract; everything else as it was.  want: per tensor
    (codes, u, minmax) where the draws were not the case's own."""
    want = want or [(t["codes"], t["u"], t["minmax"]) for t in T]
    wire = res.wire0.copy()
    for s, (codes, _, _) in enumerate(want):
        o, n = G.section(s, 1, 3)
        wire[o:o + n] = codes
    bad = np.flatnonzero(res.wire != wire)
    assert bad.size == 0, "%d bytes of the wire differ, the first at %d (stage 2's codes, or a write outside them)" % (bad.size, bad[0])
    valid = np.concatenate([np.arange(G.slots(s).start, G.slots(s).stop) for s in range(G.nseg)])
    u_want = np.concatenate([u for _, u, _ in want])
    assert valid.size == sum(G.Ms) == u_want.size
    bad = np.flatnonzero(res.u.view(np.uint32)[valid] != rc.bits(u_want))
    assert bad.size == 0, "u differs in %d of %d subvectors, the first in slot %d" % (bad.size, valid.size, valid[bad[0]])
    mm = np.array([m for _, _, m in want], np.uint32)
    bad = np.flatnonzero((res.minmax != mm).any(axis=1))
    assert bad.size == 0, "seg_minmax differs for %d tensors, the first %d (M = %d)" % (bad.size, bad[0], G.Ms[bad[0]])
    assert np.array_equal(res.v.view(np.uint32), res.v0.view(np.uint32)), "the gradients changed"


@pytest.mark.parametrize("which", [0, 1], ids=["above_the_bound", "one_short_of_twice_the_bound"])
@pytest.mark.parametrize("d,K", [(8, 64), (16, 256), (32, 64)])
def test_encode_runs_that_cross_tensors(d, K, which):
    """Five large tensors with 300 small ones (1, 63, 64, 65, 127, 129, 200 subvectors in turn) between them, more tiles than
    twice the waves the launch can have resident: every wave's run holds two tiles or more, and runs cross tensors.  The second
    total is no multiple of the waves: some waves run one tile more than others."""
    cus = _cus()
    bound = 2 * cus * 4 * min(8, (160 * 1024) // rc.pw_lds_bytes(d))
    total = rc.multi_tile_totals(d, cus)[which]
    G, T = rc.encode_case(rc.multi_tile_Ms(d, cus, total), d, K, 1, 100 + d + which, zero_rows=False)
    assert G.ntiles == total > bound      # tiles_per_wave = ntiles / (4 * blocks) >= 2: blocks <= CUs * resident blocks per CU <= bound / 8
    assert which == 0 or (total + 1) % (4 * cus) == 0      # ... and ntiles % waves != 0: waves is a multiple of 4 * CUs
    check_encode(G, T, run_encode(G, T))


@pytest.mark.parametrize("level_bytes", [0, 1, 2, 4])
def test_encode_on_stage1_as_it_can_arrive(level_bytes):
    """Level 0 and the top level, lb == ub, lb == ub == 0 (every norm 0), f32 norms and 1-, 2- and 4-byte levels, subvectors whose
    residual is exactly zero (code K - 1, u = +0), tensors of 1, 63, 64 and 65 subvectors, draws 0, 1 and 1.5."""
    G, T = rc.encode_case([1, 63, 64, 65, 700, 7, 129, 64, 300], 16, 256, level_bytes, 21 + level_bytes, kinds=("ordinary", "equal", "zero"))
    res = run_encode(G, T)
    check_encode(G, T, res)
    for s, t in enumerate(T):
        o, _ = G.section(s, 1, 3)
        assert (res.wire[o:o + t["M"]][t["zero"]] == 255).all() and not res.u.view(np.uint32)[G.slots(s)][t["zero"]].any()


@pytest.mark.parametrize("K,d", rc.SERVED)
def test_encode_at_every_served_shape(K, d):
    """One to eight row blocks of 32 codewords (the first K codewords and their own pseudo-inverse) at every d."""
    from gq_amd import native
    assert native.rq_batched_serves(d, K, torch.uint8)
    G, T = rc.encode_case(rc.SERVED_MS, d, K, 1, K + d)
    check_encode(G, T, run_encode(G, T))


def _walk_groups():
    """(runs in a child process with $GQ_PVQ_EPS set: the library reads it once)"""
    for d, K, Ms in rc.WALK_GROUPS:
        G, T = rc.encode_case(Ms, d, K, 1, 5 + d)
        check_encode(G, T, run_encode(G, T))
    print("ok")


@pytest.mark.parametrize("eps", ["1e-3", "-1e-3"], ids=["wave_walk", "term_by_term"])
def test_walks_behind_the_fast_path(eps):
    """$GQ_PVQ_EPS widened: most lanes leave the lane-local walk for the wave walk (negative: the term-by-term walk), through
    this kernel's staging; three groups against the contract."""
    env = dict(os.environ, GQ_PVQ_EPS=eps)
    root = os.path.dirname(HERE)
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_rq_contract as t; t._walk_groups()"
            % (HERE, root, os.path.join(root, "gradient-quantization_amd")))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("mode", [DEVICE, COUNTER])
def test_encode_draw_streams(mode):
    """The sampler's uniforms recomputed on the host -- uniform01(seed ^ RQ_CODE_SALT, slot), the seed resolved from the
    { seed, step } words in counter mode -- reproduce the codes through the contract; a counter-mode launch leaves
    { resolved seed ^ RQ_LEVEL2_SALT, 0 } in level2_words and the { seed, step } words as they were."""
    from test_gpu_pvq import _uniform01_host
    d, K, seed, step = 16, 256, 0x1234ABCD5678EF01, 5
    G, T = rc.encode_case([65, 1, 900, 64, 130], d, K, 1, 77)
    res = run_encode(G, T, mode=mode, seed=seed, step=step)
    eff = rc.resolve_seed(seed, step) if mode == COUNTER else seed
    cb1, cdag, _ = rc.codebooks(d, K)
    want = []
    for s, t in enumerate(T):
        r = _uniform01_host(eff ^ rc.RQ_CODE_SALT, list(range(G.slots(s).start, G.slots(s).stop)))
        want.append(rc.encode2(t["v"], t["codes1"], t["norm1"], cb1, cdag, r))
    check_encode(G, T, res, want)
    assert sum(int((w[0] != t["codes"]).sum()) for w, t in zip(want, T)) > sum(G.Ms) // 2      # (not the case's own draws)
    if mode == COUNTER:
        assert res.level2 == [eff ^ rc.RQ_LEVEL2_SALT, 0] and res.words == [seed, step]
    else:
        assert res.level2 == [0x5A5A5A5A5A5A5A5A] * 2


# ---- the decode ---------------------------------------------------------------------------------------------------------------------
def run_decode(G, rows, R, cb1, cb2, mode, vs=None, no_err=()):
    """One gq_rq_decode_sum_batched launch over the first R rows -> `out` (numpy), or in ERROR mode the error buffers' buffer."""
    from gq_amd import native
    from types import SimpleNamespace
    cb1_t = _t(cb1)
    cb2_t = cb1_t if cb2 is cb1 else _t(cb2)
    gathered = _t(rows)
    out = torch.full((G.out_floats,), OUT_FILL, dtype=torch.float32, device=_dev())
    res = SimpleNamespace()
    vptrs = eptrs = None
    if mode == rc.ERROR:
        vbuf, vptrs, res.voffs, res.v0 = _place(vs)
        ebuf, eptrs, res.eoffs, res.e0 = _place([np.full(v.size, OUT_FILL, np.float32) for v in vs], fill=OUT_FILL)
        eptrs = [0 if s in no_err else p for s, p in enumerate(eptrs)]
    b = _batch(G, cb1_t, cb2_t, _t(rc.codebooks(G.d, G.K)[1]), grad_ptrs=vptrs, err_ptrs=eptrs)
    b.decode(gathered[:R, :G.ub], R, None if mode == rc.ERROR else out, mode=mode)
    torch.cuda.synchronize()
    res.out = out.cpu().numpy()
    if mode == rc.ERROR:
        res.v, res.err = vbuf.cpu().numpy(), ebuf.cpu().numpy()
    assert np.array_equal(gathered.cpu().numpy(), rows), "the payloads changed"
    return res


def check_out(G, res, want, lo=0, hi=None, eq=np.array_equal):
    """Tensors lo .. hi - 1 of `out` against the contract; every other float of `out` still holds its fill."""
    hi = G.nseg if hi is None else hi
    exp = np.full(G.out_floats, OUT_FILL, np.float32)
    for s in range(lo, hi):
        exp[G.out_off[s]:G.out_off[s] + G.Ms[s] * G.d] = want[s]
    if eq is np.array_equal:
        bad = np.flatnonzero(res.out.view(np.uint32) != exp.view(np.uint32))
        assert bad.size == 0, "%d floats of out differ, the first at %d" % (bad.size, bad[0])
    else:
        assert eq(res.out, exp)


@pytest.mark.parametrize("d,K,two", [(8, 64, False), (16, 256, False), (32, 64, True)])
def test_decode_past_one_pass_of_the_grid(d, K, two):
    """More padded slots than one pass of the grid covers, R = 3, over a ragged list: every workgroup strides twice or more, and
    the tile -> tensor lookup changes inside its stride."""
    cus = _cus()
    G, P, cb1, cb2 = rc.decode_case(rc.decode_multi_pass_Ms(d, cus), d, K, 1, 3, 300 + d, two_images=two)
    assert G.ntiles * 64 > cus * 8 * (256 // (d // 4))      # blocks are capped at CUs * 8, a block covers 256 / (d / 4) slots a pass
    res = run_decode(G, rc.gathered_rows(G, P, 3), 3, cb1, cb2, rc.MEAN)
    check_out(G, res, rc.decode_want(G, P, cb1, cb2, rc.MEAN))


DECODE_CONFIGS = [(16, 256, 1, False), (16, 256, 0, True), (32, 256, 2, True), (8, 64, 4, False), (32, 256, 0, False), (8, 96, 2, True)]


@pytest.mark.parametrize("R", rc.DECODE_RS)
@pytest.mark.parametrize("d,K,level_bytes,two", DECODE_CONFIGS, ids=["d%d_K%d_lb%d_%s" % (c[0], c[1], c[2], "two_images" if c[3] else "one_image") for c in DECODE_CONFIGS])
def test_decode_mean_of_hand_built_payloads(d, K, level_bytes, two, R):
    """R payloads 48 bytes further apart than a payload is long, garbage between the sections; one codebook image and two
    (d = 32, K = 256: 73,728 bytes of LDS); f32 norms and 1-, 2- and 4-byte levels; R = 1 in MEAN and in PLAIN mode."""
    G, P, cb1, cb2 = rc.decode_case(rc.RAGGED, d, K, level_bytes, R, 10 * R + d, two_images=two)
    assert (cb1 is cb2) != two
    rows = rc.gathered_rows(G, P, R, extra=48)
    check_out(G, run_decode(G, rows, R, cb1, cb2, rc.MEAN), rc.decode_want(G, P, cb1, cb2, rc.MEAN))
    if R == 1:
        check_out(G, run_decode(G, rows, 1, cb1, cb2, rc.PLAIN), rc.decode_want(G, P, cb1, cb2, rc.PLAIN))


@pytest.mark.parametrize("R", [3, 5, rc.GQ_ODD_DIV_MAX, rc.GQ_ODD_DIV_MAX + 2])
def test_decode_at_the_ends_of_the_float_range(R):
    """f32 norms that make the sums subnormal, finite near FLT_MAX and infinite, and +-inf / NaN in one payload; odd R on both
    sides of GQ_ODD_DIV_MAX: the four-operation quotient against the true division (any NaN equals any NaN)."""
    G, P, cb1, cb2 = rc.decode_case([5, 64, 131], 16, 256, 0, R, 7 + R, special="range")
    res = run_decode(G, rc.gathered_rows(G, P, R), R, cb1, cb2, rc.MEAN)
    check_out(G, res, rc.decode_want(G, P, cb1, cb2, rc.MEAN), eq=rc.same)


@pytest.mark.parametrize("level_bytes", [0, 1, 2, 4])
def test_decode_signed_zeros(level_bytes):
    """Tensor 1: both stages decode to -0; tensor 2: the two stages cancel exactly.  +0 in MEAN (R = 3 and 1) and PLAIN mode, and
    error = v - (+0) = v, a -0 of v kept."""
    G, P, cb1, cb2 = rc.decode_case(rc.RAGGED, 16, 256, level_bytes, 3, 5, special="zeros")
    rows = rc.gathered_rows(G, P, 3)
    for R, mode in ((3, rc.MEAN), (1, rc.MEAN), (1, rc.PLAIN)):
        res = run_decode(G, rows, R, cb1, cb2, mode)
        check_out(G, res, rc.decode_want(G, [p[:R] for p in P], cb1, cb2, mode))
        for s in (1, 2):
            assert not res.out.view(np.uint32)[G.out_off[s]:G.out_off[s] + G.Ms[s] * 16].any()
    vs = [rc.f32(np.where(np.arange(M * 16) % 5 == 0, -0.0, np.arange(M * 16) - 40.0)) for M in G.Ms]
    res = run_decode(G, rows, 1, cb1, cb2, rc.ERROR, vs=vs)
    for s in (1, 2):
        o = res.eoffs[s]
        assert np.array_equal(res.err[o:o + vs[s].size].view(np.uint32), rc.bits(vs[s]))


@pytest.mark.parametrize("d,K,level_bytes,two", [(16, 256, 1, False), (32, 256, 0, True), (8, 64, 2, True)])
def test_decode_error_mode(d, K, level_bytes, two):
    """GQ_RQ_ERROR called directly with out == NULL: error = v - x into column 7's buffers; every third row has a null error
    pointer and the buffer it would have had keeps its fill; v is read from column 0 and left unchanged."""
    G, P, cb1, cb2 = rc.decode_case(rc.RAGGED, d, K, level_bytes, 1, 60 + d, two_images=two)
    rs = np.random.RandomState(d)
    vs = [rc.f32(rs.randn(M * d) * 1e-2) for M in G.Ms]
    no_err = set(range(0, G.nseg, 3))
    res = run_decode(G, rc.gathered_rows(G, P, 1), 1, cb1, cb2, rc.ERROR, vs=vs, no_err=no_err)
    want = rc.decode_want(G, P, cb1, cb2, rc.ERROR, vs=vs)
    exp = res.e0.copy()
    for s in range(G.nseg):
        if s not in no_err:
            exp[res.eoffs[s]:res.eoffs[s] + vs[s].size] = want[s]
    assert np.array_equal(res.err.view(np.uint32), exp.view(np.uint32)), "the error buffers, or a write outside them"
    assert np.array_equal(res.v.view(np.uint32), res.v0.view(np.uint32)), "v changed"
    assert (res.out == OUT_FILL).all()


@pytest.mark.parametrize("lo,hi", [(2, 6), (1, 3), (5, 7)])
def test_decode_of_a_part_equals_the_slices_of_the_full_decode(lo, hi):
    """RQBatch.part() semantics: tables of tensors lo .. hi - 1 with their first tiles rebased and tile_seg renumbered decode to
    the matching slices of the full decode (which the contract gives), and nothing else of `out` is written."""
    G, P, cb1, cb2 = rc.decode_case(rc.RAGGED, 16, 256, 1, 3, 91)
    assert 0 < lo < hi < G.nseg
    from gq_amd import native
    rows = rc.gathered_rows(G, P, 3)
    want = rc.decode_want(G, P, cb1, cb2, rc.MEAN)
    full = run_decode(G, rows, 3, cb1, cb2, rc.MEAN)
    check_out(G, full, want)
    cb_t = _t(cb1)
    whole = _batch(G, cb_t, cb_t, _t(rc.codebooks(16, 256)[1]))
    t1, t2, tile_seg, nseg, ntiles = G.tables(lo=lo, hi=hi)
    part = whole.part(_t(t1.reshape(-1)), _t(t2.reshape(-1)), _t(tile_seg), nseg, ntiles)
    assert isinstance(part, native.RQBatch) and part.b1.s.nseg == hi - lo and part.b1.s.ntiles == ntiles
    out = torch.full((G.out_floats,), OUT_FILL, dtype=torch.float32, device=_dev())
    part.decode(_t(rows)[:, :G.ub], 3, out)
    torch.cuda.synchronize()
    from types import SimpleNamespace
    check_out(G, SimpleNamespace(out=out.cpu().numpy()), want, lo, hi)
    a, b = G.out_off[lo], G.out_off[hi - 1] + G.Ms[hi - 1] * 16
    assert np.array_equal(out.cpu().numpy()[a:b].view(np.uint32), full.out[a:b].view(np.uint32))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _refusal_rig(K=256, n_bit2=None, cdag_shift=0):
    from types import SimpleNamespace
    d = 16
    Ms = [65, 7]
    G = rc.Group(Ms, d, K, 1, 6)
    full = rc.codebooks(d, 256)[0]
    cb = _t(full[:K])
    buf = torch.zeros(K * d + 4, dtype=torch.float32, device=_dev())
    cdag = buf[cdag_shift:cdag_shift + K * d].view(K, d)
    rs = np.random.RandomState(K)
    rows = rs.randint(0, 32, size=(2, G.ub)).astype(np.uint8)      # (codes below every K used here)
    vbuf, vptrs, _, v0 = _place([rc.f32(rs.randn(M * d)) for M in Ms])
    S = SimpleNamespace(G=G, rows0=rows, rows=_t(rows), v0=v0, vbuf=vbuf)
    S.u = torch.full((G.ntiles * 64,), OUT_FILL, dtype=torch.float32, device=_dev())
    S.minmax = torch.tensor([[-1, 0]] * G.nseg, dtype=torch.int32, device=_dev())
    S.out = torch.full((G.out_floats,), OUT_FILL, dtype=torch.float32, device=_dev())
    S.r = torch.rand(G.ntiles * 64, device=_dev())
    S.b = _batch(G, cb, cb, cdag, grad_ptrs=vptrs, u_flat2=S.u, seg_minmax2=S.minmax)
    if n_bit2 is not None:
        S.b.b2.s.n_bit = n_bit2
    return S


def _nothing_written(S):
    torch.cuda.synchronize()
    assert np.array_equal(S.rows.cpu().numpy(), S.rows0) and bool((S.u == OUT_FILL).all()) and bool((S.out == OUT_FILL).all())
    assert S.minmax.cpu().tolist() == [[-1, 0]] * S.G.nseg and np.array_equal(S.vbuf.cpu().numpy(), S.v0)


@pytest.mark.parametrize("what", ["plain_R2", "error_R2", "K48", "n_bit_disagrees", "c_dagger_unaligned"])
def test_refusals_return_an_error_and_write_nothing(what):
    from gq_amd import native
    S = _refusal_rig(K=48 if what == "K48" else 256, n_bit2=5 if what == "n_bit_disagrees" else None,
                     cdag_shift=1 if what == "c_dagger_unaligned" else 0)
    calls = []
    if what in ("plain_R2", "error_R2"):
        mode = native.RQ_PLAIN if what == "plain_R2" else native.RQ_ERROR
        calls.append(lambda: S.b.decode(S.rows, 2, S.out, mode=mode))
    elif what == "c_dagger_unaligned":
        assert S.b.keep[0].data_ptr() % 16 == 4
        calls.append(lambda: S.b.encode2(S.rows[0], native.RANDOM_GIVEN, 0, S.r))
    else:
        calls.append(lambda: S.b.encode2(S.rows[0], native.RANDOM_GIVEN, 0, S.r))
        calls.append(lambda: S.b.decode(S.rows, 2, S.out))
        calls.append(lambda: S.b.decode(S.rows[:1], 1, S.out, mode=native.RQ_PLAIN))
    for call in calls:
        with pytest.raises(native.GQNativeError):
            call()
        _nothing_written(S)
    if what in ("plain_R2", "error_R2", "c_dagger_unaligned"):      # the same rig is served when asked properly
        S.b.decode(S.rows, 2, S.out)
        torch.cuda.synchronize()
        assert not bool((S.out[S.G.out_off[0]:S.G.out_off[0] + 65 * 16] == OUT_FILL).all())
