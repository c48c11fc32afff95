"""The ProbabilisticVectorCompressor's sampler restated in numpy -- float32 and float64 operations one at a time, from the CPU
oracle's projections -- and the inputs of tests/test_gpu_zz_pvq_contract.py: draws that put the sampler's threshold ON a running
sum of its inverse-CDF walk and a ladder of f32 ulps to both sides of it.  TEST INFRASTRUCTURE ONLY; nothing here comes from a GPU.
tests/test_pvq_contract.py checks without a GPU what is claimed here: that walk() and the oracle agree, that every requested
on-threshold draw was built, and that the mutations a kernel could carry change codes on these inputs.

The rule (csrc/pvq.hip's header; probabilistic_vector_compressor.py:47-61):
    p = c_dagger . v (fmaf chain);  l1 = sum_k |p_k| (sequential f32);  cum_k = f32(sum_{i<=k} f64(|p_i| / l1));
    code = first k with cum_k >= f32(r - 1e-5f), else K - 1;  u = sign(p_code) * l1.
A uniform draw lies within the one-sweep kernel's window (EPS) of a running sum about once in 2^13 subvectors, and never ON one:
here every finite row of a table that has a request is given a draw whose threshold is exactly j ulps from cum_k, j from LADDER,
k from targets() -- the first and last codewords, the half (7 | 8) and run (15 | 16 | 17) boundaries of the one-sweep kernel's
bracket, the matrix instruction's row block (31 | 32)."""
import functools
from types import SimpleNamespace

import numpy as np

import hsq_encode_contract as ec
import oracle
import rq_contract as rc

F = np.float32
C5 = F(1e-5)
EPS = 1.0625 * 2.0 ** -22                 # pw_eps_from_env's default (csrc/pvq_walk.hpp)
LADDER = (0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6, 8, -8, 16, -16, 64, -64)
ONE_SWEEP = [(d, K) for d in (8, 16, 32) for K in (32, 96, 256)]       # pvq_encode_walk_kernel: walk_serves() of csrc/pvq.hip
TWO_SWEEP = [(12, 100), (10, 33), (4, 16), (16, 250), (48, 512)]       # pvq_encode_lds_kernel; K = 512 has int32 codes
CAPPED = [(8, 32), (16, 256), (32, 96)]   # the grid-capped tables
VALU_D = (4, 8, 12, 16, 24, 32, 64)       # dispatch_pvq's list of pvq_encode_kernel instantiations
M_TABLE = 64 * 5 + 17                     # six tiles, the last one ragged
M_CAPPED = 64 * 40 + 17                   # with $GQ_CU_COUNT=1 a wave walks several tiles and prefetches tile t + nw
MULTI_MS = (1, 63, 64, 65, 337)
EF_SCALE = 0.3
MIDPOINTS = 8
FLT_MAX = float(np.finfo(np.float32).max)
PATTERN = ("gauss", "gauss", "tiny28", "gauss", "spike", "gauss", "tiny12", "gauss", "big9", "gauss", "below", "gauss", "gauss",
           "spike", "gauss", "gauss")
SPECIAL = ("zero", "overflow", "subnormal", "nan", "inf", "infpair")


def step(a, j):
    """The f32 j ulps from the positive finite f32 a (None when that leaves the positive floats)."""
    b = int(F(a).view(np.uint32)) + int(j)
    if not 0 < b < 0x7F800000:
        return None
    return np.uint32(b).view(np.float32)


# ---- the rule, restated -------------------------------------------------------------------------------------------------------------
def terms(p):
    """(l1, q) of the projections p [M, K]: l1 by sequential f32 adds of |p_k|, k ascending; q_k = |p_k| / l1, an f32 division."""
    a = np.abs(rc.f32(p))
    with np.errstate(all="ignore"):
        l1 = np.zeros(a.shape[0], np.float32)
        for k in range(a.shape[1]):
            l1 = l1 + a[:, k]
        q = a / l1[:, None]
    assert l1.dtype == np.float32 and q.dtype == np.float32
    return l1, q


def running(q, dtype=np.float64):
    """The sequential running sum of the terms in `dtype`, k ascending -> [M, K] of dtype."""
    out = np.empty(q.shape, dtype)
    acc = np.zeros(q.shape[0], dtype)
    with np.errstate(all="ignore"):
        for k in range(q.shape[1]):
            acc = acc + q[:, k].astype(dtype)
            out[:, k] = acc
    return out


def threshold(r):
    with np.errstate(all="ignore"):
        return rc.f32(r) - C5


def first_at_or_above(cum, thr, strict=False):
    """The first k with cum_k >= thr (strict: >), else K - 1; a NaN never compares."""
    with np.errstate(all="ignore"):
        hit = cum > thr[:, None] if strict else cum >= thr[:, None]
    return np.where(hit.any(axis=1), hit.argmax(axis=1), cum.shape[1] - 1).astype(np.int32)


def projection(p, codes, l1):
    """u = sign(p_code) * l1, sign(+-0) = 0, a NaN gives NaN."""
    with np.errstate(all="ignore"):
        return np.sign(rc.f32(p)[np.arange(len(codes)), codes]) * l1


def walk(p, r):
    """-> (codes int32[M], u f32[M], cum f32[M, K], l1 f32[M]) of the oracle's projections p and the draws r."""
    l1, q = terms(p)
    with np.errstate(all="ignore"):
        cum = running(q).astype(np.float32)
    codes = first_at_or_above(cum, threshold(r))
    return codes, projection(p, codes, l1), cum, l1


# ---- what a kernel could do instead: NOT the contract ---------------------------------------------------------------------------------
def _in_run(cum, thr, start, length):
    """start + the terms of the run [start, start + length) whose running sum stayed below thr: the walk confined to a run."""
    idx = start[:, None] + np.arange(length)[None, :]
    K = cum.shape[1]
    with np.errstate(all="ignore"):
        below = np.take_along_axis(cum, np.minimum(idx, K - 1), axis=1) < thr[:, None]
    return np.minimum(start + (below & (idx < K)).sum(axis=1), K - 1).astype(np.int32)


def mutant(p, r, how):
    """The codes of a sampler that is wrong in one way."""
    l1, q = terms(p)
    thr = threshold(r)
    K = q.shape[1]
    with np.errstate(all="ignore"):
        cum64 = running(q)
        cum = cum64.astype(np.float32)
        if how == "f32_sum":            # the running sum kept in f32
            return first_at_or_above(running(q, np.float32), thr)
        if how == "sum_then_divide":    # (sum_k |p_k|) / l1 in place of the sum of the quotients
            s = running(np.abs(rc.f32(p))) / l1[:, None].astype(np.float64)
            return first_at_or_above(s.astype(np.float32), thr)
        if how == "strict":             # > in place of >=
            return first_at_or_above(cum, thr, strict=True)
        if how == "double_threshold":   # r - 1e-5 formed in double
            return first_at_or_above(cum.astype(np.float64), rc.f32(r).astype(np.float64) - np.float64(C5))
        if how == "unrounded_sum":      # the double running sum compared without its rounding to f32
            return first_at_or_above(cum64, thr.astype(np.float64))
        if how == "clamp":              # the count clamped at K - 2
            return np.minimum(first_at_or_above(cum, thr), K - 2).astype(np.int32)
        nruns = (K + 15) // 16
        ends = cum[:, np.minimum(16 * np.arange(nruns) + 15, K - 1)]
        if how == "bracket":            # a run of 16 whose end boundary EQUALS the threshold is taken to lie below it
            run = np.minimum((ends <= thr[:, None]).sum(axis=1), nruns - 1)
            return _in_run(cum, thr, 16 * run, 16)
        if how == "half":               # ... and so is the half boundary inside the right run
            run = np.minimum((ends < thr[:, None]).sum(axis=1), nruns - 1)
            mid = np.take_along_axis(cum, np.minimum(16 * run + 7, K - 1)[:, None], axis=1)[:, 0]
            return _in_run(cum, thr, 16 * run + np.where(mid <= thr, 8, 0), 8)
    raise ValueError(how)


MUTATIONS = ("f32_sum", "sum_then_divide", "strict", "double_threshold", "unrounded_sum", "clamp", "bracket", "half")


def rounds_up_to_threshold(thr):
    """rounds_up_to_threshold of csrc/pvq_walk.hpp for finite thr: the double T with (float)x >= thr <=> x >= T."""
    thr = rc.f32(thr)
    mid = 0.5 * (thr.astype(np.float64) + np.nextafter(thr, F(-np.inf)).astype(np.float64))
    odd = (thr.view(np.uint32) & 1) != 0
    return np.where(odd, np.nextafter(mid, np.inf), mid)


def inside_window(tab, eps=EPS):
    """Per on-threshold entry (the midpoint entries behind the ladder's): does a running sum of the row (the exact double one) lie within eps of T?  The one-sweep kernel
    compares its own running sums, which are these up to the error eps is the bound of, with T - eps and T + eps: an entry
    inside leaves the lane-local walk for a slow walk, an entry outside is settled by it."""
    rows = np.array([e[0] for e in tab.entries + tab.extra])
    _, q = terms(tab.p[rows])
    T = rounds_up_to_threshold(threshold(tab.r[rows]))
    return (np.abs(running(q) - T[:, None]) < eps).any(axis=1)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def cdag_of(d, K):
    """A seeded c_dagger [K, d] (as tests/test_gpu_kernels.py draws one) with two rows that are all but axis-aligned (the
    other elements scaled by 1e-12, not zero: 0 * inf would be a NaN): a subvector whose elements 1 and 2 are tiny has terms far
    below 2^-29 of its l1 there."""
    c = rc.f32(np.random.RandomState(1000 * d + K).standard_normal((K, d)) * 0.3)
    for k, axis in below_rows(K):
        c[k] *= F(1e-12)
        c[k, axis] = 0.3
    return c


def below_rows(K):
    return ((5, 1), (K // 2 + 3, 2))


def targets(K, rs):
    """The codewords a threshold is put on: see the module's docstring; K - 1 is left out because cum_{K-1} = 1 up to a few
    ulps and r < 1 (code K - 1 is reached from K - 2 with j > 0).  Three random ones besides."""
    ks = sorted(set(k for k in (0, 7, 8, 15, 16, 17, 31, 32, K - 2) if 0 <= k <= K - 2))
    rest = [k for k in range(1, K - 2) if k not in ks]
    return ks + sorted(int(k) for k in rs.choice(rest, size=min(3, len(rest)), replace=False))


def rows_of(M, d, cdag, seed, special=True):
    """(x f32[M, d], kinds) -- Gaussian rows at scale 0.05, rows scaled by 1e-28, 1e-12 and 1e9, single-spike rows, rows with
    terms below 2^-29 of l1 (PATTERN in turn), and with `special` one each of SPECIAL, in different tiles and lanes."""
    rs = np.random.RandomState(seed)
    x = rc.f32(rs.standard_normal((M, d)) * 0.05)
    kinds = np.array([PATTERN[i % len(PATTERN)] for i in range(M)], dtype=object)
    if special:
        assert M >= M_TABLE
        for i, name in zip((5, 73, 161, 255, 256, M - 1), SPECIAL):
            kinds[i] = name
    c64 = cdag.astype(np.float64)
    with np.errstate(all="ignore"):
        for i, kind in enumerate(kinds):
            if kind == "tiny28":
                x[i] *= F(1e-28)
            elif kind == "tiny12":
                x[i] *= F(1e-12)
            elif kind == "big9":
                x[i] *= F(1e9)
            elif kind == "spike":
                x[i, 1:] *= F(1e-35)
            elif kind == "below":
                x[i, 1:3] *= F(1e-12)
            elif kind == "zero":
                x[i] = 0.0
            elif kind == "overflow":      # finite elements and finite projections whose sum passes FLT_MAX
                x[i] = (x[i].astype(np.float64) * (1.2 * FLT_MAX / np.abs(c64 @ x[i].astype(np.float64)).sum())).astype(np.float32)
            elif kind == "subnormal":     # l1 itself below 2^-126
                x[i] = (x[i].astype(np.float64) * (3e-39 / np.abs(c64 @ x[i].astype(np.float64)).sum())).astype(np.float32)
            elif kind == "nan":
                x[i, 3] = np.nan
            elif kind == "inf":
                x[i, 2] = np.inf
            elif kind == "infpair":
                x[i, 1], x[i, 3] = np.inf, -np.inf
    return x, kinds


def _oracle(x, cdag, r):
    M = x.shape[0]
    codes, u, l1, p, cum = oracle.pvq_encode(x.reshape(-1), cdag, r, sub_rows=M)
    return codes, u, rc.f32(l1).reshape(M), rc.f32(p).reshape(M, -1), rc.f32(cum).reshape(M, -1)


def on_threshold(x, cdag, k, j, cum=None):
    """The draw r in [0, 1) of the subvector x with f32(r - 1e-5f) exactly j f32 ulps from cum_k, searched among the f32
    neighbours of cum_k + 1e-5 -- or None: cum is not strictly increasing from k - 1 to k + 1, the target is no positive float,
    or no float in [0, 1) rounds there (cum_k + 1e-5 lies in the binade above the target's, where every other one is missed)."""
    if cum is None:
        cum = _oracle(rc.f32(x).reshape(1, -1), cdag, np.zeros(1, np.float32))[4][0]
    K = cum.size
    lo = F(0.0) if k == 0 else cum[k - 1]
    if not (k + 1 < K and lo < cum[k] < cum[k + 1]):
        return None
    t = step(cum[k], j)
    if t is None:
        return None
    r0 = F(np.float64(t) + np.float64(C5))
    for delta in (0, 1, -1, 2, -2, 3, -3, 4, -4):
        r = step(r0, delta)
        if r is not None and r < F(1.0) and F(r - C5) == t:
            return r
    return None


def place_draws(x, cdag, kinds, seed, fraction=1.0):
    """Draws for the rows x: every request (k of targets(), j of LADDER), repeated until `fraction` of the finite rows are
    taken, goes to the next unused finite row on which on_threshold() succeeds; ordinary uniform draws (0, 1e-5 and 1 - 2^-24
    among them) everywhere else, the special rows included -> (r, entries [(row, k, j)], number of requests, midpoint entries)."""
    M, K = x.shape[0], cdag.shape[0]
    rs = np.random.RandomState(seed)
    r = rs.random_sample(M).astype(np.float32)
    _, _, _, p, cum = _oracle(x, cdag, r)
    free = [int(i) for i in rs.permutation(M) if kinds[i] not in SPECIAL]
    once = [(k, j) for k in targets(K, rs) for j in LADDER]
    budget = int(fraction * len(free))
    reqs = (once * (budget // len(once) + 1))[:budget] if fraction < 1.0 else once
    assert len(once) <= len(reqs) <= len(free)
    entries = []
    for k, j in reqs:
        for n, i in enumerate(free):
            got = on_threshold(x[i], cdag, k, j, cum[i])
            if got is not None:
                r[i] = got
                entries.append((i, k, j))
                del free[n]
                break
    # ... and up to MIDPOINTS rows where (sum_i |p_i|) / l1 and the sum of the quotients round to DIFFERENT floats at some k (the
    # double sum lies next to a rounding midpoint there): the threshold goes on the larger of the two, which is cum_k or one ulp above
    l1, q = terms(p)
    with np.errstate(all="ignore"):
        s = (running(np.abs(p)) / l1[:, None].astype(np.float64)).astype(np.float32)
    extra = []
    for i in list(free):
        for k in np.flatnonzero((s[i] != cum[i]) & np.isfinite(s[i]) & np.isfinite(cum[i])):
            got = on_threshold(x[i], cdag, int(k), 0 if cum[i, k] > s[i, k] else 1, cum[i])
            if got is not None and abs(int(s[i, k].view(np.uint32)) - int(cum[i, k].view(np.uint32))) == 1:
                r[i] = got
                extra.append((i, int(k), 0 if cum[i, k] > s[i, k] else 1))
                free.remove(i)
                break
        if len(extra) == MIDPOINTS:
            break
    for i, edge in zip(free[:3], (F(0.0), C5, F(1.0) - F(2.0 ** -24))):
        r[i] = edge
    return r, entries, len(reqs), extra


def _finish(d, K, x, kinds, cdag, r, entries, requested, extra):
    codes, u, l1, p, cum = _oracle(x, cdag, r)
    return SimpleNamespace(d=d, K=K, M=x.shape[0], x=x, kinds=kinds, cdag=cdag, r=r, entries=entries, requested=requested, extra=extra,
                           codes=codes, u=u, l1=l1, p=p, cum=cum, code_np=np.uint8 if K <= 256 else np.int32)


@functools.lru_cache(maxsize=None)
def table(d, K, M=M_TABLE):
    """One flat input: rows_of() with their draws and what the oracle says of them.  The capped size spends two thirds of its
    rows on requests, the small one each request once.  Built once per process; nobody writes to it."""
    cdag = cdag_of(d, K)
    x, kinds = rows_of(M, d, cdag, 7 * d + K + M)
    r, entries, requested, extra = place_draws(x, cdag, kinds, d + K + M, fraction=1.0 if M == M_TABLE else 2.0 / 3.0)
    return _finish(d, K, x, kinds, cdag, r, entries, requested, extra)


def table_id(dk):
    return "d%d-K%d" % dk


def lb_ub(u):
    """(lb, ub) as gq_hsq_levels folds them from the encode's workspace: fminf / fmaxf drop a NaN projection."""
    return np.fmin.reduce(rc.f32(u)), np.fmax.reduce(rc.f32(u))


def fold_minmax(u):
    """rq_contract.fold_minmax over the projections that are no NaN (the multi-tensor launches' fminf / fmaxf fold)."""
    u = rc.f32(u)
    return rc.fold_minmax(u[~np.isnan(u)])


# ---- the multi-tensor cases ---------------------------------------------------------------------------------------------------------
MULTI_CASES = [(d, K, ef) for d, K in CAPPED for ef in (None, EF_SCALE)]


def multi_id(c):
    return "d%d-K%d-%s" % (c[0], c[1], "plain" if c[2] is None else "ef%g" % c[2])


@functools.lru_cache(maxsize=None)
def multi_case(d, K, ef):
    """gq_pvq_encode_batched over tensors of MULTI_MS subvectors behind one another in hsq_encode_contract.Layout's buffers
    (the special rows in the last one).  ef: with an error buffer for every tensor but each third one, v = g + RN(ef * e) one
    operation at a time; the draws are built on v.  -> what the launch is given and what it must leave."""
    lay = ec.Layout(MULTI_MS, d, 1, 1)
    cdag = cdag_of(d, K)
    rs = np.random.RandomState(31 * d + K)
    g, e, v, kinds = [], [], [], []
    for s, M in enumerate(MULTI_MS):
        x, kd = rows_of(M, d, cdag, 500 + 11 * s + d + K, special=M >= M_TABLE)
        err = None
        if ef is not None and s % 3 != 2:
            err = rc.f32(rs.standard_normal((M, d)) * 1e-2)
            err[np.array([k != "gauss" for k in kd])] = 0.0
        g.append(x)
        e.append(err)
        v.append(x if err is None else ec.ef_add(x, err, ef))
        kinds.append(kd)
    allv, allk = np.concatenate(v), np.concatenate(kinds)
    r, entries, requested, extra = place_draws(allv, cdag, allk, 77 + d + K)
    tab = _finish(d, K, allv, allk, cdag, r, entries, requested, extra)
    at = np.concatenate([[0], np.cumsum(MULTI_MS)])
    part = lambda a: [a[at[s]:at[s + 1]] for s in range(lay.nseg)]
    wire = lay.new_wire()
    for s, c in enumerate(part(tab.codes)):
        lay.put(wire, s, "codes", c.astype(np.uint8))
    return SimpleNamespace(lay=lay, tab=tab, ef=ef, cdag=cdag, has_err=[x is not None for x in e],
                           gbuf=lay.floats_of(g), ebuf=lay.floats_of(e, fill=ec.E_FILL), r_flat=lay.flat_of(part(tab.r), fill=F(np.nan)),
                           want_wire=wire, want_u=part(tab.u), want_minmax=np.array([fold_minmax(u) for u in part(tab.u)], np.uint32),
                           want_gbuf=lay.floats_of(v))


# ---- the residual case ----------------------------------------------------------------------------------------------------------------
RESIDUAL_MS = (65, 337)


@functools.lru_cache(maxsize=None)
def residual_case(d=16, K=256):
    """rq_contract.encode_case's tensors (hand-built stage 1, one-byte levels) with the draws rebuilt ON stage 2's input,
    rq_contract.stage2_input -> (Group, T, entries, number of requests): what tests/test_gpu_rq_contract.py's run_encode and
    check_encode take, and gq_pvq_encode's stage1 form tensor by tensor."""
    G, T = rc.encode_case(RESIDUAL_MS, d, K, 1, 41, zero_rows=False, edge_draws=False)
    cb1, cdag, _ = rc.codebooks(d, K)
    x = np.concatenate([rc.stage2_input(t["v"], t["codes1"], t["norm1"], cb1) for t in T])
    kinds = np.array(["gauss"] * x.shape[0], dtype=object)
    r, entries, requested, extra = place_draws(x, cdag, kinds, 43)
    tab = _finish(d, K, x, kinds, cdag, r, entries, requested, extra)
    at = 0
    for t in T:
        sl = slice(at, at + t["M"])
        t["r"], t["codes"], t["u"] = tab.r[sl], tab.codes[sl].astype(np.uint8), tab.u[sl]
        t["minmax"] = rc.fold_minmax(t["u"])
        at += t["M"]
    return G, T, tab
