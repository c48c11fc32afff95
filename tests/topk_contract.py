"""The contract of include/gq_topk.h restated in numpy with integer and float32 arithmetic only (no GPU, no call into gq_amd, the
oracle or torch.topk), and the inputs the contract tests share: tests/test_topk_contract.py checks the restatement against
independent witnesses and asserts what every input claims about itself, tests/test_gpu_topk_contract.py holds the kernels to it.

    key(v)   = bits(v) & 0x7fffffff, every NaN mapped to 0x7fffffff
    kept     = the k largest keys, the LOWEST indices among the elements whose key equals the k-th largest
    section  = k x uint32 index, ascending, then k x f32 value (bit copies)
    dense    = w * (kept ? 1 : 0)

The select reads the key in three passes (csrc/sparse_kernels.hpp: pass_shift / pass_bits): bits [20, 31), [9, 20) and [0, 9); a pick
launch of 256 threads walks a pass's histogram from the top, thread t owning the bins nbins - 1 - per * t downwards (per = 8, 8, 2)."""
import numpy as np

CHUNK = 4096
THREADS = 256
PASS_SHIFT = (20, 9, 0)
PASS_BITS = (11, 11, 9)
NAN_KEY = np.uint32(0x7fffffff)
INF_KEY = np.uint32(0x7f800000)
ONE = 0x3f800000


def f32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def bits(a):
    return f32(a).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(b, np.uint32).view(np.float32)


# ---- the contract -------------------------------------------------------------------------------------------------------
def keys(w):
    a = bits(w) & np.uint32(0x7fffffff)
    return np.where(a > INF_KEY, NAN_KEY, a)


def ranking(w):
    """Every index, by descending key; equal keys by ascending index (a stable sort)."""
    return np.argsort(-keys(w).astype(np.int64), kind="stable")


def kept(w, k, order=None):
    """The kept indices, ascending.  order: ranking(w), where a caller has it already."""
    order = ranking(w) if order is None else order
    return np.sort(order[:k]).astype(np.int64)


def section_bytes(w, k, order=None):
    idx = kept(w, k, order)
    return np.concatenate([idx.astype(np.uint32).view(np.uint8), f32(w)[idx].view(np.uint8)])


def dense(w, k, order=None):
    mask = np.zeros(f32(w).size, np.float32)
    mask[kept(w, k, order)] = 1
    with np.errstate(invalid="ignore"):
        return f32(w) * mask


def feedback(v, err, s):
    """w = f32(v + f32(s * err)): the product rounded, then the sum."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = (np.float32(s) * f32(err)).astype(np.float32)
        return (f32(v) + p).astype(np.float32)


def error_feedback(v, err, s, k):
    """-> (w, section bytes of w, dense(w), the new err = f32(w - dense)); the new v is w."""
    w = feedback(v, err, s)
    order = ranking(w)
    D = dense(w, k, order)
    with np.errstate(invalid="ignore"):
        e = (w - D).astype(np.float32)
    return w, section_bytes(w, k, order), D, e


def split_section(sec, k):
    sec = np.ascontiguousarray(sec, np.uint8)
    return sec[:4 * k].view(np.uint32), sec[4 * k:8 * k].view(np.float32)


def decode_mean(payloads, n, k, R, plain=False):
    """payloads: R pairs (uint32 index[k] strictly ascending, f32 value[k]).  A float32 accumulator that starts at +0, the payloads
    added in order, then acc / f32(R), a true division.  plain with R == 1: the values as they are, +0 elsewhere."""
    assert len(payloads) == R >= 1
    acc = np.zeros(n, np.float32)
    for idx, val in payloads:
        idx, val = np.asarray(idx, np.int64), f32(val)
        assert idx.size == val.size == k and np.all(np.diff(idx) > 0) and (k == 0 or (idx[0] >= 0 and idx[-1] < n))
        if plain and R == 1:
            acc[idx] = val
            return acc
        with np.errstate(invalid="ignore", over="ignore"):
            acc[idx] = (acc[idx] + val).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc / np.float32(R)).astype(np.float32)


# ---- what the select does with an input (for the preconditions) -------------------------------------------------------------
def pass_bin(key, p):
    return (int(key) >> PASS_SHIFT[p]) & ((1 << PASS_BITS[p]) - 1)


def pick_thread(p, b):
    """The pick thread that owns bin b of pass p, and whether b is the last (lowest) bin that thread looks at."""
    nbins = 1 << PASS_BITS[p]
    per = nbins // THREADS
    return (nbins - 1 - b) // per, (nbins - 1 - b) % per == per - 1


def select(w, k):
    """-> dict: T (threshold key), gt = #(key > T), ties = #(key == T), need = k - gt, last = the index of the last kept tie,
    bins = T's bin in the three passes."""
    assert 1 <= k <= f32(w).size
    ky = keys(w)
    T = np.sort(ky)[ky.size - k]
    gt, eq = int((ky > T).sum()), np.flatnonzero(ky == T)
    need = k - gt
    assert 1 <= need <= eq.size
    return dict(T=int(T), gt=gt, ties=int(eq.size), need=need, last=int(eq[need - 1]), bins=tuple(pass_bin(T, p) for p in range(3)))


# ---- the inputs the contract tests share ----------------------------------------------------------------------------------
def _signs(rs, n):
    return np.where(rs.rand(n) < 0.5, np.uint32(1 << 31), np.uint32(0))


def ordinary(n, seed):
    return np.random.RandomState(seed).standard_normal(n).astype(np.float32)


def heavy_tailed(n, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal(n) * 1e-3 * np.exp(3 * rs.standard_normal(n))).astype(np.float32)


NEIGHBOURS = [(5000, 37, 900), (4097, 100, 901)]      # (n, k, seed) of the ordinary tensors on either side in a three-tensor group

LOW9 = [0, 1, 255, 256, 510, 511]


def low9_input():
    """Keys 0x3f800000 + j, j in [0, 512), each one to four times, shuffled, random signs: pass 0 and pass 1 see ONE bin."""
    rs = np.random.RandomState(910)
    j = np.repeat(np.arange(512), rs.randint(1, 5, size=512))
    rs.shuffle(j)
    return from_bits((np.uint32(ONE) + j.astype(np.uint32)) | _signs(rs, j.size))


def low9_cases():
    """[(low, more, k)]: more = 0 -- k = #(key >= 0x3f800000 + low), every tie kept; more = 1 -- one more, the threshold moves down
    one bin and keeps one of its ties.  (low = 0 has no bin below it in this input, and k = n + 1 is no k.)"""
    ky = keys(low9_input())
    out = []
    for low in LOW9:
        a = int((ky >= ONE + low).sum())
        out.append((low, 0, a))
        if low:
            out.append((low, 1, a + 1))
    return out


PAIRS = {      # name: (the larger key, the smaller key)
    "one": (ONE, ONE - 1),                                   # 1.0 | nextafter(1, 0): pass-0 bins 1016 | 1015, pick threads 128 | 129
    "two": (0x40000000, 0x3fffffff),                         # 2.0 | nextafter(2, 0): pass-0 bins 1024 | 1023, threads 127 | 128 (waves 1 | 2)
    "bit9": (ONE | (1 << 9), ONE),                           # pass-1 bins 1 | 0 of one pass-0 bin
    "pass1_thread": (ONE | (1536 << 9), ONE | (1535 << 9)),  # pass-1 bins 8t + 8 | 8t + 7, t = 191: threads 63 | 64 (waves 0 | 1)
}


def pair_input(name):
    hi, lo = PAIRS[name]
    rs = np.random.RandomState(920 + sorted(PAIRS).index(name))
    n = 3001
    return from_bits(np.where(rs.rand(n) < 0.4, np.uint32(hi), np.uint32(lo)) | _signs(rs, n))


def pair_ks(name):
    a = int((keys(pair_input(name)) >= PAIRS[name][0]).sum())
    return [a - 1, a, a + 1]


SUB_MIN, SUB_MID = 1, 0x00080123      # the smallest subnormal; one in the middle of pass-0 bin 0 (pass-1 bin 1024)


def subnormal_input():
    """n = 3000: 7 normals, 400 subnormals over the whole range plus three each of SUB_MIN and SUB_MID, signed zeros elsewhere."""
    rs = np.random.RandomState(930)
    n = 3000
    b = np.zeros(n, np.uint32)
    pos = rs.permutation(n)
    b[pos[:7]] = bits(rs.standard_normal(7).astype(np.float32)) & np.uint32(0x7fffffff)
    sub = rs.randint(2, 0x800000, size=400).astype(np.uint32)
    sub = sub[sub != SUB_MID]
    b[pos[7:7 + sub.size]] = sub
    b[pos[500:503]] = SUB_MIN
    b[pos[503:506]] = SUB_MID
    return from_bits(b | _signs(rs, n))


def subnormal_cases():
    """[(name, k)]: T = SUB_MIN and SUB_MID with two of their three ties kept; T = 0 with half the zeros kept."""
    ky = keys(subnormal_input())
    return [("min", int((ky > SUB_MIN).sum()) + 2), ("mid", int((ky > SUB_MID).sum()) + 2),
            ("zero", int((ky > 0).sum()) + int((ky == 0).sum()) // 2)]


NANS = np.array([0x7fc00000, 0xffc00000, 0x7fc00001, 0xffffffff, 0x7f800001, 0xff800123, 0x7fffffff], np.uint32)


def top_input(kind):
    """n = 2000 of randn with, kind "nan": 40 NaNs of seven bit patterns (quiet and signalling, both signs); "inf": 30 infinities of
    both signs and 3 NaNs."""
    rs = np.random.RandomState(940 + (kind == "inf"))
    b = bits(rs.standard_normal(2000).astype(np.float32)).copy()
    pos = rs.permutation(2000)
    if kind == "nan":
        b[pos[:40]] = NANS[rs.randint(0, NANS.size, size=40)]
    else:
        b[pos[:30]] = np.where(rs.rand(30) < 0.5, np.uint32(0x7f800000), np.uint32(0xff800000))
        b[pos[30:33]] = NANS[:3]
    return from_bits(b)


TOP_CASES = [("nan", 10), ("inf", 12), ("inf", 33)]      # more NaNs than k; more infinities (and 3 NaNs) than k; exactly k of both


def stair_input():
    return heavy_tailed(5000, 950)


def stair_ks():
    """[(k, pick thread)]: k = the cumulative count at the END of a pass-0 pick thread's eight bins (the first, a middle and the
    last but one thread that sees any key), and one above each."""
    ky = keys(stair_input())
    hist = np.bincount(ky >> 20, minlength=2048)
    per_thread = hist[::-1].reshape(THREADS, 8).sum(1)      # thread t: bins 2047 - 8t downwards
    cum = np.cumsum(per_thread)
    seen = np.flatnonzero(per_thread)
    out = []
    for t in (seen[0], seen[seen.size // 2], seen[-2]):
        out += [(int(cum[t]), int(t)), (int(cum[t]) + 1, int(t))]
    return out


# ---- ties ------------------------------------------------------------------------------------------------------------------
TIE_N = 1048576 + 4097      # 258 items: the scan launch takes two rounds of 256
TIE_EDGES = [0, 62, 63, 64, 255, 256, 4095, 4096, 1048575, 1048576, TIE_N - 1]      # the index of the last kept tie (0: need = 1)
TIE_SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 8192]
HALF_N = 2097153


def all_equal(n, seed):
    """+-0.25, the sign at random."""
    rs = np.random.RandomState(seed)
    return from_bits(np.full(n, 0x3e800000, np.uint32) | _signs(rs, n))


def two_level(n, seed, edges=()):
    """+-1.0 with 2.0 on one element in sixteen (so that #(key > T) in front of an element is not zero); +-1.0 on `edges`, and 2.0
    on element 1 where there is one to spare."""
    rs = np.random.RandomState(seed)
    b = np.where(rs.rand(n) < 1 / 16, np.uint32(0x40000000), np.uint32(ONE)) | _signs(rs, n)
    e = np.array([i for i in edges if i < n], np.int64)
    b[e] = np.uint32(ONE) | (b[e] & np.uint32(1 << 31))
    if n > 2 and 1 not in edges:
        b[1] = 0x40000000
    return from_bits(b)


def k_for_last_tie(w, T, pos):
    """The k that makes `pos` (an element with key T) the last kept tie."""
    ky = keys(w)
    assert ky[pos] == T
    return int((ky > T).sum()) + int((ky[:pos + 1] == T).sum())


# ---- error feedback ----------------------------------------------------------------------------------------------------------
EF_N = 5000
EF_SCALES = [0.75, 1.0, 0.0, -0.0]


def fma_f32(v, err, s):
    """f32(v + s * err) with ONE rounding, where float64 holds the sum exactly (exact_fma says where); elsewhere the f64 result
    rounded again, which is only used to look for candidates."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (f32(v).astype(np.float64) + np.float64(np.float32(s)) * f32(err).astype(np.float64)).astype(np.float32)


def exact_fma(v, err, s, i):
    """Whether float64 holds v[i] + s * err[i] exactly (then fma_f32 is the fused result at i), checked in rational arithmetic."""
    from fractions import Fraction
    a, b, c = float(f32(v)[i]), float(np.float32(s)), float(f32(err)[i])
    return Fraction(a) + Fraction(b) * Fraction(c) == Fraction(a + b * c)


def ef_reorder():
    """err as large as v: the ranking of w is not the ranking of v."""
    rs = np.random.RandomState(960)
    return rs.standard_normal(EF_N).astype(np.float32), rs.standard_normal(EF_N).astype(np.float32), EF_N // 16


def ef_fma():
    """s = 0.75.  Elements i where the fused result is one ulp LARGER in magnitude than the two-rounding w get a neighbour i + 1 with
    err = 0 and v = -(the fused magnitude): with two roundings i + 1 outranks i, fused the two tie and i, the lower index, wins.
    k keeps everything down to key(w[i + 1]) of the first such pair: a fused load swaps i + 1 for i.  -> (v, err, k, the pairs' i)"""
    rs = np.random.RandomState(961)
    s = np.float32(0.75)
    v, e = rs.standard_normal(EF_N).astype(np.float32), rs.standard_normal(EF_N).astype(np.float32)
    w2, wf = feedback(v, e, s), fma_f32(v, e, s)
    cand = np.flatnonzero((keys(wf) == keys(w2) + 1) & (np.arange(EF_N) < EF_N - 1))
    pairs = []
    for i in cand:
        if len(pairs) == 8:
            break
        if exact_fma(v, e, s, i) and (not pairs or i > pairs[-1] + 1) and np.abs(w2[i]) < 0.5:
            pairs.append(int(i))
    for i in pairs:
        v[i + 1], e[i + 1] = -np.abs(wf[i]), 0
    w = feedback(v, e, s)
    k = int((keys(w) >= keys(w)[pairs[0] + 1]).sum())
    return v, e, k, pairs


def ef_ties():
    """s = 1: v a multiple of 1/8 in [-4, 4], err = +-2 - v exactly on three elements in four: |w| = 2 there, a tie v does not have."""
    rs = np.random.RandomState(962)
    v = (rs.randint(-32, 33, size=EF_N) / 8.0).astype(np.float32)
    t = np.where(rs.rand(EF_N) < 0.5, np.float32(2), np.float32(-2))
    e = np.where(rs.rand(EF_N) < 0.75, t - v, rs.standard_normal(EF_N).astype(np.float32) / 8).astype(np.float32)
    w = feedback(v, e, 1.0)
    k = int((keys(w) > 0x40000000).sum()) + int((keys(w) == 0x40000000).sum()) // 2
    return v, e, k


def ef_inf():
    """s = 0 and err = +-inf on 30 elements: w = v + 0 * inf is NaN there, ranked above everything; k = 20 keeps the lowest 20."""
    rs = np.random.RandomState(963)
    v, e = rs.standard_normal(EF_N).astype(np.float32), rs.standard_normal(EF_N).astype(np.float32)
    pos = rs.permutation(EF_N)[:30]
    e[pos] = np.where(rs.rand(30) < 0.5, np.inf, -np.inf).astype(np.float32)
    return v, e, 20


def ef_signed_zeros():
    """v of +-0 and err of both signs in front of ordinary elements: s = -0 and s = 0 give zeros of different signs in w."""
    rs = np.random.RandomState(964)
    v, e = rs.standard_normal(EF_N).astype(np.float32), rs.standard_normal(EF_N).astype(np.float32)
    v[:2000] = from_bits(_signs(rs, 2000))
    return v, e, EF_N - 1000      # k reaches into the zeros


# ---- hand-built payloads for the decode launch ----------------------------------------------------------------------------------
DEC_SIZES = [1, 4096, 4097, 12289, 20000, 5000, 300]
DEC_KS = [1, 37, 64, 131, 200, 0, 300]
DEC_PAYLOADS = 16
DEC_WINDOWS = [(0, 1), (1, 1), (0, 2), (3, 2), (0, 3), (3, 3), (0, 8), (5, 8), (0, 16)]      # (first payload, R)
DEC_UNTOUCHED = (4, 3)      # tensor 4 (n = 20000), chunk 3: no payload names an index in [12288, 16384)
BIG = [1e8, 1.0, -1e8]
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def _hot(n):
    return sorted(set(i for i in (0, 4095, 4096, 8191, 8192, n - 1) if 0 <= i < n))


def hand_payloads():
    """payloads[s][r] = (uint32 index[k] ascending and distinct, f32 value[k]) for tensor s and payload r, never the output of a
    compress.  Every payload of a tensor with k > len(hot) carries the hot indices (0, 4095, 4096, 8191, 8192, n - 1) plus a set
    of its own: r % 4 == 3 -- all of them in ONE chunk, otherwise anywhere (tensor 4: never in chunk 3).  Values: heavy-tailed,
    so the order of additions shows; in tensor 3, hot index number p carries BIG in the order PERMS[p] over the payloads 0, 1, 2;
    payload 0 carries -0 on every second index; payloads 4 and 5 carry NaN, +inf and -inf."""
    rs = np.random.RandomState(970)
    payloads = []
    for s, (n, k) in enumerate(zip(DEC_SIZES, DEC_KS)):
        hot = _hot(n)
        chunks = -(-n // CHUNK)
        per = []
        for r in range(DEC_PAYLOADS):
            if k == n:
                idx = np.arange(n)
            elif k <= len(hot):
                idx = np.array(hot[:k])
            else:
                if r % 4 == 3:
                    full = [c for c in range(chunks) if min(n, (c + 1) * CHUNK) - c * CHUNK >= k and (s, c) != DEC_UNTOUCHED]
                    c = full[(r // 4) % len(full)]
                    pool = np.arange(c * CHUNK, min(n, (c + 1) * CHUNK))
                    base = np.array([i for i in hot if pool[0] <= i <= pool[-1]], np.int64)
                else:
                    pool = np.arange(n)
                    base = np.array(hot, np.int64)
                if s == DEC_UNTOUCHED[0]:
                    pool = pool[(pool < DEC_UNTOUCHED[1] * CHUNK) | (pool >= (DEC_UNTOUCHED[1] + 1) * CHUNK)]
                rest = np.setdiff1d(pool, base)
                idx = np.sort(np.concatenate([base, rs.choice(rest, k - base.size, replace=False)]))
            val = heavy_tailed(k, 971 + 100 * s + r) * np.float32(1e3)
            if r == 0:
                val[::2] = np.float32(-0.0)
            if r in (4, 5) and k >= 3:
                val[[0, k // 2, k - 1]] = np.float32([np.nan, np.inf, -np.inf]) if r == 4 else np.float32([-np.inf, np.nan, np.inf])
            if s == 3 and r < 3:
                for p, h in enumerate(hot):
                    val[np.searchsorted(idx, h)] = np.float32(BIG[PERMS[p][r]])
            per.append((idx.astype(np.uint32), val.astype(np.float32)))
        payloads.append(per)
    return payloads
