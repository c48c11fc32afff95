"""The contract of include/gq_maurey.h restated bit for bit in numpy (no GPU, no tolerance anywhere), and the inputs the contract
tests share (tests/test_maurey_contract.py checks the restatement and the inputs on the CPU, tests/test_gpu_maurey_contract.py holds
the kernels to them).  C is the f64 running sum in the header's tree order -- 16 elements to a thread, 16 threads to a group, 16
groups to an item, a tensor's items to 256 runs of m = ceil(items / 256) consecutive items, every level added left to right
(np.cumsum is sequential) -- and C = B' + (s' + (G + (B + s))), one f64 addition at a time."""
import numpy as np

CHUNK = 4096
RUNS = 256
HEADER = 16
SIGN = np.uint32(1 << 31)


def _up(x, a=16):
    return (x + a - 1) // a * a


def _exclusive(incl, axis):
    """The exclusive prefixes of a level: +0 in front, the inclusive ones shifted by one."""
    out = np.zeros_like(incl)
    dst = [slice(None)] * incl.ndim
    src = list(dst)
    dst[axis], src[axis] = slice(1, None), slice(None, -1)
    out[tuple(dst)] = incl[tuple(src)]
    return out


def tree_cdf(w):
    """(C float64[n], T): the running sum of |w| (f32 -> f64, padded to whole items with +0) in the header's order."""
    w = np.asarray(w, np.float32).reshape(-1)
    n = w.size
    items = -(-n // CHUNK)
    m = -(-items // RUNS)
    a = np.zeros(items * CHUNK, np.float64)
    a[:n] = np.abs(w).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.cumsum(a.reshape(items, 16, 16, 16), axis=3)      # a thread's running sums
        Bi = np.cumsum(s[..., -1], axis=2)                      # the thread totals of a group, left to right
        B = _exclusive(Bi, 2)
        Gi = np.cumsum(Bi[..., -1], axis=1)                     # the group totals of an item; the last is the item's sum S
        G = _exclusive(Gi, 1)
        S = np.zeros(RUNS * m, np.float64)
        S[:items] = Gi[:, -1]
        si = np.cumsum(S.reshape(RUNS, m), axis=1)              # the items of a run
        s_run = _exclusive(si, 1).reshape(-1)[:items]
        Ri = np.cumsum(si[:, -1])                               # the 256 run totals
        B_run = np.repeat(_exclusive(Ri, 0), m)[:items]
        T = Ri[-1]
        c = B[..., None] + s
        c = G[:, :, None, None] + c
        c = s_run[:, None, None, None] + c
        c = B_run[:, None, None, None] + c
    return c.reshape(-1)[:n], T


def degenerate(T):
    return not (T > 0.0) or not (T < np.inf)


def draw_indices(w, u):
    """The element of every draw: t = (double)u * T, the largest double below T where that is not below T, the smallest i with
    t < C_i.  A degenerate tensor (T == 0, inf or NaN) gives index 0 throughout."""
    C, T = tree_cdf(w)
    u = np.asarray(u, np.float32)
    if degenerate(T):
        return np.zeros(u.size, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = u.astype(np.float64) * T
        t = np.where(t < T, t, np.nextafter(T, 0.0))
    return np.searchsorted(C, t, side="right").astype(np.int64)


def words_of_draws(w, idx, T):
    """index | (w_index < 0) << 31, ascending; a plus sign throughout for a degenerate tensor."""
    idx = np.sort(np.asarray(idx, np.int64))
    words = idx.astype(np.uint32)
    if not degenerate(T):
        words = words | np.where(np.asarray(w, np.float32)[idx] < 0, SIGN, np.uint32(0))
    return words


def section_bytes(w, u, k):
    """A tensor's wire section (uint8[16 + roundup(4k, 16)]): scale = float32(T) / float32(k), 12 zero bytes, the k words, zero
    padding."""
    u = np.asarray(u, np.float32)
    assert u.size == k
    _, T = tree_cdf(w)
    sec = np.zeros((HEADER + _up(4 * k)) // 4, np.uint32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        sec[0] = np.array(np.float32(T) / np.float32(k), np.float32).view(np.uint32)
    sec[4:4 + k] = words_of_draws(w, draw_indices(w, u), T)
    return sec.view(np.uint8)


def split_section(sec, k):
    """(scale float32, words uint32[k]) of a section's bytes."""
    sec = np.ascontiguousarray(sec)
    return sec[:4].view(np.float32)[0], sec[HEADER:HEADER + 4 * k].view(np.uint32)


def dense(words, scale, n):
    """D = scale * float32(+-m), one f32 rounding per element; +0 where nothing was drawn (or the signs cancel)."""
    words = np.asarray(words, np.uint32)
    m = np.zeros(n, np.int64)
    np.add.at(m, (words & ~SIGN).astype(np.int64), np.where(words & SIGN, -1, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float32(scale) * m.astype(np.float32)
    d[m == 0] = np.float32(0)
    return d


def decode_mean(payloads, n, plain=False):
    """f32: ((+0 + D_0) + D_1 ...) / float32(R), the payloads [(scale, words), ...] in order; plain (one payload): D_0 itself."""
    if plain:
        assert len(payloads) == 1
        return dense(payloads[0][1], payloads[0][0], n)
    acc = np.zeros(n, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for scale, words in payloads:
            acc = acc + dense(words, scale, n)
        return acc / np.float32(len(payloads))


def feedback(v, err, s):
    """w = v + s * err in f32: the product rounded, then the sum."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.float32(s) * np.asarray(err, np.float32)
        return np.asarray(v, np.float32) + p


def compress(w, u, k):
    """(section bytes, D float32[n]) of one tensor: what the compress launches leave in the wire and in `out`."""
    sec = section_bytes(w, u, k)
    scale, words = split_section(sec, k)
    return sec, dense(words, scale, np.asarray(w).size)


# ---- the inputs the contract tests share -------------------------------------------------------------------------------
def heavy_tailed(n, seed):
    """Gaussian x log-normal: magnitudes over ~12 decades, so the order of the f64 additions shows in C."""
    rs = np.random.RandomState(seed)
    return (rs.standard_normal(n) * 1e-3 * np.exp(3 * rs.standard_normal(n))).astype(np.float32)


def island_items(items):
    """Three islands of nonzero items [(first, end), ...]: 300 leading zero items (160 where the tensor has fewer than 320 items),
    at least two whole zero runs between two islands, an island's first item not the first of its run, trailing zero items."""
    m = -(-items // RUNS)
    a = 300 if items >= 320 else 160
    b = (-(-(a + 2) // m) + 2) * m + (1 if m > 1 else 0)
    c = (-(-(b + 1) // m) + 2) * m + (1 if m > 1 else 0)
    assert c + 2 < items - 1
    return [(a, a + 2), (b, b + 1), (c, c + 2)]


def islands(n, seed):
    """Zero except for island_items' items (a tenth of their elements zero too)."""
    rs = np.random.RandomState(seed)
    v = np.zeros(n, np.float32)
    for lo, hi in island_items(-(-n // CHUNK)):
        x = heavy_tailed((hi - lo) * CHUNK, rs.randint(1 << 30))
        x[rs.rand(x.size) < 0.1] = 0
        v[lo * CHUNK:hi * CHUNK] = x
    return v


def integer_case(n, lim, zero_runs, seed, density=1.0):
    """Integers in [-lim, lim] (a fraction `density` of them, the others zero), zero over every [lo, hi) of zero_runs with a nonzero
    element on either side, the last element so that T = 2^p, p <= 24: every partial sum is an integer below 2^24, exact in f32
    and f64 in any order of additions.  -> (v, p)"""
    rs = np.random.RandomState(seed)
    v = rs.randint(-lim, lim + 1, size=n).astype(np.float32)
    v[rs.rand(n) >= density] = 0
    for lo, hi in zero_runs:
        v[lo:hi] = 0
    for lo, hi in zero_runs:
        v[hi] = v[hi] if v[hi] != 0 else np.float32(1)
        if lo:
            v[lo - 1] = v[lo - 1] if v[lo - 1] != 0 else np.float32(-1)
    others = int(np.abs(v[:-1]).sum())
    p = 0
    while (1 << p) <= others:
        p += 1
    v[-1] = np.float32(((1 << p) - others) * (1 if rs.rand() < 0.5 else -1))
    assert p <= 24 and v[-1] != 0
    return v, p


def tie_draws(v, p, zero_runs, extra, seed):
    """u = C_i / T exactly on boundaries: behind the last nonzero element in front of every zero run (a run that starts at 0 gives
    t = 0), and behind `extra` more elements chosen at random.  -> (u float32, t float64); float64(u) * T == t is a precondition
    the host test asserts."""
    rs = np.random.RandomState(seed)
    C = np.cumsum(np.abs(v.astype(np.int64)))
    t = [0 if lo == 0 else int(C[lo - 1]) for lo, hi in zero_runs]
    t += [int(x) for x in C[rs.randint(0, v.size - 1, size=extra)]]
    t = np.array(t, np.float64)
    return (t / float(1 << p)).astype(np.float32), t


# n = 12,289 (three items and one element).  Zero runs: leading, across a thread edge (16), a group edge (256), an item edge
# (4096), and one that holds the whole item [8192, 12288) -- the last element carries what is left of T = 2^p.
TIE_SMALL_N = 12289
TIE_SMALL_RUNS = [(0, 5), (10, 20), (250, 262), (4090, 4100), (8185, 12288)]
# n = 1,048,577 (257 items, m = 2: a run is 8192 elements, the last run is one item of one element).  Zero runs: leading (a whole
# item and more), across a run edge, one that holds the whole run [73728, 81920), one across the item edge inside a run, and
# everything from run 100 to the last element, which is a run of its own.
TIE_LONG_N = 1048577
TIE_LONG_RUNS = [(0, 4100), (8192 * 5 - 7, 8192 * 5 + 9), (8192 * 9 - 3, 8192 * 10 + 3), (8192 * 20 + 4091, 8192 * 20 + 4101),
                 (8192 * 100 - 2, TIE_LONG_N - 1)]


def tie_case(long):
    """-> (v, u, t, p, the element every tie behind a zero run must select: the first one behind the run)"""
    if long:
        runs = TIE_LONG_RUNS
        v, p = integer_case(TIE_LONG_N, 2, runs, 102, density=0.1)
        u, t = tie_draws(v, p, runs, 4000, 103)
    else:
        runs = TIE_SMALL_RUNS
        v, p = integer_case(TIE_SMALL_N, 8, runs, 100)
        u, t = tie_draws(v, p, runs, 300, 101)
    return v, u, t, p, np.array([hi for lo, hi in runs], np.int64)


ORDER_N, ORDER_PICK = 5000, 4989
ORDER_LONG_N, ORDER_LONG_PICK = 1048577, 255 * CHUNK


def order_case(long=False):
    """Under u >= 1 the draw is the last element that moved the sum, and which one that is depends on the order of additions.
    |v| = [2^100, 2^46 x 4989, 0 x 10], mixed signs: the tree order selects 4989; a left-to-right f64 sum never moves after element 0
    (2^46 is a quarter of 2^100's ulp).
    long (257 items, m = 2): |v| = [2^100, 2^35 x 1,048,576]: an item's sum, 2^47, is half an ulp of 2^100 and a tie to even leaves
    the sum where it is, a run's two items are one ulp -- the sum moves with the runs only, and the last element to move it is the
    first one of item 255, where s' = 2^47 and B + s = 2^35 first exceed half an ulp together."""
    if long:
        v = np.full(ORDER_LONG_N, 2.0 ** 35, np.float32)
        v[0] = 2.0 ** 100
    else:
        v = np.full(ORDER_N, 2.0 ** 46, np.float32)
        v[0] = 2.0 ** 100
        v[ORDER_PICK + 1:] = 0
    v[1::3] *= -1
    return v


EDGE_U = np.array([0.0, -0.0, 1e-45, np.nextafter(np.float32(1), np.float32(0)), 1.0, 2.0, np.inf, np.nan], np.float32)


def edge_u_tensors():
    """[(name, v)]: first and last items zero; a partial last item behind trailing zeros (n = 8,200, last nonzero at 8,100); a
    first nonzero element (2^-120 in front of 2^40) that u = 0 selects and u = 1e-45 (t = 2^-149 * T) already passes."""
    rs = np.random.RandomState(110)
    a = rs.standard_normal(3 * CHUNK + 100).astype(np.float32)
    a[:CHUNK] = 0
    a[3 * CHUNK:] = 0
    a[CHUNK:CHUNK + 3] = 0
    b = rs.standard_normal(8200).astype(np.float32)
    b[8101:] = 0
    b[:2] = 0
    c = rs.standard_normal(5000).astype(np.float32)
    c[:3] = 0
    c[3], c[4] = np.float32(2.0 ** -120), np.float32(-2.0 ** 40)
    return [("zero_first_and_last_items", a), ("partial_last_item", b), ("tiny_first_element", c)]
