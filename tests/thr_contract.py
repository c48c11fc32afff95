"""include/gq_thr.h restated in numpy, one float32 / float64 operation at a time: the threshold fit (the trees as written, gq_ln as
written), the kept set, the wire section, the dense decode, error feedback and the decode-mean -- plus builders for layouts, wires,
hand-made payloads and the test inputs.  tests/test_thr_contract.py checks this file on the CPU; the GPU tests hold libgq_thr.so to
it with np.array_equal.  fit's `order`, `fused` and `recip` arguments are MUTATIONS of the contract (the CPU test shows each of them to change eta's bits on an
input built for it); the contract is their defaults."""
import struct
from fractions import Fraction

import numpy as np

f32, f64, u32 = np.float32, np.float64, np.uint32
ITEM = 4096
HDR = 16
NO_INDEX = 0xffffffff
INF_KEY = 0x7f800000
MAX_ETA = 0x7f7fffff
MAX_STAGES = 8
FLT_MAX = f32(3.4028234663852886e38)

LN_C = [0x3FF0000000000000, 0x3FD5555555555555, 0x3FC999999999999A, 0x3FC2492492492492, 0x3FBC71C71C71C71C, 0x3FB745D1745D1746,
        0x3FB3B13B13B13B14, 0x3FB1111111111111, 0x3FAE1E1E1E1E1E1E, 0x3FAAF286BCA1AF28, 0x3FA8618618618618, 0x3FA642C8590B2164]
LN_LN2 = 0x3FE62E42FEFA39EF
LN_SQRT2 = 0x3FF6A09E667F3BCD


def d_from(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def d_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(u32)


def ebits(x):
    """The bits of one f32 as a Python int."""
    return int(np.array(x, dtype=f32).reshape(1).view(u32)[0])


def from_bits(b):
    return np.ascontiguousarray(b, dtype=u32).view(f32)


def keys(w):
    a = bits(w) & u32(0x7fffffff)
    return np.where(a > INF_KEY, u32(0x7fffffff), a)


def up16(n):
    return (n + 15) & ~15


def capacity(n, k, percent=150):
    return min(n, (k * percent + 99) // 100)


def section_bytes(n, cr, percent=150):
    return HDR + up16(8 * capacity(n, n // cr, percent))


def stride_for(n, M):
    items = -(-n // ITEM)
    m = 1
    while 2 * m <= M and -(-items // (2 * m)) >= 16:
        m *= 2
    return m


def feedback(v, err, s):
    """w = v + s * err: the product rounded to f32, then the sum."""
    with np.errstate(all="ignore"):
        p = f32(s) * np.asarray(err, dtype=f32)
        return (np.asarray(v, dtype=f32) + p).astype(f32)


def gq_ln(x):
    """The header's gq_ln on Python floats (IEEE f64, one rounding per operation)."""
    b = d_bits(float(x))
    e = (b >> 52) - 1023
    mb = (b & 0x000fffffffffffff) | 0x3ff0000000000000
    mant = d_from(mb)
    if mb > LN_SQRT2:
        mant = mant * 0.5
        e = e + 1
    z = (mant - 1.0) / (mant + 1.0)
    y = z * z
    p = d_from(LN_C[11])
    for j in range(10, -1, -1):
        p = p * y
        p = p + d_from(LN_C[j])
    a = float(e) * d_from(LN_LN2)
    t = 2.0 * z
    c = t * p
    return a + c


def tree(a, order=None):
    """The balanced tree over a power-of-two number of f64 slots (order None); 'seq' and 'desc' are the mutations."""
    a = np.array(a, dtype=f64)
    assert a.size & (a.size - 1) == 0 and a.size >= 1
    if order == "seq":
        s = f64(0.0)
        for x in a:
            s = s + x
        return f64(s)
    while a.size > 1:
        a = (a[:a.size // 2] + a[a.size // 2:]) if order == "desc" else (a[0::2] + a[1::2])
    return f64(a[0])


def item_fit(w, eta, order=None):
    """(c, Sigma) of one item: w its elements (at most ITEM), eta the f32 threshold of the stage before."""
    k = keys(w)
    m = (k > ebits(eta)) & (k < INF_KEY)
    slots = np.zeros(ITEM, dtype=f64)
    slots[:w.size][m] = from_bits(k[m]).astype(f64) - f64(eta)
    return int(m.sum()), tree(slots, order)


def round_f32(t):
    with np.errstate(all="ignore"):
        f = f32(t)
    return f32(FLT_MAX) if (ebits(f) & 0x7fffffff) >= INF_KEY else f


def fit(w, k, S, m=1, order=None, fused=False, recip=False, trace=None):
    """eta_S of the fitted mode.  order / fused / recip: mutations (the item tree's order; t = fma(beta, L, eta); beta = Sigma * (1 / c))."""
    w = np.ascontiguousarray(w, dtype=f32)
    n = w.size
    nit = -(-n // ITEM)
    fit_items = list(range(0, nit, m))
    n_fit = sum(min(ITEM, n - j * ITEM) for j in fit_items)
    Q = 1
    while Q < len(fit_items):
        Q *= 2
    eta = f32(0.0)
    for s in range(1, S + 1):
        slots, c = np.zeros(Q, dtype=f64), 0
        for q, j in enumerate(fit_items):
            cj, sj = item_fit(w[j * ITEM:(j + 1) * ITEM], eta, order)
            c += cj
            slots[q] = sj
        sigma = float(tree(slots))
        chat = (float(c) * float(n)) / float(n_fit)
        if trace is not None:
            trace.append((s, c, sigma, chat, float(eta)))
        if c == 0 or chat <= float(k):
            continue
        beta = sigma * (1.0 / float(c)) if recip else sigma / float(c)
        L = gq_ln(chat / float(k)) / float(S - s + 1)
        if fused:
            t = float(Fraction(beta) * Fraction(L) + Fraction(float(eta)))      # one rounding of the exact value
        else:
            bl = beta * L
            t = float(eta) + bl
        eta = round_f32(t)
    return f32(eta)


def exceeding(w, eta):
    return keys(w) > ebits(eta)


def kept_mask(w, eta, cap):
    ex = exceeding(w, eta)
    found = int(ex.sum())
    keep = ex & (np.cumsum(ex) <= cap)
    return keep, found


def dense(w, keep):
    """w * (kept ? 1 : 0): an unkept infinity or NaN decodes to NaN, an unkept finite value to a signed zero."""
    with np.errstate(all="ignore"):
        return (np.asarray(w, dtype=f32) * keep.astype(f32)).astype(f32)


def section(w, eta, cap):
    """The wire section (uint8) of one tensor -> (bytes, keep mask, found)."""
    keep, found = kept_mask(w, eta, cap)
    idx = np.flatnonzero(keep).astype(u32)
    kept = idx.size
    sec = np.zeros(HDR + up16(8 * cap), dtype=np.uint8)
    words = sec.view(u32)
    words[0], words[1], words[2], words[3] = kept, found, ebits(eta), 0
    words[4:4 + cap] = NO_INDEX
    words[4:4 + kept] = idx
    words[4 + cap:4 + cap + kept] = bits(np.asarray(w, dtype=f32)[idx])
    return sec, keep, found


def compress(v, cr, S, eta=None, percent=150, m=1, err=None, s=None):
    """One tensor through the whole compress -> (section, dense decode, w, new err or None, eta, found)."""
    v = np.ascontiguousarray(v, dtype=f32)
    n = v.size
    k = n // cr
    assert k >= 1
    cap = capacity(n, k, percent)
    w = feedback(v, err, s) if err is not None else v
    e = f32(eta) if S == 0 else fit(w, k, S, m)
    sec, keep, found = section(w, e, cap)
    D = dense(w, keep)
    with np.errstate(all="ignore"):
        ne = (w - D).astype(f32) if err is not None else None
    return sec, D, w, ne, e, found


def split_section(sec, cap):
    words = np.ascontiguousarray(sec).view(u32)
    return words[:4], words[4:4 + cap], words[4 + cap:4 + 2 * cap].view(f32)


def decode_mean(payloads, n, cap, R, plain=False):
    """(+0 + c_0 + ... + c_{R-1}) / R over the first min(kept, cap) slots of every payload, payloads in order; plain: R == 1, the
    values as they are.  A slot whose index is not below n is skipped (the kernel's guard)."""
    assert len(payloads) == R and (not plain or R == 1)
    acc = np.zeros(n, dtype=f32)
    with np.errstate(all="ignore"):
        for sec in payloads:
            hdr, idx, val = split_section(sec, cap)
            kk = min(int(hdr[0]), cap)
            for j in range(kk):
                i = int(idx[j])
                if i < n:
                    acc[i] = val[j] if plain else f32(acc[i] + val[j])
        return acc if plain else (acc / f32(R)).astype(f32)


def layout(sizes, cr, percent=150, dense_sizes=()):
    """Wire offsets of the tensors' sections (16-byte aligned, in order), the dense table [(offset, elements)] behind them and the
    bytes of one user's wire."""
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off = up16(off + section_bytes(n, cr, percent))
    dense_tab = []
    for n in dense_sizes:
        dense_tab.append((off, n))
        off += 4 * n
    return offs, dense_tab, up16(off)


def hand_payload(n, cap, kept_field, idx, val, found=None, eta=0.0):
    """A payload built by hand: `idx` / `val` fill the first slots, the rest are pad slots; the header's kept is `kept_field` (which
    may lie: above cap it is clamped by the decode)."""
    sec = np.zeros(HDR + up16(8 * cap), dtype=np.uint8)
    words = sec.view(u32)
    words[0], words[1], words[2] = kept_field, (kept_field if found is None else found), ebits(f32(eta))
    words[4:4 + cap] = NO_INDEX
    words[4:4 + len(idx)] = np.asarray(idx, dtype=u32)
    words[4 + cap:4 + cap + len(val)] = bits(np.asarray(val, dtype=f32))
    return sec


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def gaussian(n, seed, scale=1e-3):
    return (np.random.RandomState(seed).standard_normal(n) * scale).astype(f32)


def laplace(n, seed, scale=1e-3):
    return (np.random.RandomState(seed).laplace(size=n) * scale).astype(f32)


def student(n, seed, df=3, scale=1e-3):
    return (np.random.RandomState(seed).standard_t(df, size=n) * scale).astype(f32)


def half_zero(n, seed, scale=1e-3):
    rs = np.random.RandomState(seed)
    g = rs.standard_normal(n) * scale
    g[rs.rand(n) < 0.5] = 0.0
    return g.astype(f32)


def uniform(n, seed, scale=1e-3):
    return ((np.random.RandomState(seed).rand(n) * 2 - 1) * scale).astype(f32)


FAMILIES = {"gaussian": gaussian, "laplace": laplace, "student3": student, "half_zero": half_zero, "uniform": uniform}


def specials(n, seed):
    """A Gaussian tensor with +-0, subnormals, +-inf and NaNs of both signs strewn in."""
    rs = np.random.RandomState(seed)
    v = gaussian(n, seed)
    pos = rs.permutation(n)[:16]
    vals = from_bits(np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x7f800000, 0xff800000,
                               0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x00000000], dtype=u32))
    v[pos] = vals
    return v


def few_large(n, seed, count, floor=1e-30, big=1.0):
    """`count` large values (magnitudes in [1, 2)) over a tiny floor: found = count for every eta between the two."""
    rs = np.random.RandomState(seed)
    v = (rs.standard_normal(n) * floor).astype(f32)
    pos = np.sort(rs.permutation(n)[:count])
    v[pos] = (big * (1.0 + rs.rand(count))).astype(f32) * np.where(rs.rand(count) < 0.5, -1, 1).astype(f32)
    return v


def sparse_nonzero(n, seed, count):
    """Only `count` non-zero elements."""
    rs = np.random.RandomState(seed)
    v = np.zeros(n, dtype=f32)
    v[rs.permutation(n)[:count]] = gaussian(count, seed + 1) + f32(1e-6)
    return v


def on_threshold(v, cr, S, m=1, copies=3):
    """v with `copies` elements moved exactly onto the eta the fit finds for the result (a fixed point is searched: moving
    elements moves the fit).  None when no fixed point is found in a few rounds."""
    v = v.copy()
    k = v.size // cr
    pos = np.arange(copies) * (v.size // copies) + 1
    for _ in range(8):
        eta = fit(v, k, S, m)
        if np.all(bits(np.abs(v[pos])) == ebits(eta)):
            return v, eta
        v[pos] = eta
        v[pos[1]] = -eta
    return None


def outcome_case(which, n=8193, cr=64):
    """The inputs of the GPU file's outcome test, with what the restatement says about them (tests/test_thr_contract.py asserts that
    each meets its precondition): v, the stages S, the fixed eta (S = 0), found and the eta the compress must report."""
    from types import SimpleNamespace
    if which == "far":
        n, cr = 65537, 256
    k = n // cr
    cap = capacity(n, k)
    S, eta = 0, None
    if which in ("cap", "cap+1"):      # a fixed threshold ON the (found + 1)-th largest magnitude: exactly `found` elements exceed it
        v = laplace(n, 21)
        want = cap if which == "cap" else cap + 1
        eta = np.sort(np.abs(v))[::-1][want]
    elif which == "far":               # 16 cap large values over a tiny floor: one stage lands between the two, all of them exceed
        v, S = few_large(n, 22, 16 * cap), 1
    elif which == "none":              # a fixed threshold on the largest magnitude: nothing exceeds
        v = gaussian(n, 23)
        eta = np.abs(v).max()
    elif which == "sparse":            # fewer non-zeros than k: c^ <= k at stage 1, eta stays +0
        v, S = sparse_nonzero(n, 24, k - 28), 3
    elif which == "on_eta":            # three elements exactly on the fitted eta: not exceeding
        v, _ = on_threshold(laplace(n, 25), cr, 3)
        S = 3
    else:
        raise KeyError(which)
    sec, D, w, ne, eta_out, found = compress(v, cr, S, eta)
    return SimpleNamespace(v=v, S=S, eta=None if eta is None else float(eta), cr=cr, k=k, cap=cap, found=found, eta_out=eta_out)
