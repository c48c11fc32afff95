"""The contract of include/gq_stc.h restated in numpy with integer, float32 and float64 operations one at a time (no GPU, no call
into gq_amd or torch), and the inputs the contract tests share: tests/test_stc_contract.py checks the restatement against
independent witnesses and asserts what every input claims about itself, tests/test_gpu_stc_contract.py holds the kernels to it.

    kept     = top-k's (tests/topk_contract.py): the k largest keys, the LOWEST indices among the elements with the k-th largest
    mu       = f32(S / f64(k)), +0 for k = 0, a NaN as 0x7fc00000; S = halve(items' halve(key > T ? f64(|w|) : +0)) + f64(need) * f64(|T|)
    section  = { k, bits(mu), items, 0 }, uint32 start[items], k x uint16 (position in the item | sign << 15), zeros to 16 bytes
    dense    = kept ? copysign(mu, w) : +0
"""
import numpy as np

import topk_contract as tc

CHUNK = 4096
HEADER = 16
NAN_MU = np.uint32(0x7fc00000)
SIGN = np.uint32(0x80000000)

f32, bits, from_bits, keys = tc.f32, tc.bits, tc.from_bits, tc.keys


def up16(x):
    return (x + 15) // 16 * 16


def items_of(n):
    return -(-n // CHUNK)


def section_size(n, k):
    return up16(HEADER + 4 * items_of(n) + 2 * k)


# ---- the magnitude ---------------------------------------------------------------------------------------------------------
def halve(x):
    """x: float64 [rows, m], m a power of two.  for h = m / 2 ... 1: x[j] = x[j] + x[j + h] for j < h.  -> x[:, 0]"""
    x = np.array(x, np.float64, ndmin=2)
    h = x.shape[1] // 2
    assert 2 * h == x.shape[1] or x.shape[1] == 1
    with np.errstate(invalid="ignore", over="ignore"):
        while h >= 1:
            assert x.shape[1] == 2 * h
            x = x[:, :h] + x[:, h:]
            h //= 2
    return x[:, 0]


def threshold(w, k, order=None):
    """-> (T, need, the kept indices ascending); k = 0: (None, 0, [])"""
    idx = tc.kept(w, k, order)
    if k == 0:
        return None, 0, idx
    ky = keys(w)
    T = ky[idx].min()
    return T, k - int((ky > T).sum()), idx


def kept_sum(w, k, order=None):
    """S of the header (float64), for k >= 1."""
    w = f32(w)
    T, need, _ = threshold(w, k, order)
    nit = items_of(w.size)
    x = np.zeros(nit * CHUNK, np.float64)
    mag = from_bits(bits(w) & ~SIGN).astype(np.float64)
    x[:w.size] = np.where(keys(w) > T, mag, np.float64(0.0))
    s = halve(x.reshape(nit, CHUNK))
    P = 1
    while P < nit:
        P *= 2
    padded = np.zeros(P, np.float64)
    padded[:nit] = s
    with np.errstate(invalid="ignore", over="ignore"):
        ties = np.float64(need) * np.float64(from_bits(np.array([T], np.uint32))[0])
        return halve(padded)[0] + ties


def mu_bits(w, k, order=None):
    if k == 0:
        return np.uint32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.float32(kept_sum(w, k, order) / np.float64(k))
    return NAN_MU if np.isnan(m) else np.array([m], np.float32).view(np.uint32)[0]


# ---- wire and dense decode ------------------------------------------------------------------------------------------------------
def build_section(n, k, mu, idx, signs):
    """The bytes of a section that carries the ascending indices idx with sign bits `signs` (0 / 1) at magnitude bits mu."""
    idx = np.asarray(idx, np.int64)
    nit = items_of(n)
    sec = np.zeros(section_size(n, k), np.uint8)
    head = sec[:HEADER + 4 * nit].view(np.uint32)
    head[0], head[1], head[2] = k, mu, nit
    head[4:] = np.searchsorted(idx, np.arange(nit, dtype=np.int64) * CHUNK, side="left")
    words = (idx % CHUNK).astype(np.uint16) | (np.asarray(signs, np.uint16) << np.uint16(15))
    sec[HEADER + 4 * nit:HEADER + 4 * nit + 2 * k] = words.view(np.uint8)
    return sec


def section_bytes(w, k, order=None):
    w = f32(w)
    idx = tc.kept(w, k, order)
    return build_section(w.size, k, mu_bits(w, k, order), idx, bits(w)[idx] >> np.uint32(31))


def split_section(sec, n, k):
    """-> (header uint32[4], start uint32[items], word uint16[k], the pad bytes)"""
    sec = np.ascontiguousarray(sec, np.uint8)
    nit = items_of(n)
    a = HEADER + 4 * nit
    return sec[:HEADER].view(np.uint32), sec[HEADER:a].view(np.uint32), sec[a:a + 2 * k].view(np.uint16), sec[a + 2 * k:section_size(n, k)]


def dense(w, k, order=None):
    w = f32(w)
    idx = tc.kept(w, k, order)
    d = np.zeros(w.size, np.uint32)
    d[idx] = (mu_bits(w, k, order) & ~SIGN) | (bits(w)[idx] & SIGN)
    return from_bits(d)


def error_feedback(v, err, s, k):
    """-> (w, section bytes of w, dense(w), the new err = f32(w - dense)); the new v is w."""
    w = tc.feedback(v, err, s)
    order = tc.ranking(w)
    D = dense(w, k, order)
    with np.errstate(invalid="ignore"):
        e = (w - D).astype(np.float32)
    return w, section_bytes(w, k, order), D, e


def decode_mean(sections, n, k, R, plain=False):
    """sections: R sections' bytes (any content).  k and the item count are the TABLE's; every start is clamped to k, a word whose
    bits 0-14 are not below the item's length is skipped.  A float32 accumulator that starts at +0, the payloads added in order, then
    acc / f32(R), a true division.  plain with R == 1: +-mu as it is, +0 elsewhere."""
    assert len(sections) == R >= 1
    nit = items_of(n)
    acc = np.zeros(n, np.float32)
    for sec in sections:
        sec = np.ascontiguousarray(sec, np.uint8)
        head = sec[:HEADER + 4 * nit].view(np.uint32)
        mu = head[1] & ~SIGN
        word = sec[HEADER + 4 * nit:HEADER + 4 * nit + 2 * k].view(np.uint16).astype(np.uint32)
        for t in range(nit):
            lo = min(int(head[4 + t]), k)
            hi = min(int(head[4 + t + 1]) if t + 1 < nit else k, k)
            wd = word[lo:hi]
            u = (wd & np.uint32(0x7fff)).astype(np.int64)
            ok = u < min(CHUNK, n - t * CHUNK)
            u, c = u[ok] + t * CHUNK, from_bits(mu | ((wd[ok] & np.uint32(0x8000)) << np.uint32(16)))
            assert np.unique(u).size == u.size, "an index named twice in one payload: the header leaves the value open"
            if plain and R == 1:
                acc[u] = c
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    acc[u] = (acc[u] + c).astype(np.float32)
        if plain and R == 1:
            return acc
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc / np.float32(R)).astype(np.float32)


# ---- the inputs the contract tests share -------------------------------------------------------------------------------------
SIZES = [1001, 4096, 4097, 8193, 12289]
BIG_N = 2097153      # 513 items: the scan launch takes three rounds of 256, the sum tree is padded to 1,024


def seam_input():
    """n = 12289 of +-1.0 with 2.0 on one element in sixteen; +-1.0 on 4095, 4096, 8191 and 8192 (ties on both sides of two seams)."""
    return tc.two_level(12289, 1001, edges=(4095, 4096, 8191, 8192))


def seam_ks():
    """[(k, the index of the last kept tie)]: the last kept tie is the last element of item 0, the first of item 1, and the same at
    the next seam."""
    w = seam_input()
    return [(tc.k_for_last_tie(w, tc.ONE, pos), pos) for pos in (4095, 4096, 8191, 8192)]


def lopsided_input():
    """n = 20481 (six items): item 2 is all +-8.0 (4,096 kept elements), item 4 holds 40 of +-4.0, the rest is N(0, 1) * 1e-3; with
    k = 4096 + 40 the items 0, 1, 3 and 5 keep nothing."""
    rs = np.random.RandomState(1002)
    w = (rs.standard_normal(20481) * 1e-3).astype(np.float32)
    w[2 * CHUNK:3 * CHUNK] = np.where(rs.rand(CHUNK) < 0.5, np.float32(8), np.float32(-8))
    pos = 4 * CHUNK + rs.permutation(CHUNK)[:40]
    w[pos] = np.where(rs.rand(40) < 0.5, np.float32(4), np.float32(-4))
    return w, CHUNK + 40


def special_input():
    """n = 5000: signed zeros on the first 3,000, subnormals of both signs on the next 1,000, N(0, 1) on the rest with +-inf on
    three elements and NaNs (both signs, a signalling one) on three."""
    rs = np.random.RandomState(1003)
    b = np.zeros(5000, np.uint32)
    b[:3000] = tc._signs(rs, 3000)
    b[3000:4000] = rs.randint(1, 0x800000, size=1000).astype(np.uint32) | tc._signs(rs, 1000)
    b[4000:] = bits(rs.standard_normal(1000).astype(np.float32))
    b[[4100, 4200, 4300]] = [0x7f800000, 0xff800000, 0x7f800000]
    b[[4400, 4500, 4600]] = [0x7fc00000, 0xffc00001, 0xff800123]
    return from_bits(b)


def special_cases():
    """[(name, w, k)]: the special input with its NaNs and infs kept or dropped; without them (finite mu) down to the subnormals and
    the zeros."""
    w = special_input()
    fin = w.copy()
    fin[[4100, 4200, 4300, 4400, 4500, 4600]] = np.float32(0.5)
    out = [("k%d" % k, w, k) for k in (2, 3, 5, 6, 1500)]
    out += [("finite_k%d" % k, fin, k) for k in (900, 1500, 3500)]
    sub = from_bits(bits(fin) & np.uint32(0x807fffff))      # every exponent cleared: nothing but subnormals and zeros
    out.append(("subnormal_mu", sub, 64))
    inf = w.copy()
    inf[[4400, 4500, 4600]] = np.float32(1.0)
    out.append(("inf_mu", inf, 2))      # two of the three infinities kept, no NaN: mu = +inf
    return out


def exact_input(n, seed):
    """Multiples of 2^-10 below 64 in magnitude: every partial sum of up to 2^20 of them is exact in float64 whatever the order."""
    rs = np.random.RandomState(seed)
    return (rs.randint(-65535, 65536, size=n) / 1024.0).astype(np.float32)


def hand_sections(n, k, R, seed):
    """R sections never written by a compress: payload r names k distinct indices (r % 3 == 2: all inside ONE item where k fits)
    with random signs and a magnitude of its own; payload 1 repeats payload 0's indices with the signs flipped and the SAME magnitude
    (the sum is +0 there)."""
    rs = np.random.RandomState(seed)
    nit = items_of(n)
    secs, named = [], []
    for r in range(R):
        if r == 1:
            idx, sg, mu = named[0][0], 1 - named[0][1], named[0][2]
        else:
            pool = np.arange(n)
            if r % 3 == 2:
                full = [t for t in range(nit) if min(n, (t + 1) * CHUNK) - t * CHUNK >= k]
                if full:
                    t = full[r % len(full)]
                    pool = np.arange(t * CHUNK, min(n, (t + 1) * CHUNK))
            idx = np.sort(rs.choice(pool, k, replace=False))
            sg = (rs.rand(k) < 0.5).astype(np.uint16)
            mu = np.array([abs(rs.standard_normal()) * 10.0 ** rs.randint(-3, 4)], np.float32).view(np.uint32)[0]
        named.append((idx, sg, mu))
        secs.append(build_section(n, k, mu, idx, sg))
    return secs, named


LIE_N, LIE_K = 8193, 64


def lying_section():
    """A section of n = 8,193 (three items), k = 64 whose header claims k = 2^32 - 1, whose start[1] is 2^32 - 1 and start[2] = 3 (below
    its predecessor), and whose first word names position 32,767.  The positions of the other 63 words are distinct, so item 0 -- which
    now owns all 64 -- has a defined decode; items 1 and 2 get nothing."""
    idx = np.concatenate([np.arange(32) * 128, CHUNK + np.arange(32) * 128 + 1])
    sec = build_section(LIE_N, LIE_K, np.uint32(0x3f800000), idx, np.arange(LIE_K) % 2)
    head = sec[:HEADER + 12].view(np.uint32)
    head[0], head[5], head[6] = 0xffffffff, 0xffffffff, 3
    sec[HEADER + 12:HEADER + 14] = np.array([0x7fff], np.uint16).view(np.uint8)
    return sec
