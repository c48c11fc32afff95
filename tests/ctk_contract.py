"""The contract of include/gq_ctk.h restated in numpy with integer and float32 arithmetic only (no GPU, no call into gq_amd), and the
inputs its tests share.  The key, the ranking and w = f32(v + f32(s * err)) are tests/topk_contract.py's -- the header takes them from
include/gq_topk.h word for word; what is restated here is the per-item kept set, the wire without a header, and the decode-mean.
tests/test_ctk_contract.py checks this file against independent witnesses; tests/test_gpu_zz_ctk_contract.py holds the kernels to it."""
import numpy as np

import topk_contract as tc

CHUNK = 4096
SIZES = lambda cr: [1, cr - 1, cr, 4095, 4096, 4097, 2 * 4096 + cr + 1]      # noqa: E731
CRS = [2, 16, 256, 4096]
up16 = lambda x: (x + 15) // 16 * 16      # noqa: E731


def kept_count(n, cr):
    return (n // CHUNK) * (CHUNK // cr) + (n % CHUNK) // cr


def section_size(n, cr):
    return up16(2 * kept_count(n, cr)) + up16(4 * kept_count(n, cr))


def kept(w, cr):
    """-> (the kept elements' indices in the tensor, ascending; their positions inside their items)."""
    w = tc.f32(w)
    idx = [b + tc.kept(w[b:b + CHUNK], w[b:b + CHUNK].size // cr) for b in range(0, w.size, CHUNK)]
    idx = np.concatenate(idx).astype(np.int64)
    return idx, (idx % CHUNK).astype(np.uint16)


def section_bytes(w, cr):
    idx, pos = kept(w, cr)
    sec = np.zeros(section_size(tc.f32(w).size, cr), np.uint8)
    sec[:2 * idx.size] = pos.view(np.uint8)
    sec[up16(2 * idx.size):up16(2 * idx.size) + 4 * idx.size] = tc.f32(w)[idx].view(np.uint8)
    return sec


def dense(w, cr):
    mask = np.zeros(tc.f32(w).size, np.float32)
    mask[kept(w, cr)[0]] = 1
    with np.errstate(invalid="ignore"):
        return tc.f32(w) * mask


def error_feedback(v, err, s, cr):
    """-> (w, dense(w), the new err = f32(w - dense)); the new v is w."""
    w = tc.feedback(v, err, s)
    D = dense(w, cr)
    with np.errstate(invalid="ignore"):
        return w, D, (w - D).astype(np.float32)


def decode_mean(sections, n, cr, plain=False):
    """sections: R byte arrays.  A float32 accumulator at +0, the payloads added in order (a position not below its item's length is
    skipped), then acc / f32(R), a true division; plain with R == 1: the values as they are."""
    K, kf, R = kept_count(n, cr), CHUNK // cr, len(sections)
    acc = np.zeros(n, np.float32)
    for sec in sections:
        pos = sec[:2 * K].view(np.uint16).astype(np.int64)
        val = sec[up16(2 * K):up16(2 * K) + 4 * K].view(np.float32)
        item = np.minimum(np.arange(K) // kf, n // CHUNK)      # (the short last item's entries follow the full items')
        ok = pos < np.minimum(CHUNK, n - item * CHUNK)
        at = (item * CHUNK + pos)[ok]
        with np.errstate(invalid="ignore", over="ignore"):
            acc[at] = val[ok] if plain and R == 1 else (acc[at] + val[ok]).astype(np.float32)
    if plain and R == 1:
        return acc
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc / np.float32(R)).astype(np.float32)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
KINDS = ["gauss", "student", "equal", "low7", "special"]
SPECIALS = tc.from_bits(np.array([0, 1 << 31, 1, 0x80000001, 0x007fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001], np.uint32))


def make(kind, n, seed):
    """gauss, student: ordinary and heavy-tailed (tie-free where a test asserts it); equal: every element a tie; low7: keys that differ in their last 7 bits alone; special:
    +-0, subnormals, +-inf and NaNs on one element in eight of a Gaussian."""
    rs = np.random.RandomState(seed)
    if kind == "equal":
        return tc.all_equal(n, seed)
    if kind == "low7":
        return tc.from_bits(np.uint32(tc.ONE) | rs.randint(0, 128, n).astype(np.uint32) | tc._signs(rs, n))
    w = (rs.standard_t(3, n) if kind == "student" else rs.standard_normal(n)).astype(np.float32)
    if kind == "special":
        hit = rs.rand(n) < 0.125
        w[hit] = SPECIALS[rs.randint(0, SPECIALS.size, int(hit.sum()))]
    return w


TIE_CR, TIE_LASTS = 16, [255, 259, 1023, 1027]      # the last kept tie in front of a wave seam, a lane seam, a register-step seam, behind one


def tie_input(last):
    """One item, k = 256: 2.0 on 10 elements in front and 90 behind, +-1.0 on the 196 elements last - 155 ... last + 40, 0.5 elsewhere:
    need = 156 of 196 ties, the last kept one at `last`."""
    rs = np.random.RandomState(last)
    b = np.full(CHUNK, 0x3f000000, np.uint32)
    b[:10] = b[4000:4090] = 0x40000000
    b[last - 155:last + 41] = tc.ONE
    return tc.from_bits(b | tc._signs(rs, CHUNK))


def hand_sections(n, cr, R, seed):
    """R payloads of random distinct positions per item (not ascending: the decode may not rely on it) and Gaussian values with -0, inf and
    a NaN among them; in every payload the first entry of every item names a position beyond the item's length."""
    rs = np.random.RandomState(seed)
    K, kf = kept_count(n, cr), CHUNK // cr
    secs = []
    for r in range(R):
        pos = np.concatenate([rs.permutation(min(CHUNK, n - b))[:min(CHUNK, n - b) // cr] for b in range(0, n, CHUNK)]).astype(np.uint16)
        val = rs.standard_normal(K).astype(np.float32)
        val[rs.rand(K) < 0.1] = SPECIALS[[1, 5, 7]][r % 3]
        pos[::kf] = 4096 + r                      # (skipped: not below the item's length)
        if (n % CHUNK) // cr:
            pos[(n // CHUNK) * kf] = n % CHUNK    # (the short item's: its own length, below 4,096)
        sec = np.zeros(section_size(n, cr), np.uint8)
        sec[:2 * K] = pos.view(np.uint8)
        sec[up16(2 * K):up16(2 * K) + 4 * K] = val.view(np.uint8)
        secs.append(sec)
    return secs
