"""PACKED16 of include/gq_ctk.h restated in numpy, int64 arithmetic, on top of tests/ctk_contract.py's select (no GPU, no call into gq_amd):
the levels, the section's bytes, the dense decode, the error-feedback step and the decode-mean.  tests/test_ctk_packed_contract.py checks
what the format promises; tests/test_gpu_zz_ctk_packed_contract.py holds the kernels to this file."""
import numpy as np

import ctk_contract as cc
import topk_contract as tc

CHUNK = cc.CHUNK
M32 = (1 << 32) - 1


def items_of(n):
    return -(-n // CHUNK)


def section_size(n, cr):
    return cc.up16(8 * items_of(n)) + cc.up16(2 * cc.kept_count(n, cr))


def quantise(k, T, H):
    """-> (level, decoded key) of keys k between the bounds T <= H."""
    k, T, D = np.asarray(k, np.int64), int(T), int(H) - int(T)
    lev = np.zeros(k.shape, np.int64) if D == 0 else ((k - T) * 14 + D) // (2 * D)
    return lev, T + (lev * D + 3) // 7


def encode(w, cr):
    """-> (bounds uint32 [items, 2], words uint16 [K], the dense decode f32 [n], the kept elements' indices)."""
    w = tc.f32(w)
    idx, pos = cc.kept(w, cr)
    ky, sign = tc.keys(w).astype(np.int64), (tc.bits(w) >> 31).astype(np.int64)
    with np.errstate(invalid="ignore"):
        dec = w * np.float32(0)
    bounds, words = np.zeros((items_of(w.size), 2), np.uint32), np.zeros(idx.size, np.uint16)
    for t in np.unique(idx // CHUNK):
        mine = idx // CHUNK == t
        e = idx[mine]
        T, H = ky[e].min(), ky[t * CHUNK:(t + 1) * CHUNK].max()
        lev, dk = quantise(ky[e], T, H)
        bounds[t] = T, H
        words[mine] = pos[mine].astype(np.int64) | lev << 12 | sign[e] << 15
        dec[e] = tc.from_bits((dk | sign[e] << 31).astype(np.uint32))
    return bounds, words, dec, idx


def section_bytes(w, cr):
    bounds, words, _, _ = encode(w, cr)
    sec = np.zeros(section_size(tc.f32(w).size, cr), np.uint8)
    sec[:bounds.size * 4] = bounds.reshape(-1).view(np.uint8)
    at = cc.up16(bounds.size * 4)
    sec[at:at + 2 * words.size] = words.view(np.uint8)
    return sec


def dense(w, cr):
    return encode(w, cr)[2]


def error_feedback(v, err, s, cr):
    """-> (w, dense(w), the new err = f32(w - dense)); the new v is w."""
    w = tc.feedback(v, err, s)
    D = dense(w, cr)
    with np.errstate(invalid="ignore"):
        return w, D, (w - D).astype(np.float32)


def as_f32_section(sec, n, cr):
    """The PACKED16 section as the f32 format's (pos[K], value[K]): what cc.decode_mean adds.  D = H - T in uint32 arithmetic."""
    K, kf = cc.kept_count(n, cr), CHUNK // cr
    bounds = sec[:8 * items_of(n)].view(np.uint32).astype(np.int64).reshape(-1, 2)
    at = cc.up16(8 * items_of(n))
    word = sec[at:at + 2 * K].view(np.uint16).astype(np.int64)
    item = np.minimum(np.arange(K) // kf, n // CHUNK)
    T, D = bounds[item, 0], (bounds[item, 1] - bounds[item, 0]) & M32
    dk = (T + ((word >> 12 & 7) * D + 3) // 7) & M32
    out = np.zeros(cc.section_size(n, cr), np.uint8)
    out[:2 * K] = (word & 0xfff).astype(np.uint16).view(np.uint8)
    out[cc.up16(2 * K):cc.up16(2 * K) + 4 * K] = (dk | (word >> 15) << 31).astype(np.uint32).view(np.uint8)
    return out


def decode_mean(sections, n, cr, plain=False):
    return cc.decode_mean([as_f32_section(s, n, cr) for s in sections], n, cr, plain=plain)


def hand_sections(n, cr, R, seed):
    """R payloads, never the output of a compress: distinct random positions per item in no order, random levels and signs, bounds
    T <= H that differ from item to item and from payload to payload (every third item T == H).  The short last item's first entry
    names the item's own length -- the one position 12 bits can hold that is not below it: skipped."""
    rs = np.random.RandomState(seed)
    K, secs = cc.kept_count(n, cr), []
    for r in range(R):
        pos = np.concatenate([rs.permutation(min(CHUNK, n - b))[:min(CHUNK, n - b) // cr] for b in range(0, n, CHUNK)]).astype(np.int64)
        if (n % CHUNK) // cr:
            pos[(n // CHUNK) * (CHUNK // cr)] = n % CHUNK
        T = rs.randint(0x30000000, 0x3f000000, items_of(n)).astype(np.int64)
        H = T + rs.randint(0, 0x01000000, items_of(n)) * (np.arange(items_of(n)) % 3 != 1)
        sec = np.zeros(section_size(n, cr), np.uint8)
        sec[:8 * items_of(n)] = np.stack([T, H], 1).astype(np.uint32).reshape(-1).view(np.uint8)
        at = cc.up16(8 * items_of(n))
        sec[at:at + 2 * K] = (pos | rs.randint(0, 8, K) << 12 | rs.randint(0, 2, K) << 15).astype(np.uint16).view(np.uint8)
        secs.append(sec)
    return secs
