"""The contract of include/gq_eden.h restated in numpy (no GPU, no tolerance anywhere) on top of tests/mxr_contract.py's transform and
tests/drive_contract.py's tree, layout and inputs, and the inputs the contract tests share (tests/test_eden_contract.py checks the
restatement on the CPU, tests/test_gpu_zz_eden_contract.py holds the kernels to it).  One float32 operation at a time, in the
header's own words.  The table is a parameter: with the one-magnitude table (c = [1], no thresholds) the restatement is DRIVE's."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402
import mxr_contract as mxr  # noqa: E402
import drive_contract as dc  # noqa: E402

f32, U32 = np.float32, np.uint32
BLOCK = dc.BLOCK
ITEM = dc.ITEM
UNBIASED, MSE = 0, 1
MODES = {"unbiased": UNBIASED, "mse": MSE}
BITS = (2, 3, 4)
SEEDED = dc.SEEDED
SIGN_SETS = dc.SIGN_SETS
tree_sum, sequential_sum, reversed_tree_sum = dc.tree_sum, dc.sequential_sum, dc.reversed_tree_sum
pad_blocks, rel_l2 = dc.pad_blocks, dc.rel_l2

# include/gq_eden.h's TABLES, by their bit patterns
C_BITS = {
    2: [0x3ee7d2c9, 0x3fc1555d],
    3: [0x3e7af9f8, 0x3f418990, 0x3fac0538, 0x4009b97a],
    4: [0x3e0379fd, 0x3ec6ae44, 0x3f28215e, 0x3f713d39, 0x3fa0cc2f, 0x3fcf1c25, 0x40046ac7, 0x402ee2bf],
}
T_BITS = {
    2: [0x3f7b4a0f],
    3: [0x3f002407, 0x3f866500, 0x3fdfbc17],
    4: [0x3e8435a1, 0x3f05bc40, 0x3f4caf4b, 0x3f8cb566, 0x3fb7f42a, 0x3febf8da, 0x4019a6c3],
}


class Table(object):
    """bits, the magnitudes c [L] and the thresholds t [L - 1] (float32)."""

    def __init__(self, bits, c, t):
        self.bits, self.c, self.t = bits, np.asarray(c, f32), np.asarray(t, f32)
        assert self.c.size == 1 << (bits - 1) and self.t.size == self.c.size - 1

    @property
    def code_bytes(self):
        return BLOCK * self.bits // 8


TABLES = {b: Table(b, mx.from_bits(np.array(C_BITS[b], U32)), mx.from_bits(np.array(T_BITS[b], U32))) for b in BITS}
DRIVE_TABLE = Table(1, [1.0], [])      # one magnitude: the sign alone -- include/gq_drive.h


def section_bytes(n, bits):
    nb = -(-n // BLOCK)
    return nb * (BLOCK * bits // 8) + mx._up(4 * nb)


def spread(Q):
    """sigma = sqrtf(Q * 2^-8): one multiplication, one correctly rounded square root."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.sqrt((np.asarray(Q, f32) * f32(2.0 ** -8)).astype(f32)).astype(f32)


def spread_sqrt_first(Q):
    """What the kernels must NOT compute: sqrtf(Q) / 16 -- the same number wherever Q * 2^-8 does not underflow."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (np.sqrt(np.asarray(Q, f32)).astype(f32) / f32(16.0)).astype(f32)


def thresholds(sigma, tab):
    """theta [nb, L - 1] = t_i * sigma, one multiplication each."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (tab.t[None, :] * np.asarray(sigma, f32)[:, None]).astype(f32)


def magnitudes(xp, tab, tree=tree_sum, ge=False, spread_fn=spread):
    """x' [nb, 256] -> (m uint32 [nb, 256], Q [nb], sigma [nb]): m_j = the number of i with |x'_j| > theta_i (strictly)."""
    xp = np.asarray(xp, f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a = (mx.bits_of(xp) & U32(0x7fffffff)).view(f32)
        Q = tree((xp * xp).astype(f32))
        sigma = spread_fn(Q)
        th = thresholds(sigma, tab)
        m = np.zeros(xp.shape, U32)
        for i in range(tab.t.size):
            m += ((a >= th[:, i:i + 1]) if ge else (a > th[:, i:i + 1])).astype(U32)
    return m, Q, sigma


def products_fused(a, c, tree):
    """What the kernels must NOT compute: P with the products of the odd elements fused into level 0 of the tree (an fma)."""
    p = (a * c).astype(f32)
    lvl0 = (a[:, 0::2].astype(np.float64) * c[:, 0::2].astype(np.float64) + p[:, 1::2].astype(np.float64)).astype(f32)
    return tree(np.repeat(lvl0, 2, axis=1) * np.tile(np.array([1, 0], f32), 128)[None, :])


def scales(xp, m, Q, tab, mode, tree=tree_sum, fused=False):
    """S float32 [nb] (and P, C2): |x'| * c_m and c_m * c_m through the tree, ONE division."""
    xp = np.asarray(xp, f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        a = (mx.bits_of(xp) & U32(0x7fffffff)).view(f32)
        c = tab.c[m]
        P = products_fused(a, c, tree) if fused else tree((a * c).astype(f32))
        C2 = tree((c * c).astype(f32))
        S = (Q / P).astype(f32) if mode == UNBIASED else (P / C2).astype(f32)
    S = np.where(P == 0, f32(0), S).astype(f32)
    return np.where(np.isfinite(P), S, mx.from_bits([mx.QNAN])[0]).astype(f32), P, C2


def codes_of(xp, m, tab):
    """code_j = m_j | sign bit << (b - 1)"""
    return (m | ((mx.bits_of(xp) >> U32(31)) << U32(tab.bits - 1))).astype(U32)


def pack(codes, S, bits):
    """Codes [nb, 256] and scales [nb] -> the section: element j owns bits b j ... b j + b - 1 of the block's little-endian string."""
    nb = codes.shape[0]
    cb = BLOCK * bits // 8
    planes = ((codes[:, :, None] >> np.arange(bits, dtype=U32)[None, None, :]) & U32(1)).astype(np.uint8).reshape(nb, BLOCK * bits)
    by = np.packbits(planes, axis=1, bitorder="little")
    assert by.shape == (nb, cb)
    sec = np.zeros(section_bytes(nb * BLOCK, bits), np.uint8)
    sec[:nb * cb] = by.reshape(-1)
    sec[nb * cb:nb * cb + 4 * nb] = np.ascontiguousarray(S, f32).view(np.uint8)
    return sec


def unpack(sec, n, bits):
    nb = -(-n // BLOCK)
    cb = BLOCK * bits // 8
    sec = np.asarray(sec, np.uint8)
    assert sec.size == section_bytes(n, bits)
    planes = np.unpackbits(sec[:nb * cb].reshape(nb, cb), axis=1, bitorder="little").reshape(nb, BLOCK, bits).astype(U32)
    codes = (planes << np.arange(bits, dtype=U32)[None, None, :]).sum(axis=2).astype(U32)
    S = sec[nb * cb:nb * cb + 4 * nb].copy().view(f32)
    return codes, S


def values(codes, S, tab):
    """y [nb, 256] = (S * c_m), one multiplication, with its sign bit xor-ed with the code's sign bit."""
    b = tab.bits
    m = codes & U32((1 << (b - 1)) - 1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        y = (np.asarray(S, f32)[:, None] * tab.c[m]).astype(f32)
    return (mx.bits_of(y) ^ ((codes >> U32(b - 1)) << U32(31))).view(f32)


def compress(g, bits, mode, signs, err=None, ef_scale=None, tree=tree_sum, table=None, ge=False, spread_fn=spread, fused=False):
    """One tensor -> (section uint8, D float32 [n], w, err afterwards or None, x' [nb, 256], S [nb], codes [nb, 256])."""
    tab = table or TABLES[bits]
    g = np.asarray(g, f32).reshape(-1)
    n, w = g.size, g
    if err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            p = (f32(ef_scale) * np.asarray(err, f32)).astype(f32)
            w = (g + p).astype(f32)
    xp = mxr.forward_blocks(pad_blocks(w), signs)
    m, Q, _ = magnitudes(xp, tab, tree, ge, spread_fn)
    S, _, _ = scales(xp, m, Q, tab, mode, tree, fused)
    codes = codes_of(xp, m, tab)
    D = mxr.inverse_blocks(values(codes, S, tab), signs).reshape(-1)[:n]
    new_err = None
    if err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            new_err = (w - D).astype(f32)
    return pack(codes, S, tab.bits), D, w, new_err, xp, S, codes


def mean_rotated(sections, n, bits, plain=False):
    """m [nb, 256]: the mean in the rotated domain (+0 start, payloads ascending, a true division; plain: payload 0 as it is)."""
    ys = [values(*unpack(s, n, bits), TABLES[bits]) for s in sections]
    if plain:
        assert len(ys) == 1
        return ys[0]
    acc = np.zeros_like(ys[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for y in ys:
            acc = (acc + y).astype(f32)
        return (acc / f32(len(ys))).astype(f32)


def decode_mean(sections, n, bits, signs, plain=False):
    """The mean in the rotated domain, then ONE inverse transform."""
    return mxr.inverse_blocks(mean_rotated(sections, n, bits, plain), signs).reshape(-1)[:n]


def loose_blocks(xp, S):
    """bool [nb] twice: the blocks whose NaNs the contract leaves to the hardware -- an x' that is not finite (codes, S and the
    decode), or S = +inf (the decode only)."""
    return dc.loose_blocks(xp, S)


def layout(sizes, bits, dense_sizes=()):
    """Wire offsets as the quantizer lays them out: 16-byte aligned sections, then the identity-compressed tensors' f32."""
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off = mx._up(off + section_bytes(n, bits))
    dense = []
    for n in dense_sizes:
        dense.append((off, n))
        off += 4 * n
    return offs, dense, mx._up(off)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
gaussian, student = dc.gaussian, dc.student
SIZES = [1, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 2 * 4096 + 257]      # block, step and item seams; the longest: two items and a block and a bit


def tiny(n, seed):
    """Around 2^-72: the squares are subnormals of a few bits, Q is about 2^-136 and Q * 2^-8 keeps five bits or so -- the one
    place where sqrtf(Q * 2^-8) and sqrtf(Q) / 16 differ (and where a Q that underflows to 0 with P > 0 sits next door)."""
    return np.ldexp(np.random.RandomState(seed).randn(n), -72).astype(f32)


FINITE_KINDS = dict(dc.FINITE_KINDS, tiny=tiny)


def mixed(n, seed):
    """One tensor with every finite kind in it, a block of each where n allows (kinds change at multiples of 256)."""
    kinds = [FINITE_KINDS[k] for k in sorted(FINITE_KINDS)]
    out = gaussian(n, seed)
    for b in range(-(-n // BLOCK)):
        lo, hi = b * BLOCK, min(n, (b + 1) * BLOCK)
        out[lo:hi] = kinds[(b + seed) % len(kinds)](hi - lo, seed + b)
    return out


nonfinite = dc.nonfinite

SEARCH_SEED, SEARCH_COORDS, SEARCH_CHUNK = 2022, 1 << 25, 1 << 20


@functools.lru_cache(maxsize=None)
def on_threshold_blocks():
    """The fixed-seed search: SEARCH_COORDS rotated coordinates of N(0, 1) * 1e-3 blocks under the seeded signs, looking for an
    |x'_j| that sits exactly on a theta_i -> {bits: (inputs float32 [k, 256], how many coordinates sat on a threshold)}.  Such an
    element tells `>` from `>=`."""
    rs = np.random.RandomState(SEARCH_SEED)
    found = {b: [] for b in BITS}
    count = {b: 0 for b in BITS}
    for _ in range(SEARCH_COORDS // SEARCH_CHUNK):
        w = (rs.randn(SEARCH_CHUNK // BLOCK, BLOCK) * 1e-3).astype(f32)
        xp = mxr.forward_blocks(w, SEEDED)
        a = np.abs(xp)
        sigma = spread(tree_sum((xp * xp).astype(f32)))
        for b in BITS:
            th = thresholds(sigma, TABLES[b])
            hit = np.zeros(a.shape, bool)
            for i in range(th.shape[1]):
                hit |= a == th[:, i:i + 1]
            count[b] += int(hit.sum())
            for k in np.flatnonzero(hit.any(axis=1)):
                found[b].append(w[k].copy())
    return {b: (np.array(found[b], f32).reshape(-1, BLOCK), count[b]) for b in BITS}


def on_threshold_tensor(bits):
    """The blocks the search found for `bits`, one after another (a Gaussian block where it found none: the assertion on the
    count is tests/test_eden_contract.py's)."""
    blocks = on_threshold_blocks()[bits][0]
    return blocks.reshape(-1).copy() if blocks.size else gaussian(BLOCK, 1)


KIND_SIZES = [ITEM + 300, 257, 77]


def gpu_inputs(bits):
    """The finite inputs of tests/test_gpu_zz_eden_contract.py's compress cases: name -> tensors."""
    d = {"sizes": [mixed(n, 100 + n) for n in SIZES], "on_threshold": [on_threshold_tensor(bits)]}
    for kind in sorted(FINITE_KINDS):
        d["kind_" + kind] = [FINITE_KINDS[kind](n, 500 + n) for n in KIND_SIZES]
    return d


def payloads(n, bits, R, seed):
    """R hand-built sections of n elements for the decode-mean.  The codes of block 0 walk through every code value at every one of
    a lane's eight positions (element j of payload r: (j + j // 8 + r) mod 2^b, so a lane's b bytes hold eight different codes
    and all 2^b appear at every bit position over the lanes), the others are random; scales that make the sums round, with a
    block of S = 0 (-0 is not a scale a compress writes, it is read as it is), a subnormal S, 2^100, inf, and a NaN S in payload
    0's last block; in block 1 payload 1 = payload 0 with every sign flipped: the sums cancel to +0 (+0 + y + -y), and to -0
    nowhere."""
    rs = np.random.RandomState(seed)
    nb = -(-n // BLOCK)
    j = np.arange(BLOCK)
    secs = []
    for r in range(R):
        codes = rs.randint(0, 1 << bits, (nb, BLOCK)).astype(U32)
        codes[0] = ((j + j // 8 + r) % (1 << bits)).astype(U32)
        S = np.ldexp(rs.rand(nb) + 0.5, rs.randint(-20, 4, nb)).astype(f32)
        special = [f32(0), mx.from_bits([0x00000123])[0], f32(2.0 ** 100), mx.from_bits([0x80000000])[0], f32(np.inf)]
        for b in range(2, nb):
            if (b + r) % 5 == 3:
                S[b] = special[(b // 5 + r) % len(special)]
        if r == 0:
            S[-1] = np.nan
        if r == 1 and nb > 1:
            c0, S0 = unpack(secs[0], n, bits)
            codes[1], S[1] = c0[1] ^ U32(1 << (bits - 1)), S0[1]
        secs.append(pack(codes, S, bits))
    return secs
