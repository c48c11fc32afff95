"""The contract of include/gq_drive.h restated in numpy (no GPU, no tolerance anywhere) on top of tests/mxr_contract.py's transform,
and the inputs the contract tests share (tests/test_drive_contract.py checks the restatement on the CPU,
tests/test_gpu_zz_drive_contract.py holds the kernels to it).  One float32 operation at a time, in the header's own words: the sums
are the balanced tree over the whole block, not the kernel's split into lanes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402
import mxr_contract as mxr  # noqa: E402

f32, U32 = np.float32, np.uint32
BLOCK = 256
ITEM = mx.ITEM
UNBIASED, MSE = 0, 1
MODES = {"unbiased": UNBIASED, "mse": MSE}
CODE_BYTES = BLOCK // 8
SEEDED = mxr.SEEDED
SIGN_SETS = {"zero": mxr.ZERO_SIGNS, "seeded": mxr.SEEDED, "seed2": mxr.sign_words(2)}
SIZES = [1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8193]


def section_bytes(n):
    nb = -(-n // BLOCK)
    return nb * CODE_BYTES + mx._up(4 * nb)


def pad_blocks(w):
    """A flat tensor -> float32 [nb, 256], the last block filled with +0."""
    w = np.asarray(w, f32).reshape(-1)
    nb = -(-w.size // BLOCK)
    p = np.zeros(nb * BLOCK, f32)
    p[:w.size] = w
    return p.reshape(nb, BLOCK)


def tree_sum(v):
    """[nb, 256] -> [nb]: level t = 0 ... 7 replaces neighbours at stride 2^t by their one float32 sum."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(8):
            v = (v[:, 0::2] + v[:, 1::2]).astype(f32)
    return v[:, 0]


def sequential_sum(v):
    """What the kernels must NOT compute: the elements added one after another in index order."""
    v = np.asarray(v, f32)
    acc = np.zeros(v.shape[0], f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(v.shape[1]):
            acc = (acc + v[:, j]).astype(f32)
    return acc


def reversed_tree_sum(v):
    """Nor this: the tree with the strides descending (level t adds the elements 2^(7-t) apart)."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(8):
            h = v.shape[1] // 2
            v = (v[:, :h] + v[:, h:]).astype(f32)
    return v[:, 0]


def scales(xp, mode, tree=tree_sum):
    """x' [nb, 256] -> S float32 [nb] (and L1, Q): |x'| and x' * x' through the tree, ONE division."""
    xp = np.asarray(xp, f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        a = (mx.bits_of(xp) & U32(0x7fffffff)).view(f32)
        q = (xp * xp).astype(f32)
        L1, Q = tree(a), tree(q)
        S = (Q / L1).astype(f32) if mode == UNBIASED else (L1 / f32(256.0)).astype(f32)
    S = np.where(L1 == 0, f32(0), S).astype(f32)
    return np.where(np.isfinite(L1), S, mx.from_bits([mx.QNAN])[0]).astype(f32), L1, Q


def code_bits(xp):
    """x' [nb, 256] -> uint32 [nb, 256]: the IEEE sign bit."""
    return mx.bits_of(xp) >> U32(31)


def pack(bits, S):
    """Code bits [nb, 256] and scales [nb] -> the section (element j: bit j & 7 of byte j >> 3; f32 scales; zero pad)."""
    nb = bits.shape[0]
    codes = np.packbits(bits.astype(np.uint8), axis=1, bitorder="little")
    assert codes.shape == (nb, CODE_BYTES)
    sec = np.zeros(section_bytes(nb * BLOCK), np.uint8)
    sec[:nb * CODE_BYTES] = codes.reshape(-1)
    sec[nb * CODE_BYTES:nb * CODE_BYTES + 4 * nb] = np.ascontiguousarray(S, f32).view(np.uint8)
    return sec


def unpack(sec, n):
    nb = -(-n // BLOCK)
    sec = np.asarray(sec, np.uint8)
    assert sec.size == section_bytes(n)
    bits = np.unpackbits(sec[:nb * CODE_BYTES].reshape(nb, CODE_BYTES), axis=1, bitorder="little").astype(U32)
    S = sec[nb * CODE_BYTES:nb * CODE_BYTES + 4 * nb].copy().view(f32)
    return bits, S


def values(bits, S):
    """y [nb, 256]: S of the block with its sign bit xor-ed with the code."""
    return (mx.bits_of(S)[:, None] ^ (bits.astype(U32) << U32(31))).view(f32)


def compress(g, mode, signs, err=None, ef_scale=None, tree=tree_sum):
    """One tensor -> (section uint8, D float32 [n], w, err afterwards or None, x' [nb, 256], S [nb])."""
    g = np.asarray(g, f32).reshape(-1)
    n, w = g.size, g
    if err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            p = (f32(ef_scale) * np.asarray(err, f32)).astype(f32)
            w = (g + p).astype(f32)
    xp = mxr.forward_blocks(pad_blocks(w), signs)
    S, _, _ = scales(xp, mode, tree)
    bits = code_bits(xp)
    D = mxr.inverse_blocks(values(bits, S), signs).reshape(-1)[:n]
    new_err = None
    if err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            new_err = (w - D).astype(f32)
    return pack(bits, S), D, w, new_err, xp, S


def mean_rotated(sections, n, plain=False):
    """m [nb, 256]: the mean in the rotated domain (+0 start, payloads ascending, a true division; plain: payload 0 as it is)."""
    ys = [values(*unpack(s, n)) for s in sections]
    if plain:
        assert len(ys) == 1
        return ys[0]
    acc = np.zeros_like(ys[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for y in ys:
            acc = (acc + y).astype(f32)
        return (acc / f32(len(ys))).astype(f32)


def decode_mean(sections, n, signs, plain=False):
    """The mean in the rotated domain, then ONE inverse transform."""
    return mxr.inverse_blocks(mean_rotated(sections, n, plain), signs).reshape(-1)[:n]


def decode_mean_inverse_first(sections, n, signs):
    """What the kernels must NOT compute: every payload rotated back, then the mean."""
    acc = np.zeros(n, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in sections:
            acc = (acc + decode_mean([s], n, signs, plain=True)).astype(f32)
        return (acc / f32(len(sections))).astype(f32)


def loose_blocks(xp, S):
    """bool [nb]: the blocks whose NaNs the contract leaves to the hardware -- an x' that is not finite (code bits, S and the
    decode), or S = +inf (the decode only)."""
    return ~np.isfinite(np.asarray(xp)).all(axis=1), ~np.isfinite(np.asarray(S))


def layout(sizes, dense_sizes=()):
    """Wire offsets as the quantizer lays them out: 16-byte aligned sections, then the identity-compressed tensors' f32."""
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off = mx._up(off + section_bytes(n))
    dense = []
    for n in dense_sizes:
        dense.append((off, n))
        off += 4 * n
    return offs, dense, mx._up(off)


def rel_l2(a, b):
    return mxr.rel_l2(a, b)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def gaussian(n, seed):
    return (np.random.RandomState(seed).randn(n) * 1e-3).astype(f32)


def student(n, seed):
    return (np.random.RandomState(seed).standard_t(3, n) * 1e-3).astype(f32)


def zeros_mixed(n, seed):
    """+-0 only: L1 == 0, S = +0, and the code bits are the signs IEEE gives the sums of zeros."""
    z = np.zeros(n, f32)
    z[np.random.RandomState(seed).rand(n) < 0.5] = f32(-0.0)
    return z


def subnormals(n, seed):
    """Subnormals and +-0: x' * 2^-4 rounds onto the 2^-149 grid, Q underflows to 0 (S = +0 unbiased, L1 / 256 > 0 or 0 mse)."""
    rs = np.random.RandomState(seed)
    v = mx.from_bits(rs.randint(0, 1 << 12, n).astype(U32) | (U32(1 << 31) * rs.randint(0, 2, n).astype(U32))).copy()
    v[::7] = 0
    return v


def huge(n, seed):
    """Around 2^63: every stage and L1 stay finite, the tree of Q overflows -- S = +inf in the unbiased mode, finite in mse."""
    return np.ldexp(np.random.RandomState(seed).randn(n), 63).astype(f32)


FINITE_KINDS = {"gaussian": gaussian, "student": student, "zeros": zeros_mixed, "subnormals": subnormals, "huge": huge}


def mixed(n, seed):
    """One tensor with every finite kind in it, a block of each where n allows (kinds change at multiples of 256)."""
    kinds = list(FINITE_KINDS.values())
    out = gaussian(n, seed)
    for b in range(-(-n // BLOCK)):
        lo, hi = b * BLOCK, min(n, (b + 1) * BLOCK)
        out[lo:hi] = kinds[(b + seed) % len(kinds)](hi - lo, seed + b)
    return out


def nonfinite(n=4 * BLOCK + 100):
    """One inf in a middle block and one NaN in the padded last block; the blocks between stay finite -> (w, bad blocks)."""
    w = gaussian(n, 77)
    w[BLOCK + 5] = np.inf
    w[n - 3] = mx.from_bits([0x7fc01234])[0]
    return w, [1, n // BLOCK]


def payloads(n, R, seed):
    """R hand-built sections of n elements for the decode-mean: random code bits; scales that make the sums round, with a block of
    S = 0 (payload 1: -0 is not a scale a compress writes, it is read as it is), a subnormal S, a huge S (two of them overflow the
    sum), a NaN S in payload 0's last block, and in block 0 payload 1 = payload 0 with every code flipped: the sums cancel to +0
    (+0 + S + -S), and to -0 nowhere."""
    rs = np.random.RandomState(seed)
    nb = -(-n // BLOCK)
    secs = []
    for r in range(R):
        bits = rs.randint(0, 2, (nb, BLOCK)).astype(U32)
        S = np.ldexp(rs.rand(nb) + 0.5, rs.randint(-20, 4, nb)).astype(f32)
        special = [f32(0), mx.from_bits([0x00000123])[0], f32(3e38), mx.from_bits([0x80000000])[0]]
        for b in range(nb):
            if (b + r) % 5 == 3:
                S[b] = special[(b // 5 + r) % 4]
        if r == 0:
            S[-1] = np.nan
        if r == 1:
            bits0, S0 = unpack(secs[0], n)
            bits[0], S[0] = 1 - bits0[0], S0[0]
        secs.append(pack(bits, S))
    return secs
