"""The contract of include/gq_mxr.h restated in numpy (no GPU, no tolerance anywhere) on top of tests/mx_contract.py, and the inputs
the contract tests share (tests/test_mxr_contract.py checks the restatement and the inputs' claimed preconditions on the CPU,
tests/test_gpu_mxr_contract.py holds the kernels to them).  The transform follows the header's own words -- the sign bits xor-ed
into the floats' bits, then eight stages over the whole block, each one float32 addition or subtraction per element, then one
float32 multiplication -- not the kernel's split into lanes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402

f32, U32 = np.float32, np.uint32
RBLOCK = 256
M64 = (1 << 64) - 1
ZERO_SIGNS = (0, 0, 0, 0)
ONES_SIGNS = (M64, M64, M64, M64)
SIZES = [1, 255, 256, 257, 287, 289, 511, 512, 4095, 4096, 4097, 4096 + 255, 3 * 4096 + 1]


def sign_words(seed):
    """Outputs 0 ... 3 of splitmix64 started at `seed`, whole-array form (test_mxr_contract.py has the scalar loop)."""
    state = (int(seed) + 0x9E3779B97F4A7C15 * np.arange(1, 5, dtype=object)) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return tuple(int(w) for w in (z ^ (z >> 31)))


def sign_mask(signs):
    """The four words -> uint32 [256]: 0x80000000 where element j's bit (bit j & 63 of word j >> 6) is set."""
    bits = np.array([(int(signs[j >> 6]) >> (j & 63)) & 1 for j in range(RBLOCK)], U32)
    return bits << U32(31)


def flip(x, signs):
    return (mx.bits_of(x) ^ sign_mask(signs)[None, :]).view(f32)


def stage(x, t):
    """One butterfly stage of stride 2^t over blocks x [nblk, 256]: float32 additions and subtractions of the previous values."""
    h = 1 << t
    v = x.reshape(x.shape[0], RBLOCK // (2 * h), 2, h)
    a, b = v[:, :, 0, :], v[:, :, 1, :]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(a + b).astype(f32), (a - b).astype(f32)], axis=2).reshape(x.shape[0], RBLOCK)


def stages(x, order=range(8)):
    for t in order:
        x = stage(x, t)
    return x


def scale(x):
    with np.errstate(under="ignore"):
        return (x * f32(0.0625)).astype(f32)


def forward_blocks(x, signs, order=range(8), scale_first=False):
    """[nblk, 256]: sign flip, eight stages, * 2^-4.  order / scale_first: the variants the kernels must NOT compute."""
    x = flip(np.asarray(x, f32), signs)
    if scale_first:
        return stages(scale(x), order)
    return scale(stages(x, order))


def inverse_blocks(y, signs, order=range(8)):
    """[nblk, 256]: the same eight stages, * 2^-4, sign flip."""
    return flip(scale(stages(np.asarray(y, f32), order)), signs)


def _over_blocks(fn, w, signs, **kw):
    w = np.asarray(w, f32).reshape(-1)
    nr = w.size // RBLOCK * RBLOCK
    out = w.copy()
    if nr:
        out[:nr] = fn(w[:nr].reshape(-1, RBLOCK), signs, **kw).reshape(-1)
    return out


def forward(w, signs, **kw):
    """A flat tensor -> x': its n // 256 whole blocks rotated, the last n % 256 elements as they are."""
    return _over_blocks(forward_blocks, w, signs, **kw)


def inverse(y, signs, **kw):
    return _over_blocks(inverse_blocks, y, signs, **kw)


def compress(g, fmt, signs, r=None, err=None, ef_scale=None, **kw):
    """One tensor -> (section uint8, D float32 [n], w, err afterwards or None, x')."""
    g = np.asarray(g, f32).reshape(-1)
    w = g
    if err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            p = (f32(ef_scale) * np.asarray(err, f32)).astype(f32)
            w = (g + p).astype(f32)
    xp = forward(w, signs, **kw)
    sec, Dx, _, _ = mx.compress(xp, fmt, r)
    D = inverse(Dx, signs)
    new_err = None
    if err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            new_err = (w - D).astype(f32)
    return sec, D, w, new_err, xp


def frac_draws(xp, fmt):
    """The draws that put every element of x' on the edge: r_i = frac_i, so no element rounds up (the comparison is strict) and
    an x' that is larger by one ulp anywhere does.  With them the wire shows the last bit of the forward transform."""
    wb = mx.pad_blocks(xp)
    _, e, bad = mx.block_exponents(wb, fmt)
    with np.errstate(invalid="ignore", over="ignore"):
        y = mx.scaled(np.where(bad[:, None], f32(0), wb), e)
    _, frac, _ = mx.split_element(y, fmt)
    return frac.reshape(-1)[:np.asarray(xp).size].astype(f32)


def decode_mean(sections, n, fmt, signs, plain=False):
    """The mean gq_mx.h defines, then ONE inverse rotation."""
    return inverse(mx.decode_mean(sections, n, fmt, plain), signs)


def decode_mean_inverse_first(sections, n, fmt, signs):
    """What the kernels must NOT compute: every payload rotated back, then the mean."""
    ds = [inverse(mx.decode_values(*mx.unpack(s, n, fmt), fmt)[:n], signs) for s in sections]
    acc = np.zeros(n, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in ds:
            acc = (acc + d).astype(f32)
        return (acc / f32(len(sections))).astype(f32)


def hadamard_matrix():
    """The explicit 256 x 256 +-1 matrix: H[i, j] = (-1)^popcount(i & j), as int64."""
    i = np.arange(RBLOCK)
    pc = np.array([[bin(a & b).count("1") & 1 for b in i] for a in i], np.int64)
    return 1 - 2 * pc


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(a))


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
SEEDED = sign_words(1)
SIGN_SETS = {"zero": ZERO_SIGNS, "ones": ONES_SIGNS, "seeded": SEEDED}


def gradients(n, seed):
    """mx_contract.randn with a moderate spread: heavy tails inside a rotation block, no overflow in the butterflies; the first
    rotation block (n >= 256) scaled by 2^-115, down to where w * 2^-4 is subnormal while the rotated sums * 2^-4 mostly are not --
    a scale applied before the stages would round there.  Claim (checked): finite, and every rotated value is finite."""
    g = mx.randn(n, seed, spread=2.0)
    if n >= RBLOCK:
        g[:RBLOCK] = np.ldexp(g[:RBLOCK], -115)
    return g


def payloads(n, fmt, R, seed):
    """R hand-built sections of a tensor of n elements for the decode-mean: random codes over EVERY code value (the FP8 magnitude
    code 127 included), scale bytes 110 ... 140 so that the sums inside a rotation block round; payload 0 holds scale byte 0xFF
    in the last MX block of the tensor's second rotation block (if it has one) and in its last MX block of all."""
    rs = np.random.RandomState(seed)
    F = mx.FORMATS[fmt]
    nb = -(-n // mx.BLOCK)
    secs = []
    for r in range(R):
        code = rs.randint(0, 1 << F.bits, nb * mx.BLOCK)
        code[:1 << F.bits] = np.arange(1 << F.bits)[:nb * mx.BLOCK]
        sb = rs.randint(110, 141, nb).astype(np.uint8)
        if r == 0:
            sb[-1] = 255
            if n >= 2 * RBLOCK:
                sb[15] = 255
        secs.append(mx.pack(sb, code, fmt))
    return secs


def integers(nblk, seed, top=1 << 14):
    """Integer-valued blocks with |x| <= 2^14: every sum of the eight stages is an integer below 2^23, hence exact in float32."""
    rs = np.random.RandomState(seed)
    return rs.randint(-top, top + 1, (nblk, RBLOCK)).astype(f32)


def edge_finite():
    """Finite value edges, one rotation block each (+ a tail of 40) -> (w, {name: first element}).
    zeros       +-0 only: every stage adds zeros; the signs of the results follow IEEE (x - x = +0)
    subnormals  subnormals and +-0: multiples of 2^-149 below 2^-140, the sums exact; x' = x * 2^-4 rounds onto the 2^-149 grid
    tiny        multiples of 2^-146 below 2^-134: the stages are exact, x' = x * 2^-4 is subnormal and rounds (step 3's one rounding)
    overflow    FLT_MAX twice at the block's start, zeros elsewhere: stage 0 overflows to +inf and no inf ever meets another, so
                x' is +inf on the even elements -- scale byte 0xFF in all 8 MX blocks from a finite input"""
    rs = np.random.RandomState(31)
    z = np.zeros(RBLOCK, f32)
    z[::3] = f32(-0.0)
    sub = mx.from_bits(rs.randint(0, 512, RBLOCK).astype(U32) | (U32(1 << 31) * rs.randint(0, 2, RBLOCK).astype(U32))).copy()
    sub[::7] = 0
    tiny = (rs.randint(-(1 << 12), 1 << 12, RBLOCK).astype(np.float64) * 2.0 ** -146).astype(f32)
    over = np.zeros(RBLOCK, f32)
    over[0] = over[1] = np.finfo(f32).max
    tail = mx.randn(40, 32)
    parts = [("zeros", z), ("subnormals", sub), ("tiny", tiny), ("overflow", over), ("tail", tail)]
    where, at = {}, 0
    for name, b in parts:
        where[name] = at
        at += b.size
    return np.concatenate([b for _, b in parts]), where


def edge_nonfinite():
    """One inf / one NaN in the first and the last position of a rotation block and in the unrotated tail, finite blocks between
    -> (w, {name: first element}).  Claim: an inf or NaN reaches all 256 rotated values of its block and no other block."""
    names = ["inf_first", "finite_a", "inf_last", "nan_first", "finite_b", "nan_last"]
    blocks = {nm: mx.randn(RBLOCK, 40 + i, spread=1.0) for i, nm in enumerate(names)}
    blocks["inf_first"][0] = np.inf
    blocks["inf_last"][255] = -np.inf
    blocks["nan_first"][0] = mx.from_bits([0x7fc00001])[0]
    blocks["nan_last"][255] = mx.from_bits([0xffc12345])[0]
    tail = mx.randn(100, 50, spread=1.0)
    tail[0], tail[99] = np.inf, np.nan        # the tail's first and last MX block; the block between stays finite
    where, at = {}, 0
    for nm in names:
        where[nm] = at
        at += RBLOCK
    where["tail"] = at
    return np.concatenate([blocks[nm] for nm in names] + [tail]), where


def student_t(n, dof, rng):
    return rng.standard_t(dof, n).astype(f32)


def lognormal_gaussian(n, rng):
    return (rng.standard_normal(n) * np.exp(1.5 * rng.standard_normal(n))).astype(f32)
