"""The contract of include/gq_mx.h restated bit for bit in numpy (no GPU, no tolerance anywhere), and the inputs the contract tests
share (tests/test_mx_contract.py checks the restatement and the inputs' claimed preconditions on the CPU against an explicit value
table, tests/test_gpu_mx_contract.py holds the kernels to them).  The restatement follows the header's own words -- the block
exponent in integers, then y = ldexp(|w|, -e), q, t = y / q, k = trunc(t), frac = t - k as float32 operations, one at a time --
not the kernel's shifts."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from qsgd_contract import resolve_seed, uniform01  # noqa: E402

f32, U32, U64 = np.float32, np.uint32, np.uint64
BLOCK, ITEM = 32, 4096
FP4, FP8 = 0, 1
OFF, GIVEN, DEVICE, COUNTER = 0, 1, 2, 4          # GQ_RANDOM_* of include/gq_hsq.h
QNAN = np.uint32(0x7fc00000)
CANARY = 0xA5


class Fmt(object):
    def __init__(self, bits, mb, bias, emax, mthr, cmax):
        self.bits, self.mb, self.bias, self.emax, self.mthr, self.cmax = bits, mb, bias, emax, mthr, cmax
        self.sign = 1 << (bits - 1)


FORMATS = {FP4: Fmt(4, 1, 1, 2, 0x400000, 7), FP8: Fmt(8, 3, 7, 8, 0x600000, 126)}


def _up(x, a=16):
    return (x + a - 1) // a * a


def bits_of(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(U32)


def mag(c, fmt):
    """mag(c) of the header as float64 (exact: at most 4 significant bits)."""
    F = FORMATS[fmt]
    c = np.asarray(c, np.int64)
    sub = c < (1 << F.mb)
    norm = np.ldexp(((1 << F.mb) + (c & ((1 << F.mb) - 1))).astype(np.float64), (c >> F.mb) - F.bias - F.mb)
    return np.where(sub, np.ldexp(c.astype(np.float64), 1 - F.bias - F.mb), norm)


def section_bytes(n, fmt):
    nb = -(-n // BLOCK)
    return _up(nb) + nb * BLOCK * FORMATS[fmt].bits // 8


def items_of(n):
    return -(-n // ITEM)


def pad_blocks(w):
    w = np.asarray(w, f32).reshape(-1)
    nb = -(-w.size // BLOCK)
    p = np.zeros(nb * BLOCK, f32)
    p[:w.size] = w
    return p.reshape(nb, BLOCK)


def block_exponents(wb, fmt):
    """wb: float32 [nb, 32] -> (scale bytes uint8 [nb], e int32 [nb], bad bool [nb]); integers only."""
    F = FORMATS[fmt]
    a = (bits_of(wb) & U32(0x7fffffff)).max(axis=1).astype(np.int64)
    bad = a >= 0x7f800000
    E, M = a >> 23, a & 0x7fffff
    ea = np.where(E != 0, E - 127, -126)
    over = ((E != 0) & (M > F.mthr)).astype(np.int64)
    e = np.maximum(ea - F.emax + over, -127)
    e = np.where(bad, 0, e)
    sb = np.where(bad, 255, e + 127).astype(np.uint8)
    return sb, e.astype(np.int32), bad


def split_element(y, fmt):
    """y float32 -> (c_lo int64, frac float32, q float32): the header's ELEMENT steps, float32 operations one at a time."""
    F = FORMATS[fmt]
    y = np.asarray(y, f32)
    sub = y < f32(2.0 ** (1 - F.bias))
    _, ex = np.frexp(y)                                # y = m * 2^ex, m in [0.5, 1): floor(log2 y) = ex - 1
    fl = np.where(sub, 0, ex.astype(np.int64) - 1)
    q = np.where(sub, f32(2.0 ** (1 - F.bias - F.mb)), np.ldexp(f32(1.0), (fl - F.mb).astype(np.int32))).astype(f32)
    t = (y / q).astype(f32)
    k = np.trunc(t).astype(f32)
    frac = (t - k).astype(f32)
    ki = k.astype(np.int64)
    c_lo = np.where(sub, ki, ((fl + F.bias) << F.mb) + (ki - (1 << F.mb)))
    return c_lo, frac, q


def scaled(wb, e):
    """y = ldexp(|w|, -e) per block: one rounding (glibc's ldexpf rounds to nearest even onto the subnormal grid)."""
    return np.ldexp(np.abs(wb), (-e.astype(np.int32))[:, None]).astype(f32)


def round_up(c_lo, frac, r):
    """r None: to nearest, ties to the even code; otherwise frac > r in float32."""
    if r is None:
        return (frac > f32(0.5)) | ((frac == f32(0.5)) & ((c_lo & 1) == 1))
    with np.errstate(invalid="ignore"):
        return frac > np.asarray(r, f32)


def codes_of(w, fmt, r=None):
    """w float32 [n], r float32 [n] or None -> (scale bytes [nb], codes int64 [nb * 32] with the sign bit, e [nb], bad [nb])."""
    F = FORMATS[fmt]
    wb = pad_blocks(w)
    sb, e, bad = block_exponents(wb, fmt)
    with np.errstate(invalid="ignore", over="ignore"):
        y = scaled(np.where(bad[:, None], f32(0), wb), e)
    c_lo, frac, _ = split_element(y, fmt)
    rr = None
    if r is not None:
        rr = np.zeros(wb.size, f32)
        rr[:np.asarray(w).size] = np.asarray(r, f32)
        rr = rr.reshape(wb.shape)
    c = c_lo + round_up(c_lo, frac, rr).astype(np.int64)
    sign = (bits_of(wb) >> U32(31)).astype(np.int64)
    code = np.where(bad[:, None], 0, c | (sign * F.sign))
    return sb, code.reshape(-1), e, bad


def decode_values(sb, code, fmt):
    """scale bytes [nb], codes [nb * 32] -> float32 [nb * 32]: +-ldexp(mag(c), e), inf from 2^128 on, the NaN for byte 0xFF."""
    F = FORMATS[fmt]
    code = np.asarray(code, np.int64).reshape(len(sb), BLOCK)
    c = code & (F.sign - 1)
    e = np.asarray(sb, np.int32) - 127
    with np.errstate(over="ignore"):
        m = np.ldexp(mag(c, fmt).astype(f32), e[:, None]).astype(f32)
    b = bits_of(m) | (((code >> (F.bits - 1)) & 1).astype(U32) << U32(31))
    b = np.where((np.asarray(sb) == 255)[:, None], QNAN, b).astype(U32)
    return b.view(f32).reshape(-1)


def pack(sb, code, fmt):
    """One tensor's section (uint8): the scale bytes padded to 16, then the codes (FP4: element 2i in the low nibble)."""
    nb = len(sb)
    sc = np.zeros(_up(nb), np.uint8)
    sc[:nb] = sb
    code = np.asarray(code, np.int64)
    if fmt == FP4:
        body = (code[0::2] | (code[1::2] << 4)).astype(np.uint8)
    else:
        body = code.astype(np.uint8)
    return np.concatenate([sc, body])


def unpack(sec, n, fmt):
    nb = -(-n // BLOCK)
    sb = sec[:nb]
    body = sec[_up(nb):].astype(np.int64)
    if fmt == FP4:
        code = np.empty(nb * BLOCK, np.int64)
        code[0::2], code[1::2] = body & 15, body >> 4
    else:
        code = body
    return sb, code


def draws(mode, n, first_draw=0, seed=0, step=0, given=None):
    """The n draws of a tensor whose first draw is first_draw (None for GQ_RANDOM_OFF)."""
    if mode == OFF:
        return None
    if mode == GIVEN:
        return np.asarray(given, f32)[first_draw:first_draw + n]
    if mode == COUNTER:
        seed = resolve_seed(seed, step)
    return uniform01(seed, (first_draw + np.arange(n, dtype=np.int64)).astype(U64))


def compress(g, fmt, r=None, err=None, ef_scale=None):
    """One tensor -> (section uint8, decoded float32 [n], w, err afterwards or None).  err None: no error feedback (w = g)."""
    g = np.asarray(g, f32).reshape(-1)
    n = g.size
    w = g
    if err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            p = (f32(ef_scale) * np.asarray(err, f32)).astype(f32)      # the product rounded, then the sum
            w = (g + p).astype(f32)
    sb, code, _, _ = codes_of(w, fmt, r)
    D = decode_values(sb, code, fmt)[:n]
    new_err = None
    if err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            new_err = (w - D).astype(f32)
    return pack(sb, code, fmt), D, w, new_err


def decode_mean(sections, n, fmt, plain=False):
    """acc = +0 + d_0 + d_1 + ... in payload order, then a true division by (float)R; plain with one payload: d_0 as it is."""
    R = len(sections)
    ds = [decode_values(*unpack(s, n, fmt), fmt)[:n] for s in sections]
    if plain and R == 1:
        return ds[0]
    acc = np.zeros(n, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in ds:
            acc = (acc + d).astype(f32)
        return (acc / f32(R)).astype(f32)


def same(a, b, nan_as_one=False):
    """np.array_equal on the bits; nan_as_one: every NaN counts as one pattern (where an input block is not finite)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    if a.shape != b.shape:
        return False
    ab, bb = bits_of(a).copy(), bits_of(b).copy()
    if nan_as_one:
        ab[np.isnan(a)] = QNAN
        bb[np.isnan(b)] = QNAN
    return np.array_equal(ab, bb)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def randn(n, seed, spread=3.0):
    """Heavy-tailed gradients: randn * 1e-3 * exp(spread * randn), so that blocks differ in scale by orders of magnitude."""
    rs = np.random.RandomState(seed)
    return (rs.randn(n) * 1e-3 * np.exp(spread * rs.randn(n))).astype(f32)


def from_bits(b):
    return np.asarray(b, U32).view(f32)


def block_with_max(top, rest):
    """A block of 32: `top` first, then `rest` (shorter: padded with +0)."""
    b = np.zeros(BLOCK, f32)
    b[0] = top
    b[1:1 + len(rest)] = rest
    return b


def grid_and_midpoints(fmt, s):
    """Edge 7.  Blocks whose maximum is mag(cmax) * 2^s (so e = s), holding every grid value mag(c) * 2^s and every midpoint
    (mag(c) + mag(c + 1)) / 2 * 2^s, signs alternating.  Claim: every y is a grid value (frac = 0) or frac = 0.5, both parities."""
    F = FORMATS[fmt]
    c = np.arange(F.cmax + 1)
    g = mag(c, fmt)
    mid = (g[:-1] + g[1:]) / 2
    vals = np.ldexp(np.concatenate([g, mid]), s).astype(f32)
    vals[1::2] *= f32(-1)
    top = f32(np.ldexp(mag(F.cmax, fmt), s))
    blocks = [block_with_max(top, vals[i:i + BLOCK - 1]) for i in range(0, len(vals), BLOCK - 1)]
    return np.concatenate(blocks)


def frac_equals_draw(fmt, s, seed=3):
    """Edge 8.  One block with maximum mag(cmax) * 2^s; elements in the top binade below it whose frac is j * 2^-p exactly, with
    draws r = frac (never up: the comparison is strict), r = frac - 2^-24 (up), r = 0 on frac = 0 (not up) and on frac > 0 (up).
    -> (w [32], r [32], frac [32] as claimed)"""
    F = FORMATS[fmt]
    rs = np.random.RandomState(seed)
    lo = float(mag(F.cmax - 1, fmt))             # 4 (q = 2) for FP4, 416 (q = 32) for FP8
    q = float(mag(F.cmax, fmt)) - lo
    p = 20 if fmt == FP4 else 15
    j = rs.randint(1, 1 << p, BLOCK - 1)
    j[:3] = (0, 1, (1 << p) - 1)
    frac = (j * 2.0 ** -p).astype(f32)
    w = np.ldexp(lo + q * frac.astype(np.float64), s).astype(f32)
    r = frac.copy()
    r[10:20] = (frac[10:20].astype(np.float64) - 2.0 ** -24).astype(f32)
    r[20:] = 0
    r[0] = 0
    top = f32(np.ldexp(mag(F.cmax, fmt), s))
    return block_with_max(top, w), np.concatenate([[f32(0)], r]).astype(f32), np.concatenate([[f32(0)], frac]).astype(f32)


def subnormal_y(fmt):
    """Edge 9.  One block with maximum mag(cmax) * 2^8 (e = 8) and elements so small that y = w * 2^-8 is subnormal, lies exactly
    between two subnormals (1.5 and 2.5 * 2^-149: ties to even) or rounds to zero.  Claim: every y but the first is below 2^-126."""
    F = FORMATS[fmt]
    tiny = np.array([2.0 ** -120, -2.0 ** -130, 3 * 2.0 ** -142, -5 * 2.0 ** -142, 2.0 ** -149, -2.0 ** -141, 2.0 ** -142, 1.5 * 2.0 ** -126,
                     (2 ** 23 + 1) * 2.0 ** -149, -2.0 ** -127, 7 * 2.0 ** -149], np.float64).astype(f32)
    return block_with_max(f32(mag(F.cmax, fmt) * 256.0), tiny)


def edge_blocks(fmt):
    """{name: float32 [32 * m]} -- the edge blocks 1 ... 6 of the issue (7 ... 9: grid_and_midpoints, frac_equals_draw, subnormal_y)."""
    F = FORMATS[fmt]
    z = np.zeros(BLOCK, f32)
    mixed = z.copy()
    mixed[::3] = f32(-0.0)
    min_sub = z.copy()
    min_sub[5], min_sub[9] = from_bits([1])[0], from_bits([0x80000001])[0]
    all_sub = from_bits((np.arange(BLOCK, dtype=np.int64) * 0x3ffff + 1).astype(U32) | (U32(1 << 31) * (np.arange(BLOCK) % 2).astype(U32)))
    all_sub[7] = from_bits([0x007fffff])[0]       # the largest subnormal is the block's maximum; no normal number in the block
    big = (randn(BLOCK, 11) * f32(1e30)).astype(f32)
    big[3] = np.finfo(f32).max
    big[4] = -np.finfo(f32).max
    out = {"zeros": z, "signed_zeros": mixed, "min_subnormal": min_sub, "all_subnormal": all_sub, "flt_max": big}
    for name, M in (("at_mthr", F.mthr), ("above_mthr", F.mthr + 1)):
        for E in (1, 100, 254):
            top = from_bits([(E << 23) | M])[0]
            rest = np.linspace(-1, 1, BLOCK - 1) * float(top)
            out["%s_E%d" % (name, E)] = block_with_max(top, rest.astype(f32))
    fin = randn(BLOCK, 12)
    nonfin = randn(BLOCK, 13)
    nonfin[2], nonfin[30] = np.inf, -np.inf
    nans = randn(BLOCK, 14)
    nans[0], nans[17], nans[31] = from_bits([0x7fc00001])[0], from_bits([0xffc12345])[0], from_bits([0x7f800001])[0]
    out["nonfinite"] = np.concatenate([fin, nonfin, randn(BLOCK, 15), nans, randn(BLOCK, 16)])
    return out


def edge_tensor(fmt):
    """All edge blocks back to back -> (w, {name: (first element, elements)})"""
    parts, where, at = [], {}, 0
    blocks = dict(edge_blocks(fmt))
    blocks["grid"] = grid_and_midpoints(fmt, -3)
    blocks["grid_tiny"] = grid_and_midpoints(fmt, -127)
    blocks["subnormal_y"] = subnormal_y(fmt)
    for name, b in blocks.items():
        parts.append(b)
        where[name] = (at, b.size)
        at += b.size
    return np.concatenate(parts), where


def layout(sizes, fmt, dense_sizes=()):
    """Wire offsets as the quantizer lays them out: 16-byte aligned sections, then the identity-compressed tensors' f32."""
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off = _up(off + section_bytes(n, fmt))
    dense = []
    for n in dense_sizes:
        dense.append((off, n))
        off += 4 * n
    return offs, dense, _up(off)


def payload_set(n, fmt, R, seed=5):
    """R hand-built sections of a tensor of n elements: random codes over EVERY code value (the FP8 magnitude code 127 included),
    scale bytes drawn from 0, 1, 126, 127, 253, 255 and a few random ones."""
    rs = np.random.RandomState(seed)
    F = FORMATS[fmt]
    nb = -(-n // BLOCK)
    special = np.array([0, 1, 126, 127, 253, 255, 120, 130])
    secs = []
    for r in range(R):
        code = rs.randint(0, 1 << F.bits, nb * BLOCK)
        code[:1 << F.bits] = np.arange(1 << F.bits)[:nb * BLOCK]
        sb = special[rs.randint(0, len(special), nb)].astype(np.uint8)
        sb[:len(special)] = np.roll(special, r)[:nb]
        secs.append(pack(sb, code, fmt))
    return secs
