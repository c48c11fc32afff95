"""The contract of include/gq_mx.h restated bit for bit in numpy for ANY format table -- the two 6-bit formats (FP6 E2M3, FP6 E3M2)
and their wire next to FP4 / FP8 -- with the inputs the FP6 contract tests share (tests/test_mx6_contract.py checks the restatement
on the CPU: against tests/mx_contract.py on FP4 / FP8, against explicit value tables on the new formats; the GPU tests hold the
kernels to it).  Like mx_contract.py it follows the header's own words -- the block exponent in integers, then y = ldexp(|w|, -e),
q, t = y / q, k = trunc(t), frac = t - k as float32 operations, one at a time -- not the kernel's shifts.  What does not depend on
the format (blocks, draws, the bit comparison, the random inputs) is mx_contract's own; its FORMATS table is left alone."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402
from mx_contract import (BLOCK, CANARY, COUNTER, DEVICE, GIVEN, ITEM, OFF, QNAN, Fmt, _up, bits_of, block_with_max, draws,  # noqa: E402,F401
                         from_bits, items_of, pad_blocks, randn, round_up, same, scaled)

f32, U32 = np.float32, np.uint32
FP4, FP8, FP6_E2M3, FP6_E3M2 = 0, 1, 0x23, 0x32
FP6 = (FP6_E2M3, FP6_E3M2)
FORMATS = {FP4: Fmt(4, 1, 1, 2, 0x400000, 7), FP8: Fmt(8, 3, 7, 8, 0x600000, 126),
           FP6_E2M3: Fmt(6, 3, 1, 2, 0x700000, 31), FP6_E3M2: Fmt(6, 2, 3, 4, 0x600000, 31)}
NAMES = {FP4: "fp4", FP8: "fp8", FP6_E2M3: "fp6_e2m3", FP6_E3M2: "fp6_e3m2"}


def mag(c, fmt):
    """mag(c) of the header as float64 (exact: at most 4 significant bits)."""
    F = FORMATS[fmt]
    c = np.asarray(c, np.int64)
    sub = c < (1 << F.mb)
    norm = np.ldexp(((1 << F.mb) + (c & ((1 << F.mb) - 1))).astype(np.float64), (c >> F.mb) - F.bias - F.mb)
    return np.where(sub, np.ldexp(c.astype(np.float64), 1 - F.bias - F.mb), norm)


def code_bytes(nb, fmt):
    """The code bytes of nb blocks with their zero pad: a multiple of 16 (only FP6 with an odd nb pads: 8 bytes)."""
    return _up(nb * BLOCK * FORMATS[fmt].bits // 8)


def section_bytes(n, fmt):
    nb = -(-n // BLOCK)
    return _up(nb) + code_bytes(nb, fmt)


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


def pack6(code):
    """6-bit codes [nb * 32] -> uint8 [24 nb]: per block one 192-bit little-endian bit string, element i in bits 6i .. 6i+5."""
    code = np.asarray(code, np.int64)
    assert code.size % BLOCK == 0 and np.all((code >= 0) & (code < 64))
    bits = np.unpackbits(code.astype(np.uint8)[:, None], axis=1, bitorder="little")[:, :6]      # [elements, 6], bit 0 first
    return np.packbits(bits.reshape(-1, 6 * BLOCK), axis=1, bitorder="little").reshape(-1)


def unpack6(body, nb):
    bits = np.unpackbits(np.asarray(body, np.uint8)[:24 * nb].reshape(nb, 24), axis=1, bitorder="little").reshape(-1, 6)
    return (bits.astype(np.int64) << np.arange(6)).sum(axis=1)


def pack(sb, code, fmt):
    """One tensor's section (uint8): the scale bytes padded to 16, then the codes, then zero bytes to a multiple of 16."""
    nb = len(sb)
    sc = np.zeros(_up(nb), np.uint8)
    sc[:nb] = sb
    code = np.asarray(code, np.int64)
    bits = FORMATS[fmt].bits
    if bits == 4:
        raw = (code[0::2] | (code[1::2] << 4)).astype(np.uint8)
    elif bits == 6:
        raw = pack6(code)
    else:
        raw = code.astype(np.uint8)
    body = np.zeros(code_bytes(nb, fmt), np.uint8)
    body[:raw.size] = raw
    return np.concatenate([sc, body])


def unpack(sec, n, fmt):
    nb = -(-n // BLOCK)
    sb = sec[:nb]
    body = sec[_up(nb):]
    bits = FORMATS[fmt].bits
    if bits == 4:
        code = np.empty(nb * BLOCK, np.int64)
        code[0::2], code[1::2] = body[:16 * nb].astype(np.int64) & 15, body[:16 * nb].astype(np.int64) >> 4
    elif bits == 6:
        code = unpack6(body, nb)
    else:
        code = body[:32 * nb].astype(np.int64)
    return sb, code


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


def rel_l2(w, fmt, r=None):
    """Relative L2 error of decode(compress(w)) in float64."""
    D = compress(w, fmt, r)[1].astype(np.float64)
    w = np.asarray(w, np.float64)
    return float(np.linalg.norm(D - w) / np.linalg.norm(w))


# ---- the rotation of include/gq_mxr.h in front (tests/mxr_contract.py has the transform) ---------------------------------------------
def compress_rotated(g, fmt, signs, r=None, err=None, ef_scale=None):
    """mxr_contract.compress over this module's formats -> (section, D, w, err afterwards or None, x')."""
    import mxr_contract as mxr
    g = np.asarray(g, f32).reshape(-1)
    w = g
    if err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            p = (f32(ef_scale) * np.asarray(err, f32)).astype(f32)
            w = (g + p).astype(f32)
    xp = mxr.forward(w, signs)
    sec, Dx, _, _ = compress(xp, fmt, r)
    D = mxr.inverse(Dx, signs)
    new_err = None
    if err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            new_err = (w - D).astype(f32)
    return sec, D, w, new_err, xp


def decode_mean_rotated(sections, n, fmt, signs, plain=False):
    """The mean gq_mx.h defines, then ONE inverse rotation."""
    import mxr_contract as mxr
    return mxr.inverse(decode_mean(sections, n, fmt, plain), signs)


# ---- the inputs (mx_contract's, over this module's formats) --------------------------------------------------------------------------
def grid_and_midpoints(fmt, s):
    """Blocks whose maximum is mag(cmax) * 2^s (so e = s), holding every grid value mag(c) * 2^s and every midpoint
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


# frac_equals_draw: frac = j * 2^-p.  w = lo + q * frac must be exact in float32: lo = mag(cmax - 1) lies in a binade whose ulp is
# u, and q * 2^-p >= u is needed -- FP4: lo 4, q 2, u 2^-21: p <= 22; FP8: lo 416, q 32, u 2^-15: p <= 20; E2M3: lo 7, q 0.5,
# u 2^-21: p <= 20; E3M2: lo 24, q 4, u 2^-19: p <= 21.  (mx_contract uses 20 and 15.)
FRAC_BITS = {FP4: 20, FP8: 15, FP6_E2M3: 18, FP6_E3M2: 18}


def frac_equals_draw(fmt, s, seed=3):
    """One block with maximum mag(cmax) * 2^s; elements in the top binade below it whose frac is j * 2^-p exactly, with draws
    r = frac (never up: the comparison is strict), r = frac - 2^-24 (up), r = 0 on frac = 0 (not up) and on frac > 0 (up).
    -> (w [32], r [32], frac [32] as claimed)"""
    F = FORMATS[fmt]
    rs = np.random.RandomState(seed)
    lo = float(mag(F.cmax - 1, fmt))
    q = float(mag(F.cmax, fmt)) - lo
    p = FRAC_BITS[fmt]
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
    """One block with maximum mag(cmax) * 2^8 (e = 8) and elements so small that y = w * 2^-8 is subnormal, lies exactly between
    two subnormals (1.5 and 2.5 * 2^-149: ties to even) or rounds to zero.  Claim: every y but the first is below 2^-126."""
    F = FORMATS[fmt]
    tiny = np.array([2.0 ** -120, -2.0 ** -130, 3 * 2.0 ** -142, -5 * 2.0 ** -142, 2.0 ** -149, -2.0 ** -141, 2.0 ** -142, 1.5 * 2.0 ** -126,
                     (2 ** 23 + 1) * 2.0 ** -149, -2.0 ** -127, 7 * 2.0 ** -149], np.float64).astype(f32)
    return block_with_max(f32(mag(F.cmax, fmt) * 256.0), tiny)


def edge_blocks(fmt):
    """{name: float32 [32 * m]} -- mx_contract.edge_blocks with this format's MTHR in the at / above blocks."""
    F = FORMATS[fmt]
    out = {k: v for k, v in mx.edge_blocks(FP8).items() if not k.startswith(("at_mthr", "above_mthr"))}      # (format-free blocks)
    for name, M in (("at_mthr", F.mthr), ("above_mthr", F.mthr + 1)):
        for E in (1, 100, 254):
            top = from_bits([(E << 23) | M])[0]
            rest = np.linspace(-1, 1, BLOCK - 1) * float(top)
            out["%s_E%d" % (name, E)] = block_with_max(top, rest.astype(f32))
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
    """R hand-built sections of a tensor of n elements: random codes over EVERY code value, scale bytes drawn from 0, 1, 126, 127,
    253, 255 and a few random ones."""
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


def student_t(n, dof, seed):
    return np.random.RandomState(seed).standard_t(dof, n).astype(f32)
