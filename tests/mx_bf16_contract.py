"""The tensor-side element type of include/gq_mx.h and include/gq_mxr.h (TENSOR-SIDE TYPE) restated in numpy integers: widen, narrow,
and the bf16 reference of every launch -- narrow applied to what tests/mx6_contract.py (all four formats; its rotated forms go
through tests/mxr_contract.py) computes on widened inputs.  bf16 values are uint16 arrays throughout.  Also the case builders the
CPU test (tests/test_mx_bf16_contract.py: their claimed preconditions, on the reference alone) and the GPU tests share."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx6_contract as m6  # noqa: E402

f32, U16, U32 = np.float32, np.uint16, np.uint32
FMTS = [m6.FP4, m6.FP8, m6.FP6_E2M3, m6.FP6_E3M2]
BF16_NAN = 0x7FC0
BF16_MAX = 0x7F7F           # (2 - 2^-7) * 2^127
SEAM_SIZES = [1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8193]      # lane, block, rotation block, step, item


def widen(h):
    """bf16 bits -> the float32 with the bits h << 16 (exact)."""
    return (np.asarray(h, U16).astype(U32) << U32(16)).view(f32)


def narrow(x, mode="rne"):
    """float32 -> bf16 bits, in integers on b = bits(x): a NaN gives 0x7FC0, otherwise (b + 0x7FFF + ((b >> 16) & 1)) >> 16.
    mode: 'trunc' and 'half_up' are the two wrong roundings the mutation check holds the cases against."""
    b = np.ascontiguousarray(np.asarray(x, f32)).view(U32).astype(np.uint64)
    nan = (b & 0x7fffffff) > 0x7f800000
    if mode == "rne":
        r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    elif mode == "trunc":
        r = b >> 16
    elif mode == "half_up":
        r = (b + 0x8000) >> 16
    else:
        raise ValueError(mode)
    return np.where(nan, BF16_NAN, r & 0xFFFF).astype(U16)


def compress(g16, fmt, r=None, err=None, ef_scale=None, signs=None, mode="rne", narrow_w_first=False):
    """One bf16 tensor (uint16 bits) -> (section, out as bf16 bits, the source afterwards as bf16 bits, err afterwards float32 or
    None).  signs: the rotation's sign words (include/gq_mxr.h), None: plain MX.  The arithmetic is the float32 contract's on
    widen(g16); only the stores into bf16 locations narrow, and err comes from the UNROUNDED w.
    narrow_w_first (mutation check only): w narrowed BEFORE err = w - decoded, which the contract forbids."""
    g = widen(g16)
    if narrow_w_first and err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            w = (g + (f32(ef_scale) * np.asarray(err, f32)).astype(f32)).astype(f32)
        g, err_in = widen(narrow(w)), np.zeros_like(g)
        res = m6.compress(g, fmt, r, err_in, 1.0) if signs is None else m6.compress_rotated(g, fmt, signs, r, err_in, 1.0)[:4]
    else:
        res = m6.compress(g, fmt, r, err, ef_scale) if signs is None else m6.compress_rotated(g, fmt, signs, r, err, ef_scale)[:4]
    sec, D, w, new_err = res
    return sec, narrow(D, mode), narrow(w, mode), new_err


def decode_mean(sections, n, fmt, plain=False, signs=None, mode="rne"):
    """The float32 decode-mean of the contract (inverse-rotated once under `signs`), narrowed once."""
    m = m6.decode_mean(sections, n, fmt, plain) if signs is None else m6.decode_mean_rotated(sections, n, fmt, signs, plain)
    return narrow(m, mode)


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def randn16(n, seed, spread=3.0):
    """Heavy-tailed bf16 gradients (mx_contract.randn, narrowed)."""
    return narrow(m6.randn(n, seed, spread))


SPECIALS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F, 0x0080, 0x7F7F, 0xFF7F, 0x3F80, 0xBF80], U16)    # +-0, bf16 subnormals, min normal, +-max, +-1
NONFINITE = np.array([0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F81], U16)      # +-inf, quiet NaNs, a signalling NaN


def edge_gradient(n, seed, nonfinite=True):
    """A bf16 gradient with +-0, bf16 subnormals and the largest values sprinkled in, and (nonfinite) a block with +-inf and one
    with NaNs.  Needs n >= 160 for the non-finite blocks; shorter tensors get the finite specials only."""
    g = randn16(n, seed)
    rs = np.random.RandomState(seed + 1)
    k = min(n, 64)
    at = rs.permutation(n)[:k]
    g[at] = SPECIALS[rs.randint(0, len(SPECIALS), k)]
    if nonfinite and n >= 160:
        g[100], g[101] = NONFINITE[0], NONFINITE[1]
        g[140], g[141], g[142] = NONFINITE[2], NONFINITE[3], NONFINITE[4]
    return g


def ef_case(n, seed):
    """Three records of error feedback on one tensor -> ([g_0, g_1, g_2] bf16 bits, err_0 float32, ef_scale).  The carried state
    holds +-0, subnormals, +-inf and a NaN; element 0 is the bf16 maximum with a residual of 2^119, so that the FINITE float32
    w = 2^128 - 2^119 narrows to +inf (a tie, to even); element 1 its negative; elements 2 and 3 are ties at 1.0."""
    gs = [edge_gradient(n, seed + 10 * t, nonfinite=(t == 1)) for t in range(3)]
    rs = np.random.RandomState(seed + 5)
    err = (m6.randn(n, seed + 7) * f32(0.25)).astype(f32)
    if n >= 2:
        gs[0][0], gs[0][1] = BF16_MAX, 0x8000 | BF16_MAX
        err[0], err[1] = f32(2.0 ** 119), f32(-2.0 ** 119)
    if n >= 4:      # w = 1 + 2^-8 and 1 + 3 * 2^-8: ties, the even neighbour below and above
        gs[0][2], gs[0][3] = 0x3F80, 0x3F81
        err[2], err[3] = f32(2.0 ** -8), f32(2.0 ** -8)
    if n >= 64:
        at = rs.permutation(n - 4)[:8] + 4
        err[at] = np.array([0.0, -0.0, 1e-45, -1e-42, np.inf, -np.inf, np.nan, 3e38], f32)
    return gs, err, 1.0


def run_ef(gs, err, s, fmt, rs=None, signs=None, mode="rne", narrow_w_first=False):
    """The three records of ef_case stepped through the reference -> [(section, source afterwards, err afterwards)] per record."""
    steps = []
    for t, g in enumerate(gs):
        sec, _, src, err = compress(g, fmt, rs[t] if rs is not None else None, err, s, signs, mode, narrow_w_first)
        steps.append((sec, src, err))
    return steps


def _code_of(value, fmt):
    """The code whose decoded magnitude is |value| (it must exist in the format), sign bit included; -0.0 is the signed zero."""
    F = m6.FORMATS[fmt]
    mags = m6.mag(np.arange(F.cmax + 1), fmt)
    hit = np.nonzero(mags == abs(value))[0]
    assert hit.size == 1, (value, fmt)
    return int(hit[0]) | (F.sign if np.signbit(value) else 0)


def min_mag(fmt):
    return float(m6.mag(1, fmt))


# (name, (value, scale byte) of payload 0, (value, scale byte) of payload 1): element 0 of block k of the special tensor; every value
# is a magnitude all four formats hold (0.5, 1, 1.5, 2, 4) except the format's own smallest one in "underflow".
def special_cases(fmt):
    return [
        ("tie_down", (2.0, 127), (1.0, 120)),        # mean 1 + 2^-8: halfway, the even neighbour is below (0x3F80)
        ("tie_up", (2.0, 127), (1.5, 121)),          # mean 1 + 3 * 2^-8: halfway, the even neighbour is above (0x3F82)
        ("carry", (4.0, 127), (-1.0, 119)),          # mean 2 - 2^-9: rounds up into the next exponent (0x4000)
        ("subnormal", (1.5, 0), (0.5, 0)),           # mean 2^-127: a bf16 subnormal (0x0040)
        ("minus_zero", (-0.0, 127), (-0.0, 127)),    # +0 + -0 + -0 = +0: the mean of two -0 is +0; plain R = 1 keeps the -0
        ("nan_block", (1.0, 255), (1.0, 127)),       # scale byte 0xFF: the NaN, 0x7FC0 after narrowing
        ("largest", (4.0, 252), (3.0, 252)),         # the sum 7 * 2^125 is finite, the mean 1.75 * 2^126 stays far below bf16's maximum
        ("underflow", (-min_mag(fmt), 0), (0.0, 0)),  # the smallest negative value halved: -0 after narrowing where it lies below 2^-134 (FP8)
    ]


SPECIAL_N = 257      # 9 blocks: one per case and a ragged one
DEC_SIZES = [1, 33, SPECIAL_N, 4097, 8193]
SPECIAL_AT = 2       # the special tensor's place in DEC_SIZES


def decode_payloads(fmt, R, seed=77):
    """R payloads of DEC_SIZES: mx6_contract.payload_set's random codes under the scale bytes 0, 1, 126, 127, 253, 255, with the
    special cases written over element 0 of the first blocks of tensor SPECIAL_AT in payloads 0 and 1 (payloads 2 ... hold +0
    there under scale byte 0) -> [payload][tensor] sections."""
    out = []
    for r in range(R):
        secs = [m6.payload_set(n, fmt, 1, seed=seed + 1000 * r + n)[0] for n in DEC_SIZES]
        sb, code = m6.unpack(secs[SPECIAL_AT], SPECIAL_N, fmt)
        sb, code = np.array(sb, np.uint8), np.array(code, np.int64)
        for k, (_, p0, p1) in enumerate(special_cases(fmt)):
            value, byte = (p0, p1)[r] if r < 2 else (0.0, 0)
            sb[k] = byte
            code[32 * k] = _code_of(value, fmt)
        secs[SPECIAL_AT] = m6.pack(sb, code, fmt)
        out.append(secs)
    return out


def special_means(fmt, R=2, plain=False):
    """{case name: (float32 mean bits, bf16 bits)} of the special elements at R payloads (plain: payload 0 alone, as it is)."""
    pl = decode_payloads(fmt, 1 if plain else R)
    secs = [p[SPECIAL_AT] for p in pl]
    m = m6.decode_mean(secs, SPECIAL_N, fmt, plain)
    h = narrow(m)
    return {name: (int(m6.bits_of(m)[32 * k]), int(h[32 * k])) for k, (name, _, _) in enumerate(special_cases(fmt))}


def rotated_payloads(n, fmt, R, seed):
    """mxr_contract.payloads over all four formats: random codes over every code value under the scale bytes 110 ... 140, so that
    the sums inside a rotation block are finite and round; payload 0 holds scale byte 0xFF in the tensor's last MX block and (from
    two rotation blocks on) in the last MX block of its second rotation block, whose 256 outputs are all the NaN; the third
    rotation block (if any) is a hand-built tie."""
    rs = np.random.RandomState(seed)
    F = m6.FORMATS[fmt]
    nb = -(-n // m6.BLOCK)
    secs = []
    for r in range(R):
        code = rs.randint(0, 1 << F.bits, nb * m6.BLOCK)
        code[:1 << F.bits] = np.arange(1 << F.bits)[:nb * m6.BLOCK]
        sb = rs.randint(110, 141, nb).astype(np.uint8)
        if r == 0:
            sb[-1] = 255
            if n >= 512:
                sb[15] = 255
        if n >= 768:      # the third rotation block: ONE non-zero element, so all 256 outputs are +-(its mean / 16), exactly
            code[16 * m6.BLOCK:24 * m6.BLOCK], sb[16:24] = 0, 127
            if r < 2:     # (32 + 2^-3) / 2 / 16 = 1 + 2^-8 at R = 2: a tie whose even neighbour is below, 256 times
                sb[16], code[16 * m6.BLOCK] = (131, _code_of(2.0, fmt)) if r == 0 else (124, _code_of(1.0, fmt))
        secs.append(m6.pack(sb, code, fmt))
    return secs
