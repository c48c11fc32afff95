"""Inputs and expectations of tests/test_gpu_hsq_dequant.py, in numpy float32, one operation at a time: the level quantiser
(probabilistic_scalar_compressor.py:12-27, LevelQuant of csrc/hsq_levels_common.hpp), its decode (rq_contract.level_norm ==
level_to_norm of csrc/gq_common.hpp), the codebook gather (rq_contract.stage_decode) and the mean as include/gq_hsq.h and
mean_div of csrc/gq_common.hpp state it.  Nothing here comes from a kernel.  tests/test_hsq_dequant_contract.py checks what
the inputs claim without a GPU."""
import numpy as np

import rq_contract as rc

F = np.float32
D, K = 16, 256
MS = (67, 1)      # a whole tile, a 3-subvector tail (one whole group of four short of a tile's 17th), and a lone subvector

# (lb, ub) of a tensor.  "tiny": level * range and its scaled value are subnormal; "sub": lb itself is subnormal.
REGIMES = {
    "ordinary": (F(-1.5), F(2.25)),
    "tiny": (F(0.0), F(2.0 ** -130)),
    "sub": (F(2.0 ** -140), F(2.0 ** -128)),
    "flat": (F(0.75), F(0.75)),
}


def top_level(n_bit, rounding):
    return (1 << n_bit) if rounding else (1 << n_bit) - 1


def levels_of_launch(n_bit, R, start=0):
    """Byte levels of a decode launch, [payload][tensor]: slot j of the running count over (payload, tensor, subvector) holds
    level (start + j) mod 2**n_bit; the R = 3 launch of a case goes on where its R = 1 launch ended.  n_bit = 6: every level
    0..63 is in every launch; n_bit = 8: the 68 slots of a payload cannot hold 256 levels, the two launches of a case
    (R = 1, then R = 3: 68 + 204 slots) hold every level between them, and `start` (level_start: another one per range)
    moves the plain launch's window so that the ranges between them put every level through it too."""
    n, j, out = 1 << n_bit, start + (0 if R == 1 else sum(MS)), []
    for _ in range(R):
        row = []
        for M in MS:
            row.append(((j + np.arange(M)) % n).astype(np.uint8))
            j += M
        out.append(row)
    return out


def level_start(regime):
    """Where a range's level sequence starts: 0, 64, 128, 192 -- four windows of 68 that cover 0..255."""
    return 64 * sorted(REGIMES).index(regime)


def norm(levels, n_bit, lb, ub):
    return rc.level_norm(np.ascontiguousarray(levels, dtype=np.uint8), 1, n_bit, lb, ub)


def mean(acc, R, plain):
    """mean_div: (+0 + acc) / R, a correctly rounded division; plain: the decode as it is."""
    if plain:
        return acc
    with np.errstate(all="ignore"):
        return (F(0.0) + acc) / F(R)


def decode_mean(payloads, cb, n_bit, plain):
    """payloads: R tuples (codes, levels, (lb, ub)) of one tensor, ascending -> f32[M, d]."""
    acc = None
    with np.errstate(all="ignore"):
        for codes, levels, (lb, ub) in payloads:
            dec = rc.stage_decode(codes, norm(levels, n_bit, lb, ub), cb)
            acc = dec if acc is None else acc + dec
    return mean(acc, len(payloads), plain)


def quantise(u, lb, ub, n_bit, r=None):
    """probabilistic_scalar_compressor.py:12-27: levels of the projections u (r: the draws, None = rounding off)."""
    u = rc.f32(u)
    if F(lb) - F(ub) == 0:
        return np.zeros(u.shape, np.int32)
    with np.errstate(all="ignore"):
        s = F(1 << n_bit)
        q = (u - F(lb)) / (F(ub) - F(lb))
        x = np.abs(q) * s
        c = np.minimum(np.maximum(x, F(0.0)), s - F(1.0))
        l = c.astype(np.int32)
        if r is not None:
            l = l + ((x - l.astype(np.float32)) > rc.f32(r)).astype(np.int32)
    return l


def pack6(levels):
    """GQ_LEVELS_PACKED6: four 6-bit levels per three bytes, slots past the end 0 -> uint8[3 * ceil(M / 4)]."""
    l = np.zeros((len(levels) + 3) // 4 * 4, np.uint32)
    l[:len(levels)] = np.asarray(levels).astype(np.uint32) & 63
    w = l[0::4] | (l[1::4] << 6) | (l[2::4] << 12) | (l[3::4] << 18)
    return np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], axis=1).astype(np.uint8).reshape(-1)


def projections(M, lb, ub, n_bit, seed):
    """u of one tensor with min lb and max ub exactly: lb + (ub - lb) * t for t on a grid that lands on every level, the two
    ends first.  (flat: all lb.)"""
    rs = np.random.RandomState(seed)
    s = 1 << n_bit
    t = (rs.randint(0, s, size=M) + rs.rand(M)) / s
    t[0], t[-1] = 1.0, 0.0
    if M > 2 * s:
        t[1:s + 1] = (np.arange(s) + 0.5) / s
    with np.errstate(all="ignore"):
        u = F(lb) + (F(ub) - F(lb)) * t.astype(np.float32)
    u = np.minimum(np.maximum(rc.f32(u), F(lb)), F(ub))
    u[0], u[-1] = ub, lb
    return rc.f32(u)
