"""gq_hsq_decode_sum_batched restated in numpy float32, one operation at a time, for ANY (d, K), code width and level form --
what tests/test_gpu_hsq_decode_contract.py holds the four kernel families of csrc/hsq_batched.hip to at tolerance 0 -- and the
hand-built wires of its cases: the gathered buffer, the 8-column segment table of include/gq_hsq.h and tile_seg, by numpy alone.
TEST INFRASTRUCTURE ONLY.  Nothing here comes from a kernel: the level's norm is rq_contract.level_norm, the codebook gather
rq_contract.stage_decode, the mean hsq_dequant_contract.mean.  tests/test_hsq_decode_contract.py checks without a GPU what the
inputs built here claim (that a wrong order of additions, a multiplication by 1 / R or a fused multiply-add would show)."""
import collections
import functools

import numpy as np

import hsq_dequant_contract as hc
import rq_contract as rc

F = np.float32
CANARY, OUT_FILL, GAP = 0xA5, 7.0, 8
P6 = -6                                   # GQ_LEVELS_PACKED6 of include/gq_hsq.h; the other level forms are their level_bytes: 1, 2, 4, 0 (f32 norms)
LEVEL_NP = {1: np.uint8, P6: np.uint8, 2: np.uint16, 4: np.uint32, 0: np.float32}      # a payload's levels as decode_mean takes them
SMALL_MS = (67, 1, 130, 64)               # whole tiles, tails of 3, 1 and 2 subvectors (nv < 4 in the store), a tensor that ends on a tile
# the same four, then tensors of about thirty tiles with one-subvector tensors between them: 101 tiles.  With the grid capped at a
# handful of workgroups a wave's `cur`, `nxt` and `aft` lie in different tensors, with different `left`
LONG_MS = SMALL_MS + (1900, 1, 2048, 1, 1, 1799)
TABLES = {"small": SMALL_MS, "long": LONG_MS}
REGIME_ORDER = ("ordinary", "tiny", "sub", "flat")


def _up(x, a=16):
    return (x + a - 1) // a * a


def top_level(level, n_bit):
    """The largest level of a form's cases: 2**n_bit (what stochastic rounding reaches) where the width holds it."""
    return (1 << n_bit) if level in (2, 4) else (1 << n_bit) - 1


def level_bytes_of(raw):
    return {np.dtype(np.uint8): 1, np.dtype(np.uint16): 2, np.dtype(np.uint32): 4, np.dtype(np.float32): 0}[raw.dtype]


@functools.lru_cache(maxsize=None)
def codebook(d, K):
    """The first K codewords of the shipped codebook where there is one (d = 8, 16, 32), unit Gaussian rows normalised otherwise."""
    if d in (8, 16, 32) and K <= 256:
        return rc.codebooks(d, K)[0]
    from gq_amd.codebook import normalize_rows
    return rc.f32(normalize_rows(np.random.RandomState(1000 * d + K).standard_normal((K, d)).astype(np.float32))[1])


# ---- the reference ------------------------------------------------------------------------------------------------------------
def decode_acc(payloads, cb, n_bit, reverse=False, fused=False):
    """The sum of the payloads' decodes before the mean -> f32[M, d].  payloads: R tuples (codes, levels, (lb, ub)) of one tensor;
    the levels' dtype is their form (LEVEL_NP; packed 6-bit levels come unpacked).  Per payload level * range, * 2^-n_bit, + lb,
    each rounded (rc.level_norm), then codeword * norm (rc.stage_decode); the payloads are added in ascending order, starting
    from the first payload's decode.  reverse / fused are NOT the contract: the sums a kernel with the wrong order, or with
    acc = fma(c, n, acc) behind the first payload (a float64 product and sum, rounded once to float32), would give."""
    acc = None
    with np.errstate(all="ignore"):
        for codes, raw, (lb, ub) in (payloads[::-1] if reverse else payloads):
            n = rc.level_norm(raw, level_bytes_of(raw), n_bit, lb, ub)
            if acc is not None and fused:
                c = rc.f32(cb)[np.asarray(codes).astype(np.intp)]
                acc = (c.astype(np.float64) * n.astype(np.float64)[:, None] + acc.astype(np.float64)).astype(np.float32)
                continue
            dec = rc.stage_decode(codes, n, cb)
            acc = dec if acc is None else acc + dec
    return acc


def decode_mean(payloads, cb, n_bit, plain):
    """(+0 + acc) / R, a correctly rounded division; plain: R = 1 exactly as decoded, a -0 stays -0."""
    assert not plain or len(payloads) == 1
    return hc.mean(decode_acc(payloads, cb, n_bit), len(payloads), plain)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.sqrt(((a - b) ** 2).sum()) / np.sqrt((b ** 2).sum()))


# ---- the wire ------------------------------------------------------------------------------------------------------------------
class Wire(object):
    """R users' payloads of the tensors Ms, every payload with its own codes, levels and (lb, ub).

    One payload: per tensor codes | levels | (lb, ub), every section 16-byte aligned and padded to 16 bytes as gq_amd.codecs pads
    it, with 16 more bytes that belong to nobody behind it; every byte that is not a section's is CANARY (the padding the
    word-wide loads read included).  `buf`: 16 canary bytes, the R payloads `P` bytes apart, 16 canary bytes.  `table`: the 8
    columns of include/gq_hsq.h [ptr, M, first tile, codes, levels, (lb, ub), out, err].  Every tensor's span of `out` has GAP
    floats that belong to nobody round it and starts on a multiple of out_align floats (1: also off it)."""

    def __init__(self, Ms, d, K, code_bytes, level, n_bit, R, regimes, seed, out_align=4):
        self.Ms, self.d, self.K, self.code_bytes, self.level, self.n_bit, self.R = tuple(int(m) for m in Ms), d, K, code_bytes, level, n_bit, R
        self.cb = codebook(d, K)
        self.lead = 16
        rows, self.sections, off, tile = [], [], 0, 0
        out = GAP + (1 if out_align == 1 else 0)
        for s, M in enumerate(self.Ms):
            at = []
            for nbytes in (M * code_bytes, self.level_section_bytes(M), 8):
                at.append(off)
                self.sections.append((s, off, nbytes))
                off = _up(off + nbytes) + 16
            rows.append([0, M, tile, at[0], at[1], at[2], out, 0])
            tile += (M + 63) // 64
            out = _up(out + M * d + GAP, out_align)
        self.table, self.P, self.out_floats, self.ntiles = np.array(rows, np.int64), off, out, tile
        self.tile_seg = np.repeat(np.arange(len(self.Ms), dtype=np.int32), [(M + 63) // 64 for M in self.Ms])
        self._fill(regimes, seed)

    def level_section_bytes(self, M):
        return 3 * ((M + 3) // 4) if self.level == P6 else M * {1: 1, 2: 2, 4: 4, 0: 4}[self.level]

    def regime_of(self, s):
        return self.regimes[s % len(self.regimes)]

    def bounds(self, s, r):
        """(lb, ub) of tensor s in payload r: the regime's, lb scaled by 1, 1/2, 3/4, 1/4 and ub by 1, 9/8, 5/4 from payload to
        payload (an exact scaling: "tiny" keeps lb = 0, "sub" a subnormal lb); "flat": lb = ub."""
        lb, ub = hc.REGIMES[self.regime_of(s)]
        lb, ub = F(lb * F((1.0, 0.5, 0.75, 0.25)[r % 4])), F(ub * F((1.0, 1.125, 1.25)[r % 3]))
        return (ub, ub) if self.regime_of(s) == "flat" else (lb, ub)

    def _fill(self, regimes, seed):
        """Codes: uniform below K, but subvector 0 of every tensor carries in every payload the first codeword that has a negative
        element, at level 0: in the "tiny" regime (lb = 0) that element decodes to -0 in every payload.  Levels: the free slots
        of the running count over (payload, tensor, subvector) hold level j mod (top + 1).  f32 norms: Gaussians with a zero, and
        (lb, ub) = NaN, which nothing may read into the result."""
        self.regimes = tuple(regimes)
        rs = np.random.RandomState(seed)
        nlev = top_level(self.level, self.n_bit) + 1
        c0 = int(np.nonzero((self.cb < 0).any(axis=1))[0][0])
        ctype = np.uint8 if self.code_bytes == 1 else np.int32
        self.buf = np.full(self.lead + self.R * self.P + 16, CANARY, np.uint8)
        self.payloads = [[] for _ in self.Ms]
        j = 0
        for r in range(self.R):
            base = self.lead + r * self.P
            for s, M in enumerate(self.Ms):
                codes = rs.randint(0, self.K, size=M).astype(ctype)
                codes[0] = c0
                if self.level == 0:
                    raw = rc.f32(rs.standard_normal(M) * 0.37)
                    raw[0] = 0.0
                    lb, ub = F(np.nan), F(np.nan)
                    section = raw.view(np.uint8)
                else:
                    raw = np.zeros(M, LEVEL_NP[self.level])
                    raw[1:] = (j + np.arange(M - 1)) % nlev
                    j += M - 1
                    lb, ub = self.bounds(s, r)
                    section = hc.pack6(raw) if self.level == P6 else raw.view(np.uint8)
                _, co, lo, bo = self.table[s, 2:6]
                self.buf[base + co: base + co + M * self.code_bytes] = codes.view(np.uint8)
                self.buf[base + lo: base + lo + len(section)] = section
                self.buf[base + bo: base + bo + 8] = np.array([lb, ub], np.float32).view(np.uint8)
                self.payloads[s].append((codes, raw, (lb, ub)))

    def levels_seen(self):
        return set(np.concatenate([p[1] for rows in self.payloads for p in rows]).tolist())

    def expected(self, per_tensor):
        """`out` as a launch must leave it: per_tensor(payloads of tensor s) -> f32[M, d] in every span, OUT_FILL elsewhere."""
        want = np.full(self.out_floats, OUT_FILL, np.float32)
        for s, M in enumerate(self.Ms):
            o = int(self.table[s, 6])
            want[o: o + M * self.d] = per_tensor(self.payloads[s]).reshape(-1)
        return want

    @property
    def plain(self):
        return self.R == 1

    @functools.lru_cache(maxsize=None)
    def want(self):
        """The contract's `out` (computed once, shared, never written)."""
        w = self.expected(lambda p: decode_mean(p, self.cb, self.n_bit, self.plain))
        w.setflags(write=False)
        return w

    def spans(self):
        m = np.zeros(self.out_floats, bool)
        for s, M in enumerate(self.Ms):
            m[int(self.table[s, 6]): int(self.table[s, 6]) + M * self.d] = True
        return m


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# table: a key of TABLES; level: 1 / 2 / 4 / 0 / P6; regimes: "mixed" (tensor s in REGIME_ORDER[(s + R) % 4]: every launch
# holds every range) or "ordinary"; R = 1 is the plain decode
Case = collections.namedtuple("Case", "table d K code_bytes level n_bit R regimes")


def case_id(c):
    lv = {1: "u8", 2: "u16", 4: "i32", 0: "f32", P6: "p6"}[c.level]
    return "%s-d%d-K%d-c%d-%s-n%d-R%d%s" % (c.table, c.d, c.K, c.code_bytes, lv, c.n_bit, c.R, "" if c.regimes == "mixed" else "-" + c.regimes)


D16_FORMS = ((1, 6), (1, 8), (P6, 6))                      # (level form, n_bit) of the d = 16 / K <= 256 kernels
D16_RS = tuple(range(1, 17)) + (17, 24, 33)                  # every compile-time R; the chunked kernel: a short last chunk, whole chunks, more than four
D16_CASES = [Case("small", 16, 256, 1, lv, nb, R, "mixed") for lv, nb in D16_FORMS for R in D16_RS]
D16_CASES += [Case("small", 16, 64, 1, 1, 6, 3, "mixed"), Case("small", 16, 64, 1, P6, 6, 9, "mixed")]      # a short four-copy image
FMA_FORMS = ((1, 8), (P6, 6))
FMA_LOOSE = [Case("small", 16, 256, 1, lv, nb, R, "ordinary") for lv, nb in FMA_FORMS for R in (2, 4, 8, 16)]     # served by the fused kernels
FMA_EXACT = [Case("small", 16, 256, 1, lv, nb, R, "ordinary") for lv, nb in FMA_FORMS for R in (3, 5, 17)]        # the flag is ignored
FMA_EXACT += [Case("small", 32, 256, 1, 1, 8, 4, "ordinary"), Case("small", 16, 256, 1, 2, 8, 4, "ordinary"),
              Case("small", 32, 256, 1, 2, 8, 2, "ordinary")]
TILE_SHAPES = ((8, 1), (8, 2), (32, 1), (32, 2), (16, 2))
TILE_RS = (1, 2, 3, 4, 8, 9, 17)                             # RB = 0 / 2 / 4, a whole staging chunk, one over, three chunks
TILE_CASES = [Case("small", d, 256, 1, lv, 8, R, "mixed") for d, lv in TILE_SHAPES for R in TILE_RS]
ANY_SHAPES = ((12, 100, 1, 1), (5, 5, 1, 1), (16, 512, 4, 1), (16, 512, 4, 2), (16, 512, 4, 4), (20, 1024, 4, 1), (12, 100, 1, 0), (16, 512, 4, 0))
ANY_CASES = [Case("small", d, K, cbytes, lv, 8, R, "mixed") for d, K, cbytes, lv in ANY_SHAPES for R in (1, 3)]
STEADY_RS = (1, 3, 4, 6, 9, 13, 16, 17)                      # one R per workgroup shape, the counts no other test runs, the chunked kernel
STEADY_CASES = [Case("long", 16, 256, 1, lv, nb, R, "mixed") for lv, nb in ((1, 8), (P6, 6)) for R in STEADY_RS]
STEADY_CASES += [Case("long", d, 256, 1, lv, 8, R, "mixed") for d, lv in ((32, 2), (8, 1)) for R in (1, 3, 9)]
STEADY_CASES += [Case("long", 12, 100, 1, 1, 8, R, "mixed") for R in (1, 3)]
EXACT_CASES = D16_CASES + TILE_CASES + ANY_CASES + STEADY_CASES + FMA_EXACT
ALL_CASES = EXACT_CASES + FMA_LOOSE


def stores_float4(c):
    """Every dispatch but the any-shape kernel's one-float form (d % 4 != 0) stores float4: out offsets are multiples of 4."""
    return c.d % 4 == 0


@functools.lru_cache(maxsize=None)
def wire_of(c):
    regimes = ("ordinary",) if c.regimes == "ordinary" else tuple(REGIME_ORDER[(k + c.R) % 4] for k in range(4))
    seed = 7919 * c.R + 31 * c.d + c.K + 3 * c.n_bit + 11 * (c.level % 7) + c.code_bytes
    return Wire(TABLES[c.table], c.d, c.K, c.code_bytes, c.level, c.n_bit, c.R, regimes, seed, out_align=4 if stores_float4(c) else 1)


# ---- the single-tensor level quantiser's third trip -----------------------------------------------------------------------------
LEVELS_M = 3 * 4 * 256 * 4 + 7      # four workgroups (the grid's cap at one compute unit) of 256 threads: three or more groups of four each, and a scalar tail
LEVELS_FORMS = ((1, 8, 7), (2, 8, 8), (4, 8, 8), (P6, 6, 5))      # (level form, n_bit with rounding off, n_bit with given draws: the top level is 2**n_bit)


@functools.lru_cache(maxsize=None)
def levels_case(level, n_bit, given):
    """-> (u, r or None, levels, the level section's bytes, (lb, ub)): "ordinary" projections that land on every level."""
    lb, ub = hc.REGIMES["ordinary"]
    u = hc.projections(LEVELS_M, lb, ub, n_bit, seed=n_bit + 40)
    r = np.random.RandomState(n_bit).rand(LEVELS_M).astype(np.float32) if given else None
    l = hc.quantise(u, u.min(), u.max(), n_bit, r)
    section = hc.pack6(l) if level == P6 else l.astype(LEVEL_NP[level]).view(np.uint8)
    return u, r, l, section, (F(u.min()), F(u.max()))
