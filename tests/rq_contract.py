"""include/gq_rq.h restated in numpy: float32 operations one at a time, so that every rounding is visible, and the CPU oracle's
gq_oracle_pvq_encode for the sampler.  TEST INFRASTRUCTURE ONLY.  What libgq_rq.so's two launches -- gq_rq_encode2_batched and
gq_rq_decode_sum_batched -- are held to bit for bit by tests/test_gpu_rq_contract.py; this file's own checks, and one assertion
for every claim made about an input built here, are tests/test_rq_contract.py.

Also here, because both test files need them: the wire / tile / `out` layout of a hand-built group (Group) and the inputs of
every GPU test (the *_case functions), built by numpy alone so that the CPU file can assert their preconditions."""
import os

import numpy as np

import oracle

F = np.float32
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1
RQ_CODE_SALT = 0xA0761D6478BD642F        # PW_SAMPLER_SALT of csrc/pvq_walk.hpp
RQ_LEVEL2_SALT = 0xE7037ED1A0B428DB
GQ_ODD_DIV_MAX = 4097                    # csrc/gq_common.hpp
MEAN, PLAIN, ERROR = 0, 1, 2             # GQ_RQ_* of include/gq_rq.h
LEVEL_DTYPE = {0: np.float32, 1: np.uint8, 2: np.uint16, 4: np.uint32}
ENC_WAVES = 4                            # csrc/hsq_encode_common.hpp: waves of an encode workgroup
DEC_THREADS = 256                        # csrc/rq_batched.hip
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def bits(a):
    return f32(a).view(np.uint32)


def same(a, b):
    """Bitwise equal, except that any NaN equals any NaN."""
    a, b = f32(a), f32(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


# ---- the header, restated -----------------------------------------------------------------------------------------------------
def level_norm(raw, level_bytes, n_bit, lb, ub):
    """The norm a level section's word stands for.  level_bytes == 0: the f32 as it travels.  Otherwise
    RN(RN(RN(float(l) * RN(ub - lb)) * inv_s) + lb), inv_s = 1 / 2**n_bit (level_to_norm of csrc/gq_common.hpp,
    probabilistic_scalar_compressor.py:31-32: the division by s = 2**n_bit is an exact scaling)."""
    if level_bytes == 0:
        return f32(raw)
    raw = np.ascontiguousarray(raw)
    assert raw.dtype == LEVEL_DTYPE[level_bytes], raw.dtype
    with np.errstate(all="ignore"):
        rng = F(ub) - F(lb)
        t = raw.astype(np.float32) * rng
        t = t * F(2.0 ** -n_bit)
        return t + F(lb)


def stage_decode(codes, norms, cb):
    """d_k = RN(codebook_k[code] * norm), [M, d]."""
    with np.errstate(all="ignore"):
        return f32(cb)[np.asarray(codes).astype(np.intp)] * f32(norms)[:, None]


def stage2_input(v, codes1, norm1, cb1):
    """v - RN(cb1[code1] * norm1): the product rounded, then the difference (residual_compressor.py:22) -> [M, d]."""
    d = f32(cb1).shape[1]
    with np.errstate(all="ignore"):
        return f32(v).reshape(-1, d) - stage_decode(codes1, norm1, cb1)


def order_map(u):
    """order_map of csrc/hsq_pf_common.hpp on uint32: an order-preserving image of a float for integer min / max."""
    b = bits(u)
    return np.where(b >> 31 != 0, b ^ np.uint32(M32), b ^ np.uint32(0x80000000)).astype(np.uint32)


def fold_minmax(u):
    """(min, max) of one tensor's u as the launch folds them into seg_minmax: identities 0xFFFFFFFF / 0."""
    u = f32(u)
    assert not np.isnan(u).any()      # (fminf / fmaxf drop a NaN; no input here makes one)
    m = order_map(u)
    return min(M32, int(m.min())), max(0, int(m.max()))


def encode2(v, codes1, norm1, cb1, c_dagger, r):
    """Stage 2's encode of ONE tensor -> (codes uint8[M], u f32[M], (mapped min, mapped max))."""
    x = stage2_input(v, codes1, norm1, cb1)
    codes, u = oracle.pvq_encode(x.reshape(-1), c_dagger, r)
    return codes.astype(np.uint8), u, fold_minmax(u)


def decode_sum(payloads, cb1, cb2, level_bytes, n_bit, mode, v=None):
    """payloads: R tuples (codes1, raw1, (lb1, ub1), codes2, raw2, (lb2, ub2)) of one tensor, ascending.
    x_r = (0 + d1_r) + d2_r;  acc = x_0, acc += x_r;  MEAN: (+0 + acc) / R, a correctly rounded division (R == 1 too);
    PLAIN: x as it is;  ERROR: v - x.  -> f32[M * d]"""
    R = len(payloads)
    assert R >= 1 and (mode == MEAN or R == 1)
    with np.errstate(all="ignore"):
        acc = None
        for c1, r1, (lb1, ub1), c2, r2, (lb2, ub2) in payloads:
            d1 = stage_decode(c1, level_norm(r1, level_bytes, n_bit, lb1, ub1), cb1)
            d2 = stage_decode(c2, level_norm(r2, level_bytes, n_bit, lb2, ub2), cb2)
            x = (F(0.0) + d1) + d2
            acc = x if acc is None else acc + x
        if mode == MEAN:
            acc = (F(0.0) + acc) / F(R)
        elif mode == ERROR:
            acc = f32(v).reshape(acc.shape) - acc
    assert acc.dtype == np.float32
    return acc.reshape(-1)


def resolve_seed(seed, step):
    """resolve_seed of csrc/gq_common.hpp: the launch's seed from the { seed, step } words (splitmix64 of the step)."""
    z = (step + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (seed ^ z ^ (z >> 31)) & M64


# ---- the bounds the multi-tile tests assert -------------------------------------------------------------------------------------
def pw_lds_bytes(d):
    """PwShape<D>::LDS_BYTES of csrc/pvq_walk.hpp."""
    rs = d + 4
    si = 16 * rs + 4
    return (16 * si + ENC_WAVES * 64 * rs) * 4


def encode_wave_bound(d, cus):
    """Twice the most waves launch_encode2 can have resident, whatever the occupancy query answers: above it
    ntiles / waves >= 2, so every wave's run holds at least two tiles."""
    return 2 * cus * ENC_WAVES * min(8, (160 * 1024) // pw_lds_bytes(d))


def decode_pass_slots(d, cus):
    """Padded subvector slots one pass of rq_decode_sum_kernel's grid covers: above it a workgroup strides at least twice."""
    return cus * 8 * (DEC_THREADS // (d // 4))


# ---- codebooks ------------------------------------------------------------------------------------------------------------------
_CB = {}


def codebooks(d, K):
    """(cb1, c_dagger, cb_other): the first K codewords of the d-dimensional learned codebook, their own pseudo-inverse (as
    tests/test_gpu_pvq.py builds a K < 256 codebook), and a second image (the rows reversed and negated) for cb1 != cb2."""
    if (d, K) not in _CB:
        from gq_amd.codebook import load_codebook
        cb = f32(load_codebook(d, 256)[:K])
        cdag = f32(np.linalg.pinv(cb.T).astype(np.float32))
        assert cdag.shape == cb.shape
        _CB[(d, K)] = (cb, cdag, f32(-cb[::-1]))
    return _CB[(d, K)]


# ---- a hand-built group: wire, tiles, out -----------------------------------------------------------------------------------------
def _up(x, a=16):
    return (x + a - 1) // a * a


class Group(object):
    """Tensors of Ms subvectors as two HSQ sections each (codes | levels | lb, ub, stage 1 then stage 2), every section 16-byte
    aligned with at least 16 bytes that belong to nobody in front of it and behind it; one tile space; every tensor's span of
    `out` (column 6) with OUT_GAP floats that belong to nobody round it."""
    OUT_GAP = 8

    def __init__(self, Ms, d, K, level_bytes, n_bit):
        self.Ms, self.d, self.K, self.level_bytes, self.n_bit = [int(m) for m in Ms], d, K, level_bytes, n_bit
        self.nseg = len(self.Ms)
        self.lvl_size = level_bytes if level_bytes else 4
        lay = np.zeros((2, self.nseg, 8), np.int64)
        off, tile, out_off = 32, 0, self.OUT_GAP
        self.first_tile, self.out_off = [], []
        for s, M in enumerate(self.Ms):
            for k in (0, 1):
                for col, nbytes in ((3, M), (4, M * self.lvl_size), (5, 8)):
                    off = _up(off)
                    lay[k, s, col] = off
                    off = _up(off + nbytes) + 16
                lay[k, s, 1], lay[k, s, 2], lay[k, s, 6] = M, tile, out_off
            self.first_tile.append(tile)
            self.out_off.append(out_off)
            tile += (M + 63) // 64
            out_off += M * d + self.OUT_GAP
        self.layout = lay
        self.ub, self.ntiles, self.out_floats = off, tile, out_off
        self.tile_seg = np.repeat(np.arange(self.nseg, dtype=np.int32), [(M + 63) // 64 for M in self.Ms])
        assert self.tile_seg.size == self.ntiles

    def tables(self, grad_ptrs=None, err_ptrs=None, lo=0, hi=None):
        """The two segment tables of tensors lo .. hi - 1 (int64 [n, 8]), first tiles rebased to the part, and its tile_seg."""
        hi = self.nseg if hi is None else hi
        t = self.layout[:, lo:hi].copy()
        t0 = self.first_tile[lo]
        t1 = self.first_tile[hi] if hi < self.nseg else self.ntiles
        t[:, :, 2] -= t0
        if grad_ptrs is not None:
            t[0, :, 0] = np.asarray(grad_ptrs[lo:hi], np.int64)
        if err_ptrs is not None:
            t[0, :, 7] = np.asarray(err_ptrs[lo:hi], np.int64)
        return t[0], t[1], (self.tile_seg[t0:t1] - lo).astype(np.int32), hi - lo, t1 - t0

    def section(self, s, stage, col):
        """(byte offset, bytes) of tensor s's codes (col 3), levels (4) or (lb, ub) (5) section of stage 0 / 1."""
        M = self.Ms[s]
        return int(self.layout[stage, s, col]), {3: M, 4: M * self.lvl_size, 5: 8}[col]

    def put(self, row, s, stage, codes, raw, lb_ub):
        """One tensor's stage payload into a user's wire (uint8[ub])."""
        o, n = self.section(s, stage, 3)
        row[o:o + n] = np.ascontiguousarray(codes, np.uint8)
        o, n = self.section(s, stage, 4)
        row[o:o + n] = np.ascontiguousarray(raw, LEVEL_DTYPE[self.level_bytes]).view(np.uint8)
        o, n = self.section(s, stage, 5)
        row[o:o + n] = f32(lb_ub).view(np.uint8)

    def mask(self, stages=(0, 1), cols=(3, 4, 5)):
        """True on the bytes of the named sections."""
        m = np.zeros(self.ub, bool)
        for s in range(self.nseg):
            for k in stages:
                for col in cols:
                    o, n = self.section(s, k, col)
                    m[o:o + n] = True
        return m

    def slots(self, s):
        """The slice of the padded index space (u_flat, r_flat) that holds tensor s's subvectors."""
        a = self.first_tile[s] * 64
        return slice(a, a + self.Ms[s])

    def out_mask(self):
        m = np.zeros(self.out_floats, bool)
        for M, o in zip(self.Ms, self.out_off):
            m[o:o + M * self.d] = True
        return m


# ---- inputs of the encode tests -------------------------------------------------------------------------------------------------
SMALL_CYCLE = [1, 63, 64, 65, 127, 129, 200]
TOP_N_BIT = {0: 32, 1: 6, 2: 8, 4: 12}      # the n_bit each level width is tested at (uint8 holds the top level 64, int16 256)


def top_level(n_bit):
    """The largest level the level launch can emit: trunc(clamp(x, 0, s - 1)) + 1 = s = 2**n_bit (a draw below the fraction)."""
    return 1 << n_bit


def multi_tile_Ms(d, cus, total_tiles):
    """A few large tensors with a few hundred small ones (SMALL_CYCLE) between them, total_tiles tiles in all: 300 small tensors
    in four stretches of 75, five large ones round them, the last one taking what is left."""
    small = [SMALL_CYCLE[i % len(SMALL_CYCLE)] for i in range(300)]
    small_tiles = sum((m + 63) // 64 for m in small)
    big_tiles = total_tiles - small_tiles
    assert big_tiles >= 5
    each = big_tiles // 5
    Ms = []
    for k in range(5):
        tiles = each if k < 4 else big_tiles - 4 * each
        Ms.append(tiles * 64 - (k * 13) % 64)      # (ragged ends: the last tile of a large tensor is not full either)
        if k < 4:
            Ms += small[75 * k:75 * (k + 1)]
    return Ms


def multi_tile_totals(d, cus):
    """The two totals of a multi-tile case: just above the bound, and one tile short of twice the bound (a multiple of
    4 * CUs less one is no multiple of the launch's waves, 4 * CUs * resident blocks: waves_with_one_more is neither 0 nor all)."""
    b = encode_wave_bound(d, cus)
    return b + 37, 2 * b - 1


def _stage1(rs, M, K, level_bytes, n_bit, scale, kind="ordinary"):
    """Stage 1 of one tensor as it can arrive: random codes below K, random levels with level 0 and the top level present,
    bounds of the given kind -> (codes, raw, (lb, ub))."""
    codes = rs.randint(0, K, size=M).astype(np.uint8)
    if level_bytes == 0:
        raw = f32(rs.randn(M) * scale)
        if kind == "zero":
            raw[:] = 0.0
        return codes, raw, (F(0.0), F(0.0))
    top = top_level(n_bit)
    raw = rs.randint(0, top + 1, size=M)
    raw[-1] = 0
    raw[0] = top      # (a tensor of one subvector carries the top level)
    if M > 2:
        raw[1] = 0
        raw[M // 2] = top
    lb, ub = {"ordinary": (F(-1.5 * scale), F(2.25 * scale)), "equal": (F(0.75 * scale), F(0.75 * scale)), "zero": (F(0.0), F(0.0))}[kind]
    return codes, raw.astype(LEVEL_DTYPE[level_bytes]), (lb, ub)


def encode_case(Ms, d, K, level_bytes, seed, kinds=("ordinary",), zero_rows=True, edge_draws=True):
    """Inputs of one encode2 launch and what the contract says it leaves: per tensor v, stage 1 (hand-built), the draws;
    `codes`, `u` and `minmax` from encode2().  zero_rows: every seventh subvector (and subvector 0) has v = RN(cb1[c] * norm), a
    residual of exactly zero.  edge_draws: draws 0, 1 and 1.5 among the uniform ones.  The oracle runs ONCE over all tensors."""
    n_bit = TOP_N_BIT[level_bytes]
    G = Group(Ms, d, K, level_bytes, n_bit)
    cb1, cdag, _ = codebooks(d, K)
    rs = np.random.RandomState(seed)
    T = []
    for s, M in enumerate(G.Ms):
        scale = 10.0 ** ((s % 5) - 3)
        kind = kinds[s % len(kinds)]
        codes1, raw1, (lb, ub) = _stage1(rs, M, K, level_bytes, n_bit, scale, kind)
        norm1 = level_norm(raw1, level_bytes, n_bit, lb, ub)
        v = f32(rs.randn(M, d) * scale)
        zr = np.zeros(M, bool)
        if zero_rows:
            zr[::7] = True
            v[zr] = stage_decode(codes1, norm1, cb1)[zr]
        r = rs.rand(M).astype(np.float32)
        if edge_draws:
            r[M // 3] = 0.0
            if M > 4:
                r[M // 4], r[M - 2] = 1.0, 1.5
        T.append(dict(M=M, v=v.reshape(-1), codes1=codes1, raw1=raw1, lb=lb, ub=ub, norm1=norm1, r=r, zero=zr, kind=kind))
    x = np.concatenate([stage2_input(t["v"], t["codes1"], t["norm1"], cb1) for t in T])
    codes, u = oracle.pvq_encode(x.reshape(-1), cdag, np.concatenate([t["r"] for t in T]))
    at = 0
    for t in T:
        t["codes"], t["u"] = codes[at:at + t["M"]].astype(np.uint8), u[at:at + t["M"]]
        t["minmax"] = fold_minmax(t["u"])
        at += t["M"]
    return G, T


# ---- inputs of the decode tests -------------------------------------------------------------------------------------------------
def _payload(rs, M, K, level_bytes, n_bit, scale):
    """One stage's payload written by numpy: random codes below K, random levels, chosen bounds."""
    codes = rs.randint(0, K, size=M).astype(np.uint8)
    if level_bytes == 0:
        return codes, f32(rs.randn(M) * scale), (F(0.0), F(0.0))
    raw = rs.randint(0, top_level(n_bit) + 1, size=M).astype(LEVEL_DTYPE[level_bytes])
    a, b = sorted(f32(rs.randn(2) * scale))
    return codes, raw, (a, b)


def decode_case(Ms, d, K, level_bytes, R, seed, two_images=False, special=None):
    """R payloads of a ragged group, written by numpy -> (Group, P, cb1, cb2) with P[s][r] the tuple decode_sum() takes.
    special: "zeros" (one image) -- tensor 1: both stages decode the negative codeword elements to -0 in every payload; tensor
    2: stage 2 decodes to -d1 (_cancel) -- and "range" (level_bytes 0): norms that make the sums subnormal, norms near
    FLT_MAX / R, and +-inf / NaN in one payload."""
    assert not (special == "zeros" and two_images)
    n_bit = TOP_N_BIT[level_bytes]
    G = Group(Ms, d, K, level_bytes, n_bit)
    cb1, _, other = codebooks(d, K)
    cb2 = other if two_images else cb1
    rs = np.random.RandomState(seed)
    P = []
    for s, M in enumerate(G.Ms):
        rows = []
        for r in range(R):
            scale = 10.0 ** (((s + r) % 5) - 3)
            p1 = _payload(rs, M, K, level_bytes, n_bit, scale)
            p2 = _payload(rs, M, K, level_bytes, n_bit, scale * 0.125)
            if special == "zeros" and s == 1:       # norm 0 in both stages, the same code: the negative elements are -0 twice
                z = np.zeros(M, LEVEL_DTYPE[level_bytes])
                p1 = (p1[0], z, (F(0.0), F(0.0)))
                p2 = (p1[0].copy(), z.copy(), (F(0.0), F(0.0)))
            if special == "zeros" and s == 2:       # d2 = -d1: the two stages cancel exactly
                p2 = _cancel(p1, level_bytes, K, two_images)
            if special == "range":
                p1, p2 = _range_rows(rs, M, K, r, R)
            rows.append(p1 + p2)
        P.append(rows)
    return G, P, cb1, cb2


def _cancel(p1, level_bytes, K, two_images):
    """Stage 2's payload that decodes to -d1.  One image: the same code with the norm negated -- f32 norms: -norm; levels: the
    bounds negated, level * (-(ub - lb)) * inv_s + (-lb) is -(level * (ub - lb) * inv_s + lb) rounding for rounding.  Two images
    (cb2 = -cb1 reversed): code K - 1 - c names -cb1[c], the norm stays."""
    codes, raw, (lb, ub) = p1
    if two_images:
        return (K - 1 - codes).astype(np.uint8), raw.copy(), (lb, ub)
    if level_bytes == 0:
        return codes.copy(), f32(-raw), (lb, ub)
    return codes.copy(), raw.copy(), (F(-lb), F(-ub))


FLT_MAX = float(np.finfo(np.float32).max)


def _range_rows(rs, M, K, r, R):
    """f32 norms by subvector class (index mod 4): 0 -- tiny, the sums and their means subnormal; 1 -- up to 2.5 FLT_MAX / R,
    sums that stay finite and sums that overflow; 2 -- ordinary; 3 -- ordinary, but payload min(1, R - 1) carries
    +inf in stage 1 and -inf or NaN in stage 2.  Class 1 keeps its codes and its signs from payload to payload, so that the
    sums grow: to finite values near FLT_MAX where the codeword's element is small, past it where it is not."""
    cls = np.arange(M) % 4
    n1, n2 = f32(rs.randn(M) * 1e-2), f32(rs.randn(M) * 1e-3)
    c1, c2 = rs.randint(0, K, size=M).astype(np.uint8), rs.randint(0, K, size=M).astype(np.uint8)
    tiny = cls == 0
    n1[tiny] = f32(rs.randn(M) * 3e-39)[tiny]
    n2[tiny] = f32(rs.randn(M) * 2e-41)[tiny]
    big = cls == 1
    with np.errstate(all="ignore"):
        n1[big] = f32(rs.uniform(0.5, 1, M) * (2.5 * FLT_MAX / R))[big]
        n2[big] = f32(rs.uniform(-1, 1, M) * (FLT_MAX / R))[big]
    c1[big] = (np.arange(M) % K).astype(np.uint8)[big]
    if r == min(1, R - 1):
        bad = cls == 3
        n1[bad] = np.inf
        n2[bad] = np.where(np.arange(M) % 8 == 3, F(-np.inf), F(np.nan))[bad]
    z = (F(0.0), F(0.0))
    return (c1, n1, z), (c2, n2, z)


def gathered_rows(G, P, R, extra=48, seed=1):
    """The R users' wires, user_stride_bytes = one payload + `extra`, every byte outside the sections random -> uint8[R, ub + extra]"""
    rows = np.random.RandomState(seed).randint(0, 256, size=(R, G.ub + extra)).astype(np.uint8)
    for s in range(G.nseg):
        for r in range(R):
            c1, r1, b1, c2, r2, b2 = P[s][r]
            G.put(rows[r], s, 0, c1, r1, b1)
            G.put(rows[r], s, 1, c2, r2, b2)
    return rows


def decode_want(G, P, cb1, cb2, mode, vs=None):
    """What the contract says every tensor's span of `out` (or its error buffer) holds."""
    return [decode_sum(P[s], cb1, cb2, G.level_bytes, G.n_bit, mode, None if vs is None else vs[s]) for s in range(G.nseg)]


RAGGED = [1, 63, 64, 65, 700, 7, 128, 300]
DECODE_RS = [1, 2, 3, 5, 7, 8, 9, 16]
SERVED = [(K, d) for K in (32, 64, 96, 224, 256) for d in (8, 16, 32)]
SERVED_MS = [1, 63, 64, 65, 2500, 7, 129]
WALK_GROUPS = [(16, 256, [1, 63, 64, 65, 1500, 7]), (8, 64, [65, 700]), (32, 256, [65, 700])]


def decode_multi_pass_Ms(d, cus):
    """A ragged list of more than decode_pass_slots(d, cus) padded slots: small tensors (SMALL_CYCLE) between stretches of
    3000 subvectors, so that the tile -> tensor lookup changes inside a workgroup's stride."""
    need = decode_pass_slots(d, cus) // 64 + 64
    Ms, tiles, i = [], 0, 0
    while tiles <= need:
        M = 3000 + 17 * i if i % 8 == 0 else SMALL_CYCLE[i % len(SMALL_CYCLE)]
        Ms.append(M)
        tiles += (M + 63) // 64
        i += 1
    return Ms
