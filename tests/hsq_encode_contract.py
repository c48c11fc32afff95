"""gq_hsq_encode_batched, gq_hsq_levels_batched and gq_hsq_levels_decode_batched restated in numpy float32, one operation at a
time, and the hand-built inputs of tests/test_gpu_hsq_encode_contract.py: gradients, error buffers, segment tables, wires, u_flat
and seg_minmax by numpy alone.  TEST INFRASTRUCTURE ONLY.  Nothing here comes from a GPU kernel: the encode is
oracle.hsq_encode_scalar (the literal fmaf chain from +0, first maximum of |p|, signed projection) on v = grad + RN(ef_scale *
error); the (min, max) fold rq_contract.order_map / fold_minmax; the levels hsq_dequant_contract.quantise / pack6; their decode
rq_contract.level_norm / stage_decode; the mean hsq_dequant_contract.mean.  The layout of a wire is hsq_decode_contract.Wire's:
every section 16-byte aligned and padded, 16 canary bytes that belong to nobody behind it.
tests/test_hsq_encode_contract.py checks without a GPU what the inputs built here claim."""
import collections
import functools

import numpy as np

import hsq_decode_contract as dc
import hsq_dequant_contract as hc
import oracle
import rq_contract as rc

F = np.float32
CANARY, GAP, FILL, P6 = dc.CANARY, dc.GAP, dc.OUT_FILL, dc.P6
U_FILL = F(-3.0)                          # u_flat before a launch: what a padding slot keeps
E_FILL = F(5.0)                           # an error buffer before a level launch
PREFILTER, PAGED, EXACT = 1, 2, 3         # GQ_BATCH_* of include/gq_hsq.h
PATH_NAME = {PREFILTER: "pf", PAGED: "paged", EXACT: "exact"}
OFF, GIVEN, DEVICE, KEYED = 0, 1, 2, 3    # GQ_RANDOM_*
M32 = 0xFFFFFFFF
MAPPED_NAN = (0x003FFFFF, 0xFFC00000)     # what a NaN projection folds into a tensor's words (include/gq_hsq.h)

# 70 tensors of 1 .. 64 subvectors (every size), one tile each, in front of one of five tiles: a workgroup whose run starts at
# tile 0 meets more tensors than the 64 entries of its LDS (min, max) table
MANY_MS = tuple(1 + (37 * i) % 64 for i in range(70)) + (300,)
RECORDS_MS = (1,) * 390                   # more than the 384 segment records the prefilter kernel keeps in LDS
TABLES = {"small": dc.SMALL_MS, "long": dc.LONG_MS, "many": MANY_MS, "records": RECORDS_MS}
EF_SCALES = (0.75, 0.1)


def _up(x, a=16):
    return (x + a - 1) // a * a


def batch_path(d, K, code_bytes, nseg):
    """batch_path of csrc/gq_api.hip, restated (every d here is <= 104)."""
    if d in (8, 12, 16, 24, 32) and 4 <= K <= 256 and K % 4 == 0 and code_bytes == 1:
        return PREFILTER
    if d in (8, 16, 32) and K > 256 and K % 256 == 0 and code_bytes == 4 and nseg <= 384:
        return PAGED
    return EXACT


def scale_of(s):
    """Tensor s's power of two: 2^-20 .. 2^8, neighbours far apart."""
    return F(2.0 ** (-20 + (5 * s) % 29))


# ---- codebooks with exact ties ---------------------------------------------------------------------------------------------------
def ties(K):
    """(j1, j2, j3): cb[j2] = cb[j1], cb[j3] = -cb[j1].  K >= 512: j1 on the first page, j2 on the second, j3 on the last."""
    if K >= 512:
        return 7, 256 + 9, K - 256 + 11
    return (1, K // 2, K - 1) if K >= 8 else (1, 2, 3)


def page_pair(K):
    """K >= 512: a second pair of equal rows inside the last page."""
    return (K - 256 + 40, K - 256 + 51) if K >= 512 else None


@functools.lru_cache(maxsize=None)
def codebook(d, K):
    cb = dc.codebook(d, K).copy()
    j1, j2, j3 = ties(K)
    cb[j2], cb[j3] = cb[j1], -cb[j1]
    if page_pair(K):
        a, b = page_pair(K)
        cb[b] = cb[a]
    cb.setflags(write=False)
    return cb


def top2_gap(cb, v):
    """Relative gap of the two largest |p| of every row of v, in float64."""
    p = np.sort(np.abs(v.astype(np.float64) @ cb.astype(np.float64).T), axis=1)
    return (p[:, -1] - p[:, -2]) / p[:, -1]


@functools.lru_cache(maxsize=None)
def near_ties(d, K):
    """Rows c_a +- c_b (unit scale): |p_a| = |p_b| in real arithmetic for unit rows, apart only by rounding -- the two largest
    |p| in float64 differ by less than 2^-12 relative.  a and b lie on one page of 256 and (K >= 8) are not rows of the exact
    ties and lie in different groups of four consecutive codewords, so that the prefilter's one rescored group cannot hold both."""
    cb = codebook(d, K)
    rs = np.random.RandomState(77 * d + K)
    taken = (set(ties(K)) | set(page_pair(K) or ())) if K >= 8 else set()      # (K < 8: every row but one is a tie's)
    out = []
    for _ in range(40):
        a, b = rs.randint(0, K, size=(2, 512))
        sign = np.where(rs.rand(512) < 0.5, F(1.0), F(-1.0)).astype(np.float32)
        v = rc.f32(cb[a] + sign[:, None] * cb[b])
        ok = (a != b) & (a // 256 == b // 256) & ~np.isin(a, list(taken)) & ~np.isin(b, list(taken))
        if K >= 8:
            ok &= a // 4 != b // 4
        with np.errstate(all="ignore"):
            ok &= top2_gap(cb, v) < 2.0 ** -12
        out.extend(v[ok])
        if len(out) >= 8:
            break
    assert out, "no near tie for d = %d, K = %d" % (d, K)
    return rc.f32(np.stack(out[:8]))


# ---- rows --------------------------------------------------------------------------------------------------------------------------
KINDS = ("gauss", "zero+", "zero-", "mult", "tie", "tie2", "near", "huge", "tiny", "big")
KIND = {k: i for i, k in enumerate(KINDS)}
# by (lane mod 16); lanes 5 and 58 -- whose norms steer the next tile's scale in the prefilter kernel -- are Gaussian
PATTERN = ("gauss", "gauss", "zero+", "gauss", "mult", "gauss", "tie", "gauss", "near", "gauss", "gauss", "huge", "gauss", "tiny", "zero-", "tie2")
LOGGED = ("near", "tiny")                 # kinds the first pass can never settle, wherever they lie (see kind_of)


def kind_of(s, M, r):
    """The kind of subvector r of tensor s (M subvectors).  A tensor of whole tiles has every kind in every tile; shorter ones
    start the pattern somewhere else each, so that one-subvector tensors between them show every kind.  `huge` rows only in
    every fourth tile: a wave's first tile takes its scale from its largest element, and a huge row there pushes every other row
    of the tile out of the bound's window.  `big` (2^14 times the rest) at lane 5, a lane whose norm steers the next tile's scale."""
    short = M < 64
    lane = (r + (5 * s if short else 0)) % 64
    tile = r // 64 + (s // 16 if short else s)
    k = PATTERN[lane % 16]
    if k == "huge" and tile % 4 != 2:
        k = "gauss"
    if lane == 5 and tile % 4 == 3 and not short:
        k = "big"
    return k


def rows_of(s, M, d, K, seed, scale=None):
    """-> (grad f32[M, d], kinds uint8[M]) of tensor s, all times its power of two `scale` (an exact scaling)."""
    cb, nt = codebook(d, K), near_ties(d, K)
    rs = np.random.RandomState(seed + 7919 * s)
    g = rc.f32(rs.standard_normal((M, d)) * 1e-2)
    kinds = np.array([KIND[kind_of(s, M, r)] for r in range(M)], np.uint8)
    j1, _, j3 = ties(K)
    for r in np.nonzero(kinds)[0]:
        k = KINDS[kinds[r]]
        if k == "zero+":
            g[r] = 0.0
        elif k == "zero-":
            g[r] = -0.0
        elif k == "mult":
            g[r] = F(0.01 * (1.0 + rs.rand())) * cb[rs.randint(K)]
        elif k == "tie":
            g[r] = F(2.0 ** -6) * cb[j1]
        elif k == "tie2":
            g[r] = F(2.0 ** -6) * (cb[page_pair(K)[0]] if page_pair(K) else cb[j3])
        elif k == "near":
            g[r] = F(2.0 ** -6) * nt[rs.randint(len(nt))]
        elif k == "huge":
            g[r] = rc.f32(g[r] * (F(2e-2) / np.abs(g[r]).max())) * F(1e32)       # largest element 2e30
        elif k == "tiny":
            g[r] = g[r] * F(1e-30 if r % 2 else 1e-36)                            # 1e-36: subnormal products
        elif k == "big":
            g[r] = g[r] * F(2.0 ** 14)
    with np.errstate(all="ignore"):
        g = rc.f32(g * (scale_of(s) if scale is None else F(scale)))
    return g, kinds


def errors_of(s, M, d, kinds, seed):
    """The error buffer of tensor s: Gaussian under the Gaussian rows (every eighth of them tiny, ef_scale * error subnormal),
    +0 under the others, so that v = grad + (+0) keeps their kind."""
    rs = np.random.RandomState(seed + 104729 * s + 1)
    e = rc.f32(rs.standard_normal((M, d)) * 1e-2 * scale_of(s))
    e[np.arange(M) % 8 == 3] *= F(1e-37)
    e[kinds != KIND["gauss"]] = 0.0
    return e


def ef_add(grad, err, ef_scale):
    """ps_quantizer.py:35 as include/gq_hsq.h states it: the product rounded, then the add."""
    with np.errstate(all="ignore"):
        p = F(ef_scale) * rc.f32(err)
        return rc.f32(grad) + p


def ef_add_fused(grad, err, ef_scale):
    """NOT the contract: fma(ef_scale, error, grad), rounded once."""
    with np.errstate(all="ignore"):
        return (np.float64(F(ef_scale)) * rc.f32(err).astype(np.float64) + rc.f32(grad).astype(np.float64)).astype(np.float32)


def encode_ref(v, cb, first=True, order="ascending"):
    """(codes int32[M], u f32[M]) of the rows v.  first / order are the contract; the other values are NOT: last maximum; a
    descending or pairwise chain."""
    if first and order == "ascending":
        return oracle.hsq_encode_scalar(rc.f32(v).reshape(-1), cb)
    v, cb = rc.f32(v), rc.f32(cb)
    d = cb.shape[1]
    with np.errstate(all="ignore"):
        if order == "pairwise":
            t = v[:, None, :] * cb[None, :, :]
            while t.shape[2] > 1:
                if t.shape[2] % 2:
                    t = np.concatenate([t, np.zeros(t.shape[:2] + (1,), np.float32)], axis=2)
                t = t[:, :, 0::2] + t[:, :, 1::2]
            p = t[:, :, 0]
        else:
            p = np.zeros((v.shape[0], cb.shape[0]), np.float64)
            for j in (range(d) if order == "ascending" else range(d - 1, -1, -1)):
                p = (cb[None, :, j].astype(np.float64) * v[:, j, None].astype(np.float64) + p).astype(np.float32).astype(np.float64)
            p = p.astype(np.float32)
    a = np.abs(p)
    codes = a.argmax(axis=1) if first else a.shape[1] - 1 - a[:, ::-1].argmax(axis=1)
    return codes.astype(np.int32), p[np.arange(len(p)), codes]


# ---- the layout: one user's wire, the tables, the float buffers ------------------------------------------------------------------
class Layout(object):
    """One user's wire of the tensors Ms -- per tensor codes | levels | (lb, ub), laid out as hsq_decode_contract.Wire lays a
    payload out, then the dense region -- and the spans of a float buffer (gradients, errors, out): GAP floats that belong to
    nobody round every span, spans on multiples of 4 floats where d % 4 == 0 and off them otherwise."""

    def __init__(self, Ms, d, code_bytes, level, dense=()):
        self.Ms, self.d, self.code_bytes, self.level, self.dense = tuple(int(m) for m in Ms), d, code_bytes, level, tuple(dense)
        rows, off, tile = [], 0, 0
        fo = GAP + (0 if d % 4 == 0 else 1)
        self.sections = {}
        for s, M in enumerate(self.Ms):
            at = []
            for name, nbytes in (("codes", M * code_bytes), ("levels", self.level_section_bytes(M)), ("lbub", 8)):
                at.append(off)
                self.sections[(s, name)] = (off, nbytes)
                off = _up(off + nbytes) + 16
            rows.append([0, M, tile, at[0], at[1], at[2], fo, 0])
            tile += (M + 63) // 64
            fo = _up(fo + M * d + GAP, 4 if d % 4 == 0 else 1) + (0 if d % 4 == 0 else s % 2)
        self.dense_off = off + 4                      # (a multiple of 4 only)
        off = self.dense_off
        self.dense_at = []
        for n in self.dense:
            self.dense_at.append(off)
            off += 4 * n
        self.P = _up(off) + 16
        self.table, self.floats, self.ntiles, self.nseg = np.array(rows, np.int64), fo, tile, len(self.Ms)
        self.tile_seg = np.repeat(np.arange(self.nseg, dtype=np.int32), [(M + 63) // 64 for M in self.Ms])
        self.first = self.table[:, 2] * 64            # a tensor's first slot of u_flat / r_flat

    def level_section_bytes(self, M):
        return 3 * ((M + 3) // 4) if self.level == P6 else M * {1: 1, 2: 2, 4: 4, 0: 4}[self.level]

    def span(self, s):
        o = int(self.table[s, 6])
        return slice(o, o + self.Ms[s] * self.d)

    def slots(self, s):
        return slice(int(self.first[s]), int(self.first[s]) + self.Ms[s])

    def floats_of(self, per_tensor, fill=FILL):
        """A float buffer: per_tensor[s] (or None: the span keeps `fill`) in every span, `fill` elsewhere."""
        buf = np.full(self.floats, fill, np.float32)
        for s in range(self.nseg):
            if per_tensor[s] is not None:
                buf[self.span(s)] = rc.f32(per_tensor[s]).reshape(-1)
        return buf

    def flat_of(self, per_tensor, fill=U_FILL):
        """u_flat / r_flat: tensor s at [first tile * 64, + M); the padding slots hold `fill`."""
        buf = np.full(self.ntiles * 64, fill, np.float32)
        for s in range(self.nseg):
            buf[self.slots(s)] = per_tensor[s]
        return buf

    def unpadded_of(self, per_tensor):
        """NOT the contract: u indexed without the tile padding."""
        buf = np.full(self.ntiles * 64, U_FILL, np.float32)
        cat = np.concatenate([rc.f32(x) for x in per_tensor])
        buf[:cat.size] = cat
        return buf

    def put(self, wire, s, name, data):
        off, nbytes = self.sections[(s, name)]
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert data.size == nbytes, (name, data.size, nbytes)
        wire[off: off + nbytes] = data

    def new_wire(self):
        return np.full(self.P, CANARY, np.uint8)

    def code_np(self):
        return np.uint8 if self.code_bytes == 1 else np.int32

    def level_section(self, levels):
        """The bytes of a level section from the levels (or, level form 0, the f32 projections)."""
        if self.level == P6:
            return hc.pack6(levels)
        if self.level == 0:
            return rc.f32(levels).view(np.uint8)
        return np.asarray(levels).astype(dc.LEVEL_NP[self.level]).view(np.uint8)

    def norms(self, levels, n_bit, lb, ub):
        """rq_contract.level_norm of what a section holds (packed levels come unpacked: bytes)."""
        if self.level == 0:
            return rc.f32(levels)
        lv = 1 if self.level == P6 else self.level
        return rc.level_norm(np.asarray(levels).astype(dc.LEVEL_NP[lv]), lv, n_bit, lb, ub)


# ---- encode cases ---------------------------------------------------------------------------------------------------------------------
# ef: None (ef_scale = NaN) or an index into EF_SCALES; special: None or "nonfinite"
ECase = collections.namedtuple("ECase", "table d K code_bytes ef path special")


def ecase_id(c):
    return "%s-%s-d%d-K%d-c%d-%s%s" % (PATH_NAME[c.path], c.table, c.d, c.K, c.code_bytes,
                                       "plain" if c.ef is None else "ef%g" % EF_SCALES[c.ef], "-" + c.special if c.special else "")


def _e(table, d, K, cbytes, ef, special=None):
    return ECase(table, d, K, cbytes, ef, batch_path(d, K, cbytes, len(TABLES[table])), special)


def _both(table, d, K, cbytes):
    """EF off and on; the two ef_scales alternate over the shapes."""
    return [_e(table, d, K, cbytes, None), _e(table, d, K, cbytes, (d + K // 4) % 2)]


PF_CASES = [c for d in (8, 12, 16, 24, 32) for c in _both("small", d, 256, 1)]
PF_CASES += [_e("small", 16, K, 1, i % 2) for i, K in enumerate((4, 32, 64, 132))] + [_e("small", d, 64, 1, None) for d in (8, 32)]
PF_CASES += [_e("records", d, 32, 1, i % 2) for i, d in enumerate((12, 16, 32))]
PAGED_SHAPES = ((8, 512), (16, 512), (16, 768), (32, 512))
PAGED_CASES = [c for d, K in PAGED_SHAPES for c in _both("small", d, K, 4)]
EXACT_SHAPES = ((16, 256, 4), (16, 250, 1), (5, 5, 1), (3, 32, 1), (33, 300, 4), (100, 512, 4), (104, 64, 1))
EXACT_CASES = [c for d, K, cb_ in EXACT_SHAPES for c in _both("small", d, K, cb_)] + _both("records", 16, 512, 4)
NONFINITE_CASES = [_e("small", 16, 256, 1, None, "nonfinite"), _e("small", 16, 512, 4, None, "nonfinite"),
                   _e("small", 12, 101, 1, None, "nonfinite")]
# the grid-capped child's: one workgroup, every wave many tiles across tensors, the (min, max) table's overflow
STEADY_SHAPES = ((16, 256, 1), (8, 256, 1), (32, 256, 1), (12, 256, 1), (16, 64, 1), (16, 512, 4), (32, 512, 4), (12, 101, 1))
STEADY_CASES = [_e(t, d, K, cb_, ef) for t in ("long", "many") for d, K, cb_ in STEADY_SHAPES for ef in (None, (d // 4) % 2)]
ENCODE_CASES = PF_CASES + PAGED_CASES + EXACT_CASES + STEADY_CASES
CHAIN_CASES = [_e("long", 16, 256, 1, 0), _e("long", 16, 512, 4, 1), _e("long", 12, 101, 1, 0)]


class Encode(object):
    """The inputs of an encode case and the state the launch must leave."""

    def __init__(self, c):
        self.c, self.Ms, self.cb = c, TABLES[c.table], codebook(c.d, c.K)
        self.lay = Layout(self.Ms, c.d, c.code_bytes, 1)
        self.ef_scale = None if c.ef is None else EF_SCALES[c.ef]
        seed = 31 * c.d + c.K + 7 * c.code_bytes + (0 if c.ef is None else 1000 * (c.ef + 1))
        self.grads, self.kinds, self.errs = [], [], []
        for s, M in enumerate(self.Ms):
            g, k = rows_of(s, M, c.d, c.K, seed)
            if c.special == "nonfinite" and s == 0:       # one row with an infinity, one with a NaN, in different tiles
                g[9, 3], g[65, c.d - 1] = F(np.inf), F(np.nan)
            self.grads.append(g)
            self.kinds.append(k)
            has = self.ef_scale is not None and s % 3 != 1    # every third tensor has no error buffer
            self.errs.append(errors_of(s, M, c.d, k, seed) if has else None)
        self.v = [g if e is None else ef_add(g, e, self.ef_scale) for g, e in zip(self.grads, self.errs)]
        self.gbuf, self.ebuf = self.lay.floats_of(self.grads), self.lay.floats_of(self.errs)

    def encode(self, v=None, **how):
        """Per tensor (codes, u): ONE oracle call over every row of the case."""
        v = self.v if v is None else v
        codes, u = encode_ref(np.concatenate(v), self.cb, **how)
        cut = np.cumsum(self.Ms)[:-1]
        return list(zip(np.split(codes, cut), np.split(u, cut)))

    @functools.lru_cache(maxsize=None)
    def want(self):
        """-> dict: wire, u_flat, minmax (None in the non-finite case's tensor 0), gbuf, ebuf -- computed once, shared."""
        enc = self.encode()
        wire = self.lay.new_wire()
        for s, (codes, _) in enumerate(enc):
            self.lay.put(wire, s, "codes", codes.astype(self.lay.code_np()))
        mm = np.array([(M32, 0) if np.isnan(u).any() else rc.fold_minmax(u) for _, u in enc], np.uint32)
        out = dict(wire=wire, u_flat=self.lay.flat_of([u for _, u in enc]), minmax=mm, gbuf=self.lay.floats_of(self.v), ebuf=self.ebuf,
                   codes=[c_ for c_, _ in enc], u=[u for _, u in enc])
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return out


@functools.lru_cache(maxsize=None)
def encode_of(c):
    return Encode(c)


# ---- level cases ------------------------------------------------------------------------------------------------------------------------
# level: 1 / 2 / 4 / 0 / P6; mode: OFF / GIVEN (bit for bit), DEVICE / KEYED (the draws' cases); route: the launcher of
# csrc/gq_api.hip the case is for (an id only)
LCase = collections.namedtuple("LCase", "table d K code_bytes level n_bit mode write_error ndense route")
DENSE = (5, 1000, 17)


def lcase_id(c):
    lv = {1: "u8", 2: "u16", 4: "i32", 0: "f32", P6: "p6"}[c.level]
    return "%s-%s-d%d-K%d-c%d-%s-n%d-%s-we%d-dense%d" % (c.route, c.table, c.d, c.K, c.code_bytes, lv, c.n_bit,
                                                         ("off", "given", "device", "keyed")[c.mode], c.write_error, c.ndense)


def level_route(d, K, code_bytes, level, n_bit, write_error):
    """Which launcher of gq_hsq_levels_batched (csrc/gq_api.hip:94-112) serves the descriptor, restated."""
    pf = d in (8, 16, 32) and K <= 256 and code_bytes == 1
    if level == P6 or (pf and level == 1 and 1 <= n_bit <= 8):
        return "ef_d" if write_error and d != 16 else "d16"
    if write_error and pf and level == 2 and 1 <= n_bit <= 15:
        return "ef16"
    return "any"


def _l(table, d, K, cbytes, level, n_bit, mode, we, ndense):
    return LCase(table, d, K, cbytes, level, n_bit, mode, we, ndense, level_route(d, K, cbytes, level, n_bit, we))


def _modes(level, n_bit):
    """(mode, n_bit) pairs of a form: OFF at n_bit, GIVEN at the largest n_bit whose top level 2^n_bit still fits the width."""
    fits = {1: 7, P6: 5, 2: 15, 4: 30, 0: 30}[level]
    return ((OFF, n_bit), (GIVEN, min(n_bit, fits)))


LEVEL_CASES = []
for _we in (0, 1):
    for _i, (_d, _lv, _nb) in enumerate(((16, 1, 8), (16, P6, 6), (8, 1, 8), (32, 1, 8))):
        LEVEL_CASES += [_l("small", _d, 256, 1, _lv, nb, m, _we, 3 * ((_i + _we) % 2)) for m, nb in _modes(_lv, _nb)]
    for _i, _d in enumerate((8, 16, 32)):
        LEVEL_CASES += [_l("small", _d, 256, 1, 2, 8, GIVEN, _we, 0), _l("small", _d, 256, 1, 2, 15, OFF, _we, 3),
                        _l("small", _d, 256, 1, 2, 1, GIVEN, _we, 0)]
    for _d, _K, _cb in ((12, 100, 1), (5, 5, 1), (16, 512, 4)):
        for _i, _lv in enumerate((1, 2, 4, 0)):
            LEVEL_CASES += [_l("small", _d, _K, _cb, _lv, nb, m, _we, 3 * (_i % 2)) for m, nb in _modes(_lv, 8)]
LEVEL_STEADY = [_l(t, d, 256, 1, lv, nb, GIVEN, 1, 3) for t in ("long", "many") for d, lv, nb in ((16, 1, 7), (16, P6, 5), (32, 1, 7), (8, 2, 8))]
LEVEL_STEADY += [_l("long", 12, 100, 1, 2, 8, GIVEN, 1, 3)]
# one case per route for the on-device draws
DRAW_CASES = [_l("small", 16, 256, 1, 1, 7, DEVICE, 1, 0), _l("small", 16, 256, 1, P6, 5, KEYED, 1, 0), _l("small", 8, 256, 1, 1, 7, KEYED, 1, 0),
              _l("small", 32, 256, 1, 2, 8, DEVICE, 1, 0), _l("small", 12, 100, 1, 2, 8, KEYED, 1, 3), _l("small", 16, 256, 1, 2, 8, DEVICE, 0, 0)]

# fused: (case, plain, tail)
FCase = collections.namedtuple("FCase", "l plain tail")


def fcase_id(f):
    return "%s-%s-%s" % (lcase_id(f.l), "plain" if f.plain else "mean", "tail" if f.tail else "notail")


FUSED_SERVED = [FCase(_l("small", d, 256, 1, lv, nb, m, we, 3 if tail else 0), plain, tail)
                for d in (8, 16, 32) for lv in (1, 2) for i, (m, nb) in enumerate(_modes(lv, 8))
                for we in (0, 1) for plain, tail in (((i + we) % 2, 0), ((i + we + 1) % 2, 1))]
FUSED_UNSERVED = [FCase(_l("small", d, K, 1, lv, nb, GIVEN, 1, 3), plain, 1)
                  for (d, K, lv, nb), plain in zip(((12, 100, 1, 7), (16, 256, P6, 5), (16, 256, 4, 8)), (0, 1, 0))]
FUSED_STEADY = [FCase(_l(t, d, 256, 1, lv, 8 if lv == 2 else 7, GIVEN, 1, 3), 0, 1) for t in ("long", "many") for d, lv in ((16, 1), (32, 2))]
RNG_PAIRS, RESET_WORDS = 3, 5


def fused_served(c):
    """`served` of gq_hsq_levels_decode_batched (csrc/gq_api.hip), restated."""
    top = (1 << c.n_bit) - (1 if c.mode == OFF else 0)
    return (c.d in (8, 16, 32) and c.K <= 256 and c.code_bytes == 1 and c.level in (1, 2) and 1 <= c.n_bit <= (8 if c.level == 1 else 15)
            and not (c.level == 1 and top > 255))


class Levels(object):
    """A level launch's inputs -- hand-built u_flat and seg_minmax (hsq_dequant_contract.projections: on every level, the two
    ends first), random codes in the wire, Gaussian v, draws -- and the state it must leave.  Tensor s lives in the range
    REGIME_ORDER[s % 4]; every third tensor has no error buffer."""

    def __init__(self, c):
        self.c, self.Ms, self.cb = c, TABLES[c.table], codebook(c.d, c.K)
        self.lay = Layout(self.Ms, c.d, c.code_bytes, c.level, DENSE[:c.ndense])
        rs = np.random.RandomState(17 * c.d + c.K + 5 * c.n_bit + (c.level % 7) + 3 * c.mode)
        self.u, self.r, self.codes, self.v, self.bounds = [], [], [], [], []
        for s, M in enumerate(self.Ms):
            regime = dc.REGIME_ORDER[s % 4]
            lb, ub = hc.REGIMES[regime]
            if regime == "ordinary":          # every tensor its own scale; "tiny" and "sub" keep their subnormal ends
                lb, ub = F(lb * scale_of(s)), F(ub * scale_of(s))
            elif regime == "flat":
                lb = ub = F(ub * scale_of(s))
            u = hc.projections(M, lb, ub, c.n_bit if c.level else 8, seed=s + 40)
            self.u.append(u)
            self.bounds.append((F(u.min()), F(u.max())))        # (a one-subvector tensor: lb == ub)
            self.r.append(rs.rand(M).astype(np.float32))
            self.codes.append(rs.randint(0, c.K, size=M).astype(self.lay.code_np()))
            self.v.append(rc.f32(rs.standard_normal((M, c.d)) * 1e-2))
        self.has_err = [bool(c.write_error) and s % 3 != 1 for s in range(len(self.Ms))]
        self.minmax = np.array([[int(rc.order_map(F(x)).reshape(-1)[0]) for x in b] for b in self.bounds], np.uint32)
        self.u_flat, self.r_flat = self.lay.flat_of(self.u), self.lay.flat_of(self.r, fill=F(0.5))
        self.gbuf = self.lay.floats_of(self.v)
        self.ebuf = np.full(self.lay.floats, E_FILL, np.float32)
        self.dense_src = [rc.f32(rs.standard_normal(n)) for n in self.lay.dense]
        self.wire0 = self.lay.new_wire()
        for s in range(len(self.Ms)):
            self.lay.put(self.wire0, s, "codes", self.codes[s])

    def levels(self, bounds=None, u=None, r="own", how="contract"):
        """Per tensor the levels (level form 0: the projections).  bounds / u / how are the contract's unless given -- the
        mutations of tests/test_hsq_encode_contract.py pass others."""
        c, out = self.c, []
        for s in range(len(self.Ms)):
            lb, ub = (bounds or self.bounds)[s]
            us = (u or self.u)[s]
            if c.level == 0:
                out.append(us)
                continue
            rr = (self.r[s] if c.mode == GIVEN else None) if isinstance(r, str) else r[s]
            out.append(quantise_mutant(us, lb, ub, c.n_bit, rr, how) if how != "contract" else hc.quantise(us, lb, ub, c.n_bit, rr))
        return out

    def want(self, levels=None, plain=False):
        """-> dict: wire, ebuf, out, dense_out.  levels: the levels the wire holds (the draws' cases pass what the launch wrote)."""
        c, lay = self.c, self.lay
        levels = self.levels() if levels is None else levels
        wire, errs, outs = self.wire0.copy(), [], []
        for s in range(len(self.Ms)):
            lb, ub = self.bounds[s]
            lay.put(wire, s, "levels", lay.level_section(levels[s]))
            if c.level != 0:
                lay.put(wire, s, "lbub", np.array([lb, ub], np.float32))      # level form 0: the 8 bytes are not written
            dec = rc.stage_decode(self.codes[s], lay.norms(levels[s], c.n_bit, lb, ub), self.cb)
            with np.errstate(all="ignore"):
                errs.append(self.v[s] - dec if self.has_err[s] else None)
            outs.append(hc.mean(dec, 1, plain))
        for at, src in zip(lay.dense_at, self.dense_src):
            wire[at: at + 4 * src.size] = src.view(np.uint8)
        dense = np.concatenate(self.dense_src) if self.dense_src else np.zeros(0, np.float32)
        return dict(wire=wire, ebuf=lay.floats_of(errs, fill=E_FILL), out=lay.floats_of(outs), dense_out=hc.mean(dense, 1, False))


def quantise_mutant(u, lb, ub, n_bit, r, how):
    """NOT the contract: "minus1" divides by 2^n_bit - 1 levels; "late" divides by ub - lb after the scaling."""
    u = rc.f32(u)
    if F(lb) - F(ub) == 0:
        return np.zeros(u.shape, np.int32)
    with np.errstate(all="ignore"):
        s = F(1 << n_bit)
        if how == "minus1":
            x = np.abs((u - F(lb)) / (F(ub) - F(lb))) * (s - F(1.0))
        else:
            x = np.abs(((u - F(lb)) * s) / (F(ub) - F(lb)))
        l = np.minimum(np.maximum(x, F(0.0)), s - F(1.0)).astype(np.int32)
        if r is not None:
            l = l + ((x - l.astype(np.float32)) > rc.f32(r)).astype(np.int32)
    return l


@functools.lru_cache(maxsize=None)
def levels_of(c):
    return Levels(c)


# ---- helpers of the GPU file ------------------------------------------------------------------------------------------------------------
def order_unmap(m):
    """order_unmap of csrc/hsq_pf_common.hpp: the float a seg_minmax word stands for."""
    m = int(m)
    return np.array([m ^ (0x80000000 if m >> 31 else M32)], np.uint32).view(np.float32)[0]


def unpack6(section, M):
    """The levels of a GQ_LEVELS_PACKED6 section."""
    b = np.asarray(section, np.uint8).reshape(-1, 3).astype(np.uint32)
    w = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return np.stack([(w >> (6 * i)) & 63 for i in range(4)], axis=1).reshape(-1)[:M].astype(np.int32)


def levels_in(lay, wire, s):
    """The levels tensor s's section of `wire` holds (level forms 1, 2, 4 and P6)."""
    off, nbytes = lay.sections[(s, "levels")]
    sec = np.asarray(wire[off: off + nbytes])
    if lay.level == P6:
        return unpack6(sec, lay.Ms[s])
    return sec.view(dc.LEVEL_NP[lay.level]).astype(np.int32)


def chain_want(e, n_bit):
    """Behind an encode case `e`: gq_hsq_levels_batched (byte levels, rounding off, write_error) and the decode of the one
    payload with R = 1 -> dict wire, ebuf, out."""
    enc, lay = e.want(), e.lay
    wire, errs, outs = enc["wire"].copy(), [], []
    for s in range(lay.nseg):
        lb, ub = order_unmap(enc["minmax"][s, 0]), order_unmap(enc["minmax"][s, 1])
        levels = hc.quantise(enc["u"][s], lb, ub, n_bit, None)
        lay.put(wire, s, "levels", lay.level_section(levels))
        lay.put(wire, s, "lbub", np.array([lb, ub], np.float32))
        dec = rc.stage_decode(enc["codes"][s], lay.norms(levels, n_bit, lb, ub), e.cb)
        with np.errstate(all="ignore"):
            errs.append(None if e.errs[s] is None else e.v[s] - dec)
        outs.append(hc.mean(dec, 1, False))
    return dict(wire=wire, ebuf=_errs_over(e, errs), out=lay.floats_of(outs))


def _errs_over(e, errs):
    """The error buffer after the level launch: the residual over the old error where a tensor has one, the rest as uploaded."""
    buf = e.ebuf.copy()
    for s, x in enumerate(errs):
        if x is not None:
            buf[e.lay.span(s)] = rc.f32(x).reshape(-1)
    return buf


# the flat entry point's fix-up log (the multi-tensor launches do not write it): shapes of the prefilter and the paged kernels
LOG_SHAPES = tuple((d, 256) for d in (8, 12, 16, 24, 32)) + ((16, 32), (16, 64), (16, 132)) + PAGED_SHAPES
LOG_M = 16 * 64 + 3


@functools.lru_cache(maxsize=None)
def log_case(d, K):
    """One tensor of 17 tiles at scale 1 -> (grad, kinds, codes, u)."""
    g, kinds = rows_of(0, LOG_M, d, K, 5 * d + K, scale=1.0)
    codes, u = encode_ref(g, codebook(d, K))
    return g, kinds, codes, u
