"""The QSGD part of include/gq_hsq.h restated in numpy, one float32 operation at a time, and the inputs of
tests/test_gpu_qsgd_contract.py built from fixed seeds.  tests/test_qsgd_contract.py checks this file against the CPU oracle, the
reference's fixtures, float64 / longdouble and scalar loops, and asserts every claim made here about an input.

    norm  = NaN-propagating max |v| of the bucket
    x     = |v / norm| * s   (s = 2^n_bit; a true float32 division, then the product)
    l     = trunc(min(max(x, 0), s - 1));  l += (x - l > u) with a draw u;  sign bit = v > 0
    x NaN : level 0, the sign bit inverted
    code  = sign << (bits - 1) | l, bits 4 (element 2i in the low nibble), 8 or 16 (little-endian)
    decode: ((+-l) * norm) * 2^-n_bit, payload 0 assigned, 1 .. R-1 added in ascending order, then (+0 + sum) / R (none: plain)
    error feedback: v = g + RN(ef_scale * e), v over g, e = v - decode(code)

No torch, no GPU."""
import numpy as np

f32 = np.float32
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
OFF, GIVEN, DEVICE, KEYED, COUNTER = 0, 1, 2, 3, 4          # GQ_RANDOM_*
WIDE_CHUNK = 1024                                           # GQ_QSGD_WIDE_CHUNK
CANARY = 0xA5
U64 = np.uint64


def code_bits(n_bit, mode):
    """gq_qsgd_code_bits"""
    top = (1 << n_bit) - (1 if mode == OFF else 0)
    return 4 if top <= 7 else 8 if top <= 127 else 16 if top <= 32767 else 0


# ---- the draws (uint32 arithmetic, held in uint64 arrays and masked) ----------------------------------------------------------------
def _mul32(a, c):
    return (a * U64(c)) & U64(M32)


def uniform_bits(seed, idx):
    """uniform_bits of csrc/gq_common.hpp; seed and idx: Python ints or uint64 arrays (broadcast)"""
    seed, idx = np.asarray(seed, U64), np.asarray(idx, U64)
    lo, hi = seed & U64(M32), seed >> U64(32)
    h = ((idx & U64(M32)) + _mul32(lo, 0x9E3779B1)) & U64(M32)
    h = h ^ (h >> U64(16))
    h = _mul32(h, 0x7FEB352D)
    h = h ^ (h >> U64(15))
    h = _mul32(h, 0x846CA68B)
    h = h ^ (h >> U64(16))
    h = (h + (hi ^ _mul32(idx >> U64(32), 0x85EBCA77))) & U64(M32)
    h = _mul32(h, 0xC2B2AE3D)
    return h ^ (h >> U64(15))


def _unit(h):
    return (h >> U64(8)).astype(f32) * f32(2.0 ** -24)


def uniform01(seed, idx):
    return _unit(uniform_bits(seed, idx))


def bucket_draw(key, e):
    """bucket_draw of csrc/qsgd_batched.hip: key = uniform_bits(seed, bucket), e = element inside the bucket"""
    h = (np.asarray(key, U64) + _mul32(np.asarray(e, U64), 0x9E3779B1)) & U64(M32)
    h = h ^ (h >> U64(16))
    return _unit(_mul32(h, 0x7FEB352D))


def keyed_seed(seed, norm):
    """keyed_seed(seed, norm, norm): the stream of a bucket from the bits of its norm"""
    nb = np.asarray(norm, f32).view(np.uint32).astype(U64)
    k = (nb << U64(32)) | nb
    with np.errstate(over="ignore"):
        return U64(seed & M64) ^ (k * U64(0x9E3779B97F4A7C15)) ^ (k >> U64(29))


def resolve_seed(seed, step):
    """resolve_seed: the launch's seed from the { seed, step } words"""
    z = (step + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (seed ^ z ^ (z >> 31)) & M64


def draws(mode, seed, step, norm, first, d, wide=False):
    """The draws of buckets first .. first + len(norm) - 1 (bucketed: numbered across tensors; wide: words of norm_bits) -> [nb, d]"""
    if mode == OFF:
        return None
    if mode == COUNTER:
        seed = resolve_seed(seed, step)
    sd = keyed_seed(seed, norm)[:, None] if mode == KEYED else U64(seed & M64)
    b = (first + np.arange(len(norm), dtype=np.int64)).astype(U64)[:, None]
    e = np.arange(d, dtype=np.int64).astype(U64)[None, :]
    if wide:
        return uniform01(sd, (b << U64(32)) + e)
    return bucket_draw(uniform_bits(sd, b), e)


# ---- compress ---------------------------------------------------------------------------------------------------------------------
def bucket_norm(v):
    return np.max(np.abs(v), axis=1)        # (np.max propagates NaN, like torch.max)


def levels(v, norm, n_bit, u=None):
    """-> (level, sign bit) per element of v [nb, d]"""
    s = f32(1 << n_bit)
    with np.errstate(all="ignore"):
        q = v / norm[:, None]
        x = np.abs(q) * s
        nanq = np.isnan(x)
        c = np.minimum(np.maximum(x, f32(0)), s - f32(1))
        l = np.where(nanq, f32(0), c).astype(np.int64)
        if u is not None:
            l = l + ((x - l.astype(f32)) > u)       # (a NaN x compares false)
    return l.astype(np.uint32), ((v > 0) ^ nanq).astype(np.uint32)


def signed_level(code, bits):
    lf = (code & np.uint32((1 << (bits - 1)) - 1)).astype(f32)
    return np.where((code >> np.uint32(bits - 1)) & np.uint32(1), lf, -lf)      # level 0 with a clear sign bit: -0


def decode_one(code, norm, n_bit, bits):
    """((+-l) * norm) * 2^-n_bit of one payload, code [nb, d], norm [nb]"""
    with np.errstate(all="ignore"):
        t = signed_level(code, bits) * np.asarray(norm, f32)[:, None]
        return t * f32(2.0 ** -n_bit)


def mean_of(parts, plain):
    with np.errstate(all="ignore"):
        acc = parts[0]
        for p in parts[1:]:
            acc = acc + p
        return acc if plain and len(parts) == 1 else (acc + f32(0)) / f32(len(parts))      # (plain: the decompress of ONE payload)


def compress_tensor(g, e, ef_scale, n_bit, bits, mode, seed, step, first, wide=False):
    """One tensor g [nb, d] (e: its error buffer or None) -> norm, codes, v, new error"""
    ef = ef_scale is not None and e is not None
    with np.errstate(all="ignore"):
        v = g + f32(ef_scale) * e if ef else g
    norm = bucket_norm(v)
    l, sg = levels(v, norm, n_bit, draws(mode, seed, step, norm, first, g.shape[1], wide))
    code = l | (sg << np.uint32(bits - 1))
    with np.errstate(all="ignore"):
        e_new = v - decode_one(code, norm, n_bit, bits) if ef else e
    return norm, code, v, e_new


def pack(code, bits):
    """codes (any shape, flattened in element order) -> the bytes of the section"""
    c = np.ascontiguousarray(code, np.uint32).reshape(-1)
    if bits == 4:
        return (c[0::2] | (c[1::2] << np.uint32(4))).astype(np.uint8)
    if bits == 8:
        return c.astype(np.uint8)
    return c.astype("<u2").view(np.uint8)


def unpack(raw, bits, n):
    raw = np.ascontiguousarray(raw, np.uint8)
    if bits == 4:
        c = np.empty(n, np.uint32)
        c[0::2], c[1::2] = raw & 15, raw >> 4
        return c
    if bits == 8:
        return raw.astype(np.uint32)
    return raw.view("<u2").astype(np.uint32)


def _up(x, a=16):
    return (x + a - 1) // a * a


# ---- wire layout and tables -------------------------------------------------------------------------------------------------------
class Layout(object):
    """Tensors (d, buckets) on one user's wire: norms f32[nb] | codes, every section on 16 bytes with `gap` canary bytes round it;
    the last codes section ends the wire (ub = its end rounded up to 16, + pad).  out: tensors 4 floats apart."""

    def __init__(self, shapes, bits, wide=False, gap=16, pad=0, dense=()):
        self.shapes, self.bits, self.wide, self.nseg = list(shapes), bits, wide, len(shapes)
        self.norm_off, self.code_off, self.out_off, self.first, self.word0 = [], [], [], [], []
        off, oo, it, w = gap, 4, 0, 32
        for d, nb in self.shapes:
            assert d % 2 == 0 and 2 <= d <= 65536 and nb >= 1
            self.norm_off.append(off)
            off = _up(off + 4 * nb) + gap
            self.code_off.append(off)
            end = off + nb * d * bits // 8
            off = _up(end) + gap
            self.out_off.append(oo)
            oo += _up(nb * d, 4) + 4
            self.first.append(it)
            it += nb * ((d + WIDE_CHUNK - 1) // WIDE_CHUNK) if wide else nb
            self.word0.append(w)                    # wide: a tensor's words on lines of their own, a canary line between
            w += _up(nb, 32) + 32
        self.dense, self.dense_off = list(dense), []      # uncompressed tensors (floats each) behind the last codes section
        for n in self.dense:
            self.dense_off.append(off)
            end = off + 4 * n
            off = _up(end) + gap
        self.ub, self.out_n, self.nitems, self.nwords = _up(end) + pad, oo, it, w

    def dense_table(self, ptrs):
        return np.array([(p, o, n) for p, o, n in zip(ptrs, self.dense_off, self.dense)], np.int64).reshape(-1, 3)

    def part_table(self, lo, hi):
        """tensors lo .. hi - 1 as a launch of their own (decode: no gradient pointers): items renumbered from 0"""
        t = self.table([0] * self.nseg)[lo:hi].copy()
        t[:, 2] -= self.first[lo]
        seg = self.item_seg()
        seg = seg[(seg >= lo) & (seg < hi)] - lo
        return t, seg.astype(np.int32)

    def item_seg(self):
        n = [nb * ((d + WIDE_CHUNK - 1) // WIDE_CHUNK) if self.wide else nb for d, nb in self.shapes]
        return np.repeat(np.arange(self.nseg, dtype=np.int32), n)

    def table(self, grad_ptrs, err_ptrs=None):
        t = np.zeros((self.nseg, 8), np.int64)
        for i, (d, nb) in enumerate(self.shapes):
            t[i] = (grad_ptrs[i], d, self.first[i], self.norm_off[i], self.code_off[i], self.out_off[i],
                    self.word0[i] if self.wide else nb, err_ptrs[i] if err_ptrs is not None else 0)
        return t

    def mask(self):
        """the bytes the compress owns"""
        m = np.zeros(self.ub, bool)
        for i, (d, nb) in enumerate(self.shapes):
            m[self.norm_off[i]:self.norm_off[i] + 4 * nb] = True
            m[self.code_off[i]:self.code_off[i] + nb * d * self.bits // 8] = True
        for o, n in zip(self.dense_off, self.dense):
            m[o:o + 4 * n] = True
        return m

    def out_mask(self):
        m = np.zeros(self.out_n, bool)
        for i, (d, nb) in enumerate(self.shapes):
            m[self.out_off[i]:self.out_off[i] + nb * d] = True
        return m

    def put(self, wire, i, norm, code):
        d, nb = self.shapes[i]
        wire[self.norm_off[i]:self.norm_off[i] + 4 * nb] = np.ascontiguousarray(norm, f32).view(np.uint8)
        wire[self.code_off[i]:self.code_off[i] + nb * d * self.bits // 8] = pack(code, self.bits)

    def get(self, wire, i):
        d, nb = self.shapes[i]
        norm = wire[self.norm_off[i]:self.norm_off[i] + 4 * nb].copy().view(f32)
        raw = wire[self.code_off[i]:self.code_off[i] + nb * d * self.bits // 8]
        return norm, unpack(raw, self.bits, nb * d).reshape(nb, d)


def expect_compress(L, G, E, ef_scale, n_bit, mode, seed=0, step=0):
    """-> (wire with CANARY where the launch writes nothing, v per tensor, new error per tensor, norm per tensor)"""
    wire = np.full(L.ub, CANARY, np.uint8)
    V, EN, N = [], [], []
    for i, g in enumerate(G):
        first = L.word0[i] if L.wide else L.first[i]
        norm, code, v, en = compress_tensor(g, E[i] if E is not None else None, ef_scale, n_bit, L.bits, mode, seed, step, first, L.wide)
        L.put(wire, i, norm, code)
        V.append(v), EN.append(en), N.append(norm)
    return wire, V, EN, N


def expect_decode(L, wires, n_bit, plain, fill):
    """The decode(-mean) of R wires -> the whole `out` buffer (fill between tensors) as float32"""
    out = np.full(L.out_n, fill, f32)
    for i, (d, nb) in enumerate(L.shapes):
        parts = [decode_one(c, n, n_bit, L.bits) for n, c in (L.get(w, i) for w in wires)]
        out[L.out_off[i]:L.out_off[i] + nb * d] = mean_of(parts, plain).reshape(-1)
    return out


def inf_norm_elements(L, wires):
    """Mask over `out` of the elements of buckets whose norm is +-inf in any payload (no code for the reference's INT_MIN level,
    DESIGN.md section 2: left out of the decode comparison), and the number of such buckets."""
    m, n = np.zeros(L.out_n, bool), 0
    for i, (d, nb) in enumerate(L.shapes):
        bad = np.zeros(nb, bool)
        for w in wires:
            bad |= np.isinf(L.get(w, i)[0])
        n += int(bad.sum())
        m[L.out_off[i]:L.out_off[i] + nb * d] = np.repeat(bad, d)
    return m, n


def same_bits(a, b, nan_equal=False):
    a, b = np.ascontiguousarray(a, f32).reshape(-1), np.ascontiguousarray(b, f32).reshape(-1)
    if nan_equal:
        both = np.isnan(a) & np.isnan(b)
        return np.array_equal(a.view(np.uint32)[~both], b.view(np.uint32)[~both]) and a.shape == b.shape
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def randn(rs, nb, d, scale=1.0):
    return (rs.standard_normal((nb, d)) * scale).astype(f32)


def lpb_of(hint):
    """lanes per bucket the launcher picks for a bucket_hint (lpb_log2_of)"""
    return 2 if 0 < hint <= 16 else 4 if 0 < hint <= 32 else 8 if 0 < hint <= 64 else 16


def compress_path(d, lpb):
    """the body of qsgd_compress_batched4_kernel a bucket of d elements takes with lpb lanes per bucket"""
    if d % 8:
        return "pairs"
    return "walk" if d > 16 * lpb else "reg2" if d > 8 * lpb else "reg1"


P64, P20, P102 = f32(2.0 ** -64), f32(2.0 ** 20), f32(2.0 ** -102)
EDGE_KINDS = ("lo", "lo_pred", "hi", "hi_succ", "min", "zero")


def edge_bucket(kind, d, rs):
    """One bucket at an edge of quotient_window(): 2^-64 <= norm <= 2^20, min |v| >= 2^-102 per lane (8 consecutive elements)"""
    sign = np.where(rs.rand(d) < 0.5, -1.0, 1.0)
    v = (rs.uniform(0.05, 0.99, d) * sign).astype(f32)
    top = {"lo": P64, "lo_pred": np.nextafter(P64, f32(0)), "hi": P20, "hi_succ": np.nextafter(P20, f32(np.inf))}.get(kind, f32(1))
    scale = {"lo": P64, "lo_pred": P64, "hi": P20, "hi_succ": P20}.get(kind, f32(1))
    v = v * scale                      # (a power of two: exact)
    v[5 % d] = -top
    if kind == "min":
        v[1], v[9] = P102, -np.nextafter(P102, f32(0))        # lane 0: exactly 2^-102, its neighbour: the predecessor
    if kind == "zero":
        v[3] = f32(0)
    return v


def edge_tensors(lpb, seed=1):
    """For lpb lanes per bucket: tensors of d = 8 lpb, 16 lpb (register path, one and two units a lane) and 16 lpb + 8 (unit walk),
    each twice: every edge bucket between ordinary buckets (fast path), and between buckets with a zero in every lane (division).
    -> (tensors, claims = [(tensor, bucket, kind)])"""
    rs = np.random.RandomState(seed)
    G, claims = [], []
    for d in (8 * lpb, 16 * lpb, 16 * lpb + 8):
        for slow in (False, True):
            rows = []
            for kind in EDGE_KINDS:
                other = rs.uniform(0.05, 1.0, d).astype(f32) * np.where(rs.rand(d) < 0.5, -1, 1).astype(f32)
                if slow:
                    other[2::8] = 0
                rows.append(other)
                claims.append((len(G), len(rows), kind))
                rows.append(edge_bucket(kind, d, rs))
            rows.append(rs.uniform(0.05, 1.0, d).astype(f32))
            G.append(np.stack(rows))
    return G, claims


def other_user(L, wire):
    """another user's payload over the same layout: the codes shifted by three elements, the norms scaled"""
    w2 = wire.copy()
    for i in range(L.nseg):
        norm, code = L.get(wire, i)
        L.put(w2, i, norm * f32(1.37), np.roll(code.reshape(-1), 3))
    return w2


def tie_tensor(d, nb, n_bit, mode, seed, step, first, wide=False, rs=None):
    """Buckets of norm 1 whose every other element sits exactly on its own draw: v = +-u / s, so x = u, l = 0, x - l == u (level 0;
    `>=` would give 1); element 0 is the norm itself: x = s, l = s - 1, x - l = 1 > u: the top level 2^n_bit."""
    rs = rs or np.random.RandomState(11)
    norm = np.ones(nb, f32)
    u = draws(mode, seed, step, norm, first, d, wide)
    v = u * f32(2.0 ** -n_bit) * np.where(rs.rand(nb, d) < 0.5, f32(-1), f32(1))
    v[:, 0] = 1
    return v.astype(f32)


MATRIX_D = lambda lpb: [2, 6, 8, 10, 8 * lpb, 8 * lpb + 8, 16 * lpb, 16 * lpb + 2, 16 * lpb + 8, 2048]      # noqa: E731
HINTS = (0, 8, 16, 32, 64, 128)
N_BIT_OF = {(4, OFF): 3, (8, OFF): 6, (16, OFF): 9, (4, 1): 2, (8, 1): 5, (16, 1): 8}        # the widest n_bit of a width


def pairwise(factors, seed=0):
    """A small set of tuples in which every pair of values of two different factors occurs (greedy)"""
    rs = np.random.RandomState(seed)
    names = list(factors)
    need = {(a, x, b, y) for i, a in enumerate(names) for b in names[i + 1:] for x in factors[a] for y in factors[b]}
    out = []
    while need:
        best, gain = None, -1
        for _ in range(60):
            t = {n: factors[n][rs.randint(len(factors[n]))] for n in names}
            g = sum((a, t[a], b, t[b]) in need for i, a in enumerate(names) for b in names[i + 1:])
            if g > gain:
                best, gain = t, g
        if gain == 0:       # finish with a tuple built round a missing pair
            a, x, b, y = next(iter(need))
            best[a], best[b] = x, y
        out.append(best)
        need -= {(a, best[a], b, best[b]) for i, a in enumerate(names) for b in names[i + 1:]}
    return out


MATRIX_FACTORS = {"di": list(range(10)), "hint": list(HINTS), "bits": [4, 8, 16], "ef": [False, True], "nseg": [1, 256, 257],
                  "mode": [OFF, DEVICE, KEYED, COUNTER]}
MATRIX = pairwise(MATRIX_FACTORS)


def matrix_case(c, seed=5):
    """A tuple of MATRIX -> (shapes, tensors, errors or None, n_bit): the tensor under test (37 buckets: the last quad is partial
    for every buckets-per-wave 4 ... 32) first, one-bucket tensors of d = 8 and 10 behind it up to nseg"""
    rs = np.random.RandomState(seed + c["di"])
    d = MATRIX_D(lpb_of(c["hint"]))[c["di"]]
    shapes = [(d, 37)] + [((8, 10)[i & 1], 1) for i in range(c["nseg"] - 1)]
    G = [randn(rs, nb, dd) for dd, nb in shapes]
    G[0][3] = 0                                   # a zero bucket
    G[0][7, 1] = 0                                # a zero beside ordinary elements
    E = [randn(rs, nb, dd, 0.3) for dd, nb in shapes] if c["ef"] else None
    return shapes, G, E, N_BIT_OF[(c["bits"], 0 if c["mode"] == OFF else 1)]


def err_absent(c, i):
    """inside an error-feedback launch these tensors have error pointer 0"""
    return c["ef"] and c["nseg"] > 1 and i % 5 == 2


MANY_D = (8, 16, 24, 32, 40, 10, 18)      # register path and pairs, interleaved; every 16th tensor: 264 > 16 * 16, the unit walk


def many_shapes(cus, nseg, items_per_wave=3, bpw=4):
    """nseg tensors of interleaved widths with buckets enough that each of the at most cus * 32 waves (2,048 threads a CU / 256 = 8
    workgroups of 4 waves) runs items_per_wave items of bpw buckets or more"""
    need = cus * 32 * items_per_wave * bpw
    nb = -(-need // nseg) + 1
    return [(264 if i % 16 == 6 else MANY_D[i % len(MANY_D)], nb + (i % 3)) for i in range(nseg)]


SPECIAL_NORMS = np.array([1.0, 2.0 ** -140, 3.0e38, np.nan, -0.0, 0.0, -1.5, 2.0 ** -126], f32)
SPECIAL_AT, INF_AT = (0, 1, 2, 5, 6, 7, 8, 9), (3, 4)      # buckets of tensor 0: the specials move from payload to payload, +-inf stay


def payload_wires(L, R, seed=2):
    """R hand-built wires over L: every code value 0 .. 2^bits - 1 (levels above 2^n_bit - 1 too), norms ordinary and special"""
    rs = np.random.RandomState(seed)
    wires = []
    for r in range(R):
        w = np.full(L.ub, CANARY, np.uint8)
        for i, (d, nb) in enumerate(L.shapes):
            code = (np.arange(nb * d, dtype=np.uint32) * np.uint32(1 + 2 * r) + np.uint32(r + 7 * i)) & np.uint32((1 << L.bits) - 1)
            norm = rs.uniform(0.1, 4.0, nb).astype(f32)
            if i == 0:
                norm[list(SPECIAL_AT)] = np.roll(SPECIAL_NORMS, r)
                norm[list(INF_AT)] = (np.inf, -np.inf)          # the two excluded buckets, the same in every payload
            L.put(w, i, norm, code.reshape(nb, d))
        wires.append(w)
    return wires


def dec_shapes(bits):
    """the decode's tensors: one unit, pairs, d < 8, further units, one bucket; at 16 bits 65,536 elements to hold every code;
    the wire ends with buckets of 6 codes"""
    return [(16, 10), (6, 5), (2, 3), (136, 2), (10, 7), (8, 1)] + ([(256, 256)] if bits == 16 else []) + [(6, 4)]


WIDE_D = (2, 34, 1022, 1024, 1026, 2050, 3 * 1024 + 6)


def wide_shapes(cus, chunks_per_wave=3):
    """Wide tensors: WIDE_D with several buckets each, then tensors of d = 2 ... 66 (one chunk a bucket) until each of the cus * 8 * 4
    waves has a run of chunks_per_wave chunks or more"""
    shapes = [(d, 3) for d in WIDE_D]
    have = sum(nb * ((d + WIDE_CHUNK - 1) // WIDE_CHUNK) for d, nb in shapes)
    need = cus * 32 * chunks_per_wave
    i = 0
    while have < need:
        nb = 5 + i % 7
        shapes.append((2 + 2 * (i * 5 % 33), nb))
        have += nb
        i += 1
    return shapes
