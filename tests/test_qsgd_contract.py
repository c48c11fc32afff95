"""tests/qsgd_contract.py against independent witnesses -- the CPU oracle, the reference's qsgd_* fixtures, float64 / longdouble, scalar
Python loops, the host restatements other tests already keep -- and one assertion for every claim tests/test_gpu_qsgd_contract.py
makes about an input.  No GPU."""
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import qsgd_contract as qc  # noqa: E402

f32 = np.float32
GOLDEN = os.path.join(HERE, "golden")
QSGD_FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "qsgd_*.npz")))


def _oracle_codes(oracle, g, n_bit, r=None):
    """oracle.qsgd_compress in the wire's terms: INT_MIN (a NaN quotient) is level 0 with the sign bit inverted"""
    norm, sg, lv = oracle.qsgd_compress(g, g.shape[1], n_bit, 0 if r is None else 1, r)
    nanq = lv == -2 ** 31
    return norm, np.where(nanq, 0, lv).reshape(g.shape).astype(np.uint32), (sg.astype(bool) ^ nanq).reshape(g.shape).astype(np.uint32)


# ---- the restatement against the oracle, the fixtures, float64 and scalar loops ---------------------------------------------------
@pytest.mark.parametrize("name", QSGD_FIXTURES)
def test_levels_and_decode_match_the_reference_fixtures(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    d, n_bit, random = int(g["dim"]), int(g["n_bit"]), int(g["random"])
    v = g["x"].astype(f32).reshape(-1, d)
    norm = qc.bucket_norm(v)
    assert qc.same_bits(norm, g["norm"], True)
    l, sg = qc.levels(v, norm, n_bit, g["r"].astype(f32).reshape(-1, d) if random else None)
    ref_l, ref_s = g["levels"].reshape(-1, d).astype(np.int64), g["signs"].reshape(-1, d).astype(bool)
    nanq = ref_l == -2 ** 31
    assert np.array_equal(np.where(nanq, 0, ref_l), l) and np.array_equal(ref_s ^ nanq, sg.astype(bool))
    bits = 16
    dec = qc.decode_one(l | (sg << np.uint32(bits - 1)), norm, n_bit, bits)
    fin = ~np.repeat(np.isinf(norm), d).reshape(-1, d)          # the stated exclusion: buckets whose norm is +-inf
    assert int((~fin).any(axis=1).sum()) <= 4
    assert np.array_equal(dec[fin], g["decoded"].reshape(-1, d)[fin], equal_nan=True)


@pytest.mark.parametrize("n_bit", [1, 2, 6, 8, 15])
@pytest.mark.parametrize("lpb", [2, 4, 8, 16])
def test_edge_inputs_hold_their_claims_and_match_the_oracle(oracle, n_bit, lpb):
    G, claims = qc.edge_tensors(lpb)
    assert [g.shape[1] for g in G] == [8 * lpb] * 2 + [16 * lpb] * 2 + [16 * lpb + 8] * 2
    assert [qc.compress_path(g.shape[1], lpb) for g in G] == ["reg1"] * 2 + ["reg2"] * 2 + ["walk"] * 2
    for t, b, kind in claims:
        v = G[t][b]
        n, lanes = np.abs(v).max(), np.abs(v).reshape(-1, 8).min(axis=1)
        if kind == "lo":
            assert n == f32(2.0 ** -64) and lanes.min() >= f32(2.0 ** -102)
        elif kind == "lo_pred":
            assert n == np.nextafter(f32(2.0 ** -64), f32(0)) and n < f32(2.0 ** -64)
        elif kind == "hi":
            assert n == f32(2.0 ** 20)
        elif kind == "hi_succ":
            assert n == np.nextafter(f32(2.0 ** 20), f32(np.inf)) and n > f32(2.0 ** 20)
        elif kind == "min":
            assert n == 1 and lanes[0] == f32(2.0 ** -102) and lanes[1] == np.nextafter(f32(2.0 ** -102), f32(0))
        else:
            assert n == 1 and lanes[0] == 0 and np.count_nonzero(v[:8]) == 7
        # the neighbours: ordinary (inside the window, every lane) in the even tensors, a zero in every lane in the odd ones
        for o in (G[t][b - 1],):
            ol = np.abs(o).reshape(-1, 8).min(axis=1)
            assert (np.all(ol == 0) if t & 1 else np.all(ol >= f32(2.0 ** -102))) and f32(2.0 ** -64) <= np.abs(o).max() <= f32(2.0 ** 20)
    s = f32(1 << n_bit)
    for g in G:
        norm, l, sg = _oracle_codes(oracle, g, n_bit)
        l2, s2 = qc.levels(g, qc.bucket_norm(g), n_bit)
        assert qc.same_bits(norm, qc.bucket_norm(g)) and np.array_equal(l, l2) and np.array_equal(sg, s2)
        # the quotient against longdouble: RN(|v| / norm) in float32, then the product by s (exact: a power of two, no overflow)
        q = (np.abs(g).astype(np.longdouble) / norm.astype(np.longdouble)[:, None]).astype(f32)
        x = q * s
        assert np.array_equal(np.minimum(x, s - 1).astype(np.int64), l2)
    # norm / s with the largest s reaches 2^-79: the caller's test is on norm, at 2^-64
    assert f32(2.0 ** -64) / f32(2 ** 15) == f32(2.0 ** -79)


@pytest.mark.parametrize("ci", range(0, len(qc.MATRIX), 3))
def test_matrix_inputs_match_the_oracle(oracle, ci):
    c = qc.MATRIX[ci]
    shapes, G, E, n_bit = qc.matrix_case(c)
    assert qc.code_bits(n_bit, c["mode"]) == c["bits"] and len(shapes) == c["nseg"] and shapes[0][1] == 37
    assert all(37 % bpw for bpw in (4, 8, 16, 32)) and not G[0][3].any() and G[0][7, 1] == 0 and G[0][7].any()
    scale = f32(0.75)
    for i, g in enumerate(G[:3]):
        e = E[i] if E is not None and not qc.err_absent(c, i) else None
        v = g + scale * e if e is not None else g
        norm, l, sg = _oracle_codes(oracle, v, n_bit)
        n2, code, v2, en = qc.compress_tensor(g, e, 0.75, n_bit, c["bits"], qc.OFF, 0, 0, 0)
        assert qc.same_bits(v, v2) and qc.same_bits(norm, n2) and np.array_equal(code, l | (sg << np.uint32(c["bits"] - 1)))
        if e is not None:
            lv = np.where(sg == 1, l.astype(np.int64), -l.astype(np.int64)).astype(np.int32)      # a NaN quotient: level 0 either way
            dec = oracle.qsgd_decompress(norm, np.ones(l.size, np.uint8), lv, g.shape[1], n_bit).reshape(g.shape)
            assert np.array_equal(en, v - dec)
            # a fused multiply-add in v = g + ef_scale * e gives another bit pattern somewhere in this input
            fused = (g.astype(np.float64) + np.float64(scale) * e.astype(np.float64)).astype(f32)
            if i == 0:
                assert not qc.same_bits(fused, v)


def test_matrix_covers_every_pair_and_every_path():
    F = qc.MATRIX_FACTORS
    names = list(F)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert {(c[a], c[b]) for c in qc.MATRIX} == {(x, y) for x in F[a] for y in F[b]}, (a, b)
    assert len(qc.MATRIX) <= 100
    paths = {(qc.lpb_of(c["hint"]), qc.compress_path(qc.MATRIX_D(qc.lpb_of(c["hint"]))[c["di"]], qc.lpb_of(c["hint"]))) for c in qc.MATRIX}
    assert paths == {(l, p) for l in (2, 4, 8, 16) for p in ("pairs", "reg1", "reg2", "walk")}
    # hints that disagree with d: hint 8 with d = 2048, hint 0 with d = 8
    assert any(c["hint"] == 8 and c["di"] == 9 for c in qc.MATRIX) and any(c["hint"] == 0 and c["di"] == 2 for c in qc.MATRIX)
    assert [qc.lpb_of(h) for h in qc.HINTS] == [16, 2, 2, 4, 8, 16]


def test_packing_and_decode_against_scalar_loops():
    rs = np.random.RandomState(0)
    for bits, n_bit in ((4, 2), (8, 5), (16, 8)):
        code = rs.randint(0, 1 << bits, size=(3, 10)).astype(np.uint32)
        code[0, :4] = (0, 1 << (bits - 1), (1 << bits) - 1, (1 << (bits - 1)) - 1)
        raw = qc.pack(code, bits)
        flat = code.reshape(-1)
        if bits == 4:
            want = [int(flat[2 * i]) | int(flat[2 * i + 1]) << 4 for i in range(flat.size // 2)]        # element 2i in the low nibble
        elif bits == 8:
            want = [int(c) for c in flat]
        else:
            want = [b for c in flat for b in (int(c) & 255, int(c) >> 8)]                              # little-endian
        assert raw.tolist() == want and np.array_equal(qc.unpack(raw, bits, flat.size), flat)
        norm = np.array([1.5, -0.0, 3e38], f32)
        dec = qc.decode_one(code, norm, n_bit, bits)
        for b in range(3):
            for j in range(10):
                c = int(code[b, j])
                l, sgn = c & ((1 << (bits - 1)) - 1), c >> (bits - 1)
                with np.errstate(all="ignore"):
                    t = f32(f32(f32(l) * f32(2 * sgn - 1)) * norm[b]) / f32(1 << n_bit)               # qsgd_compressor.py:69-70
                assert qc.same_bits(dec[b, j], t), (bits, b, j)
        assert np.signbit(dec[0, 0]) and dec[0, 0] == 0 and not np.signbit(dec[0, 1])                 # level 0, sign bit clear: -0
        assert not np.signbit(qc.mean_of([dec], False)[0, 0]) and np.signbit(qc.mean_of([dec], True)[0, 0])


@pytest.mark.parametrize("bits", [4, 8, 16])
def test_payload_wires_hold_every_code_and_the_mean_is_the_oracles(oracle, bits):
    shapes = qc.dec_shapes(bits)
    L = qc.Layout(shapes, bits)
    n_bit = {4: 2, 8: 5, 16: 8}[bits]
    for R in (1, 3, 5, 6, 7, 9):
        wires = qc.payload_wires(L, R)
        seen = set()
        for w in wires:
            for i in range(L.nseg):
                seen |= set(L.get(w, i)[1].reshape(-1).tolist())
        assert len(seen) == 1 << bits                              # every code value
        assert max(seen) & ((1 << (bits - 1)) - 1) > (1 << n_bit)           # levels above 2^n_bit - 1 among them
        n0 = L.get(wires[0], 0)[0]
        assert np.isnan(n0).sum() == 1 and np.isinf(n0).sum() == 2 and (n0 == 0).sum() == 2 and (np.abs(n0) < 2.0 ** -126).sum() == 3
        skip, n = qc.inf_norm_elements(L, wires)
        assert n == 2 and not skip[L.out_off[1]:].any()         # the excluded buckets: two, the same in every payload
        for k in qc.SPECIAL_AT[:min(R, 8)]:                     # every other special norm is compared, in one payload or another
            assert len({L.get(w, 0)[0][k].tobytes() for w in wires}) == min(R, 8)
        parts = []
        for w in wires:
            dec = []
            for i, (d, nb) in enumerate(L.shapes):
                norm, code = L.get(w, i)
                l = (code & np.uint32((1 << (bits - 1)) - 1)).astype(np.int32)
                dec.append(oracle.qsgd_decompress(norm, (code >> np.uint32(bits - 1)).astype(np.uint8), l, d, n_bit))
            parts.append(np.concatenate(dec))
        want = oracle.mean_users(np.stack(parts))
        got = qc.expect_decode(L, wires, n_bit, False, 7.0)[L.out_mask()]
        assert qc.same_bits(got, want, True)
        if R in (3, 5, 6, 7):       # for these sums a multiplication by 1 / R differs from the division
            acc = qc.mean_of(parts, True)
            with np.errstate(all="ignore"):
                other = (acc + f32(0)) * (f32(1) / f32(R))
            assert not qc.same_bits(other, want, True)
    assert L.mask().sum() == sum(4 * nb + nb * d * bits // 8 for d, nb in shapes) and L.ub % 16 == 0
    assert L.code_off[-1] + 4 * 6 * bits // 8 == L.ub or (4 * 6 * bits // 8) % 16        # the wire ends with its last codes


# ---- the one de-quantiser (csrc/qsgd_common.hpp) --------------------------------------------------------------------------------------
DEQ_NORMS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00000123, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                      0x00800001, 0x00FFFFFF, 0x01000000, 0x3F800000, 0xBFC00000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7E967699, 0x7F800000,
                      0xFF800000, 0x7FC00000, 0xFFC00001], np.uint32).view(f32)


@pytest.mark.parametrize("n_bit", [1, 2, 6, 8, 15, 30])
def test_the_two_spellings_of_the_dequantiser_are_the_same_bits(n_bit):
    """qsgd_compressor.py:69-70 as (l * (2 sign - 1)) * norm / s, and as ((+-l) * norm) * 2^-n_bit with the sign on the float's sign bit
    (decode_one, the form the kernels use): l * -1 = -l and 0 * -1 = -0 exactly, and both scalings are one correct rounding of the same
    exact real -- for every code of the 4- and 8-bit widths and (at five norms) of the 16-bit width, a sample of 16-bit codes elsewhere;
    norms 0, -0, subnormals, the smallest normals, 2^-126 (1 + ulp), huge, +-inf, NaN.  Any NaN equals any NaN."""
    assert DEQ_NORMS[9] == f32(2.0 ** -126) * (f32(1) + f32(2.0 ** -23)) and np.isnan(DEQ_NORMS[-2:]).all() and np.isinf(DEQ_NORMS[-4:-2]).all()
    assert np.signbit(DEQ_NORMS[1]) and DEQ_NORMS[1] == 0 and (np.abs(DEQ_NORMS[2:7]) < f32(2.0 ** -126)).all()
    s, inv_s = f32(1 << n_bit), f32(2.0 ** -n_bit)
    assert f32(1) / s == inv_s
    rs = np.random.RandomState(n_bit)
    for bits in (4, 8, 16):
        every = np.arange(1 << bits, dtype=np.uint32)
        norms = DEQ_NORMS if bits < 16 else np.concatenate([DEQ_NORMS[[0, 2, 9, 14, 17]], DEQ_NORMS, rs.randint(0, 1 << 32, 40, dtype=np.int64).astype(np.uint32).view(f32)])
        code = np.stack([every if bits < 16 or i < 5 else rs.randint(0, 1 << 16, every.size).astype(np.uint32) for i in range(norms.size)])
        l, sgn = code & np.uint32((1 << (bits - 1)) - 1), code >> np.uint32(bits - 1)
        with np.errstate(all="ignore"):
            a = (l.astype(f32) * (f32(2) * sgn.astype(f32) - f32(1))) * norms[:, None] / s
        b = qc.decode_one(code, norms, n_bit, bits)
        assert a.dtype == f32 and b.dtype == f32 and qc.same_bits(a, b, True)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        sub = np.isfinite(a) & (np.abs(a) < f32(2.0 ** -126)) & (a != 0)
        assert sub.any() or n_bit == 30               # subnormal results are among them (2^-30: those norms' products round to 0)


# ---- the draws ----------------------------------------------------------------------------------------------------------------------
def test_draws_agree_with_the_other_host_restatements():
    import importlib
    import rq_contract
    pvq = importlib.import_module("test_gpu_pvq")
    idx = [0, 1, 5, (7 << 32) + 3, (123456 << 32) + 1025, 2 ** 40 + 17]
    for seed in (0, 1, 0x9E3779B97F4A7C15, 0xFFFFFFFFFFFFFFFF, 0x1234567):
        assert np.array_equal(qc.uniform01(seed, np.array(idx, np.uint64)), pvq._uniform01_host(seed, idx))
        for step in (0, 1, 2 ** 63):
            assert qc.resolve_seed(seed, step) == rq_contract.resolve_seed(seed, step)
    # bucket_draw / keyed_seed: scalar Python integers
    key, e = 0xDEADBEEF, 77
    h = (key + e * 0x9E3779B1) & qc.M32
    h ^= h >> 16
    h = (h * 0x7FEB352D) & qc.M32
    assert qc.bucket_draw(key, e) == f32(h >> 8) * f32(2.0 ** -24)
    nb = int(np.array(1.5, f32).view(np.uint32))
    k = (nb << 32) | nb
    assert int(qc.keyed_seed(5, f32(1.5))) == 5 ^ ((k * 0x9E3779B97F4A7C15) & qc.M64) ^ (k >> 29)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("mode", [qc.DEVICE, qc.KEYED, qc.COUNTER])
def test_tie_tensors_sit_on_their_draws(wide, mode):
    n_bit, d, nb, first = 5, 34, 4, 1000
    v = qc.tie_tensor(d, nb, n_bit, mode, 0x1234567, 1, first, wide)
    norm = qc.bucket_norm(v)
    assert np.all(norm == 1)
    u = qc.draws(mode, 0x1234567, 1, norm, first, d, wide)
    x = np.abs(v / norm[:, None]) * f32(1 << n_bit)
    assert np.array_equal(x[:, 1:], u[:, 1:])                   # x - l == u exactly, l = 0
    l, _ = qc.levels(v, norm, n_bit, u)
    assert np.all(l[:, 1:] == 0) and np.all(l[:, 0] == 1 << n_bit)        # this draw reaches level 2^n_bit
    assert np.all(qc.levels(v, norm, n_bit, np.nextafter(u, f32(-1)))[0][:, 1:][u[:, 1:] > 0] == 1)
    if mode == qc.KEYED:        # equal data, equal norm bits, other bucket indices: other draws
        assert not np.array_equal(u[0], u[1])
    assert not np.array_equal(u, qc.draws(mode, 0x1234567, 0, norm, first, d, wide)) or mode != qc.COUNTER


# ---- sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [64, 256, 304])
def test_many_item_and_wide_shapes_reach_three_items_a_wave(cus):
    for nseg in (200, 256, 257):
        L = qc.Layout(qc.many_shapes(cus, nseg), 4)
        assert L.nitems >= cus * 32 * 3 * 4 and sum(d * nb for d, nb in L.shapes) < 6e6 * cus / 256
        ds = [d for d, _ in L.shapes]
        assert all(a != b for a, b in zip(ds, ds[1:])) and {qc.compress_path(d, 16) for d in ds} == {"reg1", "pairs", "walk"}
    W = qc.Layout(qc.wide_shapes(cus), 4, wide=True)
    assert W.nitems >= cus * 32 * 3 and [d for d, _ in W.shapes[:7]] == list(qc.WIDE_D)
    seg = W.item_seg()
    per = -(-W.nitems // (cus * 32))
    runs = [len(set(seg[i:i + per].tolist())) for i in range(0, W.nitems, per)]
    assert per >= 3 and np.mean(np.array(runs) > 1) > 0.3       # a wave's run crosses tensor boundaries
    assert all(w % 32 == 0 for w in W.word0) and W.word0[1] - W.word0[0] >= 64


def test_the_windows_lower_edge_is_conservative():
    """quotient_window() admits norm >= 2^-64.  Markstein's step (q0 = RN(a y), r = fma(-q0, b, a), RN(q0 + r y)) with b = norm / s and
    y = RN(1 / norm) * s, computed here in exact rational arithmetic with one rounding per operation, still equals the division
    for norms down to 2^-80 and |v| >= 2^-102: r is a multiple of 2^-46 |v| >= 2^-148 and nothing on the way is subnormal.  So
    the buckets just under the edge pin the true division's result, not a place where the quick quotient would be wrong."""
    from fractions import Fraction as Fr

    def rn(x):
        if x == 0:
            return f32(0)
        sgn, x, e = (-1 if x < 0 else 1), abs(x), -149
        while x / Fr(2) ** e >= 1 << 24:
            e += 1
        m = x / Fr(2) ** e
        fl, rem = m.numerator // m.denominator, m - m.numerator // m.denominator
        fl += rem > Fr(1, 2) or (rem == Fr(1, 2) and fl & 1)
        return f32(sgn * float(fl) * 2.0 ** e)

    rs = np.random.RandomState(7)
    for n_bit in (1, 8, 15):
        s = f32(1 << n_bit)
        norm = np.exp2(rs.uniform(-80, -64, 150)).astype(f32)
        a = np.maximum(np.exp2(rs.uniform(-102, np.log2(norm.astype(np.float64)))).astype(f32), f32(2.0 ** -102))
        a[::3] = (rs.randint(1, int(s) + 1, a[::3].size) * norm[::3].astype(np.float64) / float(s)).astype(f32)      # x beside an integer
        a = np.minimum(np.maximum(a, f32(2.0 ** -102)), norm)
        for ai, ni in zip(a, norm):
            b, y = ni * (f32(1) / s), (f32(1) / ni) * s
            q0 = rn(Fr(float(ai)) * Fr(float(y)))
            r = rn(Fr(float(ai)) - Fr(float(q0)) * Fr(float(b)))
            x = rn(Fr(float(q0)) + Fr(float(r)) * Fr(float(y)))
            assert x == (ai / ni) * s
