"""tests/eden_contract.py checked on the CPU (no GPU): the tables of include/gq_eden.h against the Lloyd-Max conditions in float64, the
restatement against tests/drive_contract.py at one magnitude and against a float64 nearest-centroid search, what the two scales
promise, the order and form of every operation (each mutation changes wire bits on the GPU test's own inputs), the preconditions of
those inputs, the wire layout, and the error figures the README quotes."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402
import mxr_contract as mxr  # noqa: E402
import drive_contract as dc  # noqa: E402
import eden_contract as ec  # noqa: E402

f32, U32 = np.float32, np.uint32
ROOT = os.path.dirname(HERE)
LLOYD_MAX_MSE = {2: 0.117482, 3: 0.034548, 4: 0.009501}


def _pdf(z):
    return math.exp(-0.5 * z * z) / math.sqrt(2 * math.pi) if math.isfinite(z) else 0.0


def _cdf(z):
    return 0.5 * (1 + math.erf(z / math.sqrt(2))) if math.isfinite(z) else 1.0


@pytest.mark.parametrize("bits", ec.BITS)
def test_tables_are_the_lloyd_max_fixed_point(bits):
    """In float64: every c_i is the mean of |z| on its cell and every t_i the midpoint of its neighbours, within 1e-6 relative;
    both ascend strictly; the mean squared error the table implies is Lloyd-Max's, within 1e-5."""
    tab = ec.TABLES[bits]
    c, t = tab.c.astype(np.float64), tab.t.astype(np.float64)
    assert list(mx.bits_of(tab.c)) == ec.C_BITS[bits] and list(mx.bits_of(tab.t)) == ec.T_BITS[bits]
    assert np.all(np.diff(c) > 0) and np.all(np.diff(t) > 0) and c[0] > 0
    edges = [0.0] + list(t) + [math.inf]
    mse = 1.0
    for i in range(c.size):
        lo, hi = edges[i], edges[i + 1]
        p, m1 = _cdf(hi) - _cdf(lo), _pdf(lo) - _pdf(hi)
        assert abs(m1 / p - c[i]) <= 1e-6 * c[i], (bits, i)
        mse += 2 * (p * c[i] * c[i] - 2 * c[i] * m1)      # (both signs)
    for i in range(t.size):
        assert abs((c[i] + c[i + 1]) / 2 - t[i]) <= 1e-6 * t[i], (bits, i)
    print("bits %d: implied mse %.6f" % (bits, mse))
    assert abs(mse - LLOYD_MAX_MSE[bits]) <= 1e-5
    hdr = open(os.path.join(ROOT, "include", "gq_eden.h")).read()
    src = open(os.path.join(ROOT, "gradient-quantization_amd", "csrc", "eden.hip")).read()
    for v in ec.C_BITS[bits] + ec.T_BITS[bits]:
        assert "0x%08x" % v in hdr and "0x%08xu" % v in src


@pytest.mark.parametrize("mode", [ec.UNBIASED, ec.MSE])
def test_one_magnitude_is_drive(mode):
    """With the table c = [1], no thresholds, the restatement gives drive_contract.compress's section (code bits and scales) and
    dense decode bit for bit, error feedback included."""
    for n, seed in ((1, 1), (255, 2), (4096 + 300, 3), (2 * 4096 + 257, 4)):
        for kind in ("student", "zeros", "subnormals", "huge"):
            w = dc.FINITE_KINDS[kind](n, seed)
            e = dc.gaussian(n, seed + 50)
            for err, s in ((None, None), (e, 0.46211715726)):
                a = dc.compress(w, mode, dc.SEEDED, err, s)
                b = ec.compress(w, 1, mode, dc.SEEDED, err, s, table=ec.DRIVE_TABLE)
                assert np.array_equal(a[0], b[0]) and mx.same(a[1], b[1]) and mx.same(a[5], b[5])
                assert np.array_equal(dc.code_bits(a[4]), b[6])
                if err is not None:
                    assert mx.same(a[3], b[3]) and mx.same(a[2], b[2])


@pytest.mark.parametrize("bits", ec.BITS)
def test_magnitudes_against_a_float64_nearest_centroid_search(bits):
    """m_j is the index of the centroid nearest to |x'_j| / sigma in float64, except within 4 ulp of a threshold.  The share of
    such elements was estimated at <= 1e-4 when the contract was written; observed here: 0 (b = 2), 1 (b = 3) and
    1 (b = 4) of 795,648 elements, that is 0, 1.3e-6 and 1.3e-6."""
    tab = ec.TABLES[bits]
    excepted = total = 0
    for w in (dc.gaussian(1 << 17, 1), dc.student(1 << 17, 2), dc.student(4096 + 300, 3), dc.gaussian(1 << 17, 5) * f32(1e4)):
        for signs in (dc.SEEDED, mxr.ZERO_SIGNS):
            xp = mxr.forward_blocks(dc.pad_blocks(w), signs)
            m, Q, sigma = ec.magnitudes(xp, tab)
            x64 = xp.astype(np.float64)
            s64 = np.sqrt((x64 * x64).sum(axis=1) / 256)
            r = np.abs(x64) / s64[:, None]
            want = np.abs(r[:, :, None] - tab.c.astype(np.float64)[None, None, :]).argmin(axis=2)
            th = ec.thresholds(sigma, tab)
            a = np.abs(xp)
            near = np.zeros(a.shape, bool)
            for i in range(th.shape[1]):
                near |= np.abs(a.astype(np.float64) - th[:, i:i + 1].astype(np.float64)) <= 4 * np.spacing(th[:, i:i + 1]).astype(np.float64)
            assert np.array_equal(m[~near], want[~near].astype(U32))
            excepted += int(near.sum())
            total += near.size
    print("bits %d: %d of %d elements within 4 ulp of a threshold (%.2g)" % (bits, excepted, total, excepted / total))
    assert excepted / total <= 1e-4


@pytest.mark.parametrize("bits", ec.BITS)
def test_unbiased_scale_is_exact_in_the_direction_of_x(bits):
    """|<D, x> - |x|^2| <= 1e-5 |x|^2 (float64 accumulation), n = 1, 10, 255, 257 among them."""
    for n in (1, 10, 255, 257, 2048, 4097, 8193):
        for kind in ("gaussian", "student"):
            x = dc.FINITE_KINDS[kind](n, 40 + n)
            for signs in (dc.SEEDED, mxr.ZERO_SIGNS, dc.SIGN_SETS["seed2"]):
                D = ec.compress(x, bits, ec.UNBIASED, signs)[1].astype(np.float64)
                x64 = x.astype(np.float64)
                assert abs(np.dot(D, x64) - np.dot(x64, x64)) <= 1e-5 * np.dot(x64, x64), (kind, n)


@pytest.mark.parametrize("bits", ec.BITS)
def test_mse_scale_is_the_least_squares_one(bits):
    """Perturbing S by +-1 % raises every block's squared error."""
    tab = ec.TABLES[bits]
    for x in (dc.student(4096 + 300, 7), dc.gaussian(2048, 8)):
        _, _, _, _, xp, S, codes = ec.compress(x, bits, ec.MSE, dc.SEEDED)
        x64 = xp.astype(np.float64)

        def sq(scale):
            y = ec.values(codes, scale.astype(f32), tab).astype(np.float64)
            return ((y - x64) ** 2).sum(axis=1)

        base = sq(S)
        assert np.all(sq(S * f32(1.01)) > base) and np.all(sq(S * f32(0.99)) > base)


def _sections(inputs, bits, mode, **kw):
    return [ec.compress(v, bits, mode, ec.SEEDED, **kw)[0] for vs in inputs.values() for v in vs]


def _differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("bits", ec.BITS)
def test_every_mutation_changes_wire_bits_on_the_gpu_tests_inputs(bits):
    """A sequential sum, a reversed tree, `>=` for `>`, theta = t * sqrtf(Q) / 16 and an fma in P each change at least one bit of
    the wire sections of tests/test_gpu_zz_eden_contract.py's inputs.  `>=` needs an element ON a threshold: the fixed-seed search
    of 2^25 rotated coordinates (eden_contract.on_threshold_blocks) found 2 (b = 2), 3 (b = 3) and 7 (b = 4), in as many blocks.
    t * sqrtf(Q) / 16 is the same number unless Q * 2^-8 underflows: the `tiny` inputs."""
    inputs = ec.gpu_inputs(bits)
    blocks, count = ec.on_threshold_blocks()[bits]
    print("bits %d: %d coordinates on a threshold in %d blocks" % (bits, count, blocks.shape[0]))
    assert count >= 1 and blocks.shape[0] >= 1 and inputs["on_threshold"][0].size == blocks.size
    for mode in (ec.UNBIASED, ec.MSE):
        want = _sections(inputs, bits, mode)
        assert not _differs(want, _sections(inputs, bits, mode))
        assert _differs(want, _sections(inputs, bits, mode, tree=ec.sequential_sum)), "a sequential sum"
        assert _differs(want, _sections(inputs, bits, mode, tree=ec.reversed_tree_sum)), "a reversed tree"
        assert _differs(want, _sections(inputs, bits, mode, spread_fn=ec.spread_sqrt_first)), "t * sqrtf(Q) / 16"
        assert _differs(want, _sections(inputs, bits, mode, fused=True)), "an fma in P"
        on = {"on_threshold": inputs["on_threshold"]}
        a, b = _sections(on, bits, mode), _sections(on, bits, mode, ge=True)
        assert _differs(a, b), ">= for >"
        cb = ec.TABLES[bits].code_bytes
        nb = blocks.shape[0]
        changed = (a[0][:nb * cb].reshape(nb, cb) != b[0][:nb * cb].reshape(nb, cb)).any(axis=1)
        assert changed.all(), "every block the search found holds an element on a threshold"


@pytest.mark.parametrize("bits", ec.BITS)
def test_preconditions_of_the_gpu_tests_inputs(bits):
    """Every finite input rotates to finite blocks; S = +inf exactly where Q overflows (the 2^63 blocks, unbiased scale only); the
    all-zero blocks have S = +0, the subnormal ones Q = 0 and P > 0, the tiny ones a subnormal Q * 2^-8 > 0; the non-finite
    tensor's bad blocks are the two it names."""
    inputs = ec.gpu_inputs(bits)
    for mode in (ec.UNBIASED, ec.MSE):
        for name, vs in inputs.items():
            for v in vs:
                assert np.isfinite(v).all()
                _, D, _, _, xp, S, _ = ec.compress(v, bits, mode, ec.SEEDED)
                bad_x, bad_s = ec.loose_blocks(xp, S)
                assert not bad_x.any() and not np.isnan(S).any()
                with np.errstate(over="ignore"):
                    Q = ec.tree_sum((xp * xp).astype(f32))
                assert np.array_equal(bad_s, np.isinf(Q) if mode == ec.UNBIASED else np.zeros(S.size, bool))
                if name == "kind_huge":      # (Q = |w|^2 overflows wherever a block holds more than a handful of elements)
                    held = np.minimum(v.size - 256 * np.arange(S.size), 256)
                    assert np.isinf(Q[held >= 16]).all() and (mode == ec.MSE or np.isposinf(S[held >= 16]).all())
                elif name != "sizes":
                    assert np.isfinite(S).all() and np.isfinite(D).all() and not np.isinf(Q).any()
                if name == "kind_zeros":
                    assert not mx.bits_of(S).any()
                if name == "kind_subnormals":
                    assert not Q.any() and (not mx.bits_of(S).any() if mode == ec.UNBIASED else (S > 0).all())
                if name == "kind_tiny":
                    q8 = (Q * f32(2.0 ** -8)).astype(f32)
                    held = np.minimum(v.size - 256 * np.arange(S.size), 256)      # (a last block of one element: Q = 0 with P > 0)
                    assert np.all(q8[held >= 16] > 0) and np.all(q8 < f32(2.0 ** -126)) and np.all(S[held >= 16] > 0)
        assert any(np.isinf(ec.compress(v, bits, ec.UNBIASED, ec.SEEDED)[5]).any() for v in inputs["sizes"])
        w, bad = ec.nonfinite()
        _, D, _, _, xp, S, _ = ec.compress(w, bits, mode, ec.SEEDED)
        assert list(np.flatnonzero(ec.loose_blocks(xp, S)[0])) == bad and np.all(mx.bits_of(S[bad]) == mx.QNAN)
        for b in range(S.size):
            blk = D[b * 256:(b + 1) * 256]
            assert np.isnan(blk).all() if b in bad else (np.isfinite(S[b]) and np.isfinite(blk).all())


@pytest.mark.parametrize("bits", ec.BITS)
def test_wire_layout(bits):
    """Pack and unpack round-trip; a lane's eight codes are the b bytes at byte b * lane; scales, pad and section sizes."""
    cb = 32 * bits
    for n in (1, 255, 256, 257, 1024, 1025, 4097):
        nb = -(-n // 256)
        assert ec.section_bytes(n, bits) == nb * cb + (4 * nb + 15) // 16 * 16 and ec.section_bytes(n, bits) % 16 == 0
        x = dc.student(n, n)
        sec, D, _, _, xp, S, codes = ec.compress(x, bits, ec.UNBIASED, ec.SEEDED)
        assert sec.size == ec.section_bytes(n, bits) and not sec[nb * (cb + 4):].any()
        for b, lane in ((0, 0), (nb - 1, 31), (nb - 1, 1), (nb // 2, 17)):
            word = int.from_bytes(bytes(sec[cb * b + bits * lane:cb * b + bits * lane + bits]), "little")
            assert [(word >> (bits * k)) & ((1 << bits) - 1) for k in range(8)] == list(codes[b, 8 * lane:8 * lane + 8])
        sign = codes >> U32(bits - 1)
        assert np.array_equal(sign, mx.bits_of(xp) >> U32(31)) and codes.max() < 1 << bits
        assert np.array_equal(sec[nb * cb:nb * (cb + 4)].view("<f4"), S)
        c2, S2 = ec.unpack(sec, n, bits)
        assert np.array_equal(c2, codes) and np.array_equal(mx.bits_of(S2), mx.bits_of(S))
        assert np.array_equal(mx.bits_of(ec.decode_mean([sec], n, bits, ec.SEEDED, plain=True)), mx.bits_of(D))
    rs = np.random.RandomState(bits)
    codes = rs.randint(0, 1 << bits, (3, 256)).astype(U32)
    S = rs.rand(3).astype(f32)
    c2, S2 = ec.unpack(ec.pack(codes, S, bits), 3 * 256, bits)
    assert np.array_equal(c2, codes) and np.array_equal(S2, S)
    offs, dense, ub = ec.layout([300, 5000], bits, [10])
    assert offs == [0, ec.section_bytes(300, bits)] and dense == [(offs[1] + ec.section_bytes(5000, bits), 10)] and ub % 16 == 0
    # the hand-built payloads hold every code value at every one of a lane's eight positions
    pc = np.stack([ec.unpack(s, 600, bits)[0][0] for s in ec.payloads(600, bits, 1 << bits, 5)])
    for k in range(8):
        assert set(pc[:, k::8].reshape(-1).tolist()) == set(range(1 << bits))
        assert all(set(pc[r, k::8].tolist()) == set(range(1 << bits)) for r in range(pc.shape[0]))


README_TABLE = {      # relative L2 error of decode(compress(x)), 262,144 elements, sign seed 1: (unbiased, mse)
    ("gaussian", 2): (0.3635, 0.3415), ("gaussian", 3): (0.1872, 0.1840), ("gaussian", 4): (0.0969, 0.0964),
    ("student", 2): (0.3583, 0.3370), ("student", 3): (0.1841, 0.1810), ("student", 4): (0.0947, 0.0943),
}


def test_error_table_of_the_readme():
    """N(0, 1) * 1e-3 (numpy.random.default_rng(3)) and Student-t(3) * 1e-3 (default_rng(4)) at 262,144 elements, sign seed 1: the
    table the README prints, to 4 digits; the mse figures sit on sqrt(Lloyd-Max MSE) within 0.01 for the Gaussian."""
    xs = {"gaussian": (np.random.default_rng(3).standard_normal(262144) * 1e-3).astype(f32),
          "student": (np.random.default_rng(4).standard_t(3, 262144) * 1e-3).astype(f32)}
    readme = open(os.path.join(ROOT, "README.md")).read()
    for (kind, bits), want in sorted(README_TABLE.items()):
        got = tuple(round(ec.rel_l2(xs[kind], ec.compress(xs[kind], bits, ec.MODES[m], mxr.sign_words(1))[1]), 4) for m in ("unbiased", "mse"))
        print("%-8s b = %d  unbiased %.4f  mse %.4f" % (kind, bits, got[0], got[1]))
        assert got == want
        assert "%.4f / %.4f" % want in readme
        if kind == "gaussian":
            assert abs(got[1] - math.sqrt(LLOYD_MAX_MSE[bits])) <= 0.01 and got[0] >= got[1]


def test_the_mean_over_seeds_averages_out():
    """The mean of 256 decodes of one 4,096-element vector under the sign seeds 100 ... 355.  Unbiased scale: the errors of
    independent rotations are uncorrelated, so the error falls by about sqrt(256) = 16 -- asserted <= 1.25 / 16 of the single
    shot's (observed 0.0229, 0.0120, 0.0060 for b = 2, 3, 4 against 0.364, 0.187, 0.097 single shot; DRIVE at one bit: 0.048
    against 0.755).  The mse scale keeps its shrinkage towards 0, about the Lloyd-Max MSE itself (observed 0.1179, 0.0358, 0.0110)."""
    v = (np.random.default_rng(3).standard_normal(4096) * 1e-3).astype(f32)
    for bits in ec.BITS:
        mean, single = {}, {}
        for m in ("unbiased", "mse"):
            acc = np.zeros(4096)
            for k in range(256):
                D = ec.compress(v, bits, ec.MODES[m], mxr.sign_words(100 + k))[1]
                acc += D
            single[m] = ec.rel_l2(v, D)
            mean[m] = ec.rel_l2(v, acc / 256)
        print("b = %d: single shot %s, mean of 256 seeds %s" % (bits, single, mean))
        assert mean["unbiased"] <= 1.25 / 16 * single["unbiased"] and mean["unbiased"] < 0.048
        assert mean["mse"] >= 0.5 * LLOYD_MAX_MSE[bits] and mean["mse"] > mean["unbiased"]
