"""tests/thr_contract.py -- the numpy restatement of include/gq_thr.h the GPU tests compare against -- checked on the CPU: gq_ln against
math.log, the tree orders, the fused multiply-add and the reciprocal that must each change bits, the kept set against a scalar loop and against
top-k's decode rule, the preconditions of the GPU file's inputs, the wire layout and the README's estimator table."""
import math
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import thr_contract as tc  # noqa: E402
import topk_contract as tk  # noqa: E402

f32, f64, u32 = np.float32, np.float64, np.uint32


def test_the_header_states_what_the_restatement_uses():
    h = open(os.path.join(ROOT, "include", "gq_thr.h")).read()
    for j, c in enumerate(tc.LN_C):
        assert ("0x%016X" % c) in h and tc.d_from(c) == 1.0 / (2 * j + 1)
    assert ("0x%016X" % tc.LN_LN2) in h and tc.d_from(tc.LN_LN2) == math.log(2.0)
    assert ("0x%016X" % tc.LN_SQRT2) in h and tc.d_from(tc.LN_SQRT2) == math.sqrt(2.0)
    for name, v in (("GQ_THR_CHUNK", tc.ITEM), ("GQ_THR_HEADER_BYTES", tc.HDR), ("GQ_THR_MAX_STAGES", tc.MAX_STAGES)):
        assert int(re.search(r"#define %s (\d+)" % name, h).group(1)) == v


def test_gq_ln_against_math_log():
    """Relative error <= 1e-13 on integer ratios c / k up to 2^31 and on a dense grid (the fit calls it with c^ / k > 1 only)."""
    rs = np.random.RandomState(0)
    xs = [float(x) for x in np.linspace(1.0, 4.0, 30001)[1:]] + [float(x) for x in np.geomspace(1.0 + 1e-9, 2.0 ** 31, 20000)]
    for _ in range(20000):
        k = int(rs.randint(1, 1 << 20))
        c = int(rs.randint(k + 1, 1 << 31))
        xs.append(float(c) / float(k))
    xs += [math.sqrt(2.0), tc.d_from(tc.LN_SQRT2 + 1), tc.d_from(tc.LN_SQRT2 - 1), 2.0, 2.0 ** 31, 1.0 + 2.0 ** -52]
    worst = max(abs(tc.gq_ln(x) - math.log(x)) / math.log(x) for x in xs)
    print("gq_ln: worst relative error %.3g over %d points" % (worst, len(xs)))
    assert worst <= 1e-13
    assert tc.gq_ln(1.0) == 0.0


def _bisect(e, lo, hi):
    """Adjacent f32 bit patterns lo < hi with e(lo) != e(hi), for e monotone in the bits; None when e(lo) == e(hi) at the start."""
    elo = e(lo)
    if e(hi) == elo:
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if e(mid) == elo:
            lo = mid
        else:
            hi = mid
    return lo, hi


def _val(b):
    return tc.from_bits(np.array([b], dtype=u32))[0]


def _mutation_shows(mutant, seeds, S=1):
    """Some input on which the mutant's eta differs in bits.  A last-bit difference in f64 reaches eta's bits only where the
    contract's t sits on an f32 rounding boundary, so the inputs are built for it: one item of 2^53-sized and unit-sized magnitudes
    plus two tuning elements, the first bisected to where eta changes, the second (far smaller) bisected inside the first's last
    step -- together they move Sigma in steps below its last bit."""
    kw = dict(k=16, S=S)
    tiny = f32(2.0 ** -20)      # (the second tuning element at rest: non-zero, so that it always counts)
    for seed in seeds:
        rs = np.random.RandomState(seed)
        base = np.where(rs.rand(4096) < 0.02, 2.0 ** 53, 1.0 + rs.rand(4096)).astype(f32)
        base[rs.rand(4096) < 0.3] *= f32(-1)
        base[7] = f32(0)      # (c = 4,095: a division by c that is no shift of the exponent)

        def make(x1, x2, base=base):
            v = base.copy()
            v[1234], v[2345] = x1, x2
            return v

        c1 = _bisect(lambda b: tc.ebits(tc.fit(make(_val(b), tiny), **kw)), tc.ebits(f32(2.0 ** 33)), tc.ebits(f32(2.0 ** 37)))
        if c1 is None:
            continue
        x1 = _val(c1[0])
        step = f32(_val(c1[1]) - x1)
        c2 = _bisect(lambda b: tc.ebits(tc.fit(make(x1, _val(b)), **kw)), tc.ebits(tiny), tc.ebits(f32(step * 2)))
        for x2 in ([_val(b) for b in c2] if c2 else [tiny]):
            v = make(x1, x2)
            if tc.ebits(tc.fit(v, **kw)) != tc.ebits(tc.fit(v, **dict(kw, **mutant))):
                return True
    return False


@pytest.mark.parametrize("order", ["seq", "desc"])
def test_tree_order_changes_eta(order):
    """A sequential and a descending-stride sum of the item's f64 terms each change eta's bits on an input built for it."""
    assert _mutation_shows(dict(order=order), range(10))


def _place(n, seed, big, rest):
    """One item of n elements: `big` at scattered places with scattered signs, `rest` everywhere else."""
    rs = np.random.RandomState(seed)
    v = np.full(n, rest, dtype=f32)
    pos = np.sort(rs.permutation(n)[:len(big)])
    v[pos] = np.asarray(big, dtype=f32)
    v[rs.rand(n) < 0.4] *= f32(-1)
    return v, pos


def test_a_reciprocal_changes_eta():
    """beta = Sigma * (1 / c) instead of Sigma / c changes eta's bits on an input built for it.  One stage, one item, c = 4,095 (no
    power of two): one zero, 4,092 elements of magnitude 1 and three tuning elements on disjoint bit ranges (steps 2^-13, 2^-37 and
    2^-40), so that Sigma is ANY multiple of 2^-40 in range and every partial sum of the tree is exact.  The two quotients differ by
    one f64 ulp at most, which reaches eta only where t = beta * L sits on an f32 rounding midpoint: for each midpoint M the search
    solves Sigma = M * c / L and looks at the f64 neighbours of the solution."""
    n, k, c = 4096, 16, 4095
    L = tc.gq_ln(float(c) / float(k))
    hit = None
    for j in range(1, 4000):
        M = 7.5 + (j + 0.5) * 2.0 ** -21
        N0 = int(round(M * c / L * 2.0 ** 40))
        for N in range(N0 - 4, N0 + 5):
            R = N - 4092 * 2 ** 40                                # the tuning elements' share, in units of 2^-40
            ma, mb, md = R >> 27, (R >> 3) & 0xffffff, R & 7
            sigma = N * 2.0 ** -40
            if (2 ** 23 <= ma < 2 ** 24 and mb and md
                    and tc.ebits(tc.round_f32((sigma / float(c)) * L)) != tc.ebits(tc.round_f32((sigma * (1.0 / float(c))) * L))):
                hit = N
                break
        if hit:
            break
    assert hit is not None
    v, pos = _place(n, 5, [ma * 2.0 ** -13, mb * 2.0 ** -37, md * 2.0 ** -40], 1.0)
    v[[i for i in range(n) if i not in set(pos.tolist())][0]] = f32(0.0)
    trace = []
    eta = tc.fit(v, k, 1, trace=trace)
    assert trace[0][1] == c and trace[0][2] == hit * 2.0 ** -40
    assert tc.ebits(eta) != tc.ebits(tc.fit(v, k, 1, recip=True))


def test_a_fused_multiply_add_changes_eta():
    """t = fma(beta, L, eta) instead of the rounded product, then the sum, changes eta's bits on an input built for it.  At stage 1
    eta_0 = +0 and the two agree always, so: two stages, one item of 4,096 non-zeros, k = 16.  The small elements are tuned to make
    eta_1 = 1.0f; c_2 elements exceed it: all but one of magnitude X in [32, 128) and one in (1, 2), so Sigma_2 = N * 2^-23 for ANY
    integer N in range, added exactly in any order.  fma and the two roundings differ by one f64 ulp of t at most, which reaches
    eta_2 only where t sits on an f32 rounding midpoint: for each midpoint M = 16 + (j + 1/2) 2^-19 the search solves
    N = (M - 1) * c_2 / L_2 * 2^23 in fixed point (44 fraction bits, exact modulo 2^64) and keeps the M whose solution is an integer
    to within a few ulps of t."""
    from fractions import Fraction
    n, k = 4096, 16
    hit = None
    for c2 in (24, 20, 28, 32, 36, 40):
        L2 = tc.gq_ln(float(c2) / float(k))
        K = Fraction(8 * c2) / Fraction(L2)                      # N = A * K with A = 15 * 2^20 + 2 j + 1
        Kfix = int(K * 2 ** 44)
        A = np.uint64(15 * 2 ** 20 + 1) + np.uint64(2) * np.arange(2 ** 23, dtype=np.uint64)
        frac = (A * np.uint64(Kfix)) & np.uint64(2 ** 44 - 1)    # (wraps modulo 2^64, which the low 44 bits do not see)
        near = np.flatnonzero((frac < np.uint64(2 ** 28)) | (frac > np.uint64(2 ** 44 - 2 ** 28)))
        for i in near:
            N = int(round(int(A[i]) * K))
            beta = (N * 2.0 ** -23) / float(c2)
            std = 1.0 + beta * L2
            fused = float(Fraction(beta) * Fraction(L2) + 1)
            if tc.ebits(tc.round_f32(std)) != tc.ebits(tc.round_f32(fused)):
                hit = N
                break
        if hit:
            break
    assert hit is not None
    a64 = ((hit - 2 ** 22) // (c2 - 1)) // 64 * 64               # X - 1 in units of 2^-23, a multiple of 2^-17
    b = hit - (c2 - 1) * a64                                     # the element in (1, 2): 1 + b * 2^-23
    assert 0 < b < 2 ** 23 and 32.0 <= 1.0 + a64 * 2.0 ** -23 < 128.0
    big = [1.0 + a64 * 2.0 ** -23] * (c2 - 1) + [1.0 + b * 2.0 ** -23]
    L1 = tc.gq_ln(float(n) / float(k)) / 2.0
    small = (float(n) / L1 - sum(big)) / (n - c2)                # eta_1 = (Sigma_1 / 4096) * L1 = 1.0
    assert 0.0 < small < 0.9
    v, pos = _place(n, 6, big, small)
    tune = [i for i in range(n) if i not in set(pos.tolist())][0]
    for _ in range(8):                                           # one small element takes up what rounding the others left
        trace = []
        tc.fit(v, k, 2, trace=trace)
        if len(trace) == 2 and trace[1][4] == 1.0:
            break
        v[tune] = f32(abs(float(v[tune])) + (float(n) / L1 - trace[0][2]))
    assert trace[1][4] == 1.0 and trace[1][1] == c2 and trace[1][2] == hit * 2.0 ** -23
    assert tc.ebits(tc.fit(v, k, 2)) != tc.ebits(tc.fit(v, k, 2, fused=True))


@pytest.mark.parametrize("make", [tc.specials, tc.laplace, tc.half_zero])
def test_kept_set_against_a_scalar_loop_and_topk(make):
    n, cr = 8193, 64
    v = make(n, 9)
    k = n // cr
    cap = tc.capacity(n, k)
    for eta in [f32(0.0), f32(1e-3), f32(3e-3), tc.FLT_MAX, tc.fit(v, k, 3)]:
        keep, found = tc.kept_mask(v, eta, cap)
        eb = tc.ebits(eta)
        want, cnt = np.zeros(n, dtype=bool), 0
        for i in range(n):
            b = int(tc.bits(v[i:i + 1])[0]) & 0x7fffffff
            key = 0x7fffffff if b > 0x7f800000 else b
            if key > eb:
                cnt += 1
                want[i] = cnt <= cap
        assert cnt == found and np.array_equal(keep, want)
    # at equal threshold top-k keeps the same set and decodes the same tensor: T = the (kk + 1)-th largest key, kk = #(key > T)
    ks = np.sort(tc.keys(v))[::-1]
    T = int(ks[k])
    kk = int((tc.keys(v) > T).sum())
    if 0 < kk <= cap and int(ks[kk - 1]) > T:
        keep, found = tc.kept_mask(v, tc.from_bits(np.array([T], dtype=u32))[0], cap)
        assert found == kk
        if kk == 0 or ks[kk - 1] != ks[kk]:
            assert np.array_equal(np.flatnonzero(keep), np.sort(tk.kept(v, kk))) and np.array_equal(tc.bits(tc.dense(v, keep)), tk.bits(tk.dense(v, kk)))


def test_preconditions_of_the_gpu_inputs():
    c = {w: tc.outcome_case(w) for w in ["cap", "cap+1", "far", "none", "sparse", "on_eta"]}
    assert c["cap"].found == c["cap"].cap and c["cap+1"].found == c["cap+1"].cap + 1
    far = c["far"]      # (65,537 elements: 17 items, the kept ones all in the first two, exceeding ones up to the sixteenth)
    assert far.found == 16 * far.cap == int((np.abs(far.v) >= 1).sum()) and far.S == 1 and 0 < far.eta_out < 1
    assert np.flatnonzero(np.abs(far.v) >= 1)[far.cap - 1] < 2 * tc.ITEM and np.flatnonzero(np.abs(far.v) >= 1)[-1] >= 15 * tc.ITEM
    assert c["none"].found == 0 and np.isfinite(c["none"].v).all()
    assert c["sparse"].found == int((c["sparse"].v != 0).sum()) < c["sparse"].k and tc.ebits(c["sparse"].eta_out) == 0
    on = c["on_eta"]
    assert int((tc.keys(on.v) == tc.ebits(on.eta_out)).sum()) == 3 and on.found <= on.cap
    assert not tc.exceeding(on.v, on.eta_out)[tc.keys(on.v) == tc.ebits(on.eta_out)].any()
    for w in ("cap", "none"):      # fixed thresholds ON an element
        assert int((tc.keys(c[w].v) == tc.ebits(c[w].eta_out)).sum()) >= 1
    sp = tc.specials(1001, 3)
    assert int((tc.keys(sp) > tc.MAX_ETA).sum()) == 6 and int((tc.keys(sp) == tc.MAX_ETA).sum()) == 2
    assert np.isnan(sp).sum() == 4 and np.isinf(sp).sum() == 2


def test_wire_layout():
    v = tc.laplace(8193, 2)
    sec, D, w, ne, eta, found = tc.compress(v, 64, 3)
    cap = tc.capacity(8193, 128)
    assert cap == 192 and sec.size == 16 + 8 * 192 == tc.section_bytes(8193, 64)
    hdr, idx, val = tc.split_section(sec, cap)
    kept = int(hdr[0])
    assert kept == min(found, cap) and int(hdr[1]) == found and int(hdr[2]) == tc.ebits(eta) and int(hdr[3]) == 0
    assert np.all(np.diff(idx[:kept].astype(np.int64)) > 0) and np.all(idx[kept:] == tc.NO_INDEX) and not tc.bits(val[kept:]).any()
    assert np.array_equal(tc.bits(val[:kept]), tc.bits(v[idx[:kept]]))
    assert tc.section_bytes(1001, 256) == 16 + 48 and tc.capacity(1001, 3) == 5      # an odd cap: 8 zero bytes behind the values
    assert tc.capacity(300, 1, 40000) == 300                                          # never above n
    sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))
    from gq_amd.codecs import thr_section_bytes
    for n in (1001, 4097, 200704, 2359296):
        assert thr_section_bytes(n, 256, 150) == tc.section_bytes(n, 256)
    with pytest.raises(ValueError):
        thr_section_bytes(100, 256)
    # the README's figure: one user's ResNet-50 wire at cr = 256 -- the 76 tensors over 1,000 elements as 16-byte aligned sections,
    # the 85 others behind them as packed float32 (the quantizer's layout), against 94,083,376 B dense
    import json
    with open(os.path.join(HERE, "golden", "resnet50_cifar_shapes.json")) as f:
        sizes = [int(np.prod(s)) for s in json.load(f)["parameter_shapes"]]
    big, small = [n for n in sizes if n > 1000], [n for n in sizes if n <= 1000]
    assert (len(big), len(small), sum(n // 256 for n in big)) == (76, 85, 91790)
    offs, dense_tab, total = tc.layout(big, 256, 150, small)
    assert total == 1192352 and tc.layout(big, 256, 100, small)[2] == 825184
    off = 0
    for n in big:
        off = tc.up16(off + thr_section_bytes(n, 256, 150))
    assert tc.up16(off + 4 * sum(small)) == total
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "1,192,352" in readme and "825,184" in readme


TABLE_SIZES = (65536, 2359296)


@pytest.fixture(scope="module")
def table():
    """kept / k = found / k for S = 1 ... 4, cr = 256, fixed seeds; at the large size also with fit stride 8."""
    rows = {}
    for fam, make in tc.FAMILIES.items():
        for n in TABLE_SIZES:
            v = make(n, 1)
            k = n // 256
            for m in ((1, 8) if n == TABLE_SIZES[1] else (1,)):
                rows[(fam, n, m)] = [int(tc.exceeding(v, tc.fit(v, k, S, m)).sum()) / k for S in (1, 2, 3, 4)]
    return rows


def test_estimator_table(table):
    """The README's table.  Asserted: Laplace at S = 3 within 10 % of k at n >= 2^20 (the fit is exact for exponential magnitudes;
    sampling noise is ~1.6 % at k = 4,096); every input at S = 3, m = 1 within cap (1.5 k).  The rest is reported."""
    for key in sorted(table):
        print("%-10s n = %8d  m = %d   " % key + "  ".join("%.3f" % r for r in table[key]))
    assert abs(table[("laplace", 2359296, 1)][2] - 1.0) <= 0.10
    for (fam, n, m), r in table.items():
        if m == 1:
            assert 0 < r[2] <= 1.5, (fam, n, r)
