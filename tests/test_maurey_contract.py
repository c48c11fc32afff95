"""tests/maurey_contract.py against itself (no GPU): the restatement of include/gq_maurey.h against a longdouble running sum and
against integer arithmetic, and every precondition tests/test_gpu_maurey_contract.py states about its inputs -- so that the
reference the kernels are held to cannot be wrong silently."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import maurey_contract as mc  # noqa: E402


@pytest.mark.parametrize("n", [1, 17, 4097, 70001, 1048577, 2097153])
def test_tree_sum_against_longdouble(n):
    """C never decreases, ends in T and stays within n * 2^-53 * T of the longdouble running sum (the classical bound of an f64 sum
    of n terms in any order); the drawn elements are the longdouble ones wherever the draw lies more than that bound from a
    boundary, and at most 1 % of the draws lie that close."""
    v = mc.heavy_tailed(n, n % 1000)
    C, T = mc.tree_cdf(v)
    assert C.size == n and np.all(np.diff(C) >= 0) and C[-1] == T
    L = np.cumsum(np.abs(v).astype(np.longdouble))
    bound = np.longdouble(n) * np.longdouble(2.0 ** -53) * L[-1]
    worst = np.max(np.abs(C.astype(np.longdouble) - L))
    print("n = %d: |C - longdouble| <= %.3g * T (bound %.3g * T)" % (n, float(worst / L[-1]), float(bound / L[-1])))
    assert worst <= bound
    k = max(8, min(n // 33, 20000))
    u = np.random.RandomState(n % 1000 + 1).rand(k).astype(np.float32)
    idx = mc.draw_indices(v, u)
    t = u.astype(np.longdouble) * L[-1]
    want = np.searchsorted(L, t, side="right")
    below = np.where(want > 0, L[np.maximum(want - 1, 0)], np.longdouble(0))
    close = np.minimum(L[want] - t, t - below) <= bound
    print("          %d of %d draws within the bound of a boundary" % (int(close.sum()), k))
    assert close.sum() <= k // 100
    assert np.array_equal(idx[~close], want[~close])
    assert np.all(v[idx] != 0)


@pytest.mark.parametrize("long", [False, True], ids=["12289", "1048577"])
def test_integer_inputs_equal_integer_arithmetic(long):
    """The tie inputs: C is the integer running sum, T = 2^p, every u is exact (float64(u) * T is the integer t it was made from),
    every t is some C_i or 0, and a tie behind a zero run selects the first element behind the run."""
    v, u, t, p, behind = mc.tie_case(long)
    C, T = mc.tree_cdf(v)
    Ci = np.cumsum(np.abs(v.astype(np.int64)))
    assert p <= 24 and T == float(1 << p) and np.array_equal(C, Ci.astype(np.float64))
    assert u.dtype == np.float32 and np.array_equal(u.astype(np.float64) * T, t) and u.max() < 1
    assert np.all(np.isin(t, np.concatenate([[0.0], C])))
    idx = mc.draw_indices(v, u)
    assert np.array_equal(idx, np.searchsorted(Ci, t.astype(np.int64), side="right"))
    assert np.array_equal(idx[:behind.size], behind) and np.all(v[idx] != 0)
    runs = mc.TIE_LONG_RUNS if long else mc.TIE_SMALL_RUNS
    for lo, hi in runs:
        assert not v[lo:hi].any() and v[hi] != 0 and (lo == 0 or v[lo - 1] != 0)
    inside = lambda x: any(lo < x < hi for lo, hi in runs)      # an edge with zeros on both sides
    if long:
        assert -(-v.size // mc.CHUNK) == 257      # m = 2: a run is 8192 elements
        assert inside(8192 * 5) and inside(8192 * 20 + 4096) and inside(8192 * 127) and runs[-1][1] == 8192 * 128 and not v[8192 * 9:8192 * 10].any()
    else:
        assert inside(16) and inside(256) and inside(4096) and not v[8192:12288].any()


def test_the_clamp_shows_the_order_of_additions():
    """|v| = [2^100, 2^46 x 4989, 0 x 10]: with u = 1 the tree order selects 4989, a left-to-right f64 sum selects 0."""
    v = mc.order_case()
    assert v.size == mc.ORDER_N and (v < 0).any() and (v > 0).any()
    assert np.array_equal(np.abs(v[:3]), np.float32([2.0 ** 100, 2.0 ** 46, 2.0 ** 46])) and not v[mc.ORDER_PICK + 1:].any()
    C, T = mc.tree_cdf(v)
    idx = mc.draw_indices(v, np.ones(7, np.float32))
    assert np.all(idx == mc.ORDER_PICK)
    P = np.cumsum(np.abs(v).astype(np.float64))
    assert np.searchsorted(P, np.nextafter(P[-1], 0.0), side="right") == 0
    assert T != P[-1]
    # the same through the run level: only a sum that adds two items' 2^48 at a time moves 2^100 at all
    v = mc.order_case(long=True)
    assert 2.0 ** 100 + 2.0 ** 47 == 2.0 ** 100 and 2.0 ** 100 + 2.0 ** 48 != 2.0 ** 100
    assert np.all(mc.draw_indices(v, np.float32([1.0, np.inf, np.nan])) == mc.ORDER_LONG_PICK)
    P = np.cumsum(np.abs(v).astype(np.float64))
    assert np.searchsorted(P, np.nextafter(P[-1], 0.0), side="right") == 0 and mc.tree_cdf(v)[1] != P[-1]


def test_edge_draws_select_what_the_header_says():
    """u = 0 and -0 select the first element of nonzero weight; u >= 1, inf and NaN the last one that moved the sum; the inputs have
    the zero items they claim; 1e-45 discriminates on the tensor built for it."""
    for name, v in mc.edge_u_tensors():
        C, T = mc.tree_cdf(v)
        idx = mc.draw_indices(v, mc.EDGE_U)
        first = int(np.flatnonzero(v)[0])
        last_moved = int(np.flatnonzero(np.diff(np.concatenate([[0.0], C])) > 0)[-1])
        assert idx[0] == idx[1] == first, name
        assert np.all(idx[4:] == last_moved), name
        assert idx[3] <= last_moved and np.all(v[idx] != 0), name
    a, b, c = (v for _, v in mc.edge_u_tensors())
    assert not a[:mc.CHUNK].any() and not a[3 * mc.CHUNK:].any() and a.size % mc.CHUNK
    assert b.size == 8200 and b[8100] != 0 and not b[8101:].any()
    ic = mc.draw_indices(c, mc.EDGE_U)
    assert ic[0] == 3 and ic[2] == 4


def test_islands_leave_the_runs_they_claim():
    for n in (1048576, 1048577, 1310000, 2097153):
        items = -(-n // mc.CHUNK)
        m = -(-items // mc.RUNS)
        v = mc.islands(n, 7)
        nz = np.flatnonzero(np.add.reduceat(np.abs(v.astype(np.float64)), np.arange(0, n, mc.CHUNK)))
        isl = mc.island_items(items)
        assert set(nz) == set(i for lo, hi in isl for i in range(lo, hi))
        assert nz[0] >= (300 if items >= 320 else 160) and nz[-1] < items - 1
        for (_, e0), (s1, _) in zip(isl, isl[1:]):
            assert s1 // m - -(-e0 // m) >= 2      # whole zero runs in between


def test_dense_and_decode_mean_arithmetic():
    words = np.array([0, 0, 3 | (1 << 31), 5, 5 | (1 << 31)], np.uint32)
    d = mc.dense(words, np.float32(0.1), 7)
    want = np.float32([np.float32(0.1) * np.float32(2), 0, 0, np.float32(0.1) * np.float32(-1), 0, 0, 0])
    assert d.dtype == np.float32 and np.array_equal(d.view(np.uint32), want.view(np.uint32))
    z = mc.dense(words[2:3], np.float32(0.0), 7)
    assert z.view(np.uint32)[3] == 1 << 31      # 0 * -1 is -0: D itself
    assert mc.decode_mean([(np.float32(0.0), words[2:3])], 7).view(np.uint32)[3] == 0      # (+0 + -0) / 1
    two = mc.decode_mean([(np.float32(0.1), words), (np.float32(0.3), words[:2])], 7)
    assert two[0] == (np.float32(0) + np.float32(0.1) * np.float32(2) + np.float32(0.3) * np.float32(2)) / np.float32(2)
    sec, D = mc.compress(np.float32([1, -2, 0, 1]), np.float32([0.0, 0.3, 0.99]), 3)
    assert sec.size == 32 and np.array_equal(sec[16:28].view(np.uint32), np.uint32([0, 1 | (1 << 31), 3]))
    assert sec[:4].view(np.float32)[0] == np.float32(4) / np.float32(3) and not sec[4:16].any() and not sec[28:].any()
