"""tests/sketch_contract.py (the numpy restatement of include/gq_sketch.h) against plain float64 and brute force, without a GPU: the hash
is a bijection inside an item, the median network is the median, the sketch is linear, a sparse input whose nonzeros are alone in a
majority of rows comes back exactly, the wire size function, the host's window lists."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(os.path.dirname(HERE), "gradient-quantization_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import sketch_contract as sc  # noqa: E402

f32, f64 = np.float32, np.float64
ROWS = [1, 3, 5]


def brute(w, seed, rows, nwin):
    """The sketch element by element in float64, and the sum of |terms| per cell."""
    w = np.asarray(w, f64).reshape(-1)
    T, S = np.zeros((rows, nwin, sc.CHUNK), f64), np.zeros((rows, nwin, sc.CHUNK), f64)
    items = -(-w.size // sc.CHUNK)
    for j in range(rows):
        key, A = sc.row(seed, j)
        win, off = sc.item_hash(key, items, nwin)
        for a in range(items):
            x = w[a * sc.CHUNK:(a + 1) * sc.CHUNK]
            c = sc.cells(A, off[a])[:x.size]
            s = 1.0 - 2.0 * sc.signs(key, a)[:x.size]
            np.add.at(T[j, win[a]], c, s * x)
            np.add.at(S[j, win[a]], c, np.abs(x))
    return T, S


@pytest.mark.parametrize("rows", ROWS)
def test_hash_is_a_bijection_inside_an_item_and_lists_are_the_hosts(rows):
    from gq_amd import native
    items, nwin = 70, 3
    lst, starts = native.sketch_build_lists(11, rows, items, nwin)
    want = sc.lists(11, rows, items, nwin)
    for j in range(rows):
        key, A = sc.row(11, j)
        win, off = sc.item_hash(key, items, nwin)
        assert A % 2 == 1 and 0 < A < 4096 and win.min() >= 0 and win.max() < nwin
        for a in (0, 1, items - 1):
            assert np.array_equal(np.sort(sc.cells(A, off[a])), np.arange(sc.CHUNK))
        for v in range(nwin):
            got = lst[starts[j * nwin + v]:starts[j * nwin + v + 1]]
            assert np.array_equal(got & 0x7ffff, want[j][v]) and np.array_equal(got >> 19, off[want[j][v]])
    assert starts[-1] == rows * items


def test_median_network_is_the_median():
    for r in (3, 5):
        perms = np.array(list(itertools.permutations(range(r))), f32).T
        assert np.array_equal(sc.median(perms), np.full(perms.shape[1], r // 2, f32))
        x = np.random.RandomState(r).randint(-2, 3, size=(r, 4000)).astype(f32)      # (ties)
        assert np.array_equal(sc.median(x), np.median(x, axis=0).astype(f32))


@pytest.mark.parametrize("rows", ROWS)
def test_sketch_is_linear_and_matches_brute_force(rows):
    rs = np.random.RandomState(rows)
    n, nwin, seed = 4096 * 20 + 17, 2, 5
    a, b = rs.standard_normal(n), rs.standard_normal(n)
    Ta, Sa = brute(a, seed, rows, nwin)
    Tb, Sb = brute(b, seed, rows, nwin)
    Tab, _ = brute(a + b, seed, rows, nwin)
    assert np.all(np.abs(Tab - (Ta + Tb)) <= 64 * np.finfo(f64).eps * (Sa + Sb))      # (up to 20 terms per cell, each sum rounded)
    got = sc.sketch(a.astype(f32), seed, rows, nwin)
    T32, S32 = brute(a.astype(f32), seed, rows, nwin)
    assert np.all(np.abs(got - T32) <= 22 * np.finfo(f32).eps * S32)      # (at most 20 + 2 roundings of partial sums below S32)


@pytest.mark.parametrize("rows,nnz,seed", [(3, 6, 1), (5, 12, 1)])
def test_sparse_input_alone_in_a_majority_of_rows_is_recovered_exactly(rows, nnz, seed):
    n = 4096 * 12
    nwin = sc.layout(n, rows, 2)[1]
    rs = np.random.RandomState(7)
    w = np.zeros(n, f32)
    pos = rs.permutation(n)[:nnz]
    w[pos] = (rs.standard_normal(nnz) + 3).astype(f32)
    # the precondition: per element, the rows in which its cell holds a nonzero other than itself are a minority
    hit = np.zeros(n, np.int64)
    for j in range(rows):
        T, S = brute(w != 0, seed, j + 1, nwin)      # (row j alone: the last row of a (j + 1)-row sketch)
        occ = S[j]
        key, A = sc.row(seed, j)
        win, off = sc.item_hash(key, n // 4096, nwin)
        for a in range(n // 4096):
            others = occ[win[a], sc.cells(A, off[a])] - (w[a * 4096:(a + 1) * 4096] != 0)
            hit[a * 4096:(a + 1) * 4096] += others > 0
    assert hit.max() <= rows // 2, "the chosen seed does not isolate the nonzeros"
    out, _ = sc.decode_mean([sc.sketch(w, seed, rows, nwin)], n, nnz, seed)
    assert np.array_equal(out.view(np.uint32), w.view(np.uint32))


def test_wire_size():
    from gq_amd.codecs import sketch_section_bytes
    for n, rows, C in [(1000, 3, 32), (4096 * 6, 3, 32), (4096 * 6 - 4096, 3, 32), (25_000_000, 3, 32), (25_000_000, 5, 8), (4096 * 40, 1, 2)]:
        items = -(-n // 4096)
        nwin = max(1, -(-items // (C * rows)))
        want = 16 + 16384 * rows * nwin if 2 * rows * nwin <= items else 4 * n
        assert sketch_section_bytes(n, rows, C) == sc.section_bytes(n, rows, C) == want
        if want != 4 * n and n < 10 ** 6:
            assert sc.section(np.zeros(n, f32), 0, rows, C).size == want
