"""What the inputs of tests/test_gpu_hsq_decode_contract.py claim, checked without a GPU (tests/hsq_decode_contract.py): a kernel
with the wrong order of additions, a multiplication by 1 / R where the contract divides, or an accidental fused multiply-add must
not be able to pass because the data are too kind.  Every count asserted here is over the whole `out` of a case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hsq_decode_contract as dc  # noqa: E402
import hsq_dequant_contract as hc  # noqa: E402
import rq_contract as rc  # noqa: E402

F = np.float32
EXACT = sorted(set(dc.EXACT_CASES), key=dc.case_id)
ALL = sorted(set(dc.ALL_CASES), key=dc.case_id)


def _differs(w, other):
    return int((w.want().view(np.uint32) != other.view(np.uint32)).sum())


def test_the_lists_hold_what_the_gpu_file_promises():
    d16 = [c for c in dc.D16_CASES if c.K == 256]
    for lv, nb in dc.D16_FORMS:
        assert sorted(c.R for c in d16 if (c.level, c.n_bit) == (lv, nb)) == list(range(1, 18)) + [24, 33]
    assert any(c.K == 64 for c in dc.D16_CASES)
    assert {(c.d, c.level) for c in dc.TILE_CASES} == {(8, 1), (8, 2), (32, 1), (32, 2), (16, 2)}
    assert {c.R for c in dc.TILE_CASES} == {1, 2, 3, 4, 8, 9, 17}
    assert all(c.table == "long" for c in dc.STEADY_CASES) and all(c.table == "small" for c in dc.D16_CASES + dc.TILE_CASES + dc.ANY_CASES)
    assert sum((M + 63) // 64 for M in dc.LONG_MS) == 101 and dc.LONG_MS[:4] == dc.SMALL_MS
    assert [M % 64 for M in dc.SMALL_MS] == [3, 1, 2, 0]
    assert 20 * 1024 * 4 > 64 * 1024 >= 16 * 512 * 4      # which any-shape codebook is read from memory


@pytest.mark.parametrize("c", [c for c in dc.D16_CASES if c.level == 1], ids=dc.case_id)
def test_d16_byte_levels_equal_the_dequant_contract(c):
    w = dc.wire_of(c)
    for rows in w.payloads:
        a = dc.decode_mean(rows, w.cb, c.n_bit, w.plain)
        b = hc.decode_mean(rows, w.cb, c.n_bit, w.plain)
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("c", [c for c in ALL if c.R > 2], ids=dc.case_id)
def test_the_order_of_additions_shows(c):
    """(R = 2 has one order only: an IEEE addition commutes.)"""
    w = dc.wire_of(c)
    assert _differs(w, w.expected(lambda p: hc.mean(dc.decode_acc(p, w.cb, c.n_bit, reverse=True), c.R, False))) > 0


@pytest.mark.parametrize("c", [c for c in ALL if c.R & (c.R - 1)], ids=dc.case_id)
def test_the_division_shows(c):
    w = dc.wire_of(c)
    with np.errstate(all="ignore"):
        assert _differs(w, w.expected(lambda p: (F(0.0) + dc.decode_acc(p, w.cb, c.n_bit)) * (F(1.0) / F(c.R)))) > 0


@pytest.mark.parametrize("c", [c for c in EXACT if c.R > 1], ids=dc.case_id)
def test_a_fused_multiply_add_shows(c):
    w = dc.wire_of(c)
    assert _differs(w, w.expected(lambda p: hc.mean(dc.decode_acc(p, w.cb, c.n_bit, fused=True), c.R, False))) > 0


@pytest.mark.parametrize("c", dc.FMA_LOOSE, ids=dc.case_id)
def test_the_fused_sum_is_within_the_projects_bound(c):
    """Relative L2 <= 1e-6 of the exact mean over the launch's spans (the bound of
    test_fma_aggregate_is_within_1e6_of_the_oracle_mean_and_opt_in); and it is not the exact mean."""
    w = dc.wire_of(c)
    assert w.regimes == ("ordinary",)
    fused = w.expected(lambda p: hc.mean(dc.decode_acc(p, w.cb, c.n_bit, fused=True), c.R, False))
    assert _differs(w, fused) > 0
    m = w.spans()
    assert dc.rel_l2(fused[m], w.want()[m]) <= 1e-6


@pytest.mark.parametrize("c", [c for c in ALL if c.level != 0], ids=dc.case_id)
def test_every_level_occurs(c):
    w = dc.wire_of(c)
    top = dc.top_level(c.level, c.n_bit)
    assert top == (256 if c.level in (2, 4) else (1 << c.n_bit) - 1)      # 16-bit (and wider) levels: level 2**n_bit, what rounding reaches
    assert w.levels_seen() == set(range(top + 1))


@pytest.mark.parametrize("c", [c for c in EXACT if c.level != 0 and c.regimes == "mixed"], ids=dc.case_id)
def test_minus_zero(c):
    """Subvector 0 of a "tiny" tensor (lb = 0) is at level 0 in every payload, with a codeword that has a negative element: every
    payload decodes that element to -0.  The plain decode keeps it; the mean of R payloads turns it into +0."""
    w = dc.wire_of(c)
    tiny = [s for s in range(len(w.Ms)) if w.regime_of(s) == "tiny"]
    assert tiny and {w.regime_of(s) for s in range(len(w.Ms))} == set(hc.REGIMES)
    for s in tiny:
        neg = w.cb[int(w.payloads[s][0][0][0])] < 0
        assert neg.any()
        for codes, raw, (lb, ub) in w.payloads[s]:
            assert lb == 0 and raw[0] == 0
            dec = rc.stage_decode(codes[:1], rc.level_norm(raw[:1], dc.level_bytes_of(raw), c.n_bit, lb, ub), w.cb)[0]
            assert (dec.view(np.uint32)[neg] == 0x80000000).all()
        o = int(w.table[s, 6])
        got = w.want()[o:o + c.d].view(np.uint32)
        assert (got[neg] == (0x80000000 if w.plain else 0)).all()


@pytest.mark.parametrize("c", [c for c in ALL if c.level == 0], ids=dc.case_id)
def test_f32_norms_travel_as_they_are(c):
    w = dc.wire_of(c)
    for rows in w.payloads:
        for codes, raw, (lb, ub) in rows:
            assert raw.dtype == np.float32 and np.isnan(lb) and np.isnan(ub) and raw[0] == 0
    assert not np.isnan(w.want()).any()


@pytest.mark.parametrize("c", ALL, ids=dc.case_id)
def test_layout(c):
    w = dc.wire_of(c)
    nseg = len(w.Ms)
    assert w.table.shape == (nseg, 8) and not w.table[:, 0].any() and not w.table[:, 7].any()
    assert w.tile_seg.size == w.ntiles and (np.diff(w.tile_seg) >= 0).all()
    assert all((w.tile_seg == s).sum() == (M + 63) // 64 and w.tile_seg.tolist().index(s) == w.table[s, 2] for s, M in enumerate(w.Ms))
    # sections: 16-byte aligned, padded to 16 bytes, at least 16 bytes that belong to nobody behind each, none past the payload
    secs = sorted((off, nbytes) for _, off, nbytes in w.sections)
    assert len(secs) == 3 * nseg and all(off % 16 == 0 for off, _ in secs)
    ends = [off for off, _ in secs[1:]] + [w.P]
    assert all(end - (off + nbytes + 15) // 16 * 16 >= 16 for (off, nbytes), end in zip(secs, ends))
    assert w.P % 16 == 0 and w.buf.size == w.lead + c.R * w.P + 16
    assert (w.table[:, 5] % 4 == 0).all()                      # (lb, ub): float-aligned
    # every byte outside the sections is a canary; payloads of one tensor differ
    mask = np.zeros(w.buf.size, bool)
    for r in range(c.R):
        for off, nbytes in secs:
            mask[w.lead + r * w.P + off: w.lead + r * w.P + off + nbytes] = True
    assert (w.buf[~mask] == dc.CANARY).all()
    if c.R > 1:
        assert all(not np.array_equal(rows[0][0], rows[1][0]) or len(rows[0][0]) == 1 for rows in w.payloads)
        if c.level != 0:
            assert all(rows[0][2] != rows[1][2] for rows in w.payloads)
    # out: spans apart by at least GAP floats, float4 stores on multiples of 4 floats (the one-float form: off them too)
    spans = [(int(w.table[s, 6]), int(w.table[s, 6]) + M * c.d) for s, M in enumerate(w.Ms)]
    assert spans[0][0] >= dc.GAP and w.out_floats - spans[-1][1] >= dc.GAP
    assert all(b[0] - a[1] >= dc.GAP for a, b in zip(spans, spans[1:]))
    if dc.stores_float4(c):
        assert all(o % 4 == 0 for o, _ in spans)
    else:
        assert any(o % 4 for o, _ in spans)
    # a packed section is followed by a readable byte of its own payload; a tail's word-wide code load stays inside the padding
    assert all(off + (nbytes + 3) // 4 * 4 + 1 <= w.P for off, nbytes in secs)


@pytest.mark.parametrize("level,off_bit,given_bit", dc.LEVELS_FORMS)
def test_levels_third_trip_inputs(level, off_bit, given_bit):
    """M: with the grid capped at four workgroups every thread makes three trips of four projections or more, and a scalar tail
    is left; rounding off lands on every level, the given draws reach the top level 2**n_bit."""
    M, threads = dc.LEVELS_M, 4 * 256
    assert (M // 4) >= 3 * threads and M % 4 == 3 and M == 3 * 4 * 256 * 4 + 7
    for given, n_bit in ((False, off_bit), (True, given_bit)):
        u, r, l, section, (lb, ub) = dc.levels_case(level, n_bit, given)
        assert u.size == M and lb == u.min() and ub == u.max() and (r is None) == (not given)
        assert set(l.tolist()) >= set(range(1 << n_bit)) and l.max() == (1 << n_bit) - (0 if given else 1)
        assert section.size == (3 * ((M + 3) // 4) if level == dc.P6 else M * {1: 1, 2: 2, 4: 4}[level])
        assert l.max() <= {1: 255, 2: 65535, 4: 2 ** 31 - 1, dc.P6: 63}[level]
