"""What the inputs of tests/test_gpu_hsq_encode_contract.py claim, checked without a GPU (tests/hsq_encode_contract.py): a kernel
that keeps the last maximum, adds in another order, fuses the error-feedback add, takes one (lb, ub) for all tensors, divides by
the wrong count or at the wrong place, or indexes u_flat without the tile padding must not be able to pass because the data are
too kind.  Every mutation below changes the expectation of the GPU cases it is run on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hsq_decode_contract as dc  # noqa: E402
import hsq_dequant_contract as hc  # noqa: E402
import hsq_encode_contract as ec  # noqa: E402
import rq_contract as rc  # noqa: E402

F = np.float32
SMALL = [c for c in ec.PF_CASES + ec.PAGED_CASES + ec.EXACT_CASES if c.table == "small"]
SHAPES = sorted({(c.d, c.K) for c in ec.ENCODE_CASES + ec.NONFINITE_CASES + ec.CHAIN_CASES})
QUANTISED = [c for c in ec.LEVEL_CASES if c.level != 0 and c.table == "small"]


def _kind(e, name):
    return [k == ec.KIND[name] for k in e.kinds]


def test_the_lists_hold_what_the_gpu_file_promises():
    ids = lambda cases: {(c.d, c.K, c.ef is not None) for c in cases}
    assert {(d, 256, ef) for d in (8, 12, 16, 24, 32) for ef in (False, True)} <= ids(ec.PF_CASES)
    assert {(16, K, True) for K in (4, 32, 64, 132)} | {(8, 64, False), (32, 64, False)} <= ids(ec.PF_CASES)
    assert {(c.d, c.K) for c in ec.PF_CASES if c.table == "records"} == {(12, 32), (16, 32), (32, 32)}
    assert ids(ec.PAGED_CASES) == {(d, K, ef) for d, K in ((8, 512), (16, 512), (16, 768), (32, 512)) for ef in (False, True)}
    assert all(c.code_bytes == 4 for c in ec.PAGED_CASES)
    want = {(16, 256), (16, 250), (5, 5), (3, 32), (33, 300), (100, 512), (104, 64), (16, 512)}
    assert ids(ec.EXACT_CASES) == {(d, K, ef) for d, K in want for ef in (False, True)}
    assert {c.ef for c in ec.ENCODE_CASES} == {None, 0, 1} and ec.EF_SCALES == (0.75, 0.1)
    assert {c.path for c in ec.NONFINITE_CASES} == {ec.PREFILTER, ec.PAGED, ec.EXACT} == {c.path for c in ec.CHAIN_CASES}
    assert all(c.table == "long" for c in ec.CHAIN_CASES) and {c.table for c in ec.STEADY_CASES} == {"long", "many"}
    # the tables
    assert len(ec.MANY_MS) == 71 and sorted(set(ec.MANY_MS[:70])) == list(range(1, 65)) and (ec.MANY_MS[70] + 63) // 64 == 5
    assert len(ec.RECORDS_MS) == 390 > 384 and set(ec.RECORDS_MS) == {1}
    assert ec.TABLES["small"] is dc.SMALL_MS and ec.TABLES["long"] is dc.LONG_MS
    # the level routes, every one with and without the residual where it has both
    routes = {(c.route, c.write_error) for c in ec.LEVEL_CASES}
    assert routes == {("d16", 0), ("d16", 1), ("ef_d", 1), ("ef16", 1), ("any", 0), ("any", 1)}
    assert {c.route for c in ec.DRAW_CASES} == {"d16", "ef_d", "ef16", "any"} and {c.mode for c in ec.DRAW_CASES} == {ec.DEVICE, ec.KEYED}
    assert {c.ndense for c in ec.LEVEL_CASES} == {0, 3}
    assert {(c.d, c.level) for c in ec.LEVEL_CASES if c.route == "any" and c.level != 2} >= {(d, lv) for d in (12, 5, 16) for lv in (1, 4, 0)}
    assert {(c.d, c.n_bit, c.mode) for c in ec.LEVEL_CASES if c.level == 2 and c.K == 256} == {(d, nb, m) for d in (8, 16, 32)
                                                                                                for nb, m in ((8, ec.GIVEN), (15, ec.OFF), (1, ec.GIVEN))}
    assert all(ec.fused_served(f.l) for f in ec.FUSED_SERVED + ec.FUSED_STEADY) and not any(ec.fused_served(f.l) for f in ec.FUSED_UNSERVED)
    assert len(set(ec.FUSED_SERVED)) == 48
    for d in (8, 16, 32):      # every served shape: both draws, both residual settings, both means and both tails
        mine = [f for f in ec.FUSED_SERVED if f.l.d == d]
        assert {f.l.mode for f in mine} == {ec.OFF, ec.GIVEN} and {f.l.write_error for f in mine} == {0, 1}
        assert {(f.plain, f.tail) for f in mine} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {f.l.level for f in mine} == {1, 2}


@pytest.mark.parametrize("c", ec.LEVEL_CASES + ec.LEVEL_STEADY + ec.DRAW_CASES + [f.l for f in ec.FUSED_SERVED + ec.FUSED_UNSERVED + ec.FUSED_STEADY],
                         ids=ec.lcase_id)
def test_no_level_case_overflows_its_width(c):
    top = (1 << c.n_bit) - (1 if c.mode == ec.OFF else 0)
    assert c.level in (0, 4) or top <= {1: 255, 2: 65535, ec.P6: 63}[c.level]
    assert c.level != ec.P6 or (c.d == 16 and c.K <= 256 and c.code_bytes == 1 and c.n_bit <= 6)


def test_every_case_maps_to_the_path_its_list_claims():
    """batch_path of csrc/gq_api.hip restated; the GPU file confirms it against HSQBatch.path."""
    for cases, path in ((ec.PF_CASES, ec.PREFILTER), (ec.PAGED_CASES, ec.PAGED), (ec.EXACT_CASES, ec.EXACT)):
        for c in cases:
            assert c.path == path == ec.batch_path(c.d, c.K, c.code_bytes, len(ec.TABLES[c.table])), ec.ecase_id(c)
    assert ec.batch_path(16, 512, 4, 384) == ec.PAGED and ec.batch_path(16, 512, 4, 385) == ec.EXACT      # the paged path declines more records
    assert ec.batch_path(16, 256, 4, 4) == ec.EXACT and ec.batch_path(16, 250, 1, 4) == ec.EXACT and ec.batch_path(16, 132, 1, 4) == ec.PREFILTER


@pytest.mark.parametrize("d,K", SHAPES)
def test_codebooks_hold_the_ties_and_the_near_ties(d, K):
    cb = ec.codebook(d, K)
    j1, j2, j3 = ec.ties(K)
    assert j1 < j2 < j3 < K and np.array_equal(cb[j1], cb[j2]) and np.array_equal(cb[j3], -cb[j1])
    if K >= 512:
        a, b = ec.page_pair(K)
        assert j1 // 256 == 0 and j2 // 256 == 1 and j3 // 256 == K // 256 - 1 and a // 256 == b // 256 >= 1 and np.array_equal(cb[a], cb[b])
    nt = ec.near_ties(d, K)
    gap = ec.top2_gap(cb, nt)
    # below what the first pass's bound E' of DESIGN.md 4.1 (~2^-11 relative) can settle
    assert len(nt) >= 1 and (gap < 2.0 ** -12).all(), gap


@pytest.mark.parametrize("table", sorted(ec.TABLES))
def test_every_kind_lies_in_every_table(table):
    Ms = ec.TABLES[table]
    kinds = [[ec.kind_of(s, M, r) for r in range(M)] for s, M in enumerate(Ms)]
    seen = {k for row in kinds for k in row}
    assert seen >= set(ec.KINDS) - ({"big"} if max(Ms) < 128 else set()), set(ec.KINDS) - seen
    for s, M in enumerate(Ms):
        if M >= 1024:      # the long tensors: every kind in the first and in the last whole tile (a wave's first and last)
            last = (M // 64 - 1) * 64
            assert set(kinds[s][:64]) | {"huge", "big"} >= set(ec.KINDS) and set(kinds[s][last:last + 64]) | {"huge", "big"} >= set(ec.KINDS)
            assert {"huge", "big"} <= set(kinds[s])
        for r in range(M):      # the lanes whose norms steer the next tile's scale stay ordinary, but for the one big row
            if M >= 64 and r % 64 in (5, 58):
                assert kinds[s][r] in ("gauss", "big")


@pytest.mark.parametrize("c", SMALL, ids=ec.ecase_id)
def test_encode_inputs_are_not_too_kind(c):
    e = ec.encode_of(c)
    want = e.want()
    cat = lambda name: np.concatenate(_kind(e, name))
    codes, u = np.concatenate(want["codes"]), np.concatenate(want["u"])
    # the kinds do what they are for
    j1 = ec.ties(c.K)[0]
    assert (codes[cat("tie")] == j1).all() and (codes[cat("zero+") | cat("zero-")] == 0).all()
    assert (rc.bits(u[cat("zero+") | cat("zero-")]) == 0).all()
    assert (codes[cat("tie2")] == (ec.page_pair(c.K)[0] if ec.page_pair(c.K) else j1)).all()
    # last maximum instead of the first: a code changes on the tie rows
    last, _ = [np.concatenate(x) for x in zip(*e.encode(first=False))]
    assert (last[cat("tie")] != codes[cat("tie")]).all() and (last[cat("tie2")] != codes[cat("tie2")]).all()
    # another order of the chain: bits of u change on the Gaussian rows
    g = cat("gauss")
    for order in ("descending", "pairwise"):
        if c.d < 3 or (order == "pairwise" and c.d * c.K > 16 * 768):
            continue
        _, uo = [np.concatenate(x) for x in zip(*e.encode(order=order))]
        assert (rc.bits(uo[g]) != rc.bits(u[g])).any(), order
    # per-tensor (lb, ub): no two tensors share one, so a global pair is wrong for every tensor but (at most) the one that holds both ends
    mm = want["minmax"]
    assert len({tuple(r) for r in mm.tolist()}) == len(e.Ms) > 1
    if e.ef_scale is None:
        assert all(x is None for x in e.errs) and np.array_equal(rc.bits(want["gbuf"]), rc.bits(e.gbuf))
        return
    # error feedback: rows with and without a buffer, subnormal products, and a fused add shows
    assert any(x is None for x in e.errs) and any(x is not None for x in e.errs)
    fused = sub = 0
    for gr, er, v in zip(e.grads, e.errs, e.v):
        if er is None:
            assert v is gr
            continue
        fused += int((rc.bits(ec.ef_add_fused(gr, er, e.ef_scale)) != rc.bits(v)).sum())
        with np.errstate(all="ignore"):
            p = F(e.ef_scale) * er
        sub += int(((p != 0) & (np.abs(p) < F(2.0 ** -126))).sum())
    assert fused > 0 and sub > 0


@pytest.mark.parametrize("c", QUANTISED, ids=ec.lcase_id)
def test_level_inputs_are_not_too_kind(c):
    lv = ec.levels_of(c)
    want = np.concatenate(lv.levels())
    differs = lambda other: int((np.concatenate(other) != want).sum())
    top = (1 << c.n_bit) - (1 if c.mode == ec.OFF else 0)
    assert want.min() == 0 and want.max() == top          # lands on both ends; never past the width (see the case lists)
    los, his = [b[0] for b in lv.bounds], [b[1] for b in lv.bounds]
    assert differs(lv.levels(bounds=[(min(los), max(his))] * len(lv.Ms))) > 0                 # one (lb, ub) for all tensors
    if c.n_bit > 1:
        assert differs(lv.levels(how="minus1")) > 0                                           # a division by 2^n_bit - 1 levels
    # a division by ub - lb AFTER the scaling by 2^n_bit is no mutation at all: a scaling by a power of two is exact (nothing here
    # overflows), so it commutes with the correctly rounded division -- no input can tell the two apart, and none is asked to
    assert differs(lv.levels(how="late")) == 0
    # u_flat indexed without the tile padding
    flat = lv.lay.unpadded_of(lv.u)
    assert differs(lv.levels(u=[flat[lv.lay.slots(s)] for s in range(len(lv.Ms))])) > 0
    # the regimes: all four, and the flat one quantises to zeros
    assert {dc.REGIME_ORDER[s % 4] for s in range(len(lv.Ms))} == set(hc.REGIMES)
    assert all((l == 0).all() for l, (lb, ub) in zip(lv.levels(), lv.bounds) if lb == ub)
    # rows with and without an error buffer
    assert not c.write_error or (any(lv.has_err) and not all(lv.has_err))


def test_the_many_table_overflows_the_minmax_window():
    """With the grid capped at one workgroup its run starts at tile 0 and meets all 71 tensors: those from the 65th on fold
    into global memory, not into the workgroup's 64-entry LDS table."""
    lay = ec.Layout(ec.MANY_MS, 16, 1, 1)
    assert lay.nseg == 71 > 64 and lay.ntiles == 75 and int(lay.tile_seg[0]) == 0 and int(lay.tile_seg[-1]) == 70
