"""tests/pvq_contract.py checked without a GPU: its restatement of the sampler against the CPU oracle's own codes, projections
and running sums on every table; every on-threshold draw that was requested is there and is what it is said to be; every
mutation a kernel could carry changes a code on every table of the one-sweep kernel; both sides of that kernel's window are
occupied; the special rows have the l1 they are named for -- so that the inputs of tests/test_gpu_zz_pvq_contract.py cannot be
toothless, or its reference wrong, silently."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import pvq_contract as pc  # noqa: E402
import rq_contract as rc  # noqa: E402

F = np.float32
FLAT = [(d, K, pc.M_TABLE) for d, K in pc.ONE_SWEEP + pc.TWO_SWEEP] + [(d, K, pc.M_CAPPED) for d, K in pc.CAPPED]
FLAT_IDS = ["d%d-K%d-M%d" % c for c in FLAT]


def _tables():
    """Every table of the GPU file: the flat ones, the multi-tensor cases' and the residual case's."""
    for c in FLAT:
        yield "flat d%d K%d M%d" % c, pc.table(*c)
    for c in pc.MULTI_CASES:
        yield "multi " + pc.multi_id(c), pc.multi_case(*c).tab
    yield "residual", pc.residual_case()[2]


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(oracle):
    yield


def test_walk_equals_the_oracle():
    """Two independent statements of the rule: codes, u, the running sums and l1, NaN equal to NaN and bit for bit otherwise."""
    n = 0
    for name, tab in _tables():
        codes, u, cum, l1 = pc.walk(tab.p, tab.r)
        assert np.array_equal(codes, tab.codes), name
        assert rc.same(u, tab.u) and rc.same(cum, tab.cum) and rc.same(l1, tab.l1), name
        assert int(codes.max()) < tab.K and u.dtype == np.float32
        n += 1
    assert n == len(FLAT) + len(pc.MULTI_CASES) + 1


def test_every_requested_draw_was_built():
    for name, tab in _tables():
        assert len(tab.entries) == tab.requested >= 7 * len(pc.LADDER), (name, len(tab.entries), tab.requested)
        assert len(set(e[0] for e in tab.entries)) == len(tab.entries), name      # a row has one draw
        assert len(tab.extra) == pc.MIDPOINTS, (name, len(tab.extra))
        ks = set(k for _, k, _ in tab.entries)
        assert ks >= set(k for k in (0, 7, 8, 15, 16, 17, 31, 32, tab.K - 2) if k <= tab.K - 2), (name, sorted(ks))
        for k in ks:
            assert set(j for _, kk, j in tab.entries if kk == k) == set(pc.LADDER), (name, k)


def test_no_draw_below_one_reaches_the_last_running_sum():
    """Why K - 1 is no target: f32(cum_{K-1} + 1e-5) >= 1 on every finite row of every table."""
    for name, tab in _tables():
        last = tab.cum[:, -1]
        fin = np.isfinite(last) & (tab.l1 > 0) & np.isfinite(tab.l1)
        assert fin.sum() >= tab.M - len(pc.SPECIAL)
        assert (last[fin].astype(np.float64) + 1e-5 >= 1.0).all(), name


def test_on_threshold_draws_are_what_they_are_said_to_be():
    """thr exactly j ulps from cum_k, r in [0, 1), cum strictly increasing round k; j = 0 gives code k, and one ulp more of r a
    code above k."""
    for name, tab in _tables():
        both = tab.entries + tab.extra
        rows = np.array([e[0] for e in both])
        ks = np.array([e[1] for e in both])
        js = np.array([e[2] for e in both])
        assert len(set(rows)) == len(rows)
        r = tab.r[rows]
        assert ((r >= 0) & (r < 1)).all() and r.dtype == np.float32, name
        thr = pc.threshold(r)
        ck = tab.cum[rows, ks]
        assert (ck > 0).all() and np.isfinite(ck).all()
        assert np.array_equal(thr.view(np.uint32).astype(np.int64) - ck.view(np.uint32).astype(np.int64), js), name
        before = np.where(ks > 0, tab.cum[rows, np.maximum(ks - 1, 0)], F(0.0))
        assert ((before < ck) & (ck < tab.cum[rows, ks + 1])).all(), name
        on = js == 0
        assert np.array_equal(tab.codes[rows][on], ks[on]), name
        up = np.nextafter(r[on], F(2.0))
        codes_up = pc.walk(tab.p[rows][on], up)[0]
        assert (codes_up > ks[on]).all(), name
        # and the entries on the two sides of the threshold land on the two sides of k
        assert (tab.codes[rows][js < 0] <= ks[js < 0]).all() and (tab.codes[rows][js > 0] > ks[js > 0]).all(), name
        # on_threshold() as it is called from outside, without the precomputed running sums
        i, k, j = tab.entries[len(tab.entries) // 2]
        assert pc.on_threshold(tab.x[i], tab.cdag, k, j) == tab.r[i]


@pytest.mark.parametrize("how", pc.MUTATIONS)
def test_mutations_change_codes(how):
    """Every mutation changes at least one code on every table of the one-sweep kernel (flat, grid-capped, multi-tensor and
    residual: all of them are), and on the two-sweep tables whose K allows it."""
    for name, tab in _tables():
        if how in ("bracket", "half") and tab.K < 32:
            continue      # (4, 16): no run boundary at 15 inside the table
        changed = int((pc.mutant(tab.p, tab.r, how) != tab.codes).sum())
        print("%-28s %-18s changes %4d of %d codes" % (name, how, changed, tab.M))
        assert changed >= 1, (name, how)


def test_the_unmutated_statement_changes_nothing():
    """(the mutants' own scaffolding: with the contract's choices _in_run over the right run gives the oracle's codes)"""
    for name, tab in _tables():
        thr = pc.threshold(tab.r)
        nruns = (tab.K + 15) // 16
        ends = tab.cum[:, np.minimum(16 * np.arange(nruns) + 15, tab.K - 1)]
        with np.errstate(all="ignore"):
            run = np.minimum((ends < thr[:, None]).sum(axis=1), nruns - 1)
            mid = np.take_along_axis(tab.cum, np.minimum(16 * run + 7, tab.K - 1)[:, None], axis=1)[:, 0]
            fin = ~np.isnan(tab.cum).any(axis=1)
            got16 = pc._in_run(tab.cum, thr, 16 * run, 16)
            got8 = pc._in_run(tab.cum, thr, 16 * run + np.where(mid < thr, 8, 0), 8)
        assert np.array_equal(got16[fin], tab.codes[fin]) and np.array_equal(got8[fin], tab.codes[fin]), name


def test_both_sides_of_the_window_are_occupied():
    """Entries within eps of a running sum (a slow walk has to decide them) and outside it (the lane-local walk has to), per table."""
    for name, tab in _tables():
        inside = pc.inside_window(tab)
        js = np.array([e[2] for e in tab.entries + tab.extra])
        print("%-28s inside eps: %4d, outside: %4d" % (name, int(inside.sum()), int((~inside).sum())))
        assert inside.sum() >= 1 and (~inside).sum() >= 1, name
        assert inside[js == 0].all(), name      # T is half an ulp under cum_k
        # and with half the window entries move from inside to outside: what a kernel with eps halved would wrongly settle
        assert (inside & ~pc.inside_window(tab, pc.EPS / 2)).sum() >= 1, name


def test_rounds_up_to_threshold():
    rs = np.random.RandomState(1)
    thr = np.concatenate([rs.random_sample(2000).astype(np.float32), F([0.0, 0.5, 1.0, 2.0 ** -24, 1e-5]), -rs.random_sample(50).astype(np.float32)])
    T = pc.rounds_up_to_threshold(thr)
    assert (T.astype(np.float32) >= thr).all() and (np.nextafter(T, -np.inf).astype(np.float32) < thr).all()


@pytest.mark.parametrize("c", FLAT, ids=FLAT_IDS)
def test_special_rows_are_what_they_are_named(c):
    tab = pc.table(*c)
    row = {name: int(np.flatnonzero(tab.kinds == name)[0]) for name in pc.SPECIAL}
    assert all((tab.kinds == name).sum() == 1 for name in pc.SPECIAL)
    assert len(set(i // 64 for i in row.values())) == len(pc.SPECIAL) and row["infpair"] == tab.M - 1
    assert not tab.x[row["zero"]].any() and tab.l1[row["zero"]] == 0 and tab.codes[row["zero"]] == tab.K - 1
    assert rc.bits(tab.u[row["zero"]]) == 0
    o = row["overflow"]
    assert np.isfinite(tab.x[o]).all() and np.isfinite(tab.p[o]).all() and tab.l1[o] == np.inf
    assert tab.codes[o] == tab.K - 1 and np.isinf(tab.u[o])
    s = row["subnormal"]
    assert 0 < tab.l1[s] < F(2.0 ** -126) and np.isfinite(tab.u[s]) and tab.cum[s, -1] > 0.99
    assert np.isnan(tab.x[row["nan"]]).sum() == 1 and np.isnan(tab.l1[row["nan"]]) and np.isnan(tab.u[row["nan"]])
    i = row["inf"]
    assert np.isinf(tab.x[i]).sum() == 1 and tab.l1[i] == np.inf and np.isinf(tab.p[i]).all() and np.isinf(tab.u[i])
    assert tab.codes[i] == tab.K - 1
    ip = row["infpair"]
    assert sorted(tab.x[ip][np.isinf(tab.x[ip])]) == [-np.inf, np.inf] and np.isnan(tab.l1[ip]) and np.isnan(tab.u[ip])
    # the finite kinds: l1 on both sides of the range the lane-local walk accepts, terms below 2^-29 of l1 and below 2^-102
    l1 = tab.l1
    assert (l1[tab.kinds == "tiny28"] < F(2.0 ** -80)).all() and (l1[tab.kinds == "big9"] > F(2.0 ** 20)).all()
    _, q = pc.terms(tab.p[tab.kinds == "below"])
    assert ((q > 0) & (q < F(2.0 ** -29))).any(axis=1).all()
    lo, hi = pc.lb_ub(tab.u)
    assert lo <= hi and (np.isinf(lo) or np.isinf(hi))      # (lb, ub) see the infinite projections and drop the NaN ones


def test_multi_tensor_cases():
    """Error feedback: v = g + RN(ef * e) is what the table holds, every third tensor has no error buffer and keeps its
    gradient, the special rows lie in the last tensor, whose fold sees them; nothing else in the wire than codes."""
    import hsq_encode_contract as ec
    for c in pc.MULTI_CASES:
        m = pc.multi_case(*c)
        lay = m.lay
        assert lay.Ms == pc.MULTI_MS and lay.ntiles == 1 + 1 + 1 + 2 + 6
        assert m.has_err == ([True, True, False, True, True] if m.ef is not None else [False] * 5)
        at = 0
        for s, M in enumerate(lay.Ms):
            g, e, v = m.gbuf[lay.span(s)], m.ebuf[lay.span(s)], m.want_gbuf[lay.span(s)]
            if m.has_err[s]:
                with np.errstate(all="ignore"):
                    t = F(m.ef) * e
                    assert rc.same(v, g + t)
                assert s == 4 or not np.array_equal(rc.bits(v), rc.bits(g))
            else:
                assert np.array_equal(rc.bits(v), rc.bits(g)) and (e == ec.E_FILL).all()
            assert rc.same(v, m.tab.x[at:at + M].reshape(-1))
            assert np.array_equal(m.r_flat[lay.slots(s)], m.tab.r[at:at + M])
            at += M
        special = np.isin(m.tab.kinds, pc.SPECIAL)
        assert special.sum() == len(pc.SPECIAL) and special[:sum(lay.Ms[:4])].sum() == 0
        u4 = m.want_u[4]
        assert np.isnan(u4).sum() >= 2 and np.isinf(u4).sum() >= 2      # ... the fold drops the first and keeps the second
        inf_words = (int(rc.order_map(F(-np.inf)).item()), int(rc.order_map(F(np.inf)).item()))
        assert m.want_minmax[4, 0] == inf_words[0] or m.want_minmax[4, 1] == inf_words[1]
        assert (m.want_minmax[:4, 0] <= m.want_minmax[:4, 1]).all() and (m.want_minmax[1:4, 0] < m.want_minmax[1:4, 1]).all()
        assert (m.want_wire != ec.CANARY).sum() > sum(lay.Ms) // 2


def test_residual_case():
    G, T, tab = pc.residual_case()
    cb1, cdag, _ = rc.codebooks(16, 256)
    assert G.Ms == list(pc.RESIDUAL_MS) and tab.cdag is cdag
    at = 0
    for t in T:
        x = rc.stage2_input(t["v"], t["codes1"], t["norm1"], cb1)
        assert np.array_equal(rc.bits(x), rc.bits(tab.x[at:at + t["M"]]))
        codes, u, mm = rc.encode2(t["v"], t["codes1"], t["norm1"], cb1, cdag, t["r"])
        assert np.array_equal(codes, t["codes"]) and rc.same(u, t["u"]) and mm == t["minmax"]
        at += t["M"]
    assert not np.array_equal(rc.bits(tab.x.reshape(-1)), rc.bits(np.concatenate([t["v"] for t in T])))
