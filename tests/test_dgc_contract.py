"""tests/dgc_contract.py (the numpy restatement of include/gq_dgc.h) against independent witnesses, and one assertion for every
claim the GPU tests' inputs make about themselves.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import dgc_contract as dc  # noqa: E402
import topk_contract as tc  # noqa: E402


def _scalar_record(g, u, v, m, k):
    """One record, element by element in Python: float32 scalars, the kept set from a sort of (key descending, index)."""
    n = len(g)
    m = np.float32(m)
    u1, v1 = [None] * n, [None] * n
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            t = np.float32(m * np.float32(u[i]))
            u1[i] = np.float32(t + np.float32(g[i]))
            v1[i] = np.float32(np.float32(v[i]) + u1[i])

    def key(x):
        b = int(np.float32(x).view(np.uint32)) & 0x7fffffff
        return 0x7fffffff if b > 0x7f800000 else b

    order = sorted(range(n), key=lambda i: (-key(v1[i]), i))
    kept = sorted(order[:k])
    keep = set(kept)
    u_new = [np.float32(0.0) if i in keep else u1[i] for i in range(n)]
    with np.errstate(invalid="ignore"):
        v_new = [np.float32(v1[i] - np.float32(v1[i] * np.float32(1.0 if i in keep else 0.0))) for i in range(n)]
    return kept, [v1[i] for i in kept], np.array(u_new, np.float32), np.array(v_new, np.float32)


@pytest.mark.parametrize("m", dc.MOMENTA)
def test_restatement_against_a_scalar_loop(m):
    rs = np.random.RandomState(11)
    n, k = 300, 20
    u, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    su, sv = u.copy(), v.copy()
    for step in range(4):
        g = rs.standard_normal(n).astype(np.float32)
        g[::7] = np.float32(1.5)                                  # ties
        g[5], g[50], g[51], g[52] = np.float32(-0.0), np.float32(np.inf), np.float32(np.nan), np.float32(1e-42)
        sec, u, v, idx, _ = dc.record(g, u, v, m, k)
        kept, vals, su, sv = _scalar_record(g, su, sv, m, k)
        assert np.array_equal(idx, kept)
        want = np.concatenate([np.array(kept, np.uint32), dc.canon(np.array(vals, np.float32))])
        assert np.array_equal(dc.canon_section(sec, k), want)
        assert np.array_equal(dc.canon(u), dc.canon(su)) and np.array_equal(dc.canon(v), dc.canon(sv))


@pytest.mark.parametrize("m", [0.5, 0.9])
def test_restatement_against_the_papers_algorithm_in_torch(m):
    """Deep Gradient Compression, algorithm 1 with momentum correction and momentum factor masking, as plain torch statements."""
    n, k = 4000, 50
    gs = [torch.from_numpy(tc.heavy_tailed(n, 70 + s)) for s in range(5)]
    u, v = torch.zeros(n), torch.zeros(n)
    st = dc.State([n], [k], m)
    for g in gs:
        u = m * u + g
        v = v + u
        idx = torch.topk(v.abs(), k)[1]
        mask = torch.zeros(n, dtype=torch.bool)
        mask[idx] = True
        sent = v[mask].clone()      # (ascending index order)
        v = v * (~mask)
        u = u * (~mask)
        sec = st.record([g.numpy()])[0]
        assert tc.select(st.v1[0], k)["ties"] == 1      # no ties: torch.topk's choice is the contract's
        widx, wval = tc.split_section(sec, k)
        assert np.array_equal(widx, torch.nonzero(mask).view(-1).numpy().astype(np.uint32))
        assert np.array_equal(wval, sent.numpy())
        assert np.array_equal(st.u[0], u.numpy()) and np.array_equal(st.v[0], v.numpy())      # (as values: -0 == +0)


def test_m_zero_is_error_feedback_at_scale_one():
    n, k = 5000, 77
    v = np.zeros(n, np.float32)
    e = np.zeros(n, np.float32)
    u = np.zeros(n, np.float32)
    for s in range(4):
        g = tc.ordinary(n, 80 + s)
        sec, u, v, idx, v1 = dc.record(g, u, v, 0.0, k)
        w, sec2, D, e = tc.error_feedback(g, e, 1.0, k)
        assert np.array_equal(sec, sec2) and np.array_equal(tc.bits(v), tc.bits(e)) and np.array_equal(tc.bits(v1), tc.bits(w))
        assert not u[idx].any() and np.array_equal(np.delete(u, idx), np.delete(g, idx))


# ---- what the GPU tests' inputs claim --------------------------------------------------------------------------------------
def _no_threshold_ties(sizes, ks, steps, m):
    st = dc.State(sizes, ks, m)
    for gs in steps:
        st.record(gs)
        for v1, k in zip(st.v1, ks):
            if 1 <= k:
                assert tc.select(v1, k)["ties"] == 1


@pytest.mark.parametrize("m", dc.MOMENTA)
def test_untied_inputs_have_no_ties_at_any_threshold(m):
    for case in (dc.seam_case, dc.k_case, dc.many_case):
        _no_threshold_ties(*case(), m)


def test_seam_and_k_cases_are_what_they_say():
    sizes, ks, steps = dc.seam_case()
    assert sizes == [1001, 4096, 4097, 8193, 12289] and ks == [62, 256, 256, 512, 768] and len(steps) == dc.STEPS
    assert [-(-n // dc.CHUNK) for n in sizes] == [1, 1, 2, 3, 4]
    sizes, ks, steps = dc.k_case()
    assert ks == [0, 1, 5000, 6144] and sizes[2] == ks[2]
    assert -(-ks[3] // dc.CHUNK) == 2      # the mask launch: two workgroups of the tensor have indices to read
    st = dc.State(sizes, ks, 0.9)
    for gs in steps:
        st.record(gs)
        assert not st.u[2].any() and not st.v[2].any() and not np.signbit(st.u[2]).any() and not np.signbit(st.v[2]).any()   # k = n: all +0
        assert st.kept[0].size == 0


def test_tie_case_straddles_the_item_seam():
    sizes, ks, steps = dc.tie_case()
    g, k = steps[0][0], ks[0]
    sel = tc.select(g, k)
    assert sel["T"] == tc.ONE and sel["last"] == dc.TIE_LAST and sel["need"] < sel["ties"]
    kept = tc.kept(g, k)
    ties = kept[tc.keys(g)[kept] == tc.ONE]
    assert (ties < dc.CHUNK).any() and (ties >= dc.CHUNK).any() and {4095, 4096, 4097, dc.TIE_LAST} <= set(ties.tolist())
    assert tc.keys(g)[dc.TIE_LAST + 1] == tc.ONE and dc.TIE_LAST + 1 not in set(kept.tolist())      # the next tie is NOT kept
    for m in dc.MOMENTA:      # the mask hits exactly the kept set, at every step
        st = dc.State(sizes, ks, m)
        for gs in steps:
            st.record(gs)
            assert st.kept[0].size == k and not st.u[0][st.kept[0]].any()
            rest = np.delete(st.u[0], st.kept[0])
            assert np.all(rest != 0)


def test_special_case_holds_every_special_value():
    sizes, ks, steps, u0, v0 = dc.special_case()
    for a in [s[0] for s in steps] + u0 + v0:
        b = tc.bits(a)
        mag = b & np.uint32(0x7fffffff)
        assert (b == 0).any() and (b == 0x80000000).any() and ((mag > 0) & (mag < 0x800000)).any()
        assert (b == 0x7f800000).any() or (b == 0xff800000).any()
        assert np.isnan(a).sum() == tc.NANS.size
    st = dc.State(sizes, ks, 0.9, u0, v0)
    for gs in steps:
        st.record(gs)
    assert np.isnan(st.v[0]).any() and np.isnan(st.u[0]).any()      # non-finite state is carried, not dropped


def test_many_and_fcn_cases():
    sizes, ks, steps = dc.many_case()
    assert len(sizes) == 70 and min(sizes) == 1001 and max(sizes) > dc.CHUNK and all(k == n // 64 for n, k in zip(sizes, ks))
    grads = dc.fcn_grads(3, 3)
    big = [j for j, s in enumerate(dc.FCN_SHAPES) if int(np.prod(s)) > 1000]
    assert big == [0, 2]
    for user in range(3):
        _no_threshold_ties([int(np.prod(dc.FCN_SHAPES[j])) for j in big], [int(np.prod(dc.FCN_SHAPES[j])) // 64 for j in big],
                           [[grads[t][user][j] for j in big] for t in range(3)], 0.9)
