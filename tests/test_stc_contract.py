"""tests/stc_contract.py (the numpy restatement of include/gq_stc.h) against independent witnesses, and every claim its inputs make
about themselves.  No GPU."""
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import stc_contract as sc  # noqa: E402
import topk_contract as tc  # noqa: E402


def _ulp_apart(a_bits, b_bits):
    return abs(int(a_bits) - int(b_bits))


# ---- witnesses -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cr", [(1001, 8), (4097, 16), (12289, 256), (65536, 256)])
def test_against_the_torch_expression(n, cr):
    """torch.topk(abs), mean, sign on an input without ties: the same kept set; mu within one float32 ulp of the float64 mean (the
    tree rounds in float64, in another order); the dense decode is sign(w) * mu on the kept set and +0 elsewhere."""
    w = tc.ordinary(n, 7 + n)
    k = n // cr
    t = torch.from_numpy(w)
    idx = torch.topk(t.abs(), k)[1]
    assert np.array_equal(np.sort(idx.numpy()), tc.kept(w, k))
    mean = t[idx].abs().double().mean().float()
    mu = sc.mu_bits(w, k)
    assert _ulp_apart(mu, mean.numpy().view(np.uint32)) <= 1
    want = torch.zeros(n)
    want[idx] = torch.sign(t[idx]) * sc.from_bits(np.array([mu], np.uint32))[0]
    assert np.array_equal(sc.bits(sc.dense(w, k)), sc.bits(want.numpy()))


def _tree(x):
    """halve() written as a recursion on scalars: the slots of even and of odd index, each reduced, then added."""
    if len(x) == 1:
        return x[0]
    return _tree(x[0::2]) + _tree(x[1::2])


def _scalar(w, k):
    """The header with Python loops and scalars -> (bits(mu), the section's words, the starts)"""
    n = len(w)
    b = [int(x) for x in sc.bits(w)]
    key = [0x7fffffff if (x & 0x7fffffff) > 0x7f800000 else x & 0x7fffffff for x in b]
    order = sorted(range(n), key=lambda i: (-key[i], i))
    kept = sorted(order[:k])
    if k == 0:
        return 0, [], [0] * sc.items_of(n)
    T = min(key[i] for i in kept)
    need = k - sum(1 for i in range(n) if key[i] > T)
    mags = [float(np.array([x & 0x7fffffff], np.uint32).view(np.float32)[0]) for x in b]
    nit = sc.items_of(n)
    sums = []
    for t in range(nit):
        slots = [mags[i] if i < n and key[i] > T else 0.0 for i in range(t * 4096, (t + 1) * 4096)]
        sums.append(_tree(slots))
    P = 1
    while P < nit:
        P *= 2
    S = _tree(sums + [0.0] * (P - nit)) + float(need) * float(np.array([T], np.uint32).view(np.float32)[0])
    m = np.float32(S / float(k))
    mu = 0x7fc00000 if np.isnan(m) else int(np.array([m], np.float32).view(np.uint32)[0])
    words = [(i % 4096) | ((b[i] >> 31) << 15) for i in kept]
    starts = [sum(1 for i in kept if i < t * 4096) for t in range(nit)]
    return mu, words, starts


@pytest.mark.parametrize("name", ["ordinary", "two_level", "special_k5", "special_finite", "k0", "kn"])
def test_against_a_scalar_loop(name):
    w, k = {"ordinary": (tc.heavy_tailed(9000, 5), 70), "two_level": (tc.two_level(8193, 6), 700),
            "special_k5": (sc.special_input(), 5), "special_finite": (sc.special_cases()[7][1], 3500),
            "k0": (tc.ordinary(4097, 8), 0), "kn": (tc.ordinary(4097, 8), 4097)}[name]
    with np.errstate(invalid="ignore", over="ignore"):
        mu, words, starts = _scalar(w, k)
    head, start, word, pad = sc.split_section(sc.section_bytes(w, k), w.size, k)
    assert (int(head[0]), int(head[1]), int(head[2]), int(head[3])) == (k, mu, sc.items_of(w.size), 0)
    assert [int(x) for x in start] == starts and [int(x) for x in word] == words and not pad.any()
    assert sc.section_bytes(w, k).size == sc.section_size(w.size, k)


@pytest.mark.parametrize("n,k", [(4096, 4096), (12289, 300), (70000, 70000), (8193, 8000)])
def test_mu_against_exact_fractions(n, k):
    """Multiples of 2^-10: every float64 partial sum is exact, so mu is f32(f64(the exact sum) / k) whatever the tree."""
    w = sc.exact_input(n, 11 + n)
    idx = tc.kept(w, k)
    exact = sum((Fraction(float(abs(x))) for x in w[idx]), Fraction(0))
    assert exact.denominator <= 1024 and exact < 2 ** 40      # (the precondition: the sum fits float64 exactly)
    want = np.array([np.float32(float(exact) / float(k))], np.float32).view(np.uint32)[0]
    assert sc.mu_bits(w, k) == want
    if k < n:
        T, need, _ = sc.threshold(w, k)
        assert int((tc.keys(w) == T).sum()) >= need >= 1


def test_halving_order_is_not_a_running_sum():
    """An input on which the header's tree and a left-to-right float64 sum differ in the last bit of S: the order is part of the
    contract."""
    rs = np.random.RandomState(12)
    x = np.abs(rs.standard_normal(4096)) * 10.0 ** rs.randint(-8, 8, size=4096)
    tree, run = sc.halve(x)[0], 0.0
    for v in x:
        run = run + v
    assert tree != run and abs(tree - run) <= 1e-9 * tree
    assert tree == _tree(list(x))


# ---- the inputs' preconditions ------------------------------------------------------------------------------------------------------
def test_the_seam_input_straddles_both_seams():
    w = sc.seam_input()
    for k, pos in sc.seam_ks():
        T, need, idx = sc.threshold(w, k)
        ties = np.flatnonzero(tc.keys(w) == T)
        assert T == tc.ONE and ties[need - 1] == pos and need < ties.size      # the last kept tie is at pos, the next one is dropped
        assert pos in idx and ties[need] not in idx
    assert {pos % 4096 for _, pos in sc.seam_ks()} == {4095, 0}


def test_the_lopsided_input_fills_one_item_and_empties_four():
    w, k = sc.lopsided_input()
    head, start, word, _ = sc.split_section(sc.section_bytes(w, k), w.size, k)
    per_item = np.diff(np.append(start, k))
    assert list(per_item) == [0, 0, 4096, 0, 40, 0]
    assert np.array_equal(word[:4096] & 0xfff, np.arange(4096))


def test_the_special_input_keeps_and_drops_every_kind():
    w = sc.special_input()
    ky = tc.keys(w)
    assert int(np.isnan(w).sum()) == 3 and int(np.isinf(w).sum()) == 3 and int((ky == 0).sum()) == 3000
    assert int(((ky > 0) & (ky < 0x800000)).sum()) == 1000 and (sc.bits(w)[:3000] >> 31).any() and not (sc.bits(w)[:3000] >> 31).all()
    for name, x, k in sc.special_cases():
        idx, mu = tc.kept(x, k), sc.mu_bits(x, k)
        kn, ki = int(np.isnan(x[idx]).sum()), int(np.isinf(x[idx]).sum())
        if name in ("k2", "k3", "k5", "k6", "k1500"):
            assert mu == sc.NAN_MU and kn == min(k, 3) and ki == min(max(k - 3, 0), 3)
        elif name != "inf_mu":
            assert np.isfinite(x).all() and mu != sc.NAN_MU
        if name == "k1500":
            assert int(((tc.keys(x[idx]) > 0) & (tc.keys(x[idx]) < 0x800000)).sum()) > 0
        if name == "finite_k3500":
            zeros = idx[tc.keys(x[idx]) == 0]
            assert zeros.size > 0 and (sc.bits(x[zeros]) >> 31).any()      # a kept -0
            assert (sc.bits(sc.dense(x, k)[zeros]) >> 31).any()               # carries its sign into the decode
        if name == "subnormal_mu":
            assert 0 < int(mu) < 0x800000      # mu itself is a subnormal
        if name == "inf_mu":
            assert mu == 0x7f800000 and ki == 2 and kn == 0


def test_hand_sections_cancel():
    secs, named = sc.hand_sections(12289, 200, 3, 5)
    assert np.array_equal(named[0][0], named[1][0]) and np.all(named[0][1] + named[1][1] == 1) and named[0][2] == named[1][2]
    out = sc.decode_mean(secs[:2], 12289, 200, 2)
    assert not sc.bits(out).any()      # +mu + -mu = +0, and +0 / 2 = +0 everywhere
    lo, hi = named[2][0][0] // 4096, named[2][0][-1] // 4096
    assert lo == hi      # payload 2 sits in one item


def test_decode_mean_clamps_what_the_wire_claims():
    """Starts above k, a start below its predecessor, positions past the item's length: nothing outside [0, n) is named."""
    n, k = sc.LIE_N, sc.LIE_K
    out = sc.decode_mean([sc.lying_section()], n, k, 1)
    named = np.flatnonzero(out)
    assert named.size == 63 and named.max() < 4096 and set(np.abs(out[named])) == {np.float32(1.0)} and (out[named] < 0).any()


def test_error_feedback_uses_two_roundings():
    v, e, k, pairs = tc.ef_fma()
    w, sec, D, e2 = sc.error_feedback(v, e, 0.75, k)
    assert np.array_equal(sc.bits(w), sc.bits(tc.feedback(v, e, 0.75))) and not np.array_equal(sc.bits(w), sc.bits(tc.fma_f32(v, e, 0.75)))
    assert np.array_equal(sc.bits(e2), sc.bits((w - D).astype(np.float32)))
    kept = D != 0
    assert int(kept.sum()) == k and np.all(np.abs(D[kept]) == np.abs(D[kept][0]))


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def test_wire_layout():
    assert sc.section_size(1001, 3) == 32 and sc.section_size(4096, 16) == 64 and sc.section_size(4097, 16) == 64
    assert sc.section_size(8193, 0) == 32 and sc.section_size(4096, 4096) == 16 + 4 + 8192 + 12
    sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))
    from gq_amd.codecs import stc_section_bytes
    for n in (1001, 4097, 200704, 2359296):
        assert stc_section_bytes(n, 256) == sc.section_size(n, n // 256)
    assert stc_section_bytes(100, 256) == 32      # k = 0: the header and one start
    # the README's figure: one user's ResNet-50 wire at cr = 256 -- the 76 tensors over 1,000 elements as 16-byte aligned sections,
    # the 85 others behind them as packed float32 (the quantizer's layout); top-k's wire is 823,968 B, dense 94,083,376 B
    with open(os.path.join(HERE, "golden", "resnet50_cifar_shapes.json")) as f:
        sizes = [int(np.prod(s)) for s in json.load(f)["parameter_shapes"]]
    big, small = [n for n in sizes if n > 1000], [n for n in sizes if n <= 1000]
    assert (len(big), len(small), sum(n // 256 for n in big)) == (76, 85, 91790)
    off = 0
    for n in big:
        off = sc.up16(off + stc_section_bytes(n, 256))
    assert off == 208_016      # top-k: 734,320
    assert sc.up16(off + 4 * sum(small)) == 297_664      # top-k: 823,968
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "297,664" in readme and "823,968" in readme


def test_quantizer_lays_the_resnet50_wire_out_as_computed():
    from argparse import Namespace
    sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))
    from gq_amd.codecs import BatchedSTC, STCCodec
    from gq_amd.compressors import SparseTernaryCompressor
    from gq_amd.quantizers import PSQuantizer
    with open(os.path.join(HERE, "golden", "resnet50_cifar_shapes.json")) as f:
        params = [torch.nn.Parameter(torch.zeros(s)) for s in json.load(f)["parameter_shapes"]]
    args = Namespace(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=1, mode="ps",
                     cr=256)
    q = PSQuantizer(SparseTernaryCompressor, params, args)
    assert q.wire_bytes_per_user() == 297_664
    assert [g[0] for g in q._groups] == [BatchedSTC] and len(q._groups[0][1]) == 76
    assert all(type(c) is STCCodec for c in q.codecs if c.numel > 1000)


# ---- the README's error table ------------------------------------------------------------------------------------------------------
def _student_t3(n, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_t(3, size=n) * 1e-3).astype(np.float32)


def _normal(n, seed):
    return (np.random.RandomState(seed).standard_normal(n) * 1e-3).astype(np.float32)


ERROR_TABLE = {"normal": (_normal, 21), "student_t3": (_student_t3, 22)}


def _rel_l2(w, d):
    w, d = w.astype(np.float64), d.astype(np.float64)
    return float(np.sqrt(((w - d) ** 2).sum() / (w ** 2).sum()))


def test_error_table_of_the_readme():
    """Relative L2 error of decode(compress(w)) at cr = 256, n = 65,536, STC beside top-k on the same input.  Asserted: both keep the
    same set; STC's error is at least top-k's (top-k's decode is the best approximation on that set) and below 1 (the mean magnitude
    on the kept set removes energy: sum over the kept of (|w| - mu)^2 < sum of w^2 there); sum |dec| is the sum of the kept |w| to
    float32 rounding (k * mu against the float64 sum: half an ulp of mu relative, 2^-24, plus the sum's own rounding); the README
    carries the figures."""
    n, k = 65536, 256
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name, (make, seed) in ERROR_TABLE.items():
        w = make(n, seed)
        d_stc, d_topk = sc.dense(w, k), tc.dense(w, k)
        assert np.array_equal(d_stc != 0, d_topk != 0) and int((d_stc != 0).sum()) == k
        e_stc, e_topk = _rel_l2(w, d_stc), _rel_l2(w, d_topk)
        print("%-10s  stc %.4f  topk %.4f" % (name, e_stc, e_topk))
        assert e_topk <= e_stc < 1.0
        kept_abs = np.abs(w[d_stc != 0]).astype(np.float64).sum()
        assert abs(np.abs(d_stc).astype(np.float64).sum() - kept_abs) <= kept_abs * 2.0 ** -23
        assert "| %s | %.4f | %.4f |" % (name, e_stc, e_topk) in readme


def test_the_select_and_the_shared_code_are_the_sparse_header_s():
    import re
    from test_topk_host import shared_header_checks
    text = shared_header_checks("stc.hip")
    assert not re.search(r"(hist|pick)_kernel\(const", text) and "gqsp::hist_kernel<Sizes, EF>" in text and "gqsp::pick_kernel<Sizes>" in text
