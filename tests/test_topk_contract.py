"""tests/topk_contract.py against independent witnesses (no GPU): the reference's fixtures, torch.topk where there are no ties, a
brute-force loop where there are, scalar loops for the decode-mean, torch CPU ops for the error feedback -- and one assertion for
every claim tests/test_gpu_topk_contract.py makes about its inputs (which bin of which pass the threshold lands in and who owns it,
where the last kept tie sits, what a fused multiply-add, another order of additions or a multiplication by 1/R would change), so
that the reference the kernels are held to cannot be wrong, or its inputs toothless, silently."""
import glob
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import topk_contract as tc  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


def _same(a, b):
    """Bitwise equal, except that any NaN equals any NaN."""
    a, b = tc.f32(a), tc.f32(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(tc.bits(a)[~na], tc.bits(b)[~nb])


# ---- witnesses --------------------------------------------------------------------------------------------------------------
FIXTURES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "topk_*.npz")) if "x" in np.load(p).files)


def test_fixtures_found():
    assert len(FIXTURES) >= 6


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_restatement_against_the_reference_fixtures(path):
    g = np.load(path)
    x, k = g["x"], int(g["k"])
    D = tc.dense(x, k)
    if "dec" in g.files:
        assert _same(D, g["dec"])
    assert hashlib.sha256(D.tobytes()).hexdigest() == str(g["dec_sha"]) or np.isnan(D).any()
    ky = tc.keys(x)
    mine = tc.kept(x, k)
    assert mine.size == k and np.array_equal(np.sort(ky[mine]), np.sort(ky[g["kept"].astype(np.int64)]))
    idx, val = tc.split_section(tc.section_bytes(x, k), k)
    assert np.array_equal(idx, mine.astype(np.uint32)) and np.array_equal(tc.bits(val), tc.bits(x)[mine])


@pytest.mark.parametrize("n,k", [(1, 1), (257, 3), (5000, 312), (70001, 70001), (100000, 391)])
def test_kept_against_torch_topk_without_ties(n, k):
    rs = np.random.RandomState(n % 89)      # distinct magnitudes, shuffled, random signs
    x = ((rs.permutation(n) + 1) * np.where(rs.rand(n) < 0.5, -1, 1) / 1024.0).astype(np.float32)
    assert np.unique(tc.keys(x)).size == n
    want = torch.sort(torch.topk(torch.abs(torch.from_numpy(x)), k)[1])[0].numpy()
    assert np.array_equal(tc.kept(x, k), want)


def _brute_kept(w, k):
    """The k best by (key descending, index ascending), one comparison at a time."""
    ky = [int(x) for x in tc.keys(w)]
    chosen = []
    taken = [False] * len(ky)
    for _ in range(k):
        best = -1
        for i, key in enumerate(ky):
            if not taken[i] and (best < 0 or key > ky[best]):
                best = i
        taken[best] = True
        chosen.append(best)
    return np.array(sorted(chosen), np.int64)


def test_kept_against_a_brute_force_loop_with_ties():
    rs = np.random.RandomState(5)
    x = rs.randint(-3, 4, size=300).astype(np.float32)
    x[rs.rand(300) < 0.2] = np.float32(-0.0)
    x[[7, 100, 250]] = tc.from_bits(np.uint32([0x7fc00000, 0xffc00001, 0x7f800001]))
    x[[8, 9]] = [np.inf, -np.inf]
    for k in (0, 1, 2, 3, 4, 5, 50, 150, 299, 300):
        assert np.array_equal(tc.kept(x, k), _brute_kept(x, k)), k
    for name in ("one", "bit9"):
        w = tc.pair_input(name)[:400]
        for k in (1, 100, 399):
            assert np.array_equal(tc.kept(w, k), _brute_kept(w, k))
    assert np.array_equal(tc.keys(tc.from_bits(tc.NANS)), np.full(tc.NANS.size, 0x7fffffff, np.uint32))
    assert np.array_equal(tc.keys(np.float32([np.inf, -np.inf, -0.0, -1.0])), np.uint32([0x7f800000, 0x7f800000, 0, tc.ONE]))


def test_dense_keeps_the_sign_of_zero_and_makes_nan_of_inf():
    x = np.float32([3, -1, np.inf, -2, -0.0, np.nan])
    D = tc.dense(x, 2)      # NaN and inf are kept
    assert np.array_equal(tc.kept(x, 2), [2, 5])
    assert np.array_equal(tc.bits(D)[[0, 1, 3, 4]], np.uint32([0, 1 << 31, 1 << 31, 1 << 31])) and np.isinf(D[2]) and np.isnan(D[5])
    assert np.isnan(tc.dense(x, 1)[2])      # an unkept inf: inf * 0


def _loop_decode(payloads, n, R, plain, reverse=False, mul=False):
    """The decode-mean one np.float32 scalar at a time; reverse / mul: the arithmetic the contract rules out."""
    out = [np.float32(0)] * n
    if plain and R == 1:
        for i, x in zip(*payloads[0]):
            out[int(i)] = np.float32(x)
        return np.array(out, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for idx, val in (payloads[::-1] if reverse else payloads):
            for i, x in zip(idx, val):
                out[int(i)] = np.float32(out[int(i)] + np.float32(x))
        inv = np.float32(1) / np.float32(R)
        return np.array([np.float32(a * inv) if mul else np.float32(a / np.float32(R)) for a in out], np.float32)


@pytest.fixture(scope="module")
def hand():
    return tc.hand_payloads()


@pytest.mark.parametrize("first,R", tc.DEC_WINDOWS)
def test_decode_mean_against_a_scalar_loop_and_what_its_inputs_show(hand, first, R):
    """Every tensor, the windows of payloads test_gpu_topk_contract.py decodes: equal to the scalar loop; from R = 3 on the result
    differs under the reverse order of additions (two payloads commute); where R is no power of two it differs under
    acc * f32(1 / R) (a power of two divides exactly either way)."""
    order_shows = mul_shows = False
    assert sorted(set(r for _, r in tc.DEC_WINDOWS)) == [1, 2, 3, 8, 16] and first + R <= tc.DEC_PAYLOADS
    for s, (n, k) in enumerate(zip(tc.DEC_SIZES, tc.DEC_KS)):
        P = hand[s][first:first + R]
        want = _loop_decode(P, n, R, False)
        assert _same(tc.decode_mean(P, n, k, R), want)
        if R == 1:
            assert _same(tc.decode_mean(P, n, k, R, plain=True), _loop_decode(P, n, R, True))
        if k:
            order_shows |= not _same(want, _loop_decode(P, n, R, False, reverse=True))
            mul_shows |= not _same(want, _loop_decode(P, n, R, False, mul=True))
    assert order_shows == (R >= 3)
    assert mul_shows == (R & (R - 1) != 0)


def test_decode_inputs_are_what_they_claim(hand):
    for s, (n, k) in enumerate(zip(tc.DEC_SIZES, tc.DEC_KS)):
        assert len(hand[s]) == tc.DEC_PAYLOADS
        for r, (idx, val) in enumerate(hand[s]):
            assert idx.dtype == np.uint32 and val.dtype == np.float32 and idx.size == val.size == k
            assert np.all(np.diff(idx.astype(np.int64)) > 0) and (k == 0 or idx[-1] < n)
            if k > 6:
                assert np.all(np.isin(tc._hot(n), idx)) or r % 4 == 3      # 0, 4095, 4096, n - 1 among them
            if r % 4 == 3 and 6 < k < n:
                assert np.unique(idx // tc.CHUNK).size == 1      # all k in one chunk
        assert len(set(h[0].tobytes() for h in hand[s])) > 1 or k in (0, n) or k <= 6      # the users' index sets differ
    s, c = tc.DEC_UNTOUCHED
    assert tc.DEC_SIZES[s] > (c + 1) * tc.CHUNK and not any(((idx // tc.CHUNK) == c).any() for idx, _ in hand[s])
    assert 0 in tc.DEC_KS and any(k == n for n, k in zip(tc.DEC_SIZES, tc.DEC_KS))
    # 1e8, 1, -1e8 in every order on one index each: three orders give 0, the others 1 and 2 -- the order is visible
    n, k = tc.DEC_SIZES[3], tc.DEC_KS[3]
    got = tc.decode_mean(hand[3][:3], n, k, 3)[tc._hot(n)]
    sums = []
    for p in tc.PERMS:
        a = np.float32(0)
        for j in p:
            a = np.float32(a + np.float32(tc.BIG[j]))
        sums.append(np.float32(a / np.float32(3)))
    assert np.array_equal(got, np.float32(sums)) and len(set(sums)) >= 2 and sorted(tc.PERMS) == sorted(set(tc.PERMS))
    # -0: kept by plain, +0 under the mean with R = 1
    idx, val = hand[3][0]
    neg = idx[tc.bits(val) == 1 << 31].astype(np.int64)
    assert neg.size > 10
    assert np.all(tc.bits(tc.decode_mean(hand[3][:1], n, k, 1, plain=True))[neg] == 1 << 31)
    assert np.all(tc.bits(tc.decode_mean(hand[3][:1], n, k, 1))[neg] == 0)
    assert all(np.isnan(hand[3][r][1]).any() and np.isinf(hand[3][r][1]).any() for r in (4, 5))


EF_BUILDERS = {"reorder": (tc.ef_reorder, 0.75), "fma": (lambda: tc.ef_fma()[:3], 0.75), "ties": (tc.ef_ties, 1.0),
               "inf": (tc.ef_inf, 0.0), "zeros_pos": (tc.ef_signed_zeros, 0.0), "zeros_neg": (tc.ef_signed_zeros, -0.0),
               "one": (tc.ef_reorder, 1.0)}


@pytest.mark.parametrize("name", sorted(EF_BUILDERS))
def test_error_feedback_against_torch_cpu_ops(name):
    make, s = EF_BUILDERS[name]
    v, e, k = make()
    w, sec, D, e2 = tc.error_feedback(v, e, s, k)
    tv, te = torch.from_numpy(v), torch.from_numpy(e)
    tw = tv + torch.tensor(s, dtype=torch.float32) * te      # two ops: two roundings
    assert _same(w, tw.numpy())
    mask = torch.zeros(v.size)
    mask[torch.from_numpy(tc.kept(w, k))] = 1
    td = tw * mask
    assert _same(D, td.numpy()) and _same(e2, (tw - td).numpy())
    idx, val = tc.split_section(sec, k)
    assert np.array_equal(idx.astype(np.int64), tc.kept(w, k)) and _same(val, w[tc.kept(w, k)])


# ---- preconditions of tests/test_gpu_topk_contract.py --------------------------------------------------------------------------
def test_passes_as_the_kernel_file_states_them():
    src = open(os.path.join(os.path.dirname(HERE), "gradient-quantization_amd", "csrc", "sparse_kernels.hpp")).read()
    assert "return p == 0 ? 20 : (p == 1 ? 9 : 0);" in src and "return p == 2 ? 9 : 11;" in src
    assert "constexpr int THREADS = 256;" in src and "#define GQ_TOPK_CHUNK 4096" in open(
        os.path.join(os.path.dirname(HERE), "include", "gq_topk.h")).read()
    assert tc.PASS_SHIFT == (20, 9, 0) and tc.PASS_BITS == (11, 11, 9) and sum(tc.PASS_BITS) == 31
    assert tc.pick_thread(0, 2047) == (0, False) and tc.pick_thread(0, 2040) == (0, True) and tc.pick_thread(2, 0) == (255, True)


def test_low9_thresholds():
    w = tc.low9_input()
    ky = tc.keys(w)
    assert set(ky) == set(range(tc.ONE, tc.ONE + 512)) and ky.size > 512 and (w < 0).any() and (w > 0).any()
    assert set(k >> 20 for k in ky) == {1016} and set((k >> 9) & 2047 for k in ky) == {0}      # one bin in pass 0 and in pass 1
    cases = tc.low9_cases()
    assert len(cases) == 11 and sorted(set(c[0] for c in cases)) == tc.LOW9
    for low, more, k in cases:
        sel = tc.select(w, k)
        assert sel["bins"] == (1016, 0, low - more)
        if more:
            assert sel["need"] == 1 and sel["gt"] == k - 1
        else:
            assert sel["need"] == sel["ties"]      # every tie kept
    # pass 2's owners: 511 | 510 with thread 0, 256 the last bin of thread 127, 255 the first of thread 128 (waves 1 | 2), 1 | 0 thread 255
    assert [tc.pick_thread(2, b) for b in (511, 510, 256, 255, 1, 0)] == [(0, False), (0, True), (127, True), (128, False), (255, False), (255, True)]


def test_pair_thresholds():
    """k = a - 1, a, a + 1: the threshold in the upper bin with a tie left out, with every tie kept -- k is the cumulative count at
    the END of the owner's bins, the upper end of the pick's interval test -- and one past it, in the next thread's first bin."""
    owners = {"one": (0, 1016, 128, 1015, 129), "two": (0, 1024, 127, 1023, 128), "bit9": (1, 1, 255, 0, 255),
              "pass1_thread": (1, 1536, 63, 1535, 64)}
    for name, (p, bhi, thi, blo, tlo) in owners.items():
        hi, lo = tc.PAIRS[name]
        assert (tc.pass_bin(hi, p), tc.pass_bin(lo, p)) == (bhi, blo) and bhi == blo + 1
        assert tc.pick_thread(p, bhi)[0] == thi and tc.pick_thread(p, blo)[0] == tlo
        if p == 1:
            assert tc.pass_bin(hi, 0) == tc.pass_bin(lo, 0)
        w = tc.pair_input(name)
        a = int((tc.keys(w) >= hi).sum())
        assert set(tc.keys(w)) == {hi, lo} and tc.pair_ks(name) == [a - 1, a, a + 1] and 1 < a < w.size - 1
        s0, s1, s2 = (tc.select(w, k) for k in tc.pair_ks(name))
        assert (s0["T"], s0["need"], s0["ties"]) == (hi, a - 1, a) and (s1["T"], s1["need"]) == (hi, a) and (s2["T"], s2["need"], s2["gt"]) == (lo, 1, a)
    assert tc.from_bits(np.uint32([tc.PAIRS["one"][1]]))[0] == np.nextafter(np.float32(1), np.float32(0))
    assert tc.from_bits(np.uint32([tc.PAIRS["two"][1]]))[0] == np.nextafter(np.float32(2), np.float32(0))
    assert tc.PAIRS["bit9"][0] ^ tc.PAIRS["bit9"][1] == 1 << 9
    # thread seams: 128 | 129 inside wave 2 with 1016 the LAST bin of thread 128 (thread 128 is the first lane of its wave: what is
    # before it comes from the other waves alone); 127 | 128 and 63 | 64 are wave seams; 8t + 7 | 8t + 8 with t = 191
    assert tc.pick_thread(0, 1016) == (128, True) and tc.pick_thread(0, 1024) == (127, True) and tc.pick_thread(1, 1536) == (63, True)
    assert 128 % 64 == 0 and 127 // 64 != 128 // 64 and 63 // 64 != 64 // 64 and (1535, 1536) == (8 * 191 + 7, 8 * 191 + 8)


def test_subnormal_thresholds():
    w = tc.subnormal_input()
    ky = tc.keys(w)
    normals = int((ky >= 0x800000).sum())
    assert normals == 7 and ((ky > 0) & (ky < 0x800000)).sum() > 300
    want = {"min": (tc.SUB_MIN, (0, 0, 1)), "mid": (tc.SUB_MID, (0, 1024, 0x123)), "zero": (0, (0, 0, 0))}
    for name, k in tc.subnormal_cases():
        sel = tc.select(w, k)
        assert k > normals and (sel["T"], sel["bins"]) == want[name]
        if name == "zero":
            zeros = np.flatnonzero(ky == 0)
            assert 1 < sel["need"] < zeros.size
            kept_zero = zeros[:sel["need"]]
            assert (tc.bits(w)[kept_zero] == 1 << 31).any() and (tc.bits(w)[kept_zero] == 0).any()      # -0 and +0 both on the wire
            idx, val = tc.split_section(tc.section_bytes(w, k), k)
            assert np.array_equal(tc.bits(val), tc.bits(w)[idx.astype(np.int64)])
        else:
            assert (sel["need"], sel["ties"]) == (2, 3)
    assert tc.from_bits(np.uint32([1]))[0] == np.float32(1e-45)


def test_top_thresholds():
    want = {("nan", 10): (0x7fffffff, (2047, 2047, 511), 0), ("inf", 12): (0x7f800000, (2040, 0, 0), 3), ("inf", 33): (0x7f800000, (2040, 0, 0), 3)}
    for kind, k in tc.TOP_CASES:
        w = tc.top_input(kind)
        sel = tc.select(w, k)
        assert (sel["T"], sel["bins"], sel["gt"]) == want[(kind, k)]
        if kind == "nan":
            nans = np.flatnonzero(np.isnan(w))
            assert nans.size == 40 > k and np.array_equal(tc.kept(w, k), nans[:k])
            b = tc.bits(w)[nans[:k]]
            assert (b >> 31).any() and not (b >> 31).all() and np.unique(b).size >= 3      # both signs, several payloads
        else:
            assert int(np.isinf(w).sum()) == 30 and int(np.isnan(w).sum()) == 3 and (w == np.inf).any() and (w == -np.inf).any()
            assert sel["ties"] == 30 and sel["need"] == k - 3      # 33: exactly k NaNs plus infinities
    assert tc.pick_thread(0, 2040) == (0, True) and tc.pick_thread(0, 2047) == (0, False)


def test_stair_ks_sit_on_the_ends_of_the_pick_threads():
    w = tc.stair_input()
    ky = tc.keys(w)
    ks = tc.stair_ks()
    assert len(ks) == 6 and len(set(t for _, t in ks)) == 3
    for j in range(0, 6, 2):
        (k, t), (k1, _) = ks[j], ks[j + 1]
        lowest = 2047 - 8 * t - 7      # the last bin of thread t
        assert k == int(((ky >> 20) >= lowest).sum()) and k1 == k + 1 <= w.size
        a, b = tc.select(w, k), tc.select(w, k1)
        assert tc.pick_thread(0, a["bins"][0])[0] == t and a["need"] == a["ties"] or a["bins"][0] > lowest      # kr == before + sum
        assert tc.pick_thread(0, a["bins"][0])[0] == t
        assert tc.pick_thread(0, b["bins"][0])[0] > t      # kr == before + 1 of a later thread


def test_tie_inputs():
    assert -(-tc.TIE_N // tc.CHUNK) == 258 and 1048576 == 256 * tc.CHUNK and tc.TIE_EDGES[-1] == tc.TIE_N - 1
    w = tc.all_equal(tc.TIE_N, 1)
    assert np.unique(tc.keys(w)).size == 1 and (w < 0).any() and (w > 0).any()
    for pos in tc.TIE_EDGES:
        k = tc.k_for_last_tie(w, 0x3e800000, pos)
        sel = tc.select(w, k)
        assert k == pos + 1 and (sel["last"], sel["gt"], sel["need"]) == (pos, 0, pos + 1)
    w = tc.two_level(tc.TIE_N, 2, tc.TIE_EDGES)
    ky = tc.keys(w)
    assert set(ky) == {tc.ONE, 0x40000000} and ky[1] == 0x40000000
    for pos in tc.TIE_EDGES:
        sel = tc.select(w, tc.k_for_last_tie(w, tc.ONE, pos))
        assert (sel["T"], sel["last"]) == (tc.ONE, pos) and sel["gt"] == int((ky == 0x40000000).sum()) > 60000
        assert pos < 2 or (ky[:pos] > tc.ONE).any()      # #(key > T) in front of the last tie is not zero
    assert tc.select(w, tc.k_for_last_tie(w, tc.ONE, 0))["need"] == 1
    assert tc.select(w, tc.k_for_last_tie(w, tc.ONE, tc.TIE_N - 1))["need"] == int((ky == tc.ONE).sum())
    h = tc.all_equal(tc.HALF_N, 3)
    assert [tc.select(h, k)["last"] for k in (1048576, 1048577)] == [1048575, 1048576] and tc.HALF_N == 2097153
    for n in tc.TIE_SIZES:
        for make in (tc.all_equal, lambda n, s: tc.two_level(n, s)):
            x = make(n, n)
            assert x.size == n and tc.kept(x, n).size == n and tc.kept(x, 1)[0] == int(np.argmax(tc.keys(x)))


def test_error_feedback_inputs():
    """Each input has an element where fma(s, err, v) is not the two-rounding w (float64 holds the sum exactly there, so its
    rounding IS the fused result) and a fused load changes the kept set or a value on the wire."""
    for name, (make, s) in sorted(EF_BUILDERS.items()):
        v, e, k = make()
        w, wf = tc.feedback(v, e, s), tc.fma_f32(v, e, s)
        if s in (0.75,):
            diff = [i for i in np.flatnonzero(tc.bits(w) != tc.bits(wf))[:50] if tc.exact_fma(v, e, s, i)]
            assert diff, name
            on_wire = np.isin(diff, tc.kept(w, k)).any()
            assert on_wire or not np.array_equal(tc.kept(w, k), tc.kept(wf, k)), name
        else:
            assert np.array_equal(tc.bits(w)[~np.isnan(w)], tc.bits(wf)[~np.isnan(w)])      # s = 1, 0, -0: the product is exact
    v, e, k = tc.ef_reorder()
    assert not np.array_equal(tc.kept(v, k), tc.kept(tc.feedback(v, e, 0.75), k))      # err reorders the ranking
    v, e, k, pairs = tc.ef_fma()
    w, wf = tc.feedback(v, e, 0.75), tc.fma_f32(v, e, 0.75)
    assert len(pairs) >= 3 and all(tc.exact_fma(v, e, 0.75, i) for i in pairs)
    i = pairs[0]
    k2, kf = tc.kept(w, k), tc.kept(wf, k)
    assert i + 1 in k2 and i not in k2 and i in kf and i + 1 not in kf      # a fused load moves a key across the threshold
    v, e, k = tc.ef_ties()
    w = tc.feedback(v, e, 1.0)
    sel = tc.select(w, k)
    tied = np.flatnonzero(tc.keys(w) == sel["T"])
    assert sel["T"] == 0x40000000 and 1 < sel["need"] < sel["ties"] and np.unique(tc.keys(v)[tied]).size > 20
    v, e, k = tc.ef_inf()
    w = tc.feedback(v, e, 0.0)
    assert int(np.isnan(w).sum()) == 30 > k and np.array_equal(tc.kept(w, k), np.flatnonzero(np.isnan(w))[:k]) and not np.isnan(v).any()
    v, e, k = tc.ef_signed_zeros()
    wp, wn = tc.feedback(v, e, 0.0), tc.feedback(v, e, -0.0)
    assert not np.array_equal(tc.bits(wp), tc.bits(wn)) and np.array_equal(wp, wn)      # they differ in the signs of zeros alone
    assert (tc.bits(wn)[tc.kept(wn, k)] == 1 << 31).any()
