"""libgq_kmeans.so held to include/gq_kmeans.h on the MI355X: every comparison is np.array_equal against the numpy restatement
(tests/kmeans_contract.py), at every seam of the launch (point counts around a wave and a pass, every register layout of d,
codebooks of one and of several LDS chunks, LDS partial sums and global atomics, a misaligned X), on ties and degenerate rows,
with garbage in every buffer the library writes and canaries around it, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import kmeans_contract as kc
from gq_amd import codebook, native

pytestmark = pytest.mark.gpu
F = np.float32
METRIC_IDS = ["euclid", "absdot"]
GUARD = 16      # canary elements on either side of every output


def _guarded(n, dtype, dev, gen):
    """A buffer of n elements full of garbage between two runs of canaries -> (the whole buffer, the view a call writes)."""
    info = torch.iinfo(dtype)
    buf = torch.randint(max(info.min, -2 ** 62), min(info.max, 2 ** 62), (n + 2 * GUARD,), dtype=dtype, device=dev, generator=gen)
    buf[:GUARD] = 0x5A
    buf[GUARD + n:] = 0x5A
    return buf, buf[GUARD:GUARD + n]


def _canaries_hold(buf, n):
    return bool((buf[:GUARD] == 0x5A).all()) and bool((buf[GUARD + n:] == 0x5A).all())


def _dev_f32(a, dev, misalign=False):
    """A float32 array on the device between canaries; misalign: the view starts 4 bytes past a 16-byte boundary."""
    flat = torch.full((a.size + 2 * GUARD + 1,), 123.0, dtype=torch.float32, device=dev)
    start = GUARD + (1 if misalign else 0)
    assert (flat.data_ptr() + 4 * GUARD) % 16 == 0
    view = flat[start:start + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return flat, view


def gpu_run(X, C, metric, iters, misalign=False, flags=0):
    """gq_kmeans_run with garbage in workspace, labels, signs and counts -> (C, labels, signs, counts) as numpy."""
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    (N, d), K = X.shape, C.shape[0]
    _, Xd = _dev_f32(X, dev, misalign)
    Cbuf, Cd = _dev_f32(C, dev, misalign)
    lbuf, labels = _guarded(N, torch.int32, dev, gen)
    sbuf, signs = _guarded(N, torch.int8, dev, gen)
    cbuf, counts = _guarded(K, torch.int64, dev, gen)
    words = native.kmeans_workspace_bytes(K, d) // 8
    assert words == K * (d + 1)
    wbuf, ws = _guarded(words, torch.int64, dev, gen)
    native.kmeans_run(Xd, Cd, metric | flags, iters, labels, counts, ws, signs=signs)
    torch.cuda.synchronize()
    assert _canaries_hold(lbuf, N) and _canaries_hold(sbuf, N) and _canaries_hold(cbuf, K) and _canaries_hold(wbuf, words)
    start = GUARD + (1 if misalign else 0)
    assert bool((Cbuf[:start] == 123.0).all()) and bool((Cbuf[start + C.size:] == 123.0).all())
    assert bool((ws == 0).all())      # the workspace is left zero
    return Cd.cpu().numpy(), labels.cpu().numpy(), signs.cpu().numpy(), counts.cpu().numpy()


def gpu_assign(X, C, metric, misalign=False, with_signs=True):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    N = X.shape[0]
    _, Xd = _dev_f32(X, dev, misalign)
    _, Cd = _dev_f32(C, dev, misalign)
    lbuf, labels = _guarded(N, torch.int32, dev, gen)
    sbuf, signs = _guarded(N, torch.int8, dev, gen)
    native.kmeans_assign(Xd, Cd, metric, labels, signs if with_signs else None)
    torch.cuda.synchronize()
    assert _canaries_hold(lbuf, N) and _canaries_hold(sbuf, N)
    return labels.cpu().numpy(), signs.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_run(X, C, metric, iters, misalign=False, both_forms=True):
    """The library against the restatement, bit for bit; then the other accumulation form against the first."""
    want = kc.run(X, C, metric, iters)
    got = gpu_run(X, C, metric, iters, misalign)
    assert same_bits(got[0], want[0]), "centroids"
    assert np.array_equal(got[1], want[1]), "labels"
    assert np.array_equal(got[2], want[2]), "signs"
    assert np.array_equal(got[3], want[3]), "counts"
    if both_forms:
        other = gpu_run(X, C, metric, iters, misalign, flags=native.KMEANS_GLOBAL_ATOMICS)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, other)), "global atomics differ from LDS partials"
    return got


def unit_rows(n, d, seed):
    return codebook.normalize_rows(np.random.RandomState(seed).standard_normal((n, d)).astype(F))[1]


@pytest.mark.parametrize("metric", [kc.EUCLID, kc.ABSDOT], ids=METRIC_IDS)
def test_point_count_seams(metric):
    """N around a wave (63, 64, 65), one point, and a last pass that is not full (4099 = 4 * 1024 + 3 at 4 points per lane)."""
    C = unit_rows(32, 16, 7)
    for N in (1, 63, 64, 65, 4099):
        check_run(unit_rows(N, 16, N), C, metric, 2)


@pytest.mark.parametrize("metric", [kc.EUCLID, kc.ABSDOT], ids=METRIC_IDS)
def test_every_workgroup_strides(metric):
    """More than twice as many passes as workgroups: at d = 40 a lane holds one point, a pass is 256 points and the grid stops
    at GQ_KMEANS_BLOCKS_PER_CU workgroups per CU."""
    cus = native.device_info(0)[0]
    N = 2 * native.KMEANS_BLOCKS_PER_CU * cus * native.KMEANS_THREADS + 77
    assert N <= native.KMEANS_MAX_N
    check_run(unit_rows(N, 40, 5), unit_rows(2, 40, 6), metric, 1)


@pytest.mark.parametrize("metric", [kc.EUCLID, kc.ABSDOT], ids=METRIC_IDS)
def test_dimension_seams(metric):
    """Every register layout: d below, at and between multiples of four, 4 / 2 / 1 points per lane."""
    for d in (1, 3, 8, 12, 16, 24, 32, 64):
        check_run(unit_rows(1500, d, d), unit_rows(32, d, 100 + d), metric, 2)


@pytest.mark.parametrize("metric", [kc.EUCLID, kc.ABSDOT], ids=METRIC_IDS)
def test_codebook_size_seams(metric):
    """K = 1 and 2, K = 256 (LDS partial sums at d = 16), 257 (they no longer fit: global atomics), 1024 at d = 16 (two LDS
    chunks of the codebook) and at d = 64 (five), where a late chunk must not take a tie from an early one."""
    X = unit_rows(2500, 16, 21)
    for K in (1, 2, 32, 256, 257, 1024):
        check_run(X[:700] if K == 1024 else X, unit_rows(K, 16, 300 + K), metric, 2)
    C = unit_rows(1024, 64, 22)
    C[700] = C[3]      # the same row in the first and in a later chunk: the first keeps its points
    C[1023] = C[3]
    X64 = unit_rows(300, 64, 23)
    X64[:50] = C[3] * np.linspace(0.5, 1.0, 50, dtype=F)[:, None]
    got = check_run(X64, C, metric, 1)
    assert (got[1][:50] == 3).all() and got[3][700] == 0 and got[3][1023] == 0


@pytest.mark.parametrize("metric", [kc.EUCLID, kc.ABSDOT], ids=METRIC_IDS)
def test_misaligned_views(metric):
    """X and C four bytes past a 16-byte boundary (the scalar loads), d a multiple of four and not."""
    for d in (16, 6):
        X, C = unit_rows(4099, d, 31), unit_rows(32, d, 32)
        check_run(X, C, metric, 2, misalign=True)
        want = kc.assign(X, C, metric)
        got = gpu_assign(X, C, metric, misalign=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("metric", [kc.EUCLID, kc.ABSDOT], ids=METRIC_IDS)
def test_ties_and_degenerate_rows(metric):
    nz = F(-0.0)
    C = np.array([[1, 0, 0, 0],
                  [1, nz, 0, nz],      # row 0 again (a zero's sign changes no score): always empty, keeps its -0.0 bits
                  [0, 1, 0, 0],
                  [0, 0, 1, 0],
                  [0.6, 0.8, 0, 0],
                  [0, 0, 0, 1]], F)
    tiny = F(2.0 ** -42)
    X = np.array([[1, 0, 0, 0],                 # entries exactly +-1; rows 0 and 1 tie: the lower wins
                  [-1, 0, 0, 0],                # absdot: row 0, mirrored (sign -1)
                  [0, 0, 0, 0],                 # an all-zero point: every dot is +0 -> row 0, sign +
                  [nz, nz, nz, nz],             # and with negative zeros: the chain starts from +0, so the dots are +0 again
                  [0, 0, 1, 0], [0, 0, -1, 0],  # absdot: -x is mirrored onto x, the sum is 2x
                  [0, 1, tiny, 0],              # an entry below 2^-41: q = 0
                  [0.6, 0.8, 0, 0]], F)         # a cluster of one point
    got = check_run(X, C, metric, 1)
    labels, signs, counts = got[1], got[2], got[3]
    assert labels[0] == 0 and labels[2] == 0 and labels[3] == 0 and signs[2] == 1 and signs[3] == 1
    assert counts[1] == 0 and same_bits(got[0][1], C[1])      # the higher duplicate: empty and bit-unchanged
    assert labels[7] == 4 and counts[4] == 1 and counts[5] == 0 and same_bits(got[0][5], C[5])
    assert counts.sum() == X.shape[0]
    if metric == kc.ABSDOT:
        assert labels[1] == 0 and signs[1] == -1 and labels[5] == 3 and signs[5] == -1
        assert same_bits(got[0][2], np.array([0, 1, 0, 0], F))      # (the tiny entry added nothing)
        assert same_bits(got[0][3], np.array([0, 0, 1, 0], F))
        assert same_bits(got[0][4], (np.array([0.6, 0.8, 0, 0], F).astype(np.float64)
                                      / np.sqrt(np.float64(F(0.6)) ** 2 + np.float64(F(0.8)) ** 2)).astype(F))
    else:
        assert same_bits(got[0][4], X[7])      # the mean of one point is the point
    # a row holding x and -x with S = 0: one centroid, both points orthogonal to it, so both dots are +0 and both signs +
    C2, X2 = np.array([[1, 0]], F), np.array([[0, 0.5], [0, -0.5]], F)
    got2 = check_run(X2, C2, metric, 1)
    assert got2[3].tolist() == [2] and got2[2].tolist() == [1, 1]
    # absdot: r == 0, the row is unchanged; euclid: the mean of x and -x
    assert same_bits(got2[0], C2 if metric == kc.ABSDOT else np.zeros((1, 2), F))


@pytest.fixture(scope="module")
def trajectory():
    """The restatement's 20 iterations at N = 20000, d16 K64, computed once per metric: the states after 1, 2 and 20."""
    cache = {}

    def get(metric):
        if metric not in cache:
            X = kc.unit_gaussians(20000, 16, 808)
            init = np.ascontiguousarray(codebook.initial_centroids(X, 64, 808))
            C, states = init.copy(), {}
            for it in range(1, 21):
                labels, signs, _ = kc.assign(X, C, metric)
                S, n = kc.accumulate(X, labels, signs, 64)
                C = kc.update(C, S, n, metric)
                if it in (1, 2, 20):
                    states[it] = (C.copy(), labels, signs, n)
            cache[metric] = (X, init, states)
        return cache[metric]
    return get


@pytest.mark.parametrize("iters", [1, 2, 20])
@pytest.mark.parametrize("metric", [kc.EUCLID, kc.ABSDOT], ids=METRIC_IDS)
def test_iterations_equal_the_restatement(trajectory, metric, iters):
    X, init, states = trajectory(metric)
    want = states[iters]
    got = gpu_run(X, init, metric, iters)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[3], want[3]) and got[3].sum() == X.shape[0]
    again = gpu_run(X, init, metric, iters)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again))      # two runs, the same bytes
    if iters == 2:
        # the assignment alone on the centroids one iteration made: the labels the second iteration returns
        la, sa = gpu_assign(X, states[1][0], metric)
        assert np.array_equal(la, want[1]) and np.array_equal(sa, want[2])
        assert np.array_equal(gpu_assign(X, states[1][0], metric, with_signs=False)[0], want[1])


@pytest.mark.parametrize("metric", [kc.EUCLID, kc.ABSDOT], ids=METRIC_IDS)
def test_nan_and_inf_rows_keep_labels_in_range(metric):
    X = unit_rows(3000, 16, 41)
    X[5, 3], X[77, 0], X[1000], X[2000, 15], X[2999] = np.nan, np.inf, -np.inf, -np.nan, np.nan
    C = unit_rows(64, 16, 42)
    C[10, 2] = np.nan
    for K in (64, 7):
        got = gpu_run(X, C[:K].copy(), metric, 2)
        assert got[1].min() >= 0 and got[1].max() < K and set(np.unique(got[2])) <= {-1, 1}
        la, _ = gpu_assign(X, C[:K].copy(), metric)
        assert la.min() >= 0 and la.max() < K


def test_refusals():
    """Every refusal precedes any launch: the tensors are a few elements, whatever N, d or K the call claims."""
    dev = torch.device("cuda:0")
    L = native.kmeans_lib()
    X = torch.zeros(64 * 8, dtype=torch.float32, device=dev)
    C = torch.zeros(64 * 8, dtype=torch.float32, device=dev)
    labels = torch.zeros(64, dtype=torch.int32, device=dev)
    counts = torch.zeros(64, dtype=torch.int64, device=dev)
    ws = torch.zeros(64 * 9, dtype=torch.int64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

    def run(X=X, N=8, d=8, C=C, K=8, metric=0, iters=1, labels=labels, counts=counts, ws=ws, off=0):
        return L.gq_kmeans_run(ctypes.c_void_p(X.data_ptr() + off) if X is not None else p(None), ctypes.c_int64(N), ctypes.c_int(d), p(C),
                               ctypes.c_int(K), ctypes.c_int(metric), ctypes.c_int(iters), p(labels), p(None), p(counts), p(ws), p(None))

    def assign(X=X, N=8, d=8, C=C, K=8, metric=0, labels=labels):
        return L.gq_kmeans_assign(p(X), ctypes.c_int64(N), ctypes.c_int(d), p(C), ctypes.c_int(K), ctypes.c_int(metric), p(labels),
                                  p(None), p(None))

    refused = (native.ERR_INVALID_ARG, native.ERR_UNSUPPORTED)
    for kw in (dict(X=None), dict(C=None), dict(labels=None), dict(d=0), dict(d=65), dict(K=0), dict(K=4097), dict(N=0),
               dict(N=(1 << 22) + 1), dict(metric=2), dict(metric=-1), dict(metric=7 | native.KMEANS_GLOBAL_ATOMICS)):
        assert run(**kw) in refused, kw
        assert L.gq_kmeans_last_error().decode().startswith("gq_kmeans_run"), kw
        if kw != dict(metric=7 | native.KMEANS_GLOBAL_ATOMICS):
            assert assign(**kw) in refused, kw
            assert L.gq_kmeans_last_error().decode().startswith("gq_kmeans_assign"), kw
    for kw in (dict(counts=None), dict(ws=None), dict(iters=0), dict(iters=-3), dict(off=2)):
        assert run(**kw) in refused, kw
    assert assign(metric=native.KMEANS_GLOBAL_ATOMICS) in refused      # the flag belongs to gq_kmeans_run
    torch.cuda.synchronize()
    assert run() == 0 and assign() == 0      # and the same arguments, unbroken, are accepted
    torch.cuda.synchronize()
    with pytest.raises(native.GQNativeError, match="gq_kmeans_run failed"):
        native.kmeans_run(X.view(64, 8), C.view(64, 8), 5, 1, labels, counts, ws)
