"""The contract of include/gq_kmeans.h restated in numpy (no GPU, no tolerance anywhere): steps 1 to 5 of one Lloyd iteration
with every f32 operation done one at a time, fmaf restated exactly, and the accumulation in int64 with np.add.at.
tests/test_kmeans_contract.py holds this file to the C fmaf, to scipy and to the exact mean; tests/test_gpu_kmeans_contract.py
and tests/test_gpu_kmeans_api.py hold libgq_kmeans.so to this file bit for bit."""
import numpy as np

EUCLID, ABSDOT = 0, 1
METRICS = {"euclid": EUCLID, "absdot": ABSDOT}
SCALE = 2.0 ** 40
_LOW29, _HALF29, _MAG, _ONE = np.uint64(0x1FFFFFFF), np.uint64(0x10000000), np.uint64(0x7FFFFFFFFFFFFFFF), np.uint64(1)
_SUBNORMAL_BELOW = np.uint64(((1023 - 126) << 52) - 1)      # (|s| as bits) - 1 below this: 0 < |s| < 2^-126 (zero wraps to the top)
BLOCK = 2048         # points per block of `assign` (keeps the [points, K] f64 temporaries in cache)


def fmaf(a, b, c):
    """fmaf(a, b, c) of float32 arrays (broadcast), exactly: the f64 product of two f32 is exact; the f64 sum s = p + c is
    rounded once, and rounding s to f32 equals rounding the exact p + c to f32 unless s lies on an f32 tie (halfway between two
    neighbouring f32) that the exact sum does not lie on.  There TwoSum's error term says on which side the exact sum is, and s
    is nudged by one f64 ulp towards it before the cast."""
    p = np.multiply(a, b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    s = p + c
    bits = s.view(np.uint64)
    # candidates: the 29 mantissa bits an f32 in the normal range drops say "halfway", or s is in f32's subnormal range (where
    # the f32 grid is coarser) and not zero; everything else, NaN and infinities included, is cast as it is
    cand = ((bits & _LOW29) == _HALF29) | (((bits & _MAG) - _ONE) < _SUBNORMAL_BELOW)
    if cand.any():
        idx = np.nonzero(cand)
        pc, cc, sc = np.broadcast_to(p, s.shape)[idx], np.broadcast_to(c, s.shape)[idx], s[idx]
        bb = sc - pc
        err = (pc - (sc - bb)) + (cc - bb)      # TwoSum: pc + cc = sc + err exactly
        f = sc.astype(np.float32)
        lo = f.astype(np.float64)
        other = np.nextafter(f, np.where(sc > lo, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
        tie = (lo != sc) & ((sc - lo) == (other - sc))
        nudge = tie & (err != 0)
        sc = np.where(nudge, np.nextafter(sc, np.where(err > 0, np.inf, -np.inf)), sc)
        s[idx] = sc
    with np.errstate(over="ignore"):
        return s.astype(np.float32)


def chain(A, B):
    """The fmaf chain over the last axis, ascending, from +0.0f: A, B float32 [..., d] (broadcast) -> float32 [...]."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    d = A.shape[-1]
    acc = np.zeros(np.broadcast_shapes(A.shape[:-1], B.shape[:-1]), np.float32)
    for j in range(d):
        acc = fmaf(A[..., j], B[..., j], acc)
    return acc


def half_norms(C):
    """Step 1: h_k = 0.5f * chain(c_k, c_k)."""
    return (np.float32(0.5) * chain(C, C)).astype(np.float32)


def scores(X, C, metric):
    """Step 2 -> (dot float32 [N, K], t float32 [N, K])."""
    X, C = np.asarray(X, np.float32), np.asarray(C, np.float32)
    dot = chain(X[:, None, :], C[None, :, :])
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.abs(dot) if metric == ABSDOT else (dot - half_norms(C)[None, :]).astype(np.float32)
    return dot, t


def labels_of(t):
    """Step 3's walk: k ascending, strict `>`, starting with k = 0 (NaN never wins and never loses its place)."""
    N, K = t.shape
    best, label = t[:, 0].copy(), np.zeros(N, np.int32)
    for k in range(1, K):
        with np.errstate(invalid="ignore"):
            m = t[:, k] > best
        best[m] = t[m, k]
        label[m] = k
    return label


def assign(X, C, metric, with_scores=False):
    """Steps 1 to 3 -> labels int32 [N], signs int8 [N], dot float32 [N] (dot_{i,label_i}) [, t float32 [N, K]]."""
    X = np.asarray(X, np.float32)
    N = X.shape[0]
    labels, signs, dots, ts = np.empty(N, np.int32), np.empty(N, np.int8), np.empty(N, np.float32), []
    for a in range(0, N, BLOCK):
        dot, t = scores(X[a:a + BLOCK], C, metric)
        lab = labels_of(t)
        dl = dot[np.arange(lab.size), lab]
        labels[a:a + BLOCK], dots[a:a + BLOCK] = lab, dl
        with np.errstate(invalid="ignore"):
            signs[a:a + BLOCK] = np.where((dl < 0) & (metric == ABSDOT), -1, 1)
        if with_scores:
            ts.append(t)
    return (labels, signs, dots, np.concatenate(ts)) if with_scores else (labels, signs, dots)


def quantise(X):
    """q_ij = __double2ll_rn((double)x_ij * 0x1p40): the product is exact, np.rint rounds to nearest even."""
    return np.rint(np.asarray(X, np.float32).astype(np.float64) * SCALE).astype(np.int64)


def accumulate(X, labels, signs, K):
    """Step 4 -> (S int64 [K, d], n int64 [K])."""
    S, n = np.zeros((K, X.shape[1]), np.int64), np.zeros(K, np.int64)
    np.add.at(S, labels, quantise(X) * signs.astype(np.int64)[:, None])
    np.add.at(n, labels, 1)
    return S, n


def update(C, S, n, metric):
    """Step 5 -> the new centroids (float32 [K, d]); rows with n_k == 0 (or, absdot, r == 0) keep their bits."""
    out = np.array(C, dtype=np.float32, copy=True)
    f = S.astype(np.float64)
    if metric == EUCLID:
        live = n != 0
        out[live] = (f[live] / (n[live].astype(np.float64) * SCALE)[:, None]).astype(np.float32)
    else:
        ss = np.zeros(S.shape[0], np.float64)
        for j in range(S.shape[1]):
            ss = ss + f[:, j] * f[:, j]
        r = np.sqrt(ss)
        live = (n != 0) & (r != 0)
        out[live] = (f[live] / r[live][:, None]).astype(np.float32)
    return out


def run(X, C, metric, iters):
    """gq_kmeans_run -> (C after `iters` iterations, labels, signs, counts of the last assignment)."""
    X, C = np.asarray(X, np.float32), np.array(C, dtype=np.float32, copy=True)
    for _ in range(iters):
        labels, signs, _ = assign(X, C, metric)
        S, n = accumulate(X, labels, signs, C.shape[0])
        C = update(C, S, n, metric)
    return C, labels, signs, n


def unit_gaussians(N, d, seed):
    """Row-normalised Gaussians as gq_amd.codebook.train_points makes them."""
    from gq_amd.codebook import train_points
    return train_points(d, N, seed)


def inertia(X, C, labels):
    """sum_i |x_i - c_label_i|^2 in f64."""
    diff = np.asarray(X, np.float64) - np.asarray(C, np.float64)[labels]
    return float(np.sum(diff * diff))
