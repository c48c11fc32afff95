"""Codebook files: the reference's `.fvecs` wire format and row normalisation.

Host-side, one-off per compressor (the reference does this in NumPy too):
  * fvecs:  a little-endian int32 stream, one row = [d | d x float32]
            (reference utils/vecs_io.py:5-12)
  * rows are L2-normalised in float32, zero rows stay zero (utils/vec_np.py:4-10)
  * file name  codebooks/learned_codebook/angular_dim_{d}_Ks_{K}.fvecs, looked up
    relative to the cwd first, exactly like the reference
    (compressors/nearest_neighbor_compressor.py:50-51), then in $GQ_CODEBOOK_DIR,
    then in the copies shipped with this package (K = 256 for d = 8, 16 and 32: gq_amd/data/codebooks).

Any other (d, K) is trained on the device (the reference's codebook_generator.py runs scipy's kmeans2 on the host):
`train_codebook`, or from a shell

    python -m gq_amd.codebook --dim 16 --ks 64 [--metric euclid|absdot] [--iters 20] [--train-size 1000000] [--seed 808] --out DIR

which writes DIR/learned_codebook/angular_dim_16_Ks_64.fvecs; GQ_CODEBOOK_DIR=DIR then makes `codebook_path` find it.
"""
import os

import numpy as np

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "codebooks")


def read_fvecs(path):
    raw = np.fromfile(path, dtype="<i4")
    if raw.size == 0:
        raise ValueError("empty fvecs file: %s" % path)
    d = int(raw[0])
    if d <= 0 or raw.size % (d + 1) != 0:
        raise ValueError("malformed fvecs file %s (leading dimension %d, %d words)" % (path, d, raw.size))
    rows = raw.reshape(-1, d + 1)
    if not np.all(rows[:, 0] == d):
        raise ValueError("malformed fvecs file %s: inconsistent row dimensions" % path)
    return np.ascontiguousarray(rows[:, 1:]).view(np.float32)


def write_fvecs(path, array):
    """The inverse of read_fvecs: float32 [n, d] -> n rows of [d | d x float32].  The file is replaced, never appended to
    (the reference's writer appends, which is where its double-written files come from)."""
    a = np.ascontiguousarray(array, dtype="<f4")
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_fvecs needs a non-empty [n, d] array, got shape %s" % (a.shape,))
    rows = np.empty((a.shape[0], a.shape[1] + 1), dtype="<i4")
    rows[:, 0] = a.shape[1]
    rows[:, 1:] = a.view("<i4")
    with open(path, "wb") as f:
        f.write(rows.tobytes())


def normalize_rows(vecs):
    """Row-wise v / ||v||_2 in float32; rows with zero norm are returned as zeros."""
    vecs = np.asarray(vecs, dtype=np.float32)
    norms = np.sqrt(np.add.reduce(vecs * vecs, axis=1))
    col = norms[:, None]
    out = np.zeros_like(vecs)
    np.divide(vecs, col, out=out, where=col != 0)
    return norms, out


def codebook_path(dim, K):
    rel = os.path.join("learned_codebook", "angular_dim_%d_Ks_%d.fvecs" % (dim, K))
    tried = []
    for base in (os.path.join(".", "codebooks"), os.environ.get("GQ_CODEBOOK_DIR"), _DATA):
        if not base:
            continue
        p = os.path.join(base, rel)
        tried.append(p)
        if os.path.exists(p):
            return p
    raise FileNotFoundError("no codebook for dim=%d K=%d; looked in %s" % (dim, K, ", ".join(tried)))


def load_codebook(dim, K):
    """-> float32 [K, dim], row-normalised, as the reference builds `self.codewords`."""
    cb = read_fvecs(codebook_path(dim, K))
    if cb.shape != (K, dim):
        # the reference tree has a few double-written files (append-mode writer); the
        # reference would fail later on those, we fail here with a clear message
        raise ValueError("codebook %s has shape %s, expected (%d, %d)" % (codebook_path(dim, K), cb.shape, K, dim))
    return normalize_rows(cb)[1]


def repaired_dim(size, c_dim):
    """The reference's sub-dimension choice (nearest_neighbor_compressor.py:23-29,
    qsgd_compressor.py:15-22): whole tensor if c_dim == 0 or size < c_dim, else c_dim
    grown by x1.5 up to ten times until it divides `size`."""
    if c_dim == 0 or size < c_dim:
        return size
    dim = c_dim
    for _ in range(10):
        if size % dim != 0:
            dim = dim // 2 * 3
    return dim


def train_points(dim, train_size, seed):
    """The reference generator's points: RandomState(seed).normal(0, 1, (train_size, dim)) as float32, rows normalised."""
    return normalize_rows(np.random.RandomState(seed).normal(0, 1, (train_size, dim)).astype(np.float32))[1]


def initial_centroids(points, K, seed):
    """K distinct rows of `points` (scipy kmeans2's minit='points' in spirit): points[RandomState(seed).choice(N, K, replace=False)]."""
    return points[np.random.RandomState(seed).choice(points.shape[0], K, replace=False)]


def train_codebook(dim, K, train_size=1_000_000, iters=20, seed=808, metric="euclid", points=None, device=None):
    """-> float32 [K, dim]: `iters` Lloyd iterations of libgq_kmeans.so (include/gq_kmeans.h defines every bit) on the device.

    metric "euclid" is the reference's objective (the cluster mean); "absdot" is the one HSQ encodes with (the largest
    |<c, v>|, points of negative projection mirrored, unit-length centroids).  points=None: the reference generator's unit
    Gaussians (train_points); otherwise a float32 [N, dim] tensor or array, on the host or the device, whose rows are normalised
    and whose zero rows are dropped.  There is no CPU fallback: without a GPU this raises GQNativeError."""
    import torch
    from . import native
    if metric not in native.KMEANS_METRICS:
        raise ValueError("metric must be one of %s, got %r" % (sorted(native.KMEANS_METRICS), metric))
    if points is None:
        pts = train_points(dim, train_size, seed)
    else:
        pts = points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else np.asarray(points)
        if pts.dtype != np.float32 or pts.ndim != 2 or pts.shape[1] != dim:
            raise ValueError("points must be float32 [N, %d], got %s %s" % (dim, pts.dtype, pts.shape))
        norms, pts = normalize_rows(pts)
        pts = np.ascontiguousarray(pts[norms != 0])
    N = pts.shape[0]
    if not 1 <= K <= N:
        raise ValueError("K = %d centroids need at least as many non-zero points, got %d" % (K, N))
    init = np.ascontiguousarray(initial_centroids(pts, K, seed))
    if not torch.cuda.is_available():
        raise native.GQNativeError("train_codebook runs on the HIP kernels of libgq_kmeans.so: no GPU is available (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        X, C = torch.from_numpy(pts).to(dev), torch.from_numpy(init).to(dev)
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        counts = torch.empty(K, dtype=torch.int64, device=dev)
        workspace = torch.empty(native.kmeans_workspace_bytes(K, dim) // 8, dtype=torch.int64, device=dev)
        native.kmeans_run(X, C, native.KMEANS_METRICS[metric], iters, labels, counts, workspace)
        return C.cpu().numpy()


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m gq_amd.codebook", description="Train an HSQ codebook on the device and write it as "
                                 "DIR/learned_codebook/angular_dim_D_Ks_K.fvecs (GQ_CODEBOOK_DIR=DIR makes the compressors find it).")
    ap.add_argument("--dim", type=int, required=True)
    ap.add_argument("--ks", type=int, required=True)
    ap.add_argument("--metric", choices=("euclid", "absdot"), default="euclid")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train-size", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=808)
    ap.add_argument("--out", required=True, metavar="DIR")
    ap.add_argument("--force", action="store_true", help="replace an existing file")
    a = ap.parse_args(argv)
    if a.dim < 1 or a.ks < 1 or a.iters < 1 or a.train_size < a.ks:
        ap.error("--dim, --ks and --iters must be at least 1, and --train-size at least --ks")
    path = os.path.join(a.out, "learned_codebook", "angular_dim_%d_Ks_%d.fvecs" % (a.dim, a.ks))
    if os.path.exists(path) and not a.force:      # (before any work: training takes seconds, the refusal none)
        ap.error("%s exists; pass --force to replace it" % path)
    cb = train_codebook(a.dim, a.ks, train_size=a.train_size, iters=a.iters, seed=a.seed, metric=a.metric)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    write_fvecs(path, cb)
    print(path)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
