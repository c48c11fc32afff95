"""Time one Lloyd iteration of libgq_kmeans.so (gq_kmeans_run, iters = 1) on one MI355X at the size the reference's generator
trains at, next to the host's scipy:

    python tools/kmeans_time.py [--out FILE] [--n N]      (default: profiles/kmeans_time.jsonl, N = 1,000,000)

One JSON line per case (d16 K256 and d16 K64, both metrics):
  run_us                 the whole call: the zero launch, the assignment with per-workgroup LDS partial sums, the update
  run_global_atomics_us  the same with GQ_KMEANS_GLOBAL_ATOMICS: every point adds into the workspace directly (the same bits)
  assign_us              gq_kmeans_assign alone (no accumulation)
  fma_TFLOPs             2 * N * K * d over run_us: the assignment's multiply-adds alone, as a rate
  scipy_ms               scipy.cluster.vq.kmeans2(X, init, iter=1, minit='matrix') on the same points on the host (euclid only:
                         it is the only thing to compare with, the feature has no earlier version)
Times: HIP events around a window of back-to-back calls after untimed ones, median of the windows.  The centroids are
restored between windows, not between calls: a call moves them, and the next call's work is the same size."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))

from gq_amd import codebook, native  # noqa: E402


def timed(fn, reset, iters=20, warm=5, windows=5):
    reset()
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(windows):
        reset()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        res.append(s.elapsed_time(e) / iters * 1e3)
    return sorted(res)[len(res) // 2]


def case(dev, X_host, d, K, metric):
    N = X_host.shape[0]
    init = np.ascontiguousarray(codebook.initial_centroids(X_host, K, 808))
    X, C0 = torch.from_numpy(X_host).to(dev), torch.from_numpy(init).to(dev)
    C = C0.clone()
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    counts = torch.empty(K, dtype=torch.int64, device=dev)
    ws = torch.empty(native.kmeans_workspace_bytes(K, d) // 8, dtype=torch.int64, device=dev)
    m = native.KMEANS_METRICS[metric]
    reset = lambda: C.copy_(C0)
    row = {"case": "lloyd_iteration", "N": N, "d": d, "K": K, "metric": metric}
    row["run_us"] = round(timed(lambda: native.kmeans_run(X, C, m, 1, labels, counts, ws), reset), 1)
    row["run_global_atomics_us"] = round(timed(lambda: native.kmeans_run(X, C, m | native.KMEANS_GLOBAL_ATOMICS, 1, labels, counts, ws),
                                               reset), 1)
    row["assign_us"] = round(timed(lambda: native.kmeans_assign(X, C, m, labels), reset), 1)
    row["fma_TFLOPs"] = round(2.0 * N * K * d / (row["run_us"] * 1e-6) / 1e12, 2)
    if metric == "euclid":
        from scipy.cluster.vq import kmeans2
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            kmeans2(X_host, init.copy(), iter=1, minit="matrix")
            ts.append(time.perf_counter() - t)
        row["scipy_ms"] = round(sorted(ts)[1] * 1e3, 1)
        row["scipy_over_run"] = round(row["scipy_ms"] * 1e3 / row["run_us"], 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_time.jsonl"))
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/kmeans_time.py measures on an MI355X: no GPU here")
    dev = torch.device("cuda:0")
    X = codebook.train_points(16, a.n, 808)
    rows = [case(dev, X, 16, K, metric) for K in (256, 64) for metric in ("euclid", "absdot")]
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
