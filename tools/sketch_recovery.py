"""The README's table of the count sketch's recovery error, on the CPU restatement (tests/sketch_contract.py; no GPU):

    python tools/sketch_recovery.py

The relative L2 error of the decode against the true top-k of the mean: unit Gaussian noise per user plus the same 1 % heavy hitters of
+-10 in every user, n = 200,704, sketch_cr = 2, k = the number of heavy hitters, R = 1 / 8 users, 1 / 3 / 5 rows, fixed seeds.  One JSON
line."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import sketch_contract as sc  # noqa: E402
import topk_contract as tc  # noqa: E402


def main():
    n, C, k = 256 * 784, 2, 256 * 784 // 100
    table = {}
    for R in (1, 8):
        rs = np.random.RandomState(100 + R)
        h = np.zeros(n, np.float32)      # (the users share the heavy hitters: the mean keeps them, the noise averages out)
        h[rs.permutation(n)[:n // 100]] = np.float32(10.0) * np.sign(rs.standard_normal(n // 100)).astype(np.float32)
        users = [(rs.standard_normal(n).astype(np.float32) + h).astype(np.float32) for _ in range(R)]
        target = tc.dense(np.mean(np.stack(users).astype(np.float64), 0).astype(np.float32), k)
        for rows in (1, 3, 5):
            out, _ = sc.decode_mean([sc.sketch(g, 3, rows, sc.layout(n, rows, C)[1]) for g in users], n, k, 3)
            table["R%d_rows%d" % (R, rows)] = round(float(np.linalg.norm(out.astype(np.float64) - target) / np.linalg.norm(target.astype(np.float64))), 3)
    print(json.dumps({"case": "sketch_recovery", "n": n, "sketch_cr": C, "k": k, "relative_l2": table}))


if __name__ == "__main__":
    main()
