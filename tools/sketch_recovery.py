"""The README's table of the count sketch's recovery error, on the CPU restatement (tests/sketch_contract.py and, for
--sketch-recover chunked, tests/sketch_chunked_contract.py; no GPU):

    python tools/sketch_recovery.py

The relative L2 error of the decode against the true top-k of the mean: unit Gaussian noise per user plus the same 1 % heavy hitters of
+-10 in every user, n = 200,704, sketch_cr = 2, k = the number of heavy hitters (cr = 100: the chunked recovery keeps 40 of every item,
1,960 in all, against 2,007), R = 1 / 8 users, 1 / 3 / 5 rows, fixed seeds.  One JSON line."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import sketch_chunked_contract as scc  # noqa: E402
import sketch_contract as sc  # noqa: E402
import topk_contract as tc  # noqa: E402

N, C, CR = 256 * 784, 2, 100


def tables():
    """-> {"global": {"R1_rows1": ...}, "chunked": {...}}"""
    k = N // CR
    out = {"global": {}, "chunked": {}}
    for R in (1, 8):
        rs = np.random.RandomState(100 + R)
        h = np.zeros(N, np.float32)      # (the users share the heavy hitters: the mean keeps them, the noise averages out)
        h[rs.permutation(N)[:k]] = np.float32(10.0) * np.sign(rs.standard_normal(k)).astype(np.float32)
        users = [(rs.standard_normal(N).astype(np.float32) + h).astype(np.float32) for _ in range(R)]
        target = tc.dense(np.mean(np.stack(users).astype(np.float64), 0).astype(np.float32), k)
        norm = np.linalg.norm(target.astype(np.float64))
        for rows in (1, 3, 5):
            payloads = [sc.sketch(g, 3, rows, sc.layout(N, rows, C)[1]) for g in users]
            for name, dec in (("global", sc.decode_mean(payloads, N, k, 3)[0]), ("chunked", scc.decode_mean(payloads, N, CR, 3)[0])):
                out[name]["R%d_rows%d" % (R, rows)] = round(float(np.linalg.norm(dec.astype(np.float64) - target) / norm), 3)
    return out


def main():
    t = tables()
    print(json.dumps({"case": "sketch_recovery", "n": N, "sketch_cr": C, "k": N // CR, "relative_l2": t["global"],
                      "relative_l2_chunked": t["chunked"]}))


if __name__ == "__main__":
    main()
