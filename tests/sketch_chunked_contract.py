"""The chunked recovery of include/gq_sketch.h (CHUNKED RECOVERY) in numpy: tests/sketch_contract.py's decode_mean with the kept set
taken per item of 4,096 elements, len // cr of each by tests/topk_contract.py's key and tie rule.  Everything else is that module's."""
import numpy as np

import sketch_contract as sc
import topk_contract as tc


def decode_mean(payloads, n, cr, seed, E=None):
    T = sc.mean_table(payloads, E)
    est = sc.estimates(T, n, seed)
    out = np.zeros(n, sc.f32)
    for a in range(0, n, sc.CHUNK):
        idx = a + tc.kept(est[a:a + sc.CHUNK], min(sc.CHUNK, n - a) // cr)
        out[idx] = est[idx]
    if E is None:
        return out, None
    with np.errstate(invalid="ignore", over="ignore"):
        return out, (T - sc.sketch(out, seed, T.shape[0], T.shape[1])).astype(sc.f32).reshape(-1)
