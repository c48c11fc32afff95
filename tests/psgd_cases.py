"""The shapes, ranks and inputs the low-rank compressor's GPU contract tests record (tests/test_gpu_psgd_contract.py), shared with the
CPU file that holds the restatement to float64 on them and checks that the mutations change bits there (tests/test_psgd_contract.py)."""
import numpy as np

import psgd_contract as pc

f32 = np.float32

# rows shorter than a wave, a multiple of it, across two and three pieces, many rows per item and a row count off every block
# size, the three ranks on one shape, n or m equal to r, a tensor of more than two dimensions
CASES = [((33, 31), 2), ((32, 32), 4), ((4, 251), 4), ((251, 4), 4), ((5, 4097), 4), ((2, 8193), 2), ((2, 8193), 1), ((4099, 3), 2),
         ((257, 129), 1), ((257, 129), 2), ((257, 129), 4), ((4, 300), 4), ((300, 4), 4), ((2, 600), 2), ((1, 1100), 1), ((1100, 1), 1),
         ((3, 5, 70), 2)]
# a single row or a single column at rank 1: what the mutation checks cannot ask everything of (see test_psgd_contract.py)
SINGLE = [((1, 1100), 1), ((1100, 1), 1)]
CASE_IDS = ["%s-r%d" % ("x".join(map(str, s)), r) for s, r in CASES]


def mats(shapes, seed, scale=1.0):
    """One N(0, scale) matrix per shape, from one stream."""
    rs = np.random.RandomState(seed)
    return [(rs.standard_normal(pc.matrix_of(s)) * scale).astype(f32) for s in shapes]
