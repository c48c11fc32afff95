"""The contract of include/gq_dgc.h restated in numpy, one float32 operation at a time (no GPU, no call into gq_amd), on
tests/topk_contract.py for the select and the wire, and the inputs the DGC tests share: tests/test_dgc_contract.py checks the
restatement against independent witnesses and asserts what every input claims about itself, tests/test_gpu_dgc_contract.py and
tests/test_gpu_dgc_api.py hold the kernels and the quantizer to it.

    t = m * u_old;  u1 = t + g;  v1 = v_old + u1
    kept, section, decoded = gq_topk.h's rule applied to v1
    v_new = v1 - decoded;  u_new = kept ? +0 : u1

Which NaN an operation yields (sign, payload) is not part of the contract: `canon` maps every NaN to one pattern, and the tests
compare np.array_equal on canonical bits -- of u, v and the wire's values, all of which are results of arithmetic here."""
import numpy as np

import topk_contract as tc

CHUNK = tc.CHUNK
QNAN = np.uint32(0x7fc00000)


def canon(a):
    """uint32 bits of float32 `a`, every NaN as QNAN."""
    a = tc.f32(a)
    return np.where(np.isnan(a), QNAN, a.view(np.uint32))


def canon_section(sec, k):
    """A wire section (uint8[8k]) as uint32[2k]: the indices as they are, the values' NaNs as QNAN."""
    idx, val = tc.split_section(sec, k)
    return np.concatenate([idx, canon(val)])


def record(g, u, v, m, k):
    """One record of one tensor -> (section bytes, u_new, v_new, kept indices, v1)."""
    g, u, v = tc.f32(g), tc.f32(u), tc.f32(v)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = (np.float32(m) * u).astype(np.float32)
        u1 = (t + g).astype(np.float32)
        v1 = (v + u1).astype(np.float32)
        order = tc.ranking(v1)
        idx = tc.kept(v1, k, order)
        sec = tc.section_bytes(v1, k, order)
        v_new = (v1 - tc.dense(v1, k, order)).astype(np.float32)
    u_new = u1.copy()
    u_new[idx] = np.float32(0.0)
    return sec, u_new, v_new, idx, v1


class State(object):
    """u and v of one user for a list of tensors, stepped record by record.  u0 / v0: carried state to start from (default +0)."""

    def __init__(self, sizes, ks, m, u0=None, v0=None):
        self.sizes, self.ks, self.m = list(sizes), list(ks), m
        self.u = [tc.f32(a).copy() for a in u0] if u0 is not None else [np.zeros(n, np.float32) for n in sizes]
        self.v = [tc.f32(a).copy() for a in v0] if v0 is not None else [np.zeros(n, np.float32) for n in sizes]
        self.kept = self.v1 = None

    def record(self, gs):
        """-> the tensors' section bytes"""
        out = [record(g, u, v, self.m, k) for g, u, v, k in zip(gs, self.u, self.v, self.ks)]
        self.u, self.v = [o[1] for o in out], [o[2] for o in out]
        self.kept, self.v1 = [o[3] for o in out], [o[4] for o in out]
        return [o[0] for o in out]


# ---- the inputs the tests share ------------------------------------------------------------------------------------------
STEPS = 3
MOMENTA = [0.0, 0.5, 0.9]
SEAM_SIZES = [1001, 4096, 4097, 8193, 12289]      # one item, one full item, one element into the second, ... the fourth
SEAM_CR = 16


def untied(n, seed):
    """STEPS gradients of n distinct magnitudes each, drawn so that NO two |v1| of any step tie for m in MOMENTA and any of the
    k the tests use (tests/test_dgc_contract.py asserts it): heavy-tailed, the magnitudes spread over many binades."""
    return [tc.heavy_tailed(n, seed + 17 * s) for s in range(STEPS)]


def seam_case():
    """-> (sizes, ks, [the STEPS lists of gradients])"""
    gs = [untied(n, 1000 + n) for n in SEAM_SIZES]
    return SEAM_SIZES, [n // SEAM_CR for n in SEAM_SIZES], [[g[s] for g in gs] for s in range(STEPS)]


# k = 0 (cr > n), k = 1 (cr = n), k = n (cr = 1) and k = 6144 of 12289 (cr = 2): the mask launch has work in two workgroups
K_SIZES = [1500, 1500, 5000, 12289]
K_CRS = [1501, 1500, 1, 2]


def k_case():
    gs = [untied(n, 2000 + 31 * j) for j, n in enumerate(K_SIZES)]
    return K_SIZES, [n // cr for n, cr in zip(K_SIZES, K_CRS)], [[g[s] for g in gs] for s in range(STEPS)]


TIE_SIZE = 8193
TIE_LAST = 4100      # the last kept tie of the first record: the kept ties straddle the seam between items 0 and 1 (index 4096)


def tie_case():
    """One tensor of +-1.0 with 2.0 on one element in sixteen, the SAME gradient every step; k makes index TIE_LAST the last kept
    1.0 of the first record (u = v = 0: v1 = g), so ties on both sides of index 4096 are kept and ties behind TIE_LAST are not."""
    g = tc.two_level(TIE_SIZE, 3000, edges=(4095, 4096, 4097, TIE_LAST, TIE_LAST + 1))
    k = tc.k_for_last_tie(g, tc.ONE, TIE_LAST)
    return [TIE_SIZE], [k], [[g] for _ in range(STEPS)]


SPECIAL_SIZE = 5003
SPECIAL_K = 40


def special_case():
    """-> (sizes, ks, gradients per step, u0, v0): +-0, subnormals, +-inf and NaNs of several patterns in every gradient and in the
    carried state, at positions of their own and on top of one another."""
    rs = np.random.RandomState(4000)
    n = SPECIAL_SIZE

    def sprinkle(a, seed):
        r = np.random.RandomState(seed)
        b = tc.bits(a).copy()
        pos = r.permutation(n)
        b[pos[:60]] = tc._signs(r, 60)                                                   # +-0
        b[pos[60:160]] = r.randint(1, 0x800000, size=100).astype(np.uint32) | tc._signs(r, 100)      # subnormals
        b[pos[160:166]] = np.where(r.rand(6) < 0.5, np.uint32(0x7f800000), np.uint32(0xff800000))      # +-inf
        b[pos[166:173]] = tc.NANS
        return tc.from_bits(b)

    gs = [[sprinkle(rs.standard_normal(n).astype(np.float32), 4100 + s)] for s in range(STEPS)]
    u0 = [sprinkle(rs.standard_normal(n).astype(np.float32), 4200)]
    v0 = [sprinkle(rs.standard_normal(n).astype(np.float32), 4300)]
    return [n], [SPECIAL_K], gs, u0, v0


MANY = 70


def many_case():
    sizes = [1001 + 67 * j for j in range(MANY)]      # 1001 ... 5624: one and two items
    gs = [untied(n, 5000 + j) for j, n in enumerate(sizes)]
    return sizes, [n // 64 for n in sizes], [[g[s] for g in gs] for s in range(STEPS)]


FCN_SHAPES = [(256, 784), (256,), (10, 256), (10,)]      # driver.FCN's parameters: two compressed tensors, two dense ones


def fcn_grads(users, steps, seed=6000):
    """grads[step][user][parameter]"""
    return [[[tc.heavy_tailed(int(np.prod(s)), seed + 1000 * t + 100 * u + j).reshape(s) for j, s in enumerate(FCN_SHAPES)]
             for u in range(users)] for t in range(steps)]
