"""The low-rank compressor's contract on the CPU: the wire layout and sizes, which tensors are compressed, the numpy restatement of
include/gq_psgd.h (tests/psgd_contract.py) against an independent float64 witness, what the algorithm promises (orthonormal Ph, the
power iteration's convergence from the warm start, the error feedback's 1/T law, the zero-gradient rule), the README's figures, and
the mutation checks: every departure from the header's order the GPU tests are meant to catch changes bits on their inputs."""
import json
import math
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "gradient-quantization_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import psgd_contract as pc  # noqa: E402
from psgd_cases import CASES, CASE_IDS, SINGLE, mats as _mats  # noqa: E402  (the GPU cases' shapes and inputs)

f32, u32, f64 = np.float32, np.uint32, np.float64
U = pc.U


def _args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=1, mode="ps",
                psgd_rank=2, psgd_seed=0)
    base.update(kw)
    return Namespace(**base)


def _resnet50_shapes():
    with open(os.path.join(HERE, "golden", "resnet50_cifar_shapes.json")) as f:
        return [tuple(s) for s in json.load(f)["parameter_shapes"]]


RESNET50_BYTES = {1: 538_928, 2: 864_448, 4: 1_515_488}      # one user's wire; dense float32: 94,083,376


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def test_wire_layout_and_section_sizes():
    from gq_amd.codecs import psgd_section_bytes
    assert psgd_section_bytes(33, 31, 2) == pc.section_nbytes(33, 31, 2) == 528      # 16 + 8 * 64
    assert psgd_section_bytes(5, 4097, 1) == 16 + 4 * 4102 + 8                        # padded to 16
    assert psgd_section_bytes(257, 129, 4) == 16 + 16 * 386
    rs = np.random.RandomState(0)
    Ph, Qn = rs.standard_normal((5, 1)).astype(f32), rs.standard_normal((6, 1)).astype(f32)
    sec = pc.section(Ph, Qn)
    assert sec.size == 64 and list(sec[:16].view(u32)) == [5, 6, 1, 0]
    assert np.array_equal(sec[16:36].view(f32), Ph[:, 0]) and np.array_equal(sec[36:60].view(f32), Qn[:, 0]) and not sec[60:].any()
    a, b = pc.parse(sec, 5, 6, 1)
    assert np.array_equal(a, Ph) and np.array_equal(b, Qn)
    # the README's figures: one user's ResNet-50 wire -- the compressed tensors as 16-byte aligned sections, the others behind
    # them as packed float32 (the quantizer's layout)
    shapes = _resnet50_shapes()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for r, want in RESNET50_BYTES.items():
        off = 0
        for s in shapes:
            if pc.compresses(s, r):
                off = (off + psgd_section_bytes(*pc.matrix_of(s), r) + 15) // 16 * 16
        total = (off + 4 * sum(int(np.prod(s)) for s in shapes if not pc.compresses(s, r)) + 15) // 16 * 16
        assert total == want
        assert "{:,}".format(want) in readme
    assert sum(pc.compresses(s, 4) for s in shapes) == 54


def test_quantizer_lays_the_resnet50_wire_out_as_computed():
    from gq_amd.codecs import BatchedPowerSGD, DenseCodec, PowerSGDCodec
    from gq_amd.compressors import PowerSGDCompressor
    from gq_amd.quantizers import PSQuantizer
    shapes = _resnet50_shapes()
    for r, want in RESNET50_BYTES.items():
        params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
        q = PSQuantizer(PowerSGDCompressor, params, _args(psgd_rank=r, two_phase=(r == 2)))
        assert q.wire_bytes_per_user() == want
        assert [g[0] for g in q._groups] == [BatchedPowerSGD] and len(q._groups[0][1]) == 54
        assert all(type(c) is (PowerSGDCodec if pc.compresses(s, r) else DenseCodec) for c, s in zip(q.codecs, shapes))
        # the warm starts: Q0 of (seed, parameter index, user), the server's under its own key
        i = q._groups[0][1][3]
        n, m = pc.matrix_of(shapes[i])
        assert np.array_equal(params[i].psgd_q[0].numpy(), pc.q0(0, i, 0, m, r))
        if r == 2:
            assert np.array_equal(params[i].psgd_server_q.numpy(), pc.q0(0, i, pc.SERVER_USER, m, r))
        ws = q.warm_starts()
        assert sorted(ws) == q._groups[0][1]
        ws[i]["users"][0] = ws[i]["users"][0] + 1
        ptr = params[i].psgd_q[0].data_ptr()
        q.set_warm_starts(ws)
        assert params[i].psgd_q[0].data_ptr() == ptr and np.array_equal(params[i].psgd_q[0].numpy(), pc.q0(0, i, 0, m, r) + f32(1))
        with pytest.raises(ValueError, match="set_warm_starts"):
            q.set_warm_starts({0: ws[i]})


def test_which_tensors_are_compressed():
    from gq_amd.codecs import DenseCodec, PowerSGDCodec, quantizer_codec_factory
    from gq_amd.compressors import PowerSGDCompressor
    for shape, r, want in [((1, 1001), 2, False), ((1001, 1), 2, False), ((2, 501), 2, False), ((2048,), 2, False),      # (the default rank)
                           ((1, 1001), 1, False), ((1001, 1), 1, False), ((2, 501), 1, True), ((2048,), 1, False), ((2048,), 4, False), ((10, 100), 2, False), ((11, 100), 2, True), ((3, 400), 4, False), ((4, 400), 4, False),
                           ((8, 400), 4, True), ((64, 3, 7, 7), 4, True), ((256, 784), 4, True), ((10, 256), 4, True)]:
        n = int(np.prod(shape))
        c = PowerSGDCompressor(n, shape, _args(psgd_rank=r))
        assert c.compresses == pc.compresses(shape, r) == want, (shape, r)
        assert type(quantizer_codec_factory(c, n, shape)) is (PowerSGDCodec if want else DenseCodec)
    q0 = pc.q0(3, 5, 2, 40, 4)
    assert q0.min() >= -1 and q0.max() < 1 and len(np.unique(q0)) > 150 and np.linalg.matrix_rank(q0.astype(f64)) == 4
    from gq_amd.codecs import psgd_q0
    assert np.array_equal(psgd_q0(3, 5, 2, 40, 4).numpy(), q0) and not np.array_equal(q0, pc.q0(3, 5, 3, 40, 4))


# ---- the restatement against float64 -------------------------------------------------------------------------------------------
def _chain_bounds(n, m, r):
    """First-order relative error bounds (in units of U) of the header's four products, each relative to the product of the
    operands' norms: a strided chain of ceil(L / 256) fused steps, the tree's 8 additions, the folds of pieces / blocks."""
    pieces = -(-m // pc.PIECE)
    g_proj = -(-min(m, pc.PIECE) // 256) + 8 + (pieces - 1)
    g_dot = -(-n // 256) + 8
    g_back = min(n, pc.ROW_BLOCK) + (-(-n // pc.ROW_BLOCK) - 1)
    return g_proj, g_dot, g_back, r


@pytest.mark.parametrize("shape,r", CASES, ids=CASE_IDS)
def test_restatement_against_float64(shape, r):
    """On every GPU test input.  D = Ph Ph^T M is a projection of M onto span(M Q); with kappa = |M|_F |Q|_F / sigma_min(M Q) (from
    the float64 witness: a property of the input) a relative perturbation eps of P moves the projector by at most kappa * eps to first
    order.  eps: the projection's chain, then per Gram-Schmidt column at most r - 1 dots, one norm, one division (3 roundings) each;
    the back-projection and the final product add their own chains without the kappa.  Factor 2 for the second-order terms."""
    n, m = pc.matrix_of(shape)
    for seed in (100, 101, 102):
        M = _mats([shape], seed)[0]
        Q = pc.q0(77, 0, 0, m, r)
        rec = pc.record(M, Q, Q)
        Pw, Qw, Dw = pc.witness(M, Q)
        sv = np.linalg.svd(M.astype(f64) @ Q.astype(f64), compute_uv=False)
        kappa = np.linalg.norm(M.astype(f64)) * np.linalg.norm(Q.astype(f64)) / sv[-1]
        g_proj, g_dot, g_back, g_out = _chain_bounds(n, m, r)
        bound_d = 2 * U * (kappa * (g_proj + r * (g_dot + 3)) + g_back + g_out) * math.sqrt(r)
        diff = np.linalg.norm(rec.D.astype(f64) - Dw) / np.linalg.norm(Dw)
        assert diff <= bound_d, (diff, bound_d)
        # Ph^T Ph = I: modified Gram-Schmidt loses orthogonality by at most kappa(P) * eps per pair of columns
        kp = sv[0] / sv[-1]
        bound_o = 2 * U * (kp * r * (g_dot + 3) + g_dot)
        off = np.abs(rec.Ph.astype(f64).T @ rec.Ph.astype(f64) - np.eye(r)).max()
        assert off <= bound_o, (off, bound_o)
        assert not rec.reset.any()


# ---- what the algorithm promises -----------------------------------------------------------------------------------------------
def _rel(M, D):
    return float(np.linalg.norm(M.astype(f64) - D.astype(f64)) / np.linalg.norm(M.astype(f64)))


@pytest.mark.parametrize("r", [1, 2, 4])
def test_warm_start_reaches_the_best_rank_r_error(r):
    M = pc.low_rank_plus_noise(96, 80, r, 30 + r, noise=0.1)
    opt, sv = pc.best_rank_error(M, r)
    assert sv[r - 1] / sv[r] >= 4.0      # the power iteration's factor per record is (sigma_{r+1} / sigma_r)^2 <= 1 / 16
    Q0 = pc.q0(1, 0, 0, 80, r)
    Q, errs = Q0, []
    for _ in range(8):
        rec = pc.record(M, Q, Q0)
        Q = rec.Q
        errs.append(float(np.linalg.norm(M.astype(f64) - rec.D.astype(f64))))
    assert opt * (1 - 1e-6) <= errs[7] <= 1.01 * opt, (errs[7], opt)      # (below: D's own float32 rounding, nothing more)
    assert errs[0] > errs[7]


def test_error_feedback_follows_the_one_over_t_law():
    """sum_t D_t = T M - e_T (e_0 = 0, scale 1), so the running mean of the decodes misses M by exactly |e_T| / T.  |e_T| stays
    bounded: a rank-r projection of x leaves at most rho |x|, rho = sqrt(1 - r / min(n, m)) for the best one (a flat spectrum is the
    worst case), so |e_t| <= rho (|M| + |e_{t-1}|) and |e_T| <= rho / (1 - rho) |M|; and |e_1| >= the best rank-r error (Eckart-
    Young).  Hence miss_T * T / miss_1 <= K = rho / (1 - rho) * |M| / best -- from M's singular values alone.  T is chosen far
    beyond K (asserted: K < T / 4), so the bound bites: a running mean that did not approach M at all would give the ratio T, one
    whose miss shrank four times slower than 1 / T would fail too."""
    n, m, r, T = 96, 80, 2, 1024
    M = pc.low_rank_plus_noise(n, m, r, 40, noise=0.1)
    best, sv = pc.best_rank_error(M, r)
    rho = math.sqrt(1 - r / min(n, m))
    K = rho / (1 - rho) * float(np.linalg.norm(M.astype(f64))) / best
    Q0 = pc.q0(1, 0, 0, m, r)
    Q, e = Q0, np.zeros((n, m), f32)
    total, miss = np.zeros((n, m), f64), []
    for t in range(1, T + 1):
        rec = pc.record(M, Q, Q0, e, f32(1.0))
        Q, e = rec.Q, rec.e
        total += rec.D
        miss.append(float(np.linalg.norm(total / t - M)))
        assert abs(miss[-1] * t - np.linalg.norm(e.astype(f64))) <= 1e-4 * np.linalg.norm(M.astype(f64))      # (float32 rounding of e only)
    assert K < T / 4, (K, T)
    assert all(miss[t - 1] * t / miss[0] <= K for t in range(1, T + 1)), (max(miss[t - 1] * t for t in range(1, T + 1)) / miss[0], K)
    assert miss[T - 1] < miss[T // 2 - 1] < miss[T // 16 - 1] < miss[0]


def test_zero_gradient_rule():
    M = _mats([(40, 50)], 3)[0]
    Q0 = pc.q0(1, 0, 0, 50, 2)
    first = pc.record(M, Q0, Q0)
    zero = pc.record(np.zeros_like(M), first.Q, Q0)
    assert zero.reset.all() and not zero.Ph.any() and not zero.Qn.any() and not np.isnan(zero.D).any()
    assert np.array_equal(zero.Q, Q0)                       # the warm start went back; the wire carries Q' = 0 as computed
    assert not pc.parse(zero.section, 40, 50, 2)[1].any()
    after = pc.record(M, zero.Q, Q0)
    assert after.D.any() and pc.same(after.section, first.section)
    stuck = pc.record(M, zero.Qn, Q0)                       # without the rule: pinned at zero
    assert not stuck.D.any()


def test_error_table_of_the_readme():
    """Relative L2 error |M - D| / |M| of a cold (first) and of the eighth record of one 128 x 256 matrix, without error feedback."""
    readme = open(os.path.join(ROOT, "README.md")).read()
    rows = []
    for name in ("gauss", "lowrank"):
        for r in (1, 2, 4):
            M = (np.random.RandomState(10 + r).standard_normal((128, 256)).astype(f32) if name == "gauss"
                 else pc.low_rank_plus_noise(128, 256, r, 20 + r, noise=0.1))
            if name == "lowrank":      # (the README's row names this ratio)
                sv = pc.best_rank_error(M, r)[1]
                assert sv[r - 1] / sv[r] >= 5.0
            Q0 = pc.q0(1, 0, 0, 256, r)
            Q, errs = Q0, []
            for _ in range(8):
                rec = pc.record(M, Q, Q0)
                Q = rec.Q
                errs.append(_rel(M, rec.D))
            rows.append("%.3f / %.3f" % (errs[0], errs[7]))
    assert rows == ["0.994 / 0.989", "0.990 / 0.980", "0.976 / 0.959", "0.766 / 0.602", "0.546 / 0.448", "0.648 / 0.337"]
    for row in rows:
        assert row in readme


# ---- mutation checks ---------------------------------------------------------------------------------------------------------------
def _mutated(shape, r, muts):
    """Which of `muts` change the bytes of the three records a GPU case makes (section or dense decode)."""
    n, m = pc.matrix_of(shape)
    changed = {k: False for k in muts}
    Q0 = pc.q0(77, 0, 0, m, r)
    Q = {k: Q0 for k in muts + [None]}
    for step in range(3):
        M = _mats([shape], 100 + step)[0]
        recs = {k: pc.record(M, Q[k], Q0, mut=k) for k in Q}
        for k in muts:
            changed[k] |= not (np.array_equal(recs[k].section, recs[None].section) and pc.same(recs[k].D, recs[None].D))
        Q = {k: recs[k].Q for k in Q}
    return changed


_FULL = [c for c in CASES if c not in SINGLE]


@pytest.mark.parametrize("shape,r", _FULL, ids=[i for i, c in zip(CASE_IDS, CASES) if c not in SINGLE])
def test_mutations_change_bits_on_the_gpu_cases(shape, r):
    """A reduction in reversed order, an unfused multiply-add, a classical Gram-Schmidt: each changes the bytes of the three
    records a GPU case makes, so a kernel that did any of it would fail there.  Classical and modified Gram-Schmidt are the same
    operations up to rank 2, so that one is asked from rank 3 on."""
    changed = _mutated(shape, r, ["unfused", "reversed"] + (["classical"] if r >= 3 else []))
    assert all(changed.values()), changed


def test_mutations_on_a_single_row_and_a_single_column():
    """The two GPU cases the test above leaves out, and why.  One row at rank 1: Ph is P / (|P| + eps), a sign, whatever rounding P
    took, and Q' = M * (that sign) is exact -- no mutation can change a bit, which is asserted.  One column at rank 1: every value of
    P is a single product and D a single product, so only the norm's chain of ceil(1100 / 256) fused steps is left to a mutation;
    reversing it changes bits on these inputs, unfusing it does not move the rounded quotients (asserted as found, so that a change of
    the inputs that makes it bite is noticed)."""
    assert _mutated((1, 1100), 1, ["unfused", "reversed"]) == {"unfused": False, "reversed": False}
    assert _mutated((1100, 1), 1, ["unfused", "reversed"]) == {"unfused": False, "reversed": True}
