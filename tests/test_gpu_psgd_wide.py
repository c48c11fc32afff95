"""The low-rank compressor at rank 16 and 32 (csrc/psgd_wide.hip) on the MI355X against numpy float64: include/gq_psgd.h, RANKS 16
AND 32 -- the layout byte for byte, the factors within the bounds written beside each assertion (u = 2^-24), after a cold record
and after the third (the warm start in use).  DESIGN.md 4.20 has the measured defects of every case."""
import json, math, os, subprocess, sys  # noqa: E401
from argparse import Namespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import psgd_contract as pc  # noqa: E402

pytestmark = pytest.mark.gpu

f32, f64, u32 = np.float32, np.float64, np.uint32
U, CANARY, FCANARY, SEED, IDENT = 2.0 ** -24, 0xA5, -7.25, 77, 1500
# one ragged tile (rank 16 only); across the row block and the column tile; three row blocks; a row of several pieces; a long n; 4-D
SHAPES = [(48, 70), (70, 300), (130, 45), (33, 4100), (4099, 35), (40, 8, 3, 3)]
# low_rank_plus_noise seeds with kappa(M Q0) <= 64, found on the CPU (Q0 of parameter = index in SHAPES, user 0)
SEEDS = {16: [0, 0, 0, 0, 0, 0], 32: [7, 0, 0, 1, 13, 25]}


def cases(r):
    return [i for i, s in enumerate(SHAPES) if not (r == 32 and s == (48, 70))]


def lrpn(i, r, extra=0):
    n, m = pc.matrix_of(SHAPES[i])
    return pc.low_rank_plus_noise(n, m, r, SEEDS[r][i] + extra, noise=0.1)


def mgs32(P):
    P = P.astype(f32).copy()
    for j in range(P.shape[1]):
        for k in range(j):
            P[:, j] -= f32(P[:, k] @ P[:, j]) * P[:, k]
        P[:, j] /= f32(np.sqrt(P[:, j] @ P[:, j]))
    return P.astype(f64)


class Group(object):
    """A BatchedPowerSGD over SHAPES[idx] at rank r, canaries between the wire sections, per user warm starts and residuals."""

    def __init__(self, idx, r, users=1, lead=0, ident=False):
        from gq_amd.codecs import BatchedPowerSGD, PowerSGDCodec
        from gq_amd.compressors import PowerSGDCompressor
        self.idx, self.r, self.lead = idx, r, lead
        self.nm = [pc.matrix_of(SHAPES[i]) for i in idx]
        args = Namespace(psgd_rank=r, psgd_seed=SEED)
        codecs = [PowerSGDCodec(PowerSGDCompressor(n * m, SHAPES[i], args), n * m, SHAPES[i], param_index=i) for i, (n, m) in zip(idx, self.nm)]
        self.off = [16 + sum(c.nbytes + 16 for c in codecs[:k]) for k in range(len(codecs))]
        at = 16 + sum(c.nbytes + 16 for c in codecs)
        self.ident_at, self.user_bytes = at, at + (4 * IDENT + 16 if ident else 0)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.grp = BatchedPowerSGD(codecs, self.off, list(range(len(idx))), dev, 1, self.user_bytes, dense=[(at, IDENT)] if ident else None)
        self.ident = [torch.arange(IDENT, dtype=torch.float32, device=dev)] if ident else None
        self.wire = torch.empty(self.user_bytes, dtype=torch.uint8, device=dev)
        self.q0 = [[pc.q0(SEED, i, u, m, r) for i, (n, m) in zip(idx, self.nm)] for u in range(users)]
        self.q = [[torch.from_numpy(q.reshape(-1).copy()).cuda() for q in qs] for qs in self.q0]
        self.e = [[torch.zeros(n * m, device=dev) for n, m in self.nm] for _ in range(users)]
        self.out = torch.empty(self.grp.out_floats + 4 + lead, device=dev)

    def record(self, mats, user=0, ef=None, want_out=True):
        """One record, launched twice from the same state (the same bytes), the layout checked.  -> a Namespace per tensor."""
        r, q, e = self.r, self.q[user], self.e[user]
        qin, ein = [t.clone() for t in q], [t.clone() for t in e]
        g = [torch.from_numpy(np.ascontiguousarray(M, f32).reshape(-1)).cuda() for M in mats]
        out = self.out[self.lead:self.lead + self.grp.out_floats] if want_out else None
        wires = []
        for rep in range(2):
            for dst, src in zip(q + e, qin + ein):
                dst.copy_(src)
            self.wire.fill_(CANARY), self.out.fill_(FCANARY)
            self.grp._pwork.fill_(float("nan")), self.grp._cpart.fill_(3e38), self.grp._flags.fill_(-1)
            assert self.grp.encode(g, self.wire, 0, 0, (e if ef is not None else None, q, user), ef, out=out, dense=self.ident)
            torch.cuda.synchronize()
            wires.append(self.wire.cpu().numpy())
        assert np.array_equal(wires[0], wires[1]), "two compresses of the same input and state"
        wire, outh, flags = wires[0], self.out.cpu().numpy(), self.grp._flags.cpu().numpy().reshape(-1, r)
        cov, ocov, recs = np.zeros(wire.size, bool), np.zeros(outh.size, bool), []
        for s, ((n, m), o, M) in enumerate(zip(self.nm, self.off, mats)):
            k, nb = pc.HEADER + 4 * r * (n + m), pc.section_nbytes(n, m, r)
            cov[o:o + nb] = True
            assert np.array_equal(wire[o:o + 16].view(u32), [n, m, r, 0]) and not wire[o + k:o + nb].any()
            Ph, Qn = pc.parse(wire[o:], n, m, r)
            Mp = M.reshape(n, m) if ef is None else (M.reshape(n, m) + (f32(ef) * ein[s].cpu().numpy().reshape(n, m)).astype(f32)).astype(f32)
            a = self.lead + self.grp.out_off[s]
            ocov[a:a + n * m] = want_out
            recs.append(Namespace(Mp=Mp.astype(f64), Q=qin[s].cpu().numpy().reshape(m, r).astype(f64), Ph=Ph.astype(f64), Qn=Qn.astype(f64),
                                  flags=flags[s], D=outh[a:a + n * m].reshape(n, m), e=e[s].cpu().numpy().reshape(n, m),
                                  Qout=q[s].cpu().numpy().reshape(m, r), Q0=self.q0[user][s]))
        if self.ident:
            cov[self.ident_at:self.ident_at + 4 * IDENT] = True
            assert np.array_equal(wire[self.ident_at:self.ident_at + 4 * IDENT].view(f32), np.arange(IDENT, dtype=f32))
        assert np.all(wire[~cov] == CANARY) and np.all(outh[~ocov] == f32(FCANARY)), "a byte outside the sections or the decoded tensors"
        return recs


def decode_bound(factors):
    """-> (the float64 mean of Ph Q'^T over the payloads, 2 (R r + 1) u sum(|Ph| |Q'|^T) / R)."""
    R, r = len(factors), factors[0][0].shape[1]
    want = sum(Ph @ Qn.T for Ph, Qn in factors) / R
    return want, 2 * (R * r + 1) * U * sum(np.abs(Ph) @ np.abs(Qn).T for Ph, Qn in factors) / R


def check(rec, r, ef, want_out, kept=None, tag=""):
    """Assertions 2 - 6 of one record of one tensor; kept: the columns that did not reset (all of them unless stated)."""
    (n, m), kept = rec.Mp.shape, np.arange(r) if kept is None else kept
    assert np.array_equal(np.flatnonzero(rec.flags == 0), kept) and not rec.Ph[:, rec.flags != 0].any(), tag
    Pref = (rec.Mp @ rec.Q)[:, kept]
    sv = np.linalg.svd(Pref, compute_uv=False)
    kappa = sv[0] / sv[-1]
    assert kappa <= 64, "%s: precondition, kappa(P_ref) = %.1f" % (tag, kappa)
    Ph, Qr = rec.Ph[:, kept], np.linalg.qr(Pref)[0]
    span = np.abs(Ph - Qr @ (Qr.T @ Ph)).max()
    span_bound = 4 * m * U * kappa * np.abs(rec.Mp).sum(1).max() * np.abs(rec.Q).max() / sv[-1]
    W = mgs32(Pref.astype(f32))
    delta, delta_ref = np.abs(Ph.T @ Ph - np.eye(len(kept))).max(), np.abs(W.T @ W - np.eye(len(kept))).max()
    back = np.abs(rec.Qn - rec.Mp.T @ rec.Ph) - 2 * n * U * (np.abs(rec.Mp).T @ np.abs(rec.Ph))
    print("%s kappa %.1f span %.2e / %.2e delta %.2e delta_ref %.2e back %.2e" % (tag, kappa, span, span_bound, delta, delta_ref, back.max()))
    assert span <= span_bound and delta <= 4 * max(delta_ref, r * U) and back.max() <= 0, tag
    assert np.array_equal(rec.Qout, np.where(rec.flags[None, :] != 0, rec.Q0, rec.Qn.astype(f32))), tag + ": the warm start written"
    want, tol = decode_bound([(rec.Ph, rec.Qn)])
    assert not want_out or np.all(np.abs(rec.D - want) <= tol), tag + ": the dense decode"
    assert ef is None or np.all(np.abs(rec.e - (rec.Mp - want)) <= tol + U * np.abs(rec.Mp - want) + 1e-45), tag + ": the residual"


@pytest.mark.parametrize("ef", [None, 0.75], ids=["plain", "ef"])
@pytest.mark.parametrize("r,case", [(r, c) for r in (16, 32) for c in cases(r) + ["group", "gauss"]])
def test_three_records(r, case, ef):
    idx = cases(r) if case == "group" else [1] if case == "gauss" else [case]
    g = Group(idx, r, ident=case == "group")
    mats = [np.random.RandomState(5).standard_normal(pc.matrix_of(SHAPES[1])).astype(f32)] if case == "gauss" else [lrpn(i, r) for i in idx]
    for step in range(3):
        want_out = not (ef is None and step == 1)      # (no residual launch at all on that record)
        recs = g.record(mats, ef=ef, want_out=want_out)
        if step != 1:
            for i, rec in zip(idx, recs):
                check(rec, r, ef, want_out, tag="r%d %s %r step %d" % (r, case, SHAPES[i], step))


@pytest.mark.parametrize("r,idx,R", [(16, None, 3), (32, None, 3), (32, [1], 9)])
def test_decode_mean(r, idx, R):
    """R users with gradients and warm starts of their own; R = 1 and R payloads into an `out` one float off 16-byte alignment."""
    idx = cases(r) if idx is None else idx
    g = Group(idx, r, users=R, lead=1)
    rows = torch.empty((R, g.user_bytes), dtype=torch.uint8, device="cuda")
    factors = []
    for u in range(R):
        recs = g.record([lrpn(i, r, extra=100 + u) for i in idx], user=u)
        rows[u].copy_(g.wire)
        factors.append([(rec.Ph, rec.Qn) for rec in recs])
    for users in (1, R):
        g.out.fill_(FCANARY)
        g.grp.decode_into(rows[:users], users, g.out[1:1 + g.grp.out_floats])      # (4 bytes off a 16-byte boundary)
        torch.cuda.synchronize()
        host, cov = g.out.cpu().numpy(), np.zeros(g.out.numel(), bool)
        for s, (n, m) in enumerate(g.nm):
            a = 1 + g.grp.out_off[s]
            cov[a:a + n * m] = True
            want, tol = decode_bound([factors[u][s] for u in range(users)])
            assert np.all(np.abs(host[a:a + n * m].reshape(n, m) - want) <= tol), "R = %d, tensor %d" % (users, s)
        assert np.all(host[~cov] == f32(FCANARY))


@pytest.mark.parametrize("r", [16, 32])
def test_zero_gradient_and_rank_deficient(r):
    g = Group([1, 2], r)
    mats = [lrpn(i, r) for i in g.idx]
    g.record(mats, ef=1.0)
    [e.zero_() for e in g.e[0]]
    for rec in g.record([np.zeros(nm, f32) for nm in g.nm], ef=1.0):
        assert rec.flags.all() and not rec.Ph.any() and not rec.Qn.any() and np.array_equal(rec.Qout.view(u32), rec.Q0.view(u32))
    for i, rec in zip(g.idx, g.record(mats, ef=1.0)):      # from Q0 again
        assert np.array_equal(rec.Q, rec.Q0.astype(f64))
        check(rec, r, 1.0, True, tag="after the reset %r" % (SHAPES[i],))
    # rank 3 in small integers, the warm start in small integers too: P = M Q is exact and has three independent columns
    rs = np.random.RandomState(5)
    M = (rs.randint(-3, 4, (70, 3)) @ rs.randint(-3, 4, (3, 300))).astype(f32)
    g = Group([1], r)
    q = np.round(g.q0[0][0] * 8).astype(f32)
    g.q[0][0].copy_(torch.from_numpy(q.reshape(-1)))
    rec = g.record([M])[0]
    assert (rec.flags == 0).sum() == 3
    check(rec, r, None, True, kept=np.flatnonzero(rec.flags == 0), tag="rank 3")


FCN = [(256, 784), (256,), (10, 256), (10,)]      # driver.FCN: at rank 16 ONE compressed tensor, which takes the per-tensor route
FCN64 = [(256, 784), (256,), (64, 256), (64,)]    # a last layer of 64 rows: two compressed tensors, a group, graphs


def _quantize(shapes, users, graph, steps=6, **kw):
    from gq_amd.compressors import PowerSGDCompressor
    from gq_amd.quantizers import Quantizer
    grads = [[torch.from_numpy((np.random.RandomState(u).standard_normal(s) * 0.1).astype(f32)).cuda() for s in shapes] for u in range(users)]
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes]
    q = Quantizer(PowerSGDCompressor, params, Namespace(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, scale="exp", mode="ps",
                                                        num_users=users, psgd_rank=16, psgd_seed=SEED, gq_graph=graph, **kw))
    fixed = [[t.clone() for t in gs] for gs in grads]
    wires, outs = [], []
    for step in range(steps):
        for u in range(users):
            for p, t, src in zip(params, fixed[u], grads[u]):
                t.copy_(src)
                p.grad = t
            q.record(u, 1)
        wires.append(q._wire.cpu().numpy().copy())
        q.apply()
        outs.append([p.grad.detach().cpu().numpy().copy() for p in params])
    return q, wires, outs


@pytest.mark.parametrize("shapes,users,kw", [(FCN, 2, dict(ef=True, two_phase=True)), (FCN64, 2, dict(ef=True, two_phase=True)),
                                             (FCN64, 1, dict(ef=True, two_phase=False))], ids=["fcn", "fcn64-two-users", "fcn64-one-user"])
def test_quantizer_graphs_equal_eager(shapes, users, kw, monkeypatch):
    """Quantizer at rank 16: eager launches, record graphs alone (GQ_FUSE_STEP=0) and the whole-step graph where the quantizer takes
    it give the same bytes."""
    from gq_amd.codecs import PowerSGDCodec
    qe, we, oe = _quantize(shapes, users, False, **kw)
    assert [type(c) is PowerSGDCodec for c in qe.codecs] == [True, False, shapes is FCN64, False]
    assert sum(qe.record_paths.values()) == qe.record_paths["eager"]
    for fuse in ("0", "1"):
        monkeypatch.setenv("GQ_FUSE_STEP", fuse)
        qg, wg, og = _quantize(shapes, users, True, **kw)
        if shapes is FCN64 and users == 1:
            assert qg.record_paths["eager"] < sum(qg.record_paths.values()), qg.record_paths
        for st in range(len(we)):
            assert np.array_equal(we[st], wg[st]), "GQ_FUSE_STEP=%s, step %d: the wire" % (fuse, st)
            assert all(np.array_equal(a.view(u32), b.view(u32)) for a, b in zip(oe[st], og[st])), "step %d: the gradients" % st


@pytest.mark.timeout(600)
def test_train_py_runs_rank_16_with_error_feedback():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "powersgd", "--psgd-rank", "16", "--ef", "--network", "fcn",
           "--dataset", "mnist", "--num-users", "2", "--epochs", "2", "--train-size", "2048", "--log-interval", "8"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [rec["loss"] for rec in (json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")) if "loss" in rec]
    assert len(losses) >= 2 and all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], r.stdout[-2000:]
