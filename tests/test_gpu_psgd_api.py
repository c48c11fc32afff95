"""PowerSGDCompressor through the public interface on the MI355X: Quantizer(PowerSGDCompressor, ...) on the FCN shapes with three
users against the numpy contract (tests/psgd_contract.py) stepped on the CPU over three records -- plain, ef, two_phase --, the
per-tensor route, the warm starts' round trip through warm_starts() / set_warm_starts(), the refusals and train.py.  The gradients
are finite, so every comparison is on all 32 bits."""
import json
import math
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import psgd_contract as pc  # noqa: E402

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
SHAPES = [(256, 784), (256,), (10, 256), (10,)]      # driver.FCN: two compressed tensors, two identity-compressed ones
BIG = [0, 2]
USERS = 3
RANK, SEED = 2, 5


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=f32).view(u32), np.ascontiguousarray(b, dtype=f32).view(u32))


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=USERS, mode="ps",
                psgd_rank=RANK, psgd_seed=SEED)
    base.update(kw)
    return Namespace(**base)


@pytest.fixture(scope="module")
def grads():
    """[step][user][tensor], made once and left unchanged."""
    rs = np.random.RandomState(1)
    out = []
    for st in range(3):
        per = []
        for u in range(USERS):
            gs = []
            for s in SHAPES:
                a = (rs.standard_normal(s) * 0.1).astype(f32)
                a.setflags(write=False)
                gs.append(a)
            per.append(gs)
        out.append(per)
    return out


def _mean_rows(rows):
    acc = np.zeros_like(rows[0])
    for r in rows:
        acc = (acc + r).astype(f32)
    return (acc / f32(len(rows))).astype(f32)


def _ef_scale(epoch):
    return 2 / (math.exp(-epoch) + 1) - 1


def _run(grads, q=None, first_epoch=0, **kw):
    from gq_amd.compressors import PowerSGDCompressor
    from gq_amd.quantizers import Quantizer
    users = len(grads[0])
    if q is None:
        params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
        q = Quantizer(PowerSGDCompressor, params, make_args(num_users=users, **kw))
    params = q.parameters
    aggs, wires = [], []
    for epoch, step in enumerate(grads, first_epoch):
        for u, gs in enumerate(step):
            for p, a in zip(params, gs):
                p.grad = torch.from_numpy(a.copy()).cuda()
            q.record(u, epoch)
        torch.cuda.synchronize()
        wires.append(q._wire.cpu().numpy().copy())
        q.apply()
        torch.cuda.synchronize()
        aggs.append([p.grad.detach().cpu().numpy().copy() for p in params])
    return q, aggs, wires


class Model(object):
    """The parameter server stepped in numpy over the contract."""

    def __init__(self, users, ef=False, two_phase=False):
        self.users, self.ef, self.tp = users, ef, two_phase
        self.nm = [pc.matrix_of(SHAPES[i]) for i in BIG]
        self.q0 = [[pc.q0(SEED, i, u, m, RANK) for i, (n, m) in zip(BIG, self.nm)] for u in range(users)]
        self.q = [[a.copy() for a in qs] for qs in self.q0]
        self.sq0 = [pc.q0(SEED, i, pc.SERVER_USER, m, RANK) for i, (n, m) in zip(BIG, self.nm)]
        self.sq = [a.copy() for a in self.sq0]
        self.err = [[np.zeros(nm, f32) for nm in self.nm] for _ in range(users)]
        self.serr = [np.zeros(nm, f32) for nm in self.nm]

    def step(self, step, epoch):
        """-> (aggregate per tensor, sections [user][k])"""
        secs = [[None] * len(BIG) for _ in range(self.users)]
        for u, gs in enumerate(step):
            for k, i in enumerate(BIG):
                rec = pc.record(gs[i].reshape(self.nm[k]), self.q[u][k], self.q0[u][k], self.err[u][k] if self.ef else None,
                                f32(_ef_scale(epoch)) if self.ef else None)
                secs[u][k], self.q[u][k] = rec.section, rec.Q
                if self.ef:
                    self.err[u][k] = rec.e
        out = [None] * len(SHAPES)
        for k, i in enumerate(BIG):
            n, m = self.nm[k]
            mean = pc.decode_mean([secs[u][k] for u in range(self.users)], n, m, RANK)
            if self.tp:
                rec = pc.record(mean, self.sq[k], self.sq0[k], self.serr[k] if self.ef else None, f32(1.0) if self.ef else None)
                mean, self.sq[k] = rec.D, rec.Q
                if self.ef:
                    self.serr[k] = rec.e
            out[i] = mean.reshape(SHAPES[i])
        for i in range(len(SHAPES)):
            if i not in BIG:
                out[i] = _mean_rows([step[u][i] for u in range(self.users)])
        return out, secs


def _check(q, grads, aggs, wires, model, first_epoch=0):
    for st, step in enumerate(grads):
        want, secs = model.step(step, first_epoch + st)
        for u in range(model.users):
            for k, i in enumerate(BIG):
                got = wires[st][u][q.offsets[i]:q.offsets[i] + secs[u][k].size]
                assert np.array_equal(got, secs[u][k]), "step %d, user %d, tensor %d: the wire section" % (st, u, i)
        for i in range(len(SHAPES)):
            assert same(aggs[st][i], want[i]), "step %d, tensor %d: the aggregate" % (st, i)
    for u in range(model.users):
        for k, i in enumerate(BIG):
            assert same(q.parameters[i].psgd_q[u].cpu().numpy(), model.q[u][k]), "user %d, tensor %d: the warm start" % (u, i)
            if model.ef:
                assert same(q.parameters[i].error[u].cpu().numpy(), model.err[u][k]), "user %d, tensor %d: the residual" % (u, i)


@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase", "ef_two_phase"])
def test_psquantizer_against_the_contract(grads, variant):
    from gq_amd.codecs import BatchedPowerSGD, DenseCodec, PowerSGDCodec
    ef, tp = "ef" in variant, "two_phase" in variant
    q, aggs, wires = _run(grads, ef=ef, two_phase=tp)
    assert [type(c) for c in q.codecs] == [PowerSGDCodec, DenseCodec, PowerSGDCodec, DenseCodec]
    assert [g[0] for g in q._groups] == [BatchedPowerSGD]
    model = Model(USERS, ef, tp)
    _check(q, grads, aggs, wires, model)
    if tp:
        for k, i in enumerate(BIG):
            assert same(q.parameters[i].psgd_server_q.cpu().numpy(), model.sq[k])


def test_graphs_equal_eager_launches(grads):
    """One user, the same gradients in storage that stays, six steps under error feedback: the same bytes with graphs on and off."""
    from gq_amd.compressors import PowerSGDCompressor
    from gq_amd.quantizers import PSQuantizer
    gs = grads[0][0]

    def run(graph):
        params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
        q = PSQuantizer(PowerSGDCompressor, params, make_args(num_users=1, gq_graph=graph, ef=True))
        fixed = [torch.from_numpy(a.copy()).cuda() for a in gs]
        wires, outs = [], []
        for step in range(6):
            for p, a, t in zip(params, gs, fixed):
                t.copy_(torch.from_numpy(a.copy()))
                p.grad = t
            q.record(0, 1)
            q.apply()
            torch.cuda.synchronize()
            wires.append(q._wire[0].cpu().numpy().copy())
            outs.append([p.grad.detach().cpu().numpy().copy() for p in params])
        return q, wires, outs

    qe, we, oe = run(False)
    qg, wg, og = run(True)
    assert sum(qe.record_paths.values()) == qe.record_paths["eager"] == 6
    assert sum(qg.record_paths.values()) == 6 and qg.record_paths["eager"] < 6, qg.record_paths
    for st in range(6):
        assert np.array_equal(we[st], wg[st]), "step %d: the wire" % st
        assert all(same(a, b) for a, b in zip(oe[st], og[st])), "step %d: the gradients" % st
    model = Model(1, True, False)
    for st in range(6):
        want, secs = model.step([gs], 1)
        assert np.array_equal(we[st][qe.offsets[0]:qe.offsets[0] + secs[0][0].size], secs[0][0])


def test_per_tensor_route_of_the_quantizer(grads):
    """gq_no_batch: every tensor through its own codec (a one-tensor group per call) -- the same wire as the grouped launches."""
    for tp in (False, True):
        q, aggs, wires = _run(grads[:2], ef=True, two_phase=tp, gq_no_batch=True)
        assert q._groups == []
        _check(q, grads[:2], aggs, wires, Model(USERS, True, tp))


def test_per_tensor_compress():
    from gq_amd.compressors import PowerSGDCompressor
    M = (np.random.RandomState(3).standard_normal((50, 100))).astype(f32)
    c = PowerSGDCompressor(5000, (50, 100), make_args(psgd_rank=4))
    t = torch.from_numpy(M).cuda()
    Q0 = pc.q0(SEED, 0, 0, 100, 4)
    first = pc.record(M, Q0, Q0)
    d = c.decompress(c.compress(t))
    assert d.shape == t.shape and same(d.cpu().numpy(), first.D)
    assert same(c.compress(t).cpu().numpy(), pc.record(M, first.Q, Q0).D)      # (the object's own warm start stepped)
    v = torch.ones(2048, device="cuda")
    assert torch.equal(PowerSGDCompressor(2048, (2048,), make_args()).compress(v), v)      # a vector travels as it is


def test_warm_starts_round_trip(grads):
    """Two steps, the warm starts read; a fresh quantizer given them makes the third step's bytes (without them it does not)."""
    q, aggs, wires = _run(grads[:2], two_phase=True)
    state = q.warm_starts()
    assert sorted(state) == BIG and all(len(state[i]["users"]) == USERS and state[i]["server"] is not None for i in BIG)
    _, a3, w3 = _run(grads[2:], q=q, first_epoch=2)
    from gq_amd.compressors import PowerSGDCompressor
    from gq_amd.quantizers import Quantizer
    cold = Quantizer(PowerSGDCompressor, [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES], make_args(two_phase=True))
    _, ac, wc = _run(grads[2:], q=cold, first_epoch=2)
    assert not np.array_equal(wc[0], w3[0])
    fresh = Quantizer(PowerSGDCompressor, [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES], make_args(two_phase=True))
    fresh.set_warm_starts(state)
    _, af, wf = _run(grads[2:], q=fresh, first_epoch=2)
    assert np.array_equal(wf[0], w3[0]) and all(same(a, b) for a, b in zip(af[0], a3[0]))


def test_refusals():
    from gq_amd.compressors import PowerSGDCompressor
    from gq_amd.driver import build_parser, check_param_dtype
    from gq_amd.quantizers import PSQuantizer, Quantizer, RingQuantizer
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
    with pytest.raises(ValueError, match="ring mode"):
        Quantizer(PowerSGDCompressor, params, make_args(mode="ring"))
    with pytest.raises(ValueError, match="ring mode"):
        RingQuantizer(PowerSGDCompressor, params, make_args(mode="ring"))
    with pytest.raises(ValueError, match="momentum_correction"):
        PSQuantizer(PowerSGDCompressor, params, make_args(momentum_correction=0.9))
    with pytest.raises(ValueError, match="float32 parameters only"):
        PSQuantizer(PowerSGDCompressor, [torch.nn.Parameter(torch.zeros(s, device="cuda", dtype=torch.bfloat16)) for s in SHAPES], make_args())
    with pytest.raises(ValueError, match="bfloat16"):
        check_param_dtype(build_parser().parse_args(["--quantizer", "powersgd", "--param-dtype", "bfloat16"]))
    with pytest.raises(ValueError, match="fewer than"):
        PSQuantizer(PowerSGDCompressor, params, make_args(num_users=4095))
    args = build_parser().parse_args(["--quantizer", "powersgd"])
    assert (args.psgd_rank, args.psgd_seed) == (2, 0)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--quantizer", "powersgd", "--psgd-rank", "3"])


@pytest.mark.timeout(600)
def test_train_py_runs_powersgd_with_error_feedback():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "powersgd", "--psgd-rank", "4", "--ef", "--network", "fcn",
           "--dataset", "mnist", "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
