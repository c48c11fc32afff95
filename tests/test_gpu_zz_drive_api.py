"""DriveCompressor through the public interface on the MI355X: Quantizer(DriveCompressor, ...) on the FCN shapes against the numpy
contract (tests/drive_contract.py) stepped on the CPU over three records -- one user and three, ef, two_phase, both scales --, the
graph paths against eager launches bit for bit, DriveCompressor.compress on a lone tensor, and train.py.  The gradients are
finite, so every comparison is on all 32 bits.
(zz: the file runs behind the other GPU tests, like the test_gpu_z_* files -- some of those count which graph path a step takes, and
that depends on which blocks the caching allocator has handed out before them.)"""
import itertools
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
import mx_contract as mx  # noqa: E402
import mxr_contract as mxr  # noqa: E402
import drive_contract as dc  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = [(256, 784), (256,), (10, 256), (10,)]      # driver.FCN: two compressed tensors, two identity-compressed ones
BIG = [0, 2]
SEED = 5


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=3, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


def _grads(seed, users, steps):
    """Student-t gradients with +-0 sprinkled in: [step][user][tensor]."""
    rs = np.random.RandomState(seed)
    out = []
    for st in range(steps):
        per = []
        for u in range(users):
            gs = []
            for s in SHAPES:
                n = int(np.prod(s))
                a = dc.student(n, rs.randint(1 << 30))
                z = rs.rand(n)
                a[z < 0.03] = f32(0.0)
                a[(z >= 0.03) & (z < 0.06)] = f32(-0.0)
                gs.append(a.reshape(s))
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


def _run(grads, **kw):
    from gq_amd.compressors import DriveCompressor
    from gq_amd.quantizers import Quantizer
    users = len(grads[0])
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
    q = Quantizer(DriveCompressor, params, make_args(num_users=users, **kw))
    aggs, wires = [], []
    for epoch, step in enumerate(grads):
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


def _model_ps(grads, mode, signs, ef=False, two_phase=False):
    """The parameter server stepped in numpy over the contract -> (aggregates, sections) per step."""
    users = len(grads[0])
    err = [[np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG] for _ in range(users)]
    serr = [np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG]
    aggs, secs_all = [], []
    for epoch, step in enumerate(grads):
        secs = [[None] * len(BIG) for _ in range(users)]
        for u, gs in enumerate(step):
            for k, i in enumerate(BIG):
                sec, D, w, ne, _, _ = dc.compress(gs[i].reshape(-1), mode, signs, err[u][k] if ef else None, f32(_ef_scale(epoch)) if ef else None)
                secs[u][k] = sec
                if ef:
                    err[u][k] = ne
        out = [None] * len(SHAPES)
        for k, i in enumerate(BIG):
            n = int(np.prod(SHAPES[i]))
            m = dc.decode_mean([secs[u][k] for u in range(users)], n, signs)
            if two_phase:
                _, D, w, ne, _, _ = dc.compress(m, mode, signs, serr[k] if ef else None, f32(1.0) if ef else None)
                if ef:
                    serr[k] = ne
                m = D
            out[i] = m.reshape(SHAPES[i])
        for i in range(len(SHAPES)):
            if i not in BIG:
                out[i] = _mean_rows([step[u][i] for u in range(users)])
        aggs.append(out)
        secs_all.append(secs)
    return aggs, secs_all


@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase", "ef_two_phase"])
@pytest.mark.parametrize("users", [1, 3])
@pytest.mark.parametrize("scale", ["unbiased", "mse"])
def test_psquantizer_against_the_contract(scale, users, variant):
    from gq_amd.codecs import BatchedDrive, DenseCodec, DriveCodec
    ef, tp = "ef" in variant, "two_phase" in variant
    grads = _grads(1, users, 3)
    q, aggs, wires = _run(grads, ef=ef, two_phase=tp, drive_scale=scale, drive_seed=SEED)
    assert [type(c) for c in q.codecs] == [DriveCodec, DenseCodec, DriveCodec, DenseCodec]
    assert [g[0] for g in q._groups] == [BatchedDrive]
    signs = mxr.sign_words(SEED)
    assert q.compressors[0].signs == signs == q._groups[0][2].signs
    want, secs = _model_ps(grads, dc.MODES[scale], signs, ef, tp)
    for st in range(len(grads)):
        for u in range(users):
            for k, i in enumerate(BIG):
                got = wires[st][u][q.offsets[i]:q.offsets[i] + secs[st][u][k].size]
                assert np.array_equal(got, secs[st][u][k]), "step %d, user %d, tensor %d: the wire section" % (st, u, i)
        for i in range(len(SHAPES)):
            assert mx.same(aggs[st][i], want[st][i]), "step %d, tensor %d: the aggregate" % (st, i)


def test_graphs_equal_eager_launches():
    """The address-tied record graph and the whole step, then gradients at addresses that never come back (the address-free
    forms): the same bytes and the same gradients as eager launches, step for step, under error feedback."""
    from gq_amd.compressors import DriveCompressor, shared_seeds
    from gq_amd.quantizers import PSQuantizer
    grads = _grads(5, 1, 1)[0][0]

    def run(graph, moving):
        seeds = itertools.count(1000)
        with shared_seeds(lambda: next(seeds)):
            torch.manual_seed(21)
            params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
            q = PSQuantizer(DriveCompressor, params, make_args(num_users=1, gq_graph=graph, ef=True))
            fixed = [torch.from_numpy(a.copy()).cuda() for a in grads]
            hold, wires, outs = [], [], []
            for step in range(8):
                for p, a, t in zip(params, grads, fixed):
                    if moving:
                        p.grad = torch.from_numpy(a.copy()).cuda()
                        hold.append(p.grad.view(-1))      # (an alias keeps the storage: apply() rebinds the gradient itself)
                    else:
                        t.copy_(torch.from_numpy(a))
                        p.grad = t
                q.record(0, 1)
                q.apply()
                torch.cuda.synchronize()
                wires.append(q._wire[0].cpu().numpy().copy())
                outs.append([p.grad.detach().cpu().numpy().copy() for p in params])
            return q, wires, outs

    for moving in (False, True):
        qe, we, oe = run(False, moving)
        qg, wg, og = run(True, moving)
        pe, pg = qe.record_paths, qg.record_paths
        assert sum(pe.values()) == pe["eager"] == 8
        assert pg["eager"] <= 3 and sum(pg.values()) == 8, pg
        if moving:
            assert pg["graph_any_address"] + pg["whole_step_any_address"] >= 1, pg
        else:
            assert pg["graph"] + pg["whole_step"] >= 1, pg
        for st in range(8):
            assert np.array_equal(we[st], wg[st]), "step %d (moving %s): the wire" % (st, moving)
            assert all(mx.same(a, b) for a, b in zip(oe[st], og[st])), "step %d (moving %s): the gradients" % (st, moving)
    # and the first eager step is the contract's
    sec = dc.compress(grads[0].reshape(-1), dc.UNBIASED, mxr.sign_words(1), np.zeros(grads[0].size, f32), f32(_ef_scale(1)))[0]
    assert np.array_equal(we[0][qe.offsets[0]:qe.offsets[0] + sec.size], sec)


@pytest.mark.parametrize("scale", ["unbiased", "mse"])
def test_per_tensor_compress(scale):
    """DriveCompressor.compress on one tensor: the dense decode; decompress is the identity; float32 on the device only."""
    from gq_amd.compressors import DriveCompressor
    n = 5000
    v = dc.student(n, 31)
    t = torch.from_numpy(v).cuda().view(50, 100)
    c = DriveCompressor(n, t.shape, make_args(drive_scale=scale, drive_seed=SEED))
    d = c.decompress(c.compress(t))
    want = dc.compress(v, dc.MODES[scale], mxr.sign_words(SEED))[1]
    assert d.shape == t.shape and mx.same(d.cpu().numpy().reshape(-1), want)
    with pytest.raises(TypeError, match="float32"):
        c.compress(t.to(torch.bfloat16))
    with pytest.raises(TypeError, match="float32"):
        c.compress(t.cpu())


@pytest.mark.timeout(600)
def test_train_py_runs_drive():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "drive", "--network", "fcn", "--dataset", "mnist",
           "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
