"""EdenCompressor through the public interface on the MI355X: Quantizer(EdenCompressor, ...) on the FCN shapes with three users against
the numpy contract (tests/eden_contract.py) stepped on the CPU over three records -- plain, ef, two_phase, every bit width and both
scales --, the graph paths against eager launches bit for bit, EdenCompressor.compress on a lone tensor (the per-tensor route), and
train.py.  The gradients are finite, so every comparison is on all 32 bits.
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
import eden_contract as ec  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = [(256, 784), (256,), (10, 256), (10,)]      # driver.FCN: two compressed tensors, two identity-compressed ones
BIG = [0, 2]
SEED = 5
USERS = 3


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=USERS, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


@pytest.fixture(scope="module")
def grads():
    """Student-t gradients with +-0 sprinkled in: [step][user][tensor], made once and left unchanged."""
    rs = np.random.RandomState(1)
    out = []
    for st in range(3):
        per = []
        for u in range(USERS):
            gs = []
            for s in SHAPES:
                n = int(np.prod(s))
                a = ec.student(n, rs.randint(1 << 30))
                z = rs.rand(n)
                a[z < 0.03] = f32(0.0)
                a[(z >= 0.03) & (z < 0.06)] = f32(-0.0)
                a.setflags(write=False)
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
    from gq_amd.compressors import EdenCompressor
    from gq_amd.quantizers import Quantizer
    users = len(grads[0])
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
    q = Quantizer(EdenCompressor, params, make_args(num_users=users, **kw))
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


def _model_ps(grads, bits, mode, signs, ef=False, two_phase=False):
    """The parameter server stepped in numpy over the contract -> (aggregates, sections) per step."""
    users = len(grads[0])
    err = [[np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG] for _ in range(users)]
    serr = [np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG]
    aggs, secs_all = [], []
    for epoch, step in enumerate(grads):
        secs = [[None] * len(BIG) for _ in range(users)]
        for u, gs in enumerate(step):
            for k, i in enumerate(BIG):
                r = ec.compress(gs[i].reshape(-1), bits, mode, signs, err[u][k] if ef else None, f32(_ef_scale(epoch)) if ef else None)
                secs[u][k] = r[0]
                if ef:
                    err[u][k] = r[3]
        out = [None] * len(SHAPES)
        for k, i in enumerate(BIG):
            n = int(np.prod(SHAPES[i]))
            m = ec.decode_mean([secs[u][k] for u in range(users)], n, bits, signs)
            if two_phase:
                r = ec.compress(m, bits, mode, signs, serr[k] if ef else None, f32(1.0) if ef else None)
                if ef:
                    serr[k] = r[3]
                m = r[1]
            out[i] = m.reshape(SHAPES[i])
        for i in range(len(SHAPES)):
            if i not in BIG:
                out[i] = _mean_rows([step[u][i] for u in range(users)])
        aggs.append(out)
        secs_all.append(secs)
    return aggs, secs_all


@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase", "ef_two_phase"])
@pytest.mark.parametrize("scale", ["unbiased", "mse"])
@pytest.mark.parametrize("bits", ec.BITS)
def test_psquantizer_against_the_contract(grads, bits, scale, variant):
    from gq_amd.codecs import BatchedEden, DenseCodec, EdenCodec
    ef, tp = "ef" in variant, "two_phase" in variant
    q, aggs, wires = _run(grads, ef=ef, two_phase=tp, eden_bits=bits, eden_scale=scale, eden_seed=SEED)
    assert [type(c) for c in q.codecs] == [EdenCodec, DenseCodec, EdenCodec, DenseCodec]
    assert [g[0] for g in q._groups] == [BatchedEden]
    signs = mxr.sign_words(SEED)
    assert q.compressors[0].signs == signs == q._groups[0][2].signs and q._groups[0][2].bits == bits
    want, secs = _model_ps(grads, bits, ec.MODES[scale], signs, ef, tp)
    for st in range(len(grads)):
        for u in range(USERS):
            for k, i in enumerate(BIG):
                got = wires[st][u][q.offsets[i]:q.offsets[i] + secs[st][u][k].size]
                assert np.array_equal(got, secs[st][u][k]), "step %d, user %d, tensor %d: the wire section" % (st, u, i)
        for i in range(len(SHAPES)):
            assert mx.same(aggs[st][i], want[st][i]), "step %d, tensor %d: the aggregate" % (st, i)


@pytest.mark.parametrize("bits", ec.BITS)
def test_graphs_equal_eager_launches(grads, bits):
    """The address-tied record graph and the whole step, then gradients at addresses that never come back (the address-free
    forms): the same bytes and the same gradients as eager launches, step for step, under error feedback."""
    from gq_amd.compressors import EdenCompressor, shared_seeds
    from gq_amd.quantizers import PSQuantizer
    gs = grads[0][0]

    def run(graph, moving):
        seeds = itertools.count(1000)
        with shared_seeds(lambda: next(seeds)):
            torch.manual_seed(21)
            params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
            q = PSQuantizer(EdenCompressor, params, make_args(num_users=1, gq_graph=graph, ef=True, eden_bits=bits))
            fixed = [torch.from_numpy(a.copy()).cuda() for a in gs]
            hold, wires, outs = [], [], []
            for step in range(8):
                for p, a, t in zip(params, gs, fixed):
                    if moving:
                        p.grad = torch.from_numpy(a.copy()).cuda()
                        hold.append(p.grad.view(-1))      # (an alias keeps the storage: apply() rebinds the gradient itself)
                    else:
                        t.copy_(torch.from_numpy(a.copy()))
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
    sec = ec.compress(gs[0].reshape(-1), bits, ec.UNBIASED, mxr.sign_words(1), np.zeros(gs[0].size, f32), f32(_ef_scale(1)))[0]
    assert np.array_equal(we[0][qe.offsets[0]:qe.offsets[0] + sec.size], sec)


@pytest.mark.parametrize("scale", ["unbiased", "mse"])
@pytest.mark.parametrize("bits", ec.BITS)
def test_per_tensor_compress(bits, scale):
    """EdenCompressor.compress on one tensor: the dense decode; decompress is the identity; float32 on the device only."""
    from gq_amd.compressors import EdenCompressor
    n = 5000
    v = ec.student(n, 31)
    t = torch.from_numpy(v).cuda().view(50, 100)
    c = EdenCompressor(n, t.shape, make_args(eden_bits=bits, eden_scale=scale, eden_seed=SEED))
    d = c.decompress(c.compress(t))
    want = ec.compress(v, bits, ec.MODES[scale], mxr.sign_words(SEED))[1]
    assert d.shape == t.shape and mx.same(d.cpu().numpy().reshape(-1), want)
    with pytest.raises(TypeError, match="float32"):
        c.compress(t.to(torch.bfloat16))
    with pytest.raises(TypeError, match="float32"):
        c.compress(t.cpu())


@pytest.mark.timeout(600)
def test_train_py_runs_eden():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "eden", "--eden-bits", "3", "--network", "fcn", "--dataset", "mnist",
           "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
