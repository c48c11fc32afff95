"""SparseTernaryCompressor through the public interface on the MI355X: Quantizer(SparseTernaryCompressor, ...) on the FCN shapes with
three users against the numpy contract (tests/stc_contract.py) stepped on the CPU over three records -- plain, ef, two_phase --, the
graph paths against eager launches bit for bit, the per-tensor route, train.py and the refusals.  The gradients are finite, so every
comparison is on all 32 bits."""
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
import stc_contract as sc  # noqa: E402
import topk_contract as tc  # noqa: E402

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
SHAPES = [(256, 784), (256,), (10, 256), (10,)]      # driver.FCN: two compressed tensors, two identity-compressed ones
BIG = [0, 2]
USERS = 3
CR = 256


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=f32).view(u32), np.ascontiguousarray(b, dtype=f32).view(u32))


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=USERS, mode="ps", cr=CR)
    base.update(kw)
    return Namespace(**base)


@pytest.fixture(scope="module")
def grads():
    """Heavy-tailed gradients with +-0 sprinkled in: [step][user][tensor], made once and left unchanged."""
    rs = np.random.RandomState(1)
    out = []
    for st in range(3):
        per = []
        for u in range(USERS):
            gs = []
            for s in SHAPES:
                n = int(np.prod(s))
                a = tc.heavy_tailed(n, rs.randint(1 << 30))
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
    from gq_amd.compressors import SparseTernaryCompressor
    from gq_amd.quantizers import Quantizer
    users = len(grads[0])
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
    q = Quantizer(SparseTernaryCompressor, params, make_args(num_users=users, **kw))
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


def _compress(v, err=None, s=None):
    """-> (section, dense decode, the new err or None)"""
    k = v.size // CR
    if err is None:
        return sc.section_bytes(v, k), sc.dense(v, k), None
    w, sec, D, e = sc.error_feedback(v, err, s, k)
    return sec, D, e


def _model_ps(grads, ef=False, two_phase=False):
    """The parameter server stepped in numpy over the contract -> (aggregates, sections) per step."""
    users = len(grads[0])
    err = [[np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG] for _ in range(users)]
    serr = [np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG]
    aggs, secs_all = [], []
    for epoch, step in enumerate(grads):
        secs = [[None] * len(BIG) for _ in range(users)]
        for u, gs in enumerate(step):
            for k, i in enumerate(BIG):
                sec, _, e = _compress(gs[i].reshape(-1), err[u][k] if ef else None, f32(_ef_scale(epoch)) if ef else None)
                secs[u][k] = sec
                if ef:
                    err[u][k] = e
        out = [None] * len(SHAPES)
        for k, i in enumerate(BIG):
            n = int(np.prod(SHAPES[i]))
            m = sc.decode_mean([secs[u][k] for u in range(users)], n, n // CR, users)
            if two_phase:
                _, m, e = _compress(m, serr[k] if ef else None, f32(1.0) if ef else None)
                if ef:
                    serr[k] = e
            out[i] = m.reshape(SHAPES[i])
        for i in range(len(SHAPES)):
            if i not in BIG:
                out[i] = _mean_rows([step[u][i] for u in range(users)])
        aggs.append(out)
        secs_all.append(secs)
    return aggs, secs_all


@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase", "ef_two_phase"])
def test_psquantizer_against_the_contract(grads, variant):
    from gq_amd.codecs import BatchedSTC, DenseCodec, STCCodec
    ef, tp = "ef" in variant, "two_phase" in variant
    q, aggs, wires = _run(grads, ef=ef, two_phase=tp)
    assert [type(c) for c in q.codecs] == [STCCodec, DenseCodec, STCCodec, DenseCodec]
    assert [g[0] for g in q._groups] == [BatchedSTC]
    want, secs = _model_ps(grads, ef, tp)
    for st in range(len(grads)):
        for u in range(USERS):
            for k, i in enumerate(BIG):
                got = wires[st][u][q.offsets[i]:q.offsets[i] + secs[st][u][k].size]
                assert np.array_equal(got, secs[st][u][k]), "step %d, user %d, tensor %d: the wire section" % (st, u, i)
        for i in range(len(SHAPES)):
            assert same(aggs[st][i], want[st][i]), "step %d, tensor %d: the aggregate" % (st, i)


def test_graphs_equal_eager_launches(grads):
    """Gradients in storage that stays and at addresses that never come back: the same bytes and the same gradients with graphs on
    and off, step for step, under error feedback; the first step is the contract's."""
    from gq_amd.compressors import SparseTernaryCompressor, shared_seeds
    from gq_amd.quantizers import PSQuantizer
    gs = grads[0][0]

    def run(graph, moving):
        seeds = itertools.count(1000)
        with shared_seeds(lambda: next(seeds)):
            torch.manual_seed(21)
            params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
            q = PSQuantizer(SparseTernaryCompressor, params, make_args(num_users=1, gq_graph=graph, ef=True))
            fixed = [torch.from_numpy(a.copy()).cuda() for a in gs]
            hold, wires, outs = [], [], []
            for step in range(6):
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
        assert sum(pe.values()) == pe["eager"] == 6
        assert sum(pg.values()) == 6 and pg["eager"] < 6, pg      # (some step replayed from a graph)
        for st in range(6):
            assert np.array_equal(we[st], wg[st]), "step %d (moving %s): the wire" % (st, moving)
            assert all(same(a, b) for a, b in zip(oe[st], og[st])), "step %d (moving %s): the gradients" % (st, moving)
    sec = _compress(gs[0].reshape(-1), np.zeros(gs[0].size, f32), f32(_ef_scale(1)))[0]
    assert np.array_equal(we[0][qe.offsets[0]:qe.offsets[0] + sec.size], sec)


def test_per_tensor_compress():
    """SparseTernaryCompressor.compress on one tensor: the dense decode; decompress is the identity; float32 on the device only."""
    from gq_amd.compressors import SparseTernaryCompressor
    n = 5000
    v = tc.heavy_tailed(n, 31)
    t = torch.from_numpy(v).cuda().view(50, 100)
    c = SparseTernaryCompressor(n, t.shape, make_args(cr=64))
    d = c.decompress(c.compress(t))
    assert d.shape == t.shape and same(d.cpu().numpy().reshape(-1), sc.dense(v, n // 64))
    with pytest.raises(TypeError, match="float32"):
        c.compress(t.to(torch.bfloat16))
    with pytest.raises(TypeError, match="float32"):
        c.compress(t.cpu())


def test_per_tensor_route_of_the_quantizer(grads):
    """gq_no_batch: every tensor through its own codec (a one-tensor group per call) -- the same wire as the grouped launches."""
    q, aggs, wires = _run(grads[:1], ef=True, gq_no_batch=True)
    assert q._groups == []
    want, secs = _model_ps(grads[:1], ef=True)
    for u in range(USERS):
        for k, i in enumerate(BIG):
            assert np.array_equal(wires[0][u][q.offsets[i]:q.offsets[i] + secs[0][u][k].size], secs[0][u][k])
    assert all(same(aggs[0][i], want[0][i]) for i in range(len(SHAPES)))


def test_refusals():
    from gq_amd.compressors import SparseTernaryCompressor
    from gq_amd.driver import build_parser, check_param_dtype
    from gq_amd.quantizers import PSQuantizer, Quantizer, RingQuantizer
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
    with pytest.raises(ValueError, match="ring mode"):
        Quantizer(SparseTernaryCompressor, params, make_args(mode="ring"))
    with pytest.raises(ValueError, match="ring mode"):
        RingQuantizer(SparseTernaryCompressor, params, make_args(mode="ring"))
    with pytest.raises(ValueError, match="momentum_correction"):
        PSQuantizer(SparseTernaryCompressor, params, make_args(momentum_correction=0.9))
    with pytest.raises(ValueError, match="float32 parameters only"):
        PSQuantizer(SparseTernaryCompressor, [torch.nn.Parameter(torch.zeros(s, device="cuda", dtype=torch.bfloat16)) for s in SHAPES], make_args())
    with pytest.raises(ValueError, match="bfloat16"):
        check_param_dtype(build_parser().parse_args(["--quantizer", "stc", "--param-dtype", "bfloat16"]))
    with pytest.raises(ValueError, match="cr"):
        SparseTernaryCompressor(10, (10,), make_args(cr=0))


@pytest.mark.timeout(600)
def test_train_py_runs_stc_with_error_feedback():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "stc", "--cr", "64", "--ef", "--network", "fcn", "--dataset", "mnist",
           "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
