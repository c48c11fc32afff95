"""ChunkTopKCompressor through the public interface on the MI355X: Quantizer(ChunkTopKCompressor, ...) on the FCN shapes with one and three
users against the numpy contract (tests/ctk_contract.py) stepped on the CPU over three records -- plain, ef, two_phase --, graph replay
against eager launches byte for byte, the refusals and one short train.py run.  The gradients are finite: all 32 bits are compared."""
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
import ctk_contract as cc  # noqa: E402
import topk_contract as tc  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = [(256, 784), (256,), (10, 256), (10,)]      # driver.FCN: two compressed tensors, two identity-compressed ones
BIG, CR, STEPS = [0, 2], 64, 3


def make_args(**kw):
    return Namespace(**dict(dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=3,
                                 mode="ps", cr=CR), **kw))


@pytest.fixture(scope="module")
def grads():
    """Heavy-tailed gradients, [step][user][tensor], made once and left unchanged."""
    rs = np.random.RandomState(1)
    return [[[tc.heavy_tailed(int(np.prod(s)), rs.randint(1 << 30)).reshape(s) for s in SHAPES] for _ in range(3)] for _ in range(STEPS)]


def _run(grads, users, **kw):
    from gq_amd.compressors import ChunkTopKCompressor
    from gq_amd.quantizers import Quantizer
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
    q = Quantizer(ChunkTopKCompressor, params, make_args(num_users=users, **kw))
    aggs, wires = [], []
    for epoch, step in enumerate(grads):
        for u in range(users):
            for p, a in zip(params, step[u]):
                p.grad = torch.from_numpy(a.copy()).cuda()
            q.record(u, epoch)
        torch.cuda.synchronize()
        wires.append(q._wire.cpu().numpy().copy())
        q.apply()
        torch.cuda.synchronize()
        aggs.append([p.grad.detach().cpu().numpy().copy() for p in params])
    return q, aggs, wires


def _compress(v, err, s):
    """-> (section, dense decode, the new err)"""
    w, D, e = cc.error_feedback(v, err, s, CR) if err is not None else (v, cc.dense(v, CR), None)
    return cc.section_bytes(w, CR), D, e


@pytest.mark.parametrize("users", [1, 3])
@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase", "ef_two_phase"])
def test_psquantizer_against_the_contract(grads, variant, users):
    from gq_amd.codecs import BatchedChunkTopK, ChunkTopKCodec, DenseCodec
    ef, tp = "ef" in variant, "two_phase" in variant
    q, aggs, wires = _run(grads, users, ef=ef, two_phase=tp)
    assert [type(c) for c in q.codecs] == [ChunkTopKCodec, DenseCodec, ChunkTopKCodec, DenseCodec] and [g[0] for g in q._groups] == [BatchedChunkTopK]
    err = {(u, i): np.zeros(int(np.prod(SHAPES[i])), f32) if ef else None for u in range(users + 1) for i in BIG}      # (user `users`: the server)
    for epoch, step in enumerate(grads):
        for i in range(len(SHAPES)):
            n = int(np.prod(SHAPES[i]))
            if i not in BIG:
                want = tc.decode_mean([(np.arange(n), step[u][i]) for u in range(users)], n, n, users)
            else:
                secs = []
                for u in range(users):
                    sec, _, err[u, i] = _compress(step[u][i].reshape(-1), err[u, i], f32(2 / (math.exp(-epoch) + 1) - 1))
                    secs.append(sec)
                    assert np.array_equal(wires[epoch][u][q.offsets[i]:q.offsets[i] + sec.size], sec), "step %d, user %d, tensor %d: the wire" % (epoch, u, i)
                want = cc.decode_mean(secs, n, CR)
                if tp:
                    _, want, err[users, i] = _compress(want, err[users, i], f32(1.0))
            assert np.array_equal(tc.bits(aggs[epoch][i]), tc.bits(want)), "step %d, tensor %d: the aggregate" % (epoch, i)


def test_graphs_equal_eager_launches(grads):
    """Gradients in storage that stays: the same bytes and the same gradients with graphs on and off over six steps under error feedback."""
    from gq_amd.compressors import ChunkTopKCompressor
    from gq_amd.quantizers import PSQuantizer

    def run(graph):
        params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
        q = PSQuantizer(ChunkTopKCompressor, params, make_args(num_users=1, gq_graph=graph, ef=True))
        fixed = [torch.zeros(s, device="cuda") for s in SHAPES]
        seen = []
        for step in range(6):
            for p, a, t in zip(params, grads[step % STEPS][0], fixed):
                t.copy_(torch.from_numpy(a.copy()))
                p.grad = t
            q.record(0, 1)
            q.apply()
            torch.cuda.synchronize()
            seen.append([q._wire[0].cpu().numpy().copy()] + [tc.bits(p.grad.detach().cpu().numpy()) for p in params])
        return q.record_paths, seen

    (pe, eager), (pg, graph) = run(False), run(True)
    assert sum(pe.values()) == pe["eager"] == 6 and sum(pg.values()) == 6 and pg["eager"] < 6, (pe, pg)
    assert all(np.array_equal(a, b) for se, sg in zip(eager, graph) for a, b in zip(se, sg))


def test_per_tensor_compress_and_refusals():
    from gq_amd.compressors import ChunkTopKCompressor
    from gq_amd.driver import build_parser, check_param_dtype, quantizer_choices
    from gq_amd.quantizers import PSQuantizer, Quantizer
    v = tc.heavy_tailed(5000, 31)
    t = torch.from_numpy(v).cuda().view(50, 100)
    c = ChunkTopKCompressor(5000, t.shape, make_args())
    assert np.array_equal(tc.bits(c.decompress(c.compress(t)).cpu().numpy()), tc.bits(cc.dense(v, CR)))
    assert quantizer_choices["chunktopk"] is ChunkTopKCompressor
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
    with pytest.raises(ValueError, match="ring mode"):
        Quantizer(ChunkTopKCompressor, params, make_args(mode="ring"))
    with pytest.raises(ValueError, match="momentum_correction"):
        PSQuantizer(ChunkTopKCompressor, params, make_args(momentum_correction=0.9))
    with pytest.raises(ValueError, match="float32 parameters only"):
        PSQuantizer(ChunkTopKCompressor, [torch.nn.Parameter(torch.zeros(s, device="cuda", dtype=torch.bfloat16)) for s in SHAPES], make_args())
    with pytest.raises(ValueError, match="bfloat16"):
        check_param_dtype(build_parser().parse_args(["--quantizer", "chunktopk", "--param-dtype", "bfloat16"]))
    for cr in (1, 4097, True):
        with pytest.raises(ValueError, match="cr"):
            ChunkTopKCompressor(5000, (5000,), make_args(cr=cr))
    with pytest.raises(TypeError, match="float32"):
        c.compress(t.cpu())


@pytest.mark.timeout(600)
def test_train_py_runs_chunktopk_with_error_feedback():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "chunktopk", "--cr", "64", "--ef", "--network", "fcn", "--dataset", "mnist",
           "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [json.loads(ln).get("loss") for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert [v for v in losses if v is not None] and all(math.isfinite(v) for v in losses if v is not None), r.stdout[-2000:]
