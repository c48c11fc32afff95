"""args.momentum_correction through the public interface: Quantizer(TopKSparsificationCompressor, params, args) on driver.FCN's
shapes against tests/dgc_contract.py plus topk_contract's decode-mean, bit for bit on param.grad and on the state; with two_phase;
the per-tensor route; the refusals; one short train.py run."""
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
import dgc_contract as dc  # noqa: E402
import topk_contract as tc  # noqa: E402

pytestmark = pytest.mark.gpu

CR, M, USERS, STEPS = 64, 0.9, 3, 3


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="1.0", num_users=USERS, mode="ps",
                cr=CR, momentum_correction=M)
    base.update(kw)
    return Namespace(**base)


def _mean_rows(rows):
    acc = np.zeros(rows[0].shape, np.float32)
    for r in rows:
        acc = (acc + r).astype(np.float32)
    return (acc / np.float32(len(rows))).astype(np.float32)


def _run(two_phase=False, strided=False, gq_graph=None):
    """-> the quantizer.  strided: parameter 0's gradient is a transposed view (the multi-tensor path cannot address it: the group
    takes the per-tensor route)."""
    from gq_amd.compressors import TopKSparsificationCompressor
    from gq_amd.quantizers import Quantizer
    shapes = dc.FCN_SHAPES
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes]
    q = Quantizer(TopKSparsificationCompressor, params, make_args(two_phase=two_phase, gq_graph=gq_graph))
    big = [j for j, s in enumerate(shapes) if int(np.prod(s)) > 1000]
    sizes = [int(np.prod(shapes[j])) for j in big]
    ks = [n // CR for n in sizes]
    want = [dc.State(sizes, ks, M) for _ in range(USERS)]
    grads = dc.fcn_grads(USERS, STEPS)
    for step in range(STEPS):
        secs = []
        for user in range(USERS):
            for j, (p, a) in enumerate(zip(params, grads[step][user])):
                t = torch.from_numpy(a).to("cuda")
                if strided and j == 0:
                    t = t.t().contiguous().t()
                    assert not t.is_contiguous()
                p.grad = t
            before = [p.grad.clone() for p in params]
            q.record(user, 0)
            assert all(torch.equal(a.view(torch.int32), p.grad.view(torch.int32)) for a, p in zip(before, params)), "record() wrote a gradient"
            secs.append(want[user].record([grads[step][user][j] for j in big]))
        q.apply()
        torch.cuda.synchronize()
        for i, j in enumerate(big):
            n, k = sizes[i], ks[i]
            mean = tc.decode_mean([tc.split_section(secs[u][i], k) for u in range(USERS)], n, k, USERS)
            if two_phase:
                mean = tc.dense(mean, k)      # the server's re-compress of the mean: plain top-k, no momentum
            what = "step %d, parameter %d" % (step, j)
            assert np.array_equal(tc.bits(params[j].grad.cpu().numpy()), tc.bits(mean)), what + ": param.grad"
            for user in range(USERS):
                assert np.array_equal(tc.bits(params[j].dgc_u[user].cpu().numpy()), tc.bits(want[user].u[i])), what + ": u"
                assert np.array_equal(tc.bits(params[j].dgc_v[user].cpu().numpy()), tc.bits(want[user].v[i])), what + ": v"
        for j in range(len(shapes)):
            if j not in big:
                mean = _mean_rows([grads[step][u][j] for u in range(USERS)])
                assert np.array_equal(tc.bits(params[j].grad.cpu().numpy()), tc.bits(mean)), "step %d: dense parameter %d" % (step, j)
                assert not hasattr(params[j], "dgc_u")
    return q


def test_quantizer_matches_the_contract():
    q = _run()
    assert [g[0].__name__ for g in q._groups] == ["BatchedDGC"]
    assert sum(q.record_paths.values()) == USERS * STEPS


def test_quantizer_matches_the_contract_eager():
    q = _run(gq_graph=False)
    assert q.record_paths["eager"] == USERS * STEPS


def test_two_phase():
    _run(two_phase=True)


def test_per_tensor_route_gives_the_same_bits():
    q = _run(strided=True)
    assert q.record_paths["eager"] == USERS * STEPS and len(q._dgc_single) == 2


def test_refusals():
    from gq_amd.compressors import QSGDCompressor, SignSGDCompressor, TopKSparsificationCompressor
    from gq_amd.quantizers import Quantizer
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in dc.FCN_SHAPES]
    for comp in (QSGDCompressor, SignSGDCompressor):
        with pytest.raises(ValueError, match="TopKSparsificationCompressor"):
            Quantizer(comp, params, make_args())
    with pytest.raises(ValueError, match="error feedback"):
        Quantizer(TopKSparsificationCompressor, params, make_args(ef=True))
    with pytest.raises(ValueError, match="ring"):
        Quantizer(TopKSparsificationCompressor, params, make_args(mode="ring"))
    q = Quantizer(TopKSparsificationCompressor, params, make_args(momentum_correction=None))      # off: plain top-k
    assert q.dgc_m is None and not hasattr(params[0], "dgc_u") and [g[0].__name__ for g in q._groups] == ["BatchedTopK"]


@pytest.mark.timeout(600)
def test_train_py_runs_with_momentum_correction():
    import json
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--network", "fcn", "--quantizer", "topk", "--cr", "64", "--momentum-correction", "0.9",
           "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines and all(np.isfinite(ln["loss"]) for ln in lines), r.stdout[-1000:]
