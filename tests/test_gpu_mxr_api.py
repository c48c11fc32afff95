"""MXCompressor with mx_rotate = "hadamard" through the public interface on the MI355X: Quantizer(MXCompressor, ...) on the FCN
shapes with three users against the numpy contract (tests/mxr_contract.py) stepped over three records -- plain, ef, two_phase --,
graphs against eager launches bit for bit, the per-tensor compress route, mx_rotate = "none" byte for byte today's wire, and
train.py.  The stepping harness is tests/test_gpu_mx_api.py's."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402
import mxr_contract as mxr  # noqa: E402
import test_gpu_mx_api as api  # noqa: E402  (the harness: _grads, _run, _check_aggs, _check_wires)

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES, BIG, FMT = api.SHAPES, api.BIG, api.FMT
SEED = 5


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _model_ps(grads, fmt, signs, ef=False, two_phase=False, draws=None):
    """The parameter server stepped in numpy over the rotated compressor.  draws(step, user, i) -> the tensor's uniforms or None."""
    users = len(grads[0])
    err = [[np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG] for _ in range(users)]
    serr = [np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG]
    aggs, secs_all = [], []
    for epoch, step in enumerate(grads):
        secs = [[None] * len(BIG) for _ in range(users)]
        for u, gs in enumerate(step):
            for k, i in enumerate(BIG):
                r = draws(epoch, u, i) if draws else None
                sec, D, w, ne, _ = mxr.compress(gs[i].reshape(-1), fmt, signs, r, err[u][k] if ef else None,
                                                f32(api._ef_scale(epoch)) if ef else None)
                secs[u][k] = sec
                if ef:
                    err[u][k] = ne
        out = [None] * len(SHAPES)
        for k, i in enumerate(BIG):
            n = int(np.prod(SHAPES[i]))
            m = mxr.decode_mean([secs[u][k] for u in range(users)], n, fmt, signs)
            if two_phase:
                r = draws(epoch, "server", i) if draws else None
                _, D, w, ne, _ = mxr.compress(m, fmt, signs, r, serr[k] if ef else None, f32(1.0) if ef else None)
                if ef:
                    serr[k] = ne
                m = D
            out[i] = m.reshape(SHAPES[i])
        for i in range(len(SHAPES)):
            if i not in BIG:
                out[i] = api._mean_rows([step[u][i] for u in range(users)])
        aggs.append(out)
        secs_all.append(secs)
    return aggs, secs_all


@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase", "ef_two_phase"])
@pytest.mark.parametrize("fmt", ["fp4", "fp8"])
def test_psquantizer_deterministic_against_the_contract(fmt, variant):
    from gq_amd.codecs import BatchedMXR, DenseCodec, MXRCodec
    from gq_amd.quantizers import Quantizer
    ef, tp = "ef" in variant, "two_phase" in variant
    grads = api._grads(1, 3, 3)
    q, params, aggs, wires = api._run(Quantizer, grads, mx_format=fmt, ef=ef, two_phase=tp, mx_rotate="hadamard", mx_rotate_seed=SEED)
    assert [type(c) for c in q.codecs] == [MXRCodec, DenseCodec, MXRCodec, DenseCodec]
    assert [g[0] for g in q._groups] == [BatchedMXR]
    signs = mxr.sign_words(SEED)
    assert q.compressors[0].rotate == "hadamard" and q.compressors[0].rotate_signs == signs == q._groups[0][2].signs
    want, secs = _model_ps(grads, FMT[fmt], signs, ef, tp)
    api._check_wires(q, wires, secs, FMT[fmt])
    api._check_aggs(aggs, want)


def test_psquantizer_device_draws_follow_the_step_words():
    from gq_amd.quantizers import Quantizer
    grads = api._grads(3, 3, 3)
    q, params, aggs, wires = api._run(Quantizer, grads, random=1, mx_rotate="hadamard")
    state = q._rng_state.cpu().numpy().astype(np.int64)
    sizes = [int(np.prod(SHAPES[i])) for i in BIG]
    first = dict(zip(BIG, [0, sizes[0]]))
    want, secs = _model_ps(grads, mx.FP4, mxr.sign_words(1),
                           draws=lambda st, u, i: mx.draws(mx.COUNTER, int(np.prod(SHAPES[i])), first[i], int(state[u, 0]) & (2 ** 64 - 1), st))
    api._check_wires(q, wires, secs, mx.FP4)
    api._check_aggs(aggs, want)


@pytest.mark.parametrize("random", [0, 1])
def test_graphs_equal_eager_launches(random):
    """The address-tied record graph and the whole step, then moving gradients (the address-free forms): the same bytes and the
    same gradients as eager launches, step for step, under error feedback."""
    import itertools
    from gq_amd.compressors import MXCompressor, shared_seeds
    from gq_amd.quantizers import PSQuantizer
    grads = api._grads(5, 1, 1)[0][0]

    def run(graph, moving):
        seeds = itertools.count(1000)
        with shared_seeds(lambda: next(seeds)):
            torch.manual_seed(21)
            params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
            q = PSQuantizer(MXCompressor, params, api.make_args(num_users=1, random=random, gq_graph=graph, ef=True, mx_rotate="hadamard"))
            fixed = [torch.from_numpy(a.copy()).cuda() for a in grads]
            hold, wires, outs = [], [], []
            for step in range(8):
                for p, a, t in zip(params, grads, fixed):
                    if moving:
                        p.grad = torch.from_numpy(a.copy()).cuda()
                        hold.append(p.grad)
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
    sec = mxr.compress(grads[0].reshape(-1), mx.FP4, mxr.sign_words(1), None, np.zeros(grads[0].size, f32), f32(api._ef_scale(1)))[0]
    if not random:
        assert np.array_equal(we[0][qe.offsets[0]:qe.offsets[0] + sec.size], sec)


@pytest.mark.parametrize("fmt", ["fp4", "fp8"])
def test_per_tensor_compress(fmt):
    """MXCompressor.compress on one tensor: the inverse-rotated dense decode; decompress is the identity."""
    from gq_amd.compressors import MXCompressor
    n = 5000
    v = mxr.gradients(n, 31)
    t = torch.from_numpy(v).cuda().view(50, 100)
    c = MXCompressor(n, t.shape, api.make_args(mx_format=fmt, mx_rotate="hadamard", mx_rotate_seed=SEED))
    d = c.decompress(c.compress(t))
    want = mxr.compress(v, FMT[fmt], mxr.sign_words(SEED))[1]
    assert d.shape == t.shape and mx.same(d.cpu().numpy().reshape(-1), want)
    with pytest.raises(ValueError):
        MXCompressor(n, t.shape, api.make_args(mx_rotate="givens"))


def test_rotate_none_is_todays_wire_byte_for_byte():
    from gq_amd.codecs import BatchedMX
    from gq_amd.quantizers import Quantizer
    grads = api._grads(6, 3, 2)
    q0, _, aggs0, wires0 = api._run(Quantizer, grads, ef=True)
    q1, _, aggs1, wires1 = api._run(Quantizer, grads, ef=True, mx_rotate="none", mx_rotate_seed=9)
    q2, _, aggs2, wires2 = api._run(Quantizer, grads, ef=True, mx_rotate=None)
    assert [g[0] for g in q1._groups] == [g[0] for g in q2._groups] == [BatchedMX]
    for a, b, c in zip(wires0, wires1, wires2):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    api._check_aggs(aggs1, aggs0)
    api._check_aggs(aggs2, aggs0)


@pytest.mark.timeout(600)
def test_train_py_runs_mx_rotated():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "mx", "--mx-rotate", "hadamard", "--network", "fcn", "--dataset", "mnist",
           "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
