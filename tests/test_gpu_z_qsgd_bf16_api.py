"""bf16 parameters through Quantizer(QSGDCompressor, ...) on the MI355X: the FCN shapes in bf16 plus one float32 layer (two groups,
one per dtype; the bf16 identity-compressed tensors ride as float32), three users.  The reference is the float32 run on the widened
gradients: the wire is its wire byte for byte, every mean its mean narrowed once (round to nearest even, in numpy), residuals
its residuals -- plain, with error feedback, two-phase, TernGrad's wide buckets, replayed from the step graphs; and one train.py run.
One user: record + apply replayed as ONE whole-step graph.  QSGDCompressor.compress / decompress on a bf16 tensor."""
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
pytestmark = pytest.mark.gpu

f32, U16 = np.float32, np.uint16
BF, FL = torch.bfloat16, torch.float32
SHAPES = [(256, 784), (256,), (10, 256), (10,), (1280, 20), (1280,)]
DTYPES = [BF, BF, BF, BF, FL, FL]
USERS, STEPS = 3, 4


def narrow(x):
    b = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    r = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(U16)
    return np.where((b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000), U16(0x7FC0), r)


def widen(h):
    return (np.asarray(h, U16).astype(np.uint32) << np.uint32(16)).view(f32)


def _grads():
    """[step][user][tensor] float32 values that bf16 holds exactly (float32 tensors: any), zeros of both signs sprinkled in"""
    rs = np.random.RandomState(7)
    out = []
    for _ in range(STEPS):
        per = []
        for _ in range(USERS):
            gs = []
            for s, dt in zip(SHAPES, DTYPES):
                a = rs.standard_normal(int(np.prod(s))).astype(f32)
                z = rs.rand(a.size)
                a[z < 0.03], a[(z >= 0.03) & (z < 0.06)] = f32(0.0), f32(-0.0)
                gs.append(widen(narrow(a)) if dt == BF else a)
            per.append(gs)
        out.append(per)
    return out


GRADS = _grads()


def _run(dtypes, nsteps=STEPS, **kw):
    """-> per step: (the wire of all users, the means as float32 numpy, the residuals of user 0), and the quantizer"""
    from gq_amd.compressors import QSGDCompressor
    from gq_amd.quantizers import Quantizer
    base = dict(c_dim=128, k_bit=8, n_bit=2, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=USERS, mode="ps",
                cr=256, gq_graph=False)
    base.update(kw)
    users = base["num_users"]
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda", dtype=dt)) for s, dt in zip(SHAPES, dtypes)]
    q = Quantizer(QSGDCompressor, params, Namespace(**base))
    keep = [[torch.zeros(s, device="cuda", dtype=dt) for s, dt in zip(SHAPES, dtypes)] for _ in range(users)]      # gradients that keep their addresses
    steps = []
    for epoch in range(nsteps):
        step = GRADS[epoch % STEPS]
        for u, gs in enumerate(step[:users]):
            for p, a, t in zip(params, gs, keep[u]):
                t.copy_(torch.from_numpy(a).cuda().view(t.shape))      # (exact: the bf16 tensors' values are bf16 values)
                p.grad = t
            q.record(u, epoch)
        torch.cuda.synchronize()
        wire = q._wire.cpu().numpy().copy()
        q.apply()
        torch.cuda.synchronize()
        assert [p.grad.dtype for p in params] == list(dtypes)
        errs = [p.error[0].float().cpu().numpy().reshape(-1).copy() for p in params] if base["ef"] else None
        steps.append((wire, [p.grad.float().cpu().numpy().reshape(-1).copy() for p in params], errs))
    return steps, q


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


CASES = {"plain": {}, "ef": {"ef": True}, "terngrad_ef": {"c_dim": 0, "n_bit": 1, "ef": True}}


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_bf16_model_steps_as_the_float32_model_on_the_widened_gradients(case):
    ref, _ = _run([FL] * 6, **CASES[case])
    got, q = _run(DTYPES, **CASES[case])
    groups = sorted((cls.__name__, str(obj.dtype), idx) for cls, idx, obj in q._groups)
    assert groups == [("BatchedQSGD", "torch.bfloat16", [0, 2]), ("BatchedQSGD", "torch.float32", [4, 5])]
    if CASES[case].get("ef"):
        assert all(e.dtype == FL for i in (0, 2, 4, 5) for e in q.parameters[i].error)      # (the compressed tensors)
    for (w0, m0, e0), (w1, m1, e1) in zip(ref, got):
        assert np.array_equal(w0, w1), "the wire is the float32 run's"
        for i, dt in enumerate(DTYPES):
            want = widen(narrow(m0[i])) if dt == BF else m0[i]
            assert np.array_equal(_bits(want), _bits(m1[i])), "mean of tensor %d" % i
            if e0 is not None:
                assert np.array_equal(_bits(e0[i]), _bits(e1[i])), "residual of tensor %d" % i


def test_replayed_step_graphs_give_the_eager_steps():
    eager, _ = _run(DTYPES, ef=True, scale="1.0", gq_graph=False)      # (a constant scale: the graphs are keyed by it)
    graph, q = _run(DTYPES, ef=True, scale="1.0", gq_graph=True)
    assert q.record_paths["eager"] < USERS * STEPS and sum(q.graph_counts().values()) > 0, (q.record_paths, q.graph_counts())
    for (w0, m0, e0), (w1, m1, e1) in zip(eager, graph):
        assert np.array_equal(w0, w1)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(m0 + e0, m1 + e1))


def test_one_user_replays_whole_step_graphs():
    """record + apply of one user as ONE graph (the whole-step graphs need one payload per step)"""
    eager, _ = _run(DTYPES, nsteps=12, num_users=1, gq_graph=False)      # (a step graph is captured at the second sighting of a replayed record)
    graph, q = _run(DTYPES, nsteps=12, num_users=1, gq_graph=True)
    counts = q.graph_counts()
    assert counts["whole_step"] + counts["whole_step_any_address"] > 0, (counts, q.record_paths)
    assert q.record_paths["whole_step"] + q.record_paths["whole_step_any_address"] > 0, q.record_paths
    for (w0, m0, _), (w1, m1, _) in zip(eager, graph):
        assert np.array_equal(w0, w1)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(m0, m1))


def test_error_feedback_with_two_phase_keeps_a_float32_server_residual():
    """the second phase under error feedback: sum and residual inside the launch, from the unrounded sum.  The reference: the
    float32 model stepped on the same widened gradients has the same first-phase wire; its mean, narrowed, is what the server adds
    its residual to -- here only what is defined without it is held: wire, dtypes, and that the residual is no bf16 value."""
    ref, _ = _run([FL] * 6, ef=True, two_phase=True)
    got, q = _run(DTYPES, ef=True, two_phase=True)
    assert all(q.parameters[i].server_error.dtype == FL for i in (0, 2, 4, 5))
    assert np.array_equal(ref[0][0], got[0][0]), "the first step's wire is the float32 run's"
    se = q.parameters[0].server_error.cpu().numpy().reshape(-1)
    assert np.isfinite(se).all() and (_bits(se) & 0xFFFF).any(), "the residual was rounded to bf16"


def test_the_compressor_takes_a_bf16_tensor():
    from gq_amd.compressors import QSGDCompressor
    g = torch.from_numpy(GRADS[0][0][0]).cuda()      # (bf16 values held as float32)
    c = QSGDCompressor(g.numel(), SHAPES[0], Namespace(c_dim=128, n_bit=2, random=0, no_cuda=False))
    want = c.decompress(c.compress(g.view(SHAPES[0]))).cpu().numpy()
    got = c.decompress(c.compress(g.to(BF).view(SHAPES[0])))
    assert got.dtype == BF and tuple(got.shape) == SHAPES[0]
    assert np.array_equal(_bits(widen(narrow(want))), _bits(got.float().cpu().numpy()))


def test_two_phase_recompresses_the_narrowed_mean():
    from gq_amd.compressors import QSGDCompressor
    from gq_amd.codecs import QSGDCodec
    one, _ = _run(DTYPES, two_phase=False)
    two, q = _run(DTYPES, two_phase=True)
    args = q.args
    for (_, m1, _), (_, m2, _) in zip(one, two):
        for i in (0, 2):       # the bf16 group: decompress(compress(mean)) of the float32 codec on the bf16 mean, narrowed once
            n = m1[i].size
            codec = QSGDCodec(QSGDCompressor(n, SHAPES[i], args), n, SHAPES[i])
            want = codec.roundtrip(torch.from_numpy(m1[i]).cuda(), 0).cpu().numpy().reshape(-1)
            assert np.array_equal(_bits(widen(narrow(want))), _bits(m2[i])), "tensor %d" % i


def test_train_py_runs_qsgd_in_bf16():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "qsgd", "--param-dtype", "bfloat16", "--c-dim", "128", "--n-bit", "2",
           "--network", "fcn", "--dataset", "mnist", "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [json.loads(ln)["loss"] for ln in r.stdout.splitlines() if ln.startswith("{") and "loss" in json.loads(ln)]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
