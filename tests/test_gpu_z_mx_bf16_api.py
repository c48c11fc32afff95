"""bf16 gradients through the public interface on the MI355X: MXCompressor.compress on a bf16 tensor, and Quantizer(MXCompressor, ...)
with three users on the FCN shapes cast to bf16 plus ONE float32 layer (weight and bias both compressed) -- two groups, one per
dtype, and the bf16 identity-compressed tensors riding as float32 in the wire -- against tests/mx_bf16_contract.py stepped in numpy:
plain, error feedback, two_phase and ring mode, with and without the Hadamard rotation; eager and graph-replayed steps bit for bit;
and one train.py --param-dtype bfloat16 run.
(The three bf16 GPU files sort behind every other GPU test file, like tests/test_gpu_z_mx6_api.py, which says why: the graph tests
of tests/test_gpu_mx_api.py and tests/test_gpu_mxr_api.py depend on the free blocks earlier tests leave in torch's caching allocator.)"""
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
import mx6_contract as m6  # noqa: E402
import mx_bf16_contract as bx  # noqa: E402
import mxr_contract as mxr  # noqa: E402

pytestmark = pytest.mark.gpu

f32, U16 = np.float32, np.uint16
BF, FL = torch.bfloat16, torch.float32
# driver.FCN's four tensors in bf16, then a float32 Linear(20, 1100): its bias has more than 1000 elements and is compressed too
SHAPES = [(256, 784), (256,), (10, 256), (10,), (1100, 20), (1100,)]
DTYPES = [BF, BF, BF, BF, FL, FL]
BIG, SMALL = [0, 2, 4, 5], [1, 3]
FMT = {"fp4": m6.FP4, "fp8": m6.FP8}


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp",
                num_users=3, mode="ps", cr=256, mx_format="fp4")
    base.update(kw)
    return Namespace(**base)


def _ef_scale(epoch):
    return 2 / (math.exp(-epoch) + 1) - 1


def _grads(seed, users, steps):
    """[step][user][tensor]: uint16 bits for the bf16 parameters, float32 for the others; +-0 sprinkled in, and step 1 of user 1
    carries an inf and a NaN in the first tensor."""
    rs = np.random.RandomState(seed)
    out = []
    for st in range(steps):
        per = []
        for u in range(users):
            gs = []
            for s, dt in zip(SHAPES, DTYPES):
                n = int(np.prod(s))
                a = m6.randn(n, rs.randint(1 << 30))
                z = rs.rand(n)
                a[z < 0.03] = f32(0.0)
                a[(z >= 0.03) & (z < 0.06)] = f32(-0.0)
                gs.append(bx.narrow(a) if dt == BF else a)
            per.append(gs)
        out.append(per)
    if steps > 1 and users > 1:
        out[1][1][0][[5, 100000]] = [0x7F80, 0x7FC1]
    return out


def _to_dev(a, dt, shape):
    if dt == BF:
        return torch.from_numpy(a.view(np.int16).copy()).cuda().view(BF).view(shape)
    return torch.from_numpy(a.copy()).cuda().view(shape)


def _to_np(t):
    t = t.detach().reshape(-1)
    return t.view(torch.int16).cpu().numpy().view(U16).copy() if t.dtype == BF else t.cpu().numpy().copy()


def _params():
    return [torch.nn.Parameter(torch.zeros(s, device="cuda", dtype=dt)) for s, dt in zip(SHAPES, DTYPES)]


def _run(grads, **kw):
    from gq_amd.compressors import MXCompressor
    from gq_amd.quantizers import Quantizer
    users = len(grads[0])
    params = _params()
    q = Quantizer(MXCompressor, params, make_args(num_users=users, **kw))
    aggs, wires = [], []
    for epoch, step in enumerate(grads):
        for u, gs in enumerate(step):
            for p, a, dt, s in zip(params, gs, DTYPES, SHAPES):
                p.grad = _to_dev(a, dt, s)
            q.record(u, epoch)
        torch.cuda.synchronize()
        wires.append(q._wire.cpu().numpy().copy())
        q.apply()
        torch.cuda.synchronize()
        assert [p.grad.dtype for p in params] == DTYPES and [tuple(p.grad.shape) for p in params] == SHAPES
        aggs.append([_to_np(p.grad) for p in params])
    return q, params, aggs, wires


def _compress(i, g, fmt, signs, err, s):
    """-> (section, decoded, source afterwards, err afterwards) in the tensor's own type."""
    if DTYPES[i] == BF:
        return bx.compress(g, fmt, None, err, s, signs)
    return (m6.compress(g, fmt, None, err, s) if signs is None else m6.compress_rotated(g, fmt, signs, None, err, s)[:4])


def _decode_mean(i, secs, n, fmt, signs):
    if DTYPES[i] == BF:
        return bx.decode_mean(secs, n, fmt, False, signs)
    return m6.decode_mean(secs, n, fmt) if signs is None else m6.decode_mean_rotated(secs, n, fmt, signs)


def _mean_rows(rows):
    acc = np.zeros_like(rows[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for r in rows:
            acc = (acc + r).astype(f32)
        return (acc / f32(len(rows))).astype(f32)


def _model_ps(grads, fmt, signs=None, ef=False, two_phase=False):
    users = len(grads[0])
    sizes = [int(np.prod(s)) for s in SHAPES]
    err = [{i: np.zeros(sizes[i], f32) for i in BIG} for _ in range(users)]
    serr = {i: np.zeros(sizes[i], f32) for i in BIG}
    aggs, secs_all = [], []
    for epoch, step in enumerate(grads):
        secs = [dict() for _ in range(users)]
        for u, gs in enumerate(step):
            for i in BIG:
                sec, _, _, ne = _compress(i, gs[i], fmt, signs, err[u][i] if ef else None, f32(_ef_scale(epoch)) if ef else None)
                secs[u][i] = sec
                if ef:
                    err[u][i] = ne
        out = [None] * len(SHAPES)
        for i in BIG:
            m = _decode_mean(i, [secs[u][i] for u in range(users)], sizes[i], fmt, signs)
            if two_phase:      # the mean, in the tensor's own type, compressed again by the same group
                _, D, _, ne = _compress(i, m, fmt, signs, serr[i] if ef else None, f32(1.0) if ef else None)
                if ef:
                    serr[i] = ne
                m = D
            out[i] = m
        for i in SMALL:      # float32 in the wire (widened exactly), the float32 mean narrowed once
            out[i] = bx.narrow(_mean_rows([bx.widen(step[u][i]) for u in range(users)]))
        aggs.append(out)
        secs_all.append(secs)
    return aggs, secs_all


def _same(i, a, b):
    if DTYPES[i] == BF:
        return np.array_equal(a, b)
    return m6.same(a, b, nan_as_one=True)


def _check(q, aggs, wires, want, secs):
    for st, (got, exp) in enumerate(zip(aggs, want)):
        for i in range(len(SHAPES)):
            assert _same(i, got[i], exp[i]), "step %d, tensor %d" % (st, i)
    for st, step in enumerate(secs):
        for u, per in enumerate(step):
            for i, sec in per.items():
                assert np.array_equal(wires[st][u][q.offsets[i]:q.offsets[i] + sec.size], sec), "step %d, user %d, tensor %d: wire" % (st, u, i)


@pytest.mark.parametrize("rotate", ["none", "hadamard"])
@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase", "ef_two_phase"])
def test_psquantizer_against_the_contract(variant, rotate):
    from gq_amd.codecs import BatchedMX, BatchedMXR, DenseCodec
    ef, tp = "ef" in variant, "two_phase" in variant
    fmt = "fp8" if variant == "plain" else "fp4"
    grads = _grads(1, 3, 3)
    q, params, aggs, wires = _run(grads, mx_format=fmt, ef=ef, two_phase=tp, mx_rotate=rotate, mx_rotate_seed=5)
    cls = BatchedMXR if rotate == "hadamard" else BatchedMX
    assert [(g[0], g[1]) for g in q._groups] == [(cls, [0, 2]), (cls, [4, 5])]      # one group per dtype
    assert [g[2].dtype for g in q._groups] == [BF, FL] and [g[2].align for g in q._groups] == [2, 4]
    assert all(o % 8 == 0 for o in q._groups[0][2].out_off)
    assert [type(q.codecs[i]) for i in SMALL] == [DenseCodec, DenseCodec] and q._groups[0][2].ndense == 2
    if ef:
        assert all(e.dtype == FL for i in BIG for e in params[i].error)
    signs = mxr.sign_words(5) if rotate == "hadamard" else None
    want, secs = _model_ps(grads, FMT[fmt], signs, ef, tp)
    _check(q, aggs, wires, want, secs)
    # the identity-compressed bf16 tensors travelled as float32
    for u in range(3):
        o = q.offsets[1]
        assert np.array_equal(wires[2][u][o:o + 4 * 256].view(np.uint32), grads[2][u][1].astype(np.uint32) << np.uint32(16))


def test_ring_mode_against_the_contract():
    """ring_quantizer.py with bf16 gradients: user k adds the decoded running sum of user k - 1 (a bf16 addition: float32, rounded to
    nearest even once) and compresses again; the result is the last user's plain decode."""
    fmt = m6.FP4
    grads = _grads(2, 3, 2)
    q, params, aggs, wires = _run(grads, mode="ring")
    sizes = [int(np.prod(s)) for s in SHAPES]
    for st, step in enumerate(grads):
        running = None
        for u, gs in enumerate(step):
            cur = []
            for i in range(len(SHAPES)):
                g = gs[i]
                if running is not None:
                    with np.errstate(invalid="ignore", over="ignore"):
                        g = bx.narrow(bx.widen(g) + bx.widen(running[i])) if DTYPES[i] == BF else (g + running[i]).astype(f32)
                if i in BIG:
                    sec = _compress(i, g, fmt, None, None, None)[0]
                    dec = bx.decode_mean([sec], sizes[i], fmt, True) if DTYPES[i] == BF else m6.decode_mean([sec], sizes[i], fmt, True)
                    cur.append(dec)
                else:
                    cur.append(g)
            running = cur
        for i in range(len(SHAPES)):
            assert _same(i, aggs[st][i], running[i]), "step %d, tensor %d" % (st, i)


@pytest.mark.parametrize("rotate", ["none", "hadamard"])
@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase"])
def test_graphs_equal_eager_launches(variant, rotate):
    """Gradients that keep their storage (the address-tied record graph, the whole step, the apply graph) and gradients that move
    (the address-free forms): the same wire and the same bf16 / float32 gradients as eager launches, step for step."""
    from gq_amd.compressors import MXCompressor, shared_seeds
    from gq_amd.quantizers import PSQuantizer
    grads = _grads(5, 1, 1)[0][0]
    kw = dict(ef=variant == "ef", two_phase=variant == "two_phase", mx_rotate=rotate)

    def run(graph, moving):
        seeds = itertools.count(1000)
        with shared_seeds(lambda: next(seeds)):
            torch.manual_seed(21)
            params = _params()
            q = PSQuantizer(MXCompressor, params, make_args(num_users=1, gq_graph=graph, **kw))
            fixed = [_to_dev(a, dt, s) for a, dt, s in zip(grads, DTYPES, SHAPES)]
            hold, wires, outs = [], [], []
            for step in range(8):
                for p, a, dt, s, t in zip(params, grads, DTYPES, SHAPES, fixed):
                    if moving:
                        p.grad = _to_dev(a, dt, s)
                        hold.append(p.grad.detach())      # (an alias keeps the block: apply() rebinds p.grad.data, the next step's lands elsewhere)
                    else:
                        t.copy_(_to_dev(a, dt, s))
                        p.grad = t
                q.record(0, 1)
                q.apply()
                torch.cuda.synchronize()
                wires.append(q._wire[0].cpu().numpy().copy())
                outs.append([_to_np(p.grad) for p in params])
                assert [p.grad.dtype for p in params] == DTYPES
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
            assert all(_same(i, a, b) for i, (a, b) in enumerate(zip(oe[st], og[st]))), "step %d (moving %s): the gradients" % (st, moving)


@pytest.mark.parametrize("mode", ["ps", "ring"])
def test_graphs_equal_eager_launches_three_users(mode):
    """Three users per step, gradients that keep their storage per user, parameter-server and ring mode: the record graphs (one per
    user; ps: also the apply graph) against eager launches, wire and gradients bit for bit.  Ring mode has the record route only:
    a hop's decode and the final rebind are eager, and no whole-step graph exists for it (asserted)."""
    from gq_amd.compressors import MXCompressor, shared_seeds
    from gq_amd.quantizers import Quantizer
    users, steps = 3, 6
    grads = [g[0] for g in _grads(6, 1, users)]      # [user][tensor]

    def run(graph):
        seeds = itertools.count(1000)
        with shared_seeds(lambda: next(seeds)):
            torch.manual_seed(21)
            params = _params()
            q = Quantizer(MXCompressor, params, make_args(num_users=users, gq_graph=graph, mode=mode))
            fixed = [[_to_dev(a, dt, s) for a, dt, s in zip(gs, DTYPES, SHAPES)] for gs in grads]
            wires, outs = [], []
            for step in range(steps):
                for u in range(users):
                    for p, a, dt, s, t in zip(params, grads[u], DTYPES, SHAPES, fixed[u]):
                        t.copy_(_to_dev(a, dt, s))      # (ring mode adds the running sum into the gradient in place)
                        p.grad = t
                    q.record(u, 1)
                    torch.cuda.synchronize()
                    wires.append(q._wire.cpu().numpy().copy())
                q.apply()
                torch.cuda.synchronize()
                outs.append([_to_np(p.grad) for p in params])
                assert [p.grad.dtype for p in params] == DTYPES
                # apply() rebound the last user's tensors to the aggregate: that user gets storage of its own again (new addresses every
                # step: the address-free record graph), the others keep theirs (the address-tied one)
                fixed[users - 1] = [t.clone() for t in fixed[users - 1]]
            return q, wires, outs

    qe, we, oe = run(False)
    qg, wg, og = run(True)
    pe, pg = qe.record_paths, qg.record_paths
    assert sum(pe.values()) == pe["eager"] == steps * users and sum(pg.values()) == steps * users, (pe, pg)
    assert pg["graph"] + pg["graph_any_address"] >= users, pg
    if mode == "ring":
        assert pg["whole_step"] + pg["whole_step_any_address"] == 0 and qg.graph_counts()["apply"] == 0, (pg, qg.graph_counts())
    for k, (a, b) in enumerate(zip(we, wg)):
        assert np.array_equal(a, b), "record %d: the wire" % k
    for st in range(steps):
        assert all(_same(i, a, b) for i, (a, b) in enumerate(zip(oe[st], og[st]))), "step %d: the gradients" % st


@pytest.mark.parametrize("rotate", [None, "hadamard"])
@pytest.mark.parametrize("fmt", ["fp4", "fp6_e2m3", "fp6_e3m2", "fp8"])
def test_compressor_compress_takes_and_returns_bf16(fmt, rotate):
    from gq_amd.compressors import MXCompressor
    n = 4097 + 300
    c = MXCompressor(n, (n,), Namespace(mx_format=fmt, random=0, mx_rotate=rotate, mx_rotate_seed=1))
    g = bx.edge_gradient(n, 41)
    t = torch.from_numpy(g.view(np.int16).copy()).cuda().view(BF)
    out = c.compress(t)
    assert out.dtype == BF and out.shape == t.shape and c.decompress(out) is out
    want = bx.compress(g, {v: k for k, v in m6.NAMES.items()}[fmt], None, None, None, mxr.sign_words(1) if rotate else None)[1]
    assert np.array_equal(_to_np(out), want)
    assert np.array_equal(_to_np(t), g), "compress changed its input"
    assert c.compress(t.view(n // 1, 1)).shape == (n, 1)
    f = c.compress(torch.from_numpy(bx.widen(g)).cuda())
    assert f.dtype == FL      # the float32 route is untouched; where both are finite the two agree exactly without rotation
    for bad in (t.cpu(), t.to(torch.float16), t.to(torch.float64)):
        with pytest.raises(TypeError):
            c.compress(bad)


@pytest.mark.timeout(600)
def test_train_py_runs_in_bf16():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "mx", "--param-dtype", "bfloat16", "--network", "fcn", "--dataset", "mnist",
           "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
