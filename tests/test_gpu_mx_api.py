"""MXCompressor through the public interface on the MI355X: Quantizer(MXCompressor, ...) on the FCN shapes with three users against
the numpy contract (tests/mx_contract.py) stepped over three records -- plain, --ef, two_phase, ring mode --, the address-tied,
address-free and whole-step graphs against eager launches bit for bit, the per-tensor compress / decompress route, and train.py."""
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

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = [(256, 784), (256,), (10, 256), (10,)]      # driver.FCN: two compressed tensors, two identity-compressed ones
BIG = [0, 2]
FMT = {"fp4": mx.FP4, "fp8": mx.FP8}


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp",
                num_users=3, mode="ps", cr=256, mx_format="fp4")
    base.update(kw)
    return Namespace(**base)


def _grads(seed, users, steps):
    """Heavy-tailed gradients with +-0 sprinkled in; step 1 of user 1 carries an inf and a NaN in the first tensor."""
    rs = np.random.RandomState(seed)
    out = []
    for st in range(steps):
        per = []
        for u in range(users):
            gs = []
            for s in SHAPES:
                n = int(np.prod(s))
                a = mx.randn(n, rs.randint(1 << 30))
                z = rs.rand(n)
                a[z < 0.03] = f32(0.0)
                a[(z >= 0.03) & (z < 0.06)] = f32(-0.0)
                gs.append(a.reshape(s))
            per.append(gs)
        out.append(per)
    if steps > 1 and users > 1:
        out[1][1][0].reshape(-1)[[5, 100000]] = [np.inf, np.nan]
    return out


def _mean_rows(rows):
    acc = np.zeros_like(rows[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for r in rows:
            acc = (acc + r).astype(f32)
        return (acc / f32(len(rows))).astype(f32)


def _ef_scale(epoch):
    return 2 / (math.exp(-epoch) + 1) - 1


def _run(cls, grads, **kw):
    from gq_amd.compressors import MXCompressor
    users = len(grads[0])
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
    q = cls(MXCompressor, params, make_args(num_users=users, **kw))
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
    return q, params, aggs, wires


def _model_ps(grads, fmt, ef=False, two_phase=False, draws=None):
    """The parameter server stepped in numpy.  draws(step, user, i) -> the tensor's uniforms or None."""
    users = len(grads[0])
    err = [[np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG] for _ in range(users)]
    serr = [np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG]
    aggs, secs_all = [], []
    for epoch, step in enumerate(grads):
        secs = [[None] * len(BIG) for _ in range(users)]
        for u, gs in enumerate(step):
            for k, i in enumerate(BIG):
                r = draws(epoch, u, i) if draws else None
                sec, D, w, ne = mx.compress(gs[i].reshape(-1), fmt, r, err[u][k] if ef else None, f32(_ef_scale(epoch)) if ef else None)
                secs[u][k] = sec
                if ef:
                    err[u][k] = ne
        out = [None] * len(SHAPES)
        for k, i in enumerate(BIG):
            n = int(np.prod(SHAPES[i]))
            m = mx.decode_mean([secs[u][k] for u in range(users)], n, fmt)
            if two_phase:
                r = draws(epoch, "server", i) if draws else None
                _, D, w, ne = mx.compress(m, fmt, r, serr[k] if ef else None, f32(1.0) if ef else None)
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


def _check_aggs(got, want):
    for st, (g, w) in enumerate(zip(got, want)):
        for i, (a, b) in enumerate(zip(g, w)):
            assert mx.same(a, b, nan_as_one=True), "step %d, parameter %d" % (st, i)


def _check_wires(q, wires, secs_all, fmt):
    for st, secs in enumerate(secs_all):
        for u in range(len(secs)):
            for k, i in enumerate(BIG):
                off = q.offsets[i]
                assert np.array_equal(wires[st][u, off:off + secs[u][k].size], secs[u][k]), "step %d, user %d, parameter %d" % (st, u, i)


@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase", "ef_two_phase"])
@pytest.mark.parametrize("fmt", ["fp4", "fp8"])
def test_psquantizer_deterministic_against_the_contract(fmt, variant):
    from gq_amd.codecs import BatchedMX, DenseCodec, MXCodec
    from gq_amd.quantizers import Quantizer
    ef, tp = "ef" in variant, "two_phase" in variant
    grads = _grads(1, 3, 3)
    q, params, aggs, wires = _run(Quantizer, grads, mx_format=fmt, ef=ef, two_phase=tp)
    assert [type(c) for c in q.codecs] == [MXCodec, DenseCodec, MXCodec, DenseCodec]
    assert [g[0] for g in q._groups] == [BatchedMX]
    assert q.wire_bytes_per_user() == sum(mx.section_bytes(int(np.prod(SHAPES[i])), FMT[fmt]) for i in BIG) + 4 * (256 + 10) + 8
    want, secs = _model_ps(grads, FMT[fmt], ef, tp)
    _check_wires(q, wires, secs, FMT[fmt])
    _check_aggs(aggs, want)


@pytest.mark.parametrize("variant", ["plain", "ef_two_phase"])
def test_psquantizer_reference_draws_against_the_contract(variant):
    """gq_rng = "reference": one torch.rand(total) per record (and per two-phase apply) from the CPU generator, a slice per tensor."""
    from gq_amd.quantizers import Quantizer
    ef = tp = variant != "plain"
    grads = _grads(2, 3, 3)
    sizes = [int(np.prod(SHAPES[i])) for i in BIG]
    torch.manual_seed(11)
    q, params, aggs, wires = _run(Quantizer, grads, random=1, gq_rng="reference", ef=ef, two_phase=tp)
    torch.manual_seed(11)
    stream = {}
    for st in range(3):
        for u in list(range(3)) + (["server"] if tp else []):
            r = torch.rand(sum(sizes)).numpy()
            stream[(st, u)] = dict(zip(BIG, np.split(r, np.cumsum(sizes)[:-1])))
    want, secs = _model_ps(grads, mx.FP4, ef, tp, draws=lambda st, u, i: stream[(st, u)][i])
    _check_wires(q, wires, secs, mx.FP4)
    _check_aggs(aggs, want)


def test_psquantizer_device_draws_follow_the_step_words():
    """gq_rng = "device" (the default): user slot u draws from its { seed, step } pair; every aggregate steps the words."""
    from gq_amd.quantizers import Quantizer
    grads = _grads(3, 3, 3)
    q, params, aggs, wires = _run(Quantizer, grads, random=1)
    state = q._rng_state.cpu().numpy().astype(np.int64)
    assert np.all(state[:3, 1] == 3), "three aggregates, three steps"
    sizes = [int(np.prod(SHAPES[i])) for i in BIG]
    first = dict(zip(BIG, [0, sizes[0]]))
    want, secs = _model_ps(grads, mx.FP4, draws=lambda st, u, i: mx.draws(mx.COUNTER, int(np.prod(SHAPES[i])), first[i],
                                                                         int(state[u, 0]) & (2 ** 64 - 1), st))
    _check_wires(q, wires, secs, mx.FP4)
    _check_aggs(aggs, want)


@pytest.mark.parametrize("fmt", ["fp4", "fp8"])
def test_ring_mode_carries_the_decoded_tensor_exactly(fmt):
    """ring_quantizer.py: user k adds the decoded running sum to its gradient and re-compresses; the result is the last decode.
    The wire carries the decoded tensor exactly, -0 and NaN blocks included."""
    from gq_amd.quantizers import Quantizer
    grads = _grads(4, 3, 3)
    q, params, aggs, wires = _run(Quantizer, grads, mx_format=fmt, mode="ring", ef=True)
    users = 3
    err = [[np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG] for _ in range(users)]
    want = []
    for epoch, step in enumerate(grads):
        running = None
        for u, gs in enumerate(step):
            with np.errstate(invalid="ignore", over="ignore"):
                cur = [(g + running[i]).astype(f32) if running is not None else g for i, g in enumerate(gs)]
            nxt = list(cur)
            for k, i in enumerate(BIG):
                _, D, w, ne = mx.compress(cur[i].reshape(-1), FMT[fmt], None, err[u][k], f32(_ef_scale(epoch)))
                err[u][k] = ne
                nxt[i] = D.reshape(SHAPES[i])
            running = nxt
        want.append(running)
    _check_aggs(aggs, want)
    assert any(np.signbit(a[0]).any() and (a[0] == 0).any() for a in aggs)


def test_momentum_correction_stays_refused():
    from gq_amd.compressors import MXCompressor
    from gq_amd.quantizers import Quantizer
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
    with pytest.raises(ValueError, match="TopKSparsificationCompressor"):
        Quantizer(MXCompressor, params, make_args(momentum_correction=0.9))


@pytest.mark.parametrize("random", [0, 1])
def test_graphs_equal_eager_launches(random):
    """One user per step: the address-tied record graph, then the whole step; moving gradients: the address-free forms.  The
    same seeds give the same bytes and the same gradients as eager launches (gq_graph off), step for step."""
    from gq_amd.compressors import MXCompressor
    from gq_amd.quantizers import PSQuantizer
    grads = _grads(5, 1, 1)[0][0]

    def run(graph, moving):
        import itertools
        from gq_amd.compressors import shared_seeds
        seeds = itertools.count(1000)      # (the quantizer's { seed, step } pairs are seeded from this stream: the same in both runs)
        with shared_seeds(lambda: next(seeds)):
            return _run(graph, moving)

    def _run(graph, moving):
        torch.manual_seed(21)
        params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
        q = PSQuantizer(MXCompressor, params, make_args(num_users=1, random=random, gq_graph=graph, ef=True))
        fixed = [torch.from_numpy(a.copy()).cuda() for a in grads]
        hold, wires, outs = [], [], []
        for step in range(8):
            for p, a, t in zip(params, grads, fixed):
                if moving:
                    p.grad = torch.from_numpy(a.copy()).cuda()
                    hold.append(p.grad)      # (kept alive: the next step's gradients land at other addresses)
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


@pytest.mark.parametrize("fmt", ["fp4", "fp8"])
def test_per_tensor_compress_decompress(fmt):
    from gq_amd.compressors import MXCompressor
    n = 5000
    v = mx.randn(n, 31)
    v[:64] = mx.edge_tensor(FMT[fmt])[0][:64]
    t = torch.from_numpy(v).cuda().view(50, 100)
    c = MXCompressor(n, t.shape, make_args(mx_format=fmt))
    d = c.decompress(c.compress(t))
    assert d.shape == t.shape and mx.same(d.cpu().numpy().reshape(-1), mx.compress(v, FMT[fmt])[1])
    # stochastic: seeded through the codec, code for code
    from gq_amd.codecs import MXCodec
    cs = MXCompressor(n, t.shape, make_args(mx_format=fmt, random=1))
    cd = MXCodec(cs, n, (n,))
    wire = torch.zeros(cd.nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(n, device="cuda")
    cd.encode_into(t.reshape(-1), wire, 0, 0, seed=99, out=out)
    sec, D, _, _ = mx.compress(v, FMT[fmt], mx.draws(mx.DEVICE, n, 0, 99))
    assert np.array_equal(wire.cpu().numpy(), sec) and mx.same(out.cpu().numpy(), D)
    assert mx.same(cd.decode_mean(wire.view(1, -1), 0, 1, plain=True).cpu().numpy(), D)
    with pytest.raises(TypeError):
        c.compress(torch.from_numpy(v))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fmt", ["fp4", "fp8"])
def test_train_py_runs_mx(fmt):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "mx", "--mx-format", fmt, "--network", "fcn", "--dataset", "mnist",
           "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
