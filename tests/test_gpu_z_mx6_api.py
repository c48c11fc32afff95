"""MXCompressor with the two 6-bit formats through the public interface on the MI355X: Quantizer(MXCompressor, ...) on the FCN shapes
with three users against the numpy contract (tests/mx6_contract.py) stepped over three records at tolerance 0 -- plain, --ef,
two_phase, ring mode, --mx-rotate hadamard --, replayed graphs against eager launches bit for bit, the per-tensor compress /
decompress route, and train.py.  The stepping harness is tests/test_gpu_mx_api.py's.
The file's name sorts behind every other GPU test file on purpose.  test_graphs_equal_eager_launches of tests/test_gpu_mx_api.py and
tests/test_gpu_mxr_api.py expects a step's fresh gradients at addresses the quantizer has not seen.  apply() rebinds
`param.grad.data` to the aggregate, so the block a gradient was allocated in goes back to torch's caching allocator at every
step although the test keeps the tensor object, and the next step's allocation takes the smallest free block that fits, the one
at the lowest address among equals.  Whether that is the block just released -- then every step brings the same address set, the
quantizer ties its graphs to it and the test's address-free paths are never taken -- depends on the free blocks that earlier
tests of the process left in the pools.  test_per_tensor_compress_decompress below allocates and frees small blocks of its own;
run in front of those tests it makes them fail, behind them it cannot."""
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
import mx6_contract as m6  # noqa: E402
import mxr_contract as mxr  # noqa: E402
import test_gpu_mx_api as api  # noqa: E402  (the harness: _grads, _run, _mean_rows, _ef_scale, _check_aggs, _check_wires)

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES, BIG = api.SHAPES, api.BIG
FMT = {"fp6_e2m3": m6.FP6_E2M3, "fp6_e3m2": m6.FP6_E3M2}
NAMES = sorted(FMT)


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _model_ps(grads, fmt, ef=False, two_phase=False, signs=None):
    """The parameter server stepped in numpy (to nearest); signs: the rotation of include/gq_mxr.h in front."""
    users = len(grads[0])
    sizes = {i: int(np.prod(SHAPES[i])) for i in BIG}
    err = [{i: np.zeros(sizes[i], f32) for i in BIG} for _ in range(users)]
    serr = {i: np.zeros(sizes[i], f32) for i in BIG}

    def comp(v, e, s):
        if signs is None:
            return m6.compress(v, fmt, None, e, s)
        return m6.compress_rotated(v, fmt, signs, None, e, s)[:4]

    aggs, secs_all = [], []
    for epoch, step in enumerate(grads):
        secs = [[None] * len(BIG) for _ in range(users)]
        for u, gs in enumerate(step):
            for k, i in enumerate(BIG):
                sec, D, w, ne = comp(gs[i].reshape(-1), err[u][i] if ef else None, f32(api._ef_scale(epoch)) if ef else None)
                secs[u][k] = sec
                if ef:
                    err[u][i] = ne
        out = [None] * len(SHAPES)
        for k, i in enumerate(BIG):
            ss = [secs[u][k] for u in range(users)]
            m = m6.decode_mean(ss, sizes[i], fmt) if signs is None else m6.decode_mean_rotated(ss, sizes[i], fmt, signs)
            if two_phase:
                _, D, w, ne = comp(m, serr[i] if ef else None, f32(1.0) if ef else None)
                if ef:
                    serr[i] = ne
                m = D
            out[i] = m.reshape(SHAPES[i])
        for i in range(len(SHAPES)):
            if i not in BIG:
                out[i] = api._mean_rows([step[u][i] for u in range(users)])
        aggs.append(out)
        secs_all.append(secs)
    return aggs, secs_all


@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase", "ef_two_phase"])
@pytest.mark.parametrize("fmt", NAMES)
def test_psquantizer_against_the_contract(fmt, variant):
    from gq_amd.codecs import BatchedMX, DenseCodec, MXCodec
    from gq_amd.quantizers import Quantizer
    ef, tp = "ef" in variant, "two_phase" in variant
    grads = api._grads(1, 3, 3)
    q, params, aggs, wires = api._run(Quantizer, grads, mx_format=fmt, ef=ef, two_phase=tp)
    assert [type(c) for c in q.codecs] == [MXCodec, DenseCodec, MXCodec, DenseCodec]
    assert [g[0] for g in q._groups] == [BatchedMX]
    assert q.wire_bytes_per_user() == sum(m6.section_bytes(int(np.prod(SHAPES[i])), FMT[fmt]) for i in BIG) + 4 * (256 + 10) + 8
    want, secs = _model_ps(grads, FMT[fmt], ef, tp)
    api._check_wires(q, wires, secs, FMT[fmt])
    api._check_aggs(aggs, want)


@pytest.mark.parametrize("variant", ["plain", "ef_two_phase"])
@pytest.mark.parametrize("fmt", NAMES)
def test_psquantizer_behind_the_hadamard_rotation(fmt, variant):
    from gq_amd.codecs import BatchedMXR
    from gq_amd.quantizers import Quantizer
    ef = tp = variant != "plain"
    grads = api._grads(6, 3, 3)
    q, params, aggs, wires = api._run(Quantizer, grads, mx_format=fmt, ef=ef, two_phase=tp, mx_rotate="hadamard", mx_rotate_seed=1)
    assert [g[0] for g in q._groups] == [BatchedMXR]
    want, secs = _model_ps(grads, FMT[fmt], ef, tp, signs=mxr.sign_words(1))
    api._check_wires(q, wires, secs, FMT[fmt])
    api._check_aggs(aggs, want)


def test_psquantizer_device_draws_follow_the_step_words():
    from gq_amd.quantizers import Quantizer
    grads = api._grads(3, 3, 2)
    q, params, aggs, wires = api._run(Quantizer, grads, random=1, mx_format="fp6_e2m3")
    state = q._rng_state.cpu().numpy().astype(np.int64)
    sizes = [int(np.prod(SHAPES[i])) for i in BIG]
    first = dict(zip(BIG, [0, sizes[0]]))
    for st, step in enumerate(grads):
        for u, gs in enumerate(step):
            for i in BIG:
                n = int(np.prod(SHAPES[i]))
                r = m6.draws(m6.COUNTER, n, first[i], int(state[u, 0]) & (2 ** 64 - 1), st)
                sec = m6.compress(gs[i].reshape(-1), m6.FP6_E2M3, r)[0]
                off = q.offsets[i]
                assert np.array_equal(wires[st][u, off:off + sec.size], sec), "step %d, user %d, parameter %d" % (st, u, i)


@pytest.mark.parametrize("fmt", NAMES)
def test_ring_mode_carries_the_decoded_tensor_exactly(fmt):
    from gq_amd.compressors import MXCompressor
    from gq_amd.quantizers import Quantizer
    grads = api._grads(4, 3, 3)
    q, params, aggs, wires = api._run(Quantizer, grads, mx_format=fmt, mode="ring", ef=True)
    err = [[np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG] for _ in range(3)]
    want = []
    for epoch, step in enumerate(grads):
        running = None
        for u, gs in enumerate(step):
            with np.errstate(invalid="ignore", over="ignore"):
                cur = [(g + running[i]).astype(f32) if running is not None else g for i, g in enumerate(gs)]
            nxt = list(cur)
            for k, i in enumerate(BIG):
                _, D, w, ne = m6.compress(cur[i].reshape(-1), FMT[fmt], None, err[u][k], f32(api._ef_scale(epoch)))
                err[u][k] = ne
                nxt[i] = D.reshape(SHAPES[i])
            running = nxt
        want.append(running)
    api._check_aggs(aggs, want)
    with pytest.raises(ValueError, match="ring mode"):
        Quantizer(MXCompressor, params, api.make_args(mode="ring", mx_format=fmt, mx_rotate="hadamard"))      # (out of scope: stays refused)


@pytest.mark.parametrize("fmt", NAMES)
def test_graphs_equal_eager_launches(fmt):
    """Stochastic rounding from the { seed, step } words with error feedback: replayed graphs (record, then the whole step) write
    the bytes and the gradients of eager launches, step for step."""
    import itertools
    from gq_amd.compressors import MXCompressor, shared_seeds
    from gq_amd.quantizers import PSQuantizer
    grads = api._grads(5, 1, 1)[0][0]

    def run(graph):
        seeds = itertools.count(1000)
        with shared_seeds(lambda: next(seeds)):
            torch.manual_seed(21)
            params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
            q = PSQuantizer(MXCompressor, params, api.make_args(num_users=1, random=1, gq_graph=graph, ef=True, mx_format=fmt))
            fixed = [torch.from_numpy(a.copy()).cuda() for a in grads]
            wires, outs = [], []
            for step in range(8):
                for p, a, t in zip(params, grads, fixed):
                    t.copy_(torch.from_numpy(a))
                    p.grad = t
                q.record(0, 1)
                q.apply()
                torch.cuda.synchronize()
                wires.append(q._wire[0].cpu().numpy().copy())
                outs.append([p.grad.detach().cpu().numpy().copy() for p in params])
            return q, wires, outs

    qe, we, oe = run(False)
    qg, wg, og = run(True)
    pe, pg = qe.record_paths, qg.record_paths
    assert sum(pe.values()) == pe["eager"] == 8
    assert pg["eager"] <= 3 and sum(pg.values()) == 8 and pg["graph"] + pg["whole_step"] >= 1, pg
    for st in range(8):
        assert np.array_equal(we[st], wg[st]), "step %d: the wire" % st
        assert all(m6.same(a, b) for a, b in zip(oe[st], og[st])), "step %d: the gradients" % st
    assert not np.array_equal(wg[0], wg[1]), "a replay drew afresh"


@pytest.mark.parametrize("fmt", NAMES)
def test_per_tensor_compress_decompress(fmt):
    from gq_amd.codecs import MXCodec
    from gq_amd.compressors import MXCompressor
    n = 5000      # (157 blocks: the section ends with the 8 pad bytes)
    v = m6.randn(n, 31)
    v[:64] = m6.edge_tensor(FMT[fmt])[0][:64]
    t = torch.from_numpy(v).cuda().view(50, 100)
    c = MXCompressor(n, t.shape, api.make_args(mx_format=fmt))
    d = c.decompress(c.compress(t))
    assert d.shape == t.shape and m6.same(d.cpu().numpy().reshape(-1), m6.compress(v, FMT[fmt])[1])
    cs = MXCompressor(n, t.shape, api.make_args(mx_format=fmt, random=1))
    cd = MXCodec(cs, n, (n,))
    wire = torch.full((cd.nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    out = torch.empty(n, device="cuda")
    cd.encode_into(t.reshape(-1), wire, 0, 0, seed=99, out=out)
    sec, D, _, _ = m6.compress(v, FMT[fmt], m6.draws(m6.DEVICE, n, 0, 99))
    assert np.array_equal(wire.cpu().numpy(), sec) and m6.same(out.cpu().numpy(), D)
    assert m6.same(cd.decode_mean(wire.view(1, -1), 0, 1, plain=True).cpu().numpy(), D)
    # behind the rotation: the inverse-rotated dense decode
    cr = MXCompressor(n, t.shape, api.make_args(mx_format=fmt, mx_rotate="hadamard", mx_rotate_seed=7))
    dr = cr.decompress(cr.compress(t))
    assert m6.same(dr.cpu().numpy().reshape(-1), m6.compress_rotated(v, FMT[fmt], mxr.sign_words(7))[1])


@pytest.mark.timeout(600)
def test_train_py_runs_mx_fp6():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "mx", "--mx-format", "fp6_e2m3", "--network", "fcn", "--dataset", "mnist",
           "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
