"""Rotation stepping through the public interface on the MI355X: Quantizer(DriveCompressor / EdenCompressor, ...) on the FCN shapes
with drive_rotation / eden_rotation = 'step' against the numpy contracts stepped on the CPU under tests/rot_step_contract.py's words
-- three users over four rounds (plain, ef, two_phase; graphs on and off), the graph paths, a resume by set_rotation_step, 64 rounds
on one gradient, and train.py.  The gradients are finite, so every comparison is on all 32 bits.
(zz: behind the other GPU tests, like tests/test_gpu_zz_drive_api.py.)"""
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
import drive_contract as dc  # noqa: E402
import eden_contract as ec  # noqa: E402
import rot_step_contract as rs  # noqa: E402
from test_gpu_zz_drive_api import BIG, SHAPES, _ef_scale, _grads, _mean_rows, make_args  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = 5
KINDS = ["drive", "eden2", "eden4"]


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _compressor(kind):
    from gq_amd.compressors import DriveCompressor, EdenCompressor
    return DriveCompressor if kind == "drive" else EdenCompressor


def _kw(kind, scale="unbiased", rotation="step"):
    if kind == "drive":
        return dict(drive_scale=scale, drive_seed=SEED, drive_rotation=rotation)
    return dict(eden_scale=scale, eden_seed=SEED, eden_rotation=rotation, eden_bits=int(kind[-1]))


def _compress(kind, g, mode, signs, err=None, s=None):
    """-> (section, D, w, err afterwards)"""
    r = dc.compress(g, mode, signs, err, s) if kind == "drive" else ec.compress(g, int(kind[-1]), mode, signs, err, s)
    return r[0], r[1], r[2], r[3]


def _decode_mean(kind, secs, n, signs):
    return dc.decode_mean(secs, n, signs) if kind == "drive" else ec.decode_mean(secs, n, int(kind[-1]), signs)


def _model(kind, grads, mode, ef=False, two_phase=False, first_step=0, ef_scale=None):
    """The parameter server stepped in numpy: round t rotates by step_words(SEED, first_step + t), its re-compress too.
    ef_scale: a constant error-feedback scale (args.scale as a number) instead of the 'exp' schedule."""
    users = len(grads[0])
    err = [[np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG] for _ in range(users)]
    serr = [np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG]
    aggs, secs_all = [], []
    for epoch, step in enumerate(grads):
        signs = rs.step_words(SEED, first_step + epoch)
        secs = [[None] * len(BIG) for _ in range(users)]
        for u, gs in enumerate(step):
            for k, i in enumerate(BIG):
                sec, D, w, ne = _compress(kind, gs[i].reshape(-1), mode, signs, err[u][k] if ef else None,
                                          f32(_ef_scale(epoch) if ef_scale is None else ef_scale) if ef else None)
                secs[u][k] = sec
                if ef:
                    err[u][k] = ne
        out = [None] * len(SHAPES)
        for k, i in enumerate(BIG):
            n = int(np.prod(SHAPES[i]))
            m = _decode_mean(kind, [secs[u][k] for u in range(users)], n, signs)
            if two_phase:
                _, D, w, ne = _compress(kind, m, mode, signs, serr[k] if ef else None, f32(1.0) if ef else None)
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


def _run(kind, grads, keep_addresses=False, first_step=None, first_epoch=0, **kw):
    """record / apply over grads[round][user][tensor] -> (quantizer, param.grad after every apply, the wire before every apply)"""
    from gq_amd.quantizers import Quantizer
    users = len(grads[0])
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
    q = Quantizer(_compressor(kind), params, make_args(num_users=users, **kw))
    if first_step is not None:
        q.set_rotation_step(first_step)
    fixed = [[torch.zeros(s, device="cuda") for s in SHAPES] for _ in range(users)]
    aggs, wires, hold = [], [], []
    for epoch, step in enumerate(grads):
        for u, gs in enumerate(step):
            for p, a, t in zip(params, gs, fixed[u]):
                if keep_addresses:
                    t.copy_(torch.from_numpy(a))
                    p.grad = t.detach()      # (an alias: apply() rebinds the gradient object, the storage keeps its address)
                else:
                    p.grad = torch.from_numpy(a.copy()).cuda()
                    hold.append(p.grad.view(-1))      # (kept alive: these addresses never come back)
            q.record(u, first_epoch + epoch)
        torch.cuda.synchronize()
        wires.append(q._wire.cpu().numpy().copy())
        q.apply()
        torch.cuda.synchronize()
        aggs.append([p.grad.detach().cpu().numpy().copy() for p in params])
    return q, aggs, wires


def _same_as_model(q, aggs, wires, want, secs, what=""):
    for st in range(len(want)):
        for u in range(len(secs[st])):
            for k, i in enumerate(BIG):
                got = wires[st][u][q.offsets[i]:q.offsets[i] + secs[st][u][k].size]
                assert np.array_equal(got, secs[st][u][k]), "%sround %d, user %d, tensor %d: the wire section" % (what, st, u, i)
        for i in range(len(SHAPES)):
            assert mx.same(aggs[st][i], want[st][i]), "%sround %d, tensor %d: param.grad after apply()" % (what, st, i)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase"])
@pytest.mark.parametrize("kind", KINDS)
def test_three_users_four_rounds(kind, variant, graph):
    from gq_amd.codecs import BatchedDrive, BatchedEden
    ef, tp = variant == "ef", variant == "two_phase"
    grads = _grads(1, 3, 4)
    q, aggs, wires = _run(kind, grads, keep_addresses=True, ef=ef, two_phase=tp, gq_graph=graph, **_kw(kind))
    assert [g[0] for g in q._groups] == [BatchedDrive if kind == "drive" else BatchedEden]
    assert q._groups[0][2].stepped and q._groups[0][2].rotation is q._rng_state and tuple(q._rng_state.shape) == (1, 2)
    want, secs = _model(kind, grads, dc.UNBIASED, ef, tp)
    _same_as_model(q, aggs, wires, want, secs)
    assert q.rotation_step() == 4
    paths = q.record_paths
    assert sum(paths.values()) == 12
    if not graph:
        assert paths["eager"] == 12
    elif not ef:      # (under error feedback a record graph's key holds the round's ef scale, which changes every round here)
        assert paths["graph"] + paths["graph_any_address"] >= 3, paths      # (a record is captured at its second sighting: round 2 on replays)
    # and the rounds differ: the same gradients one round later are compressed under other words
    assert rs.step_words(SEED, 0) != rs.step_words(SEED, 1)


@pytest.mark.parametrize("kind", ["drive", "eden2"])
def test_record_graphs_replay_under_error_feedback(kind):
    """A constant error-feedback scale keeps the record graph's key the same from round to round: three users, eight rounds, the
    stepped compress with error feedback replays from its graphs and stays the contract's."""
    grads = _grads(4, 3, 8)
    q, aggs, wires = _run(kind, grads, keep_addresses=True, ef=True, scale="0.5", gq_graph=True, **_kw(kind))
    want, secs = _model(kind, grads, dc.UNBIASED, ef=True, ef_scale=0.5)
    _same_as_model(q, aggs, wires, want, secs)
    assert q.rotation_step() == 8
    assert q.record_paths["graph"] + q.record_paths["graph_any_address"] >= 12 and q.graph_counts()["apply"] >= 1, (q.record_paths, q.graph_counts())


@pytest.mark.parametrize("variant", ["plain", "two_phase", "ef_two_phase"])
@pytest.mark.parametrize("kind", ["drive", "eden4"])
def test_per_tensor_route(kind, variant):
    """gq_no_batch: no groups, every tensor through its codec -- the pair reaches the one-tensor launches, and with two_phase the step
    moves in a launch of its own BEHIND the per-tensor re-compress (which therefore rotates by the round's own words)."""
    ef, tp = "ef" in variant, "two_phase" in variant
    grads = _grads(2, 3, 3)
    q, aggs, wires = _run(kind, grads, ef=ef, two_phase=tp, gq_no_batch=True, **_kw(kind))
    assert not q._groups and all(q.codecs[i].rotation is q._rng_state for i in BIG)
    want, secs = _model(kind, grads, dc.UNBIASED, ef, tp)
    _same_as_model(q, aggs, wires, want, secs)
    assert q.rotation_step() == 3


@pytest.mark.parametrize("moving", [False, True], ids=["addresses_kept", "addresses_new"])
@pytest.mark.parametrize("kind", ["drive", "eden4"])
def test_graph_paths_keep_replaying(kind, moving):
    """One user, ten rounds: the record graph, the apply graphs and the whole-step graph -- tied to the gradients' addresses, or
    address-free when they never come back -- replay, and every round is the contract's at that round's step."""
    grads = _grads(7, 1, 10)
    q, aggs, wires = _run(kind, grads, keep_addresses=not moving, gq_graph=True, **_kw(kind))
    want, secs = _model(kind, grads, dc.UNBIASED)
    _same_as_model(q, aggs, wires, want, secs)
    assert q.rotation_step() == 10
    paths, counts = q.record_paths, q.graph_counts()
    assert sum(paths.values()) == 10 and paths["eager"] <= 3, paths
    if moving:
        assert paths["graph_any_address"] + paths["whole_step_any_address"] >= 5, paths
        assert paths["whole_step_any_address"] >= 1 and counts["whole_step_any_address"] >= 1, (paths, counts)
    else:
        assert paths["graph"] + paths["whole_step"] >= 5, paths
        assert paths["whole_step"] >= 1 and counts["whole_step"] >= 1, (paths, counts)


@pytest.mark.parametrize("kind", ["drive", "eden2"])
def test_apply_graphs_replay_with_three_users(kind):
    """Three users: no whole-step graph, so the aggregate replays from its own apply graphs (two, one per output-buffer turn)."""
    grads = _grads(3, 3, 8)
    q, aggs, wires = _run(kind, grads, keep_addresses=True, gq_graph=True, **_kw(kind))
    want, secs = _model(kind, grads, dc.UNBIASED)
    _same_as_model(q, aggs, wires, want, secs)
    assert q.rotation_step() == 8
    assert q.graph_counts()["apply"] >= 1 and q.record_paths["graph"] >= 12, (q.graph_counts(), q.record_paths)


@pytest.mark.parametrize("kind", ["drive", "eden4"])
def test_set_rotation_step_reproduces_a_round(kind):
    grads = _grads(1, 3, 4)
    want, _ = _model(kind, grads, dc.UNBIASED)
    q, aggs, _ = _run(kind, grads[2:3], first_step=2, first_epoch=2, **_kw(kind))
    for i in range(len(SHAPES)):
        assert mx.same(aggs[0][i], want[2][i]), "tensor %d: round 3 on a fresh quantizer set to step 2" % i
    assert q.rotation_step() == 3
    q.set_rotation_step(0)
    assert q.rotation_step() == 0
    with pytest.raises(ValueError, match="rotation is fixed"):
        _run(kind, grads[:1], **_kw(kind, rotation="fixed"))[0].rotation_step()


@pytest.mark.parametrize("kind,scale", [("drive", "unbiased"), ("eden2", "unbiased")])
def test_sixty_four_rounds_on_one_gradient(kind, scale):
    """The experiment the flag exists for: one user, one fixed gradient, 64 rounds.  Every applied gradient is the restatement's at
    that round's step, so the running mean and its error are the CPU's bit for bit (the figures are printed; the law they follow
    is tests/test_rot_step_contract.py's business)."""
    g = _grads(9, 1, 1)[0]
    rounds = 64
    q, aggs, _ = _run(kind, [g] * rounds, keep_addresses=True, **_kw(kind, scale))
    assert q.rotation_step() == rounds
    i, n = 0, int(np.prod(SHAPES[0]))
    flat = g[0][i].reshape(-1)
    acc_gpu, acc_cpu = np.zeros(n, np.float64), np.zeros(n, np.float64)
    errs = {}
    for t in range(rounds):
        D = _compress(kind, flat, dc.MODES[scale], rs.step_words(SEED, t))[1]
        assert mx.same(aggs[t][i].reshape(-1), D), "round %d: the applied gradient" % t
        acc_gpu += aggs[t][i].reshape(-1)
        acc_cpu += D
        if t + 1 in (1, 4, 16, 64):
            assert np.array_equal(acc_gpu, acc_cpu)
            errs[t + 1] = float(np.linalg.norm(acc_gpu / (t + 1) - flat) / np.linalg.norm(flat.astype(np.float64)))
    print(kind, scale, "error of the running mean:", " ".join("T=%d %.4f" % kv for kv in sorted(errs.items())))
    assert q.record_paths["whole_step"] >= 32, q.record_paths


@pytest.mark.timeout(600)
def test_train_py_runs_drive_with_a_stepped_rotation():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "drive", "--drive-rotation", "step", "--network", "fcn", "--dataset",
           "mnist", "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
