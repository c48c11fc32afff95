"""Per-user rotations through the public interface on the MI355X: Quantizer(DriveCompressor / EdenCompressor, ...) on the FCN shapes
with drive_user_rotation / eden_user_rotation = 'own' against the parameter server stepped in numpy under
tests/rot_user_contract.py's streams -- four users over four rounds (plain, ef, two_phase; graphs on and off; the fixed and the
stepped rotation), the per-tensor route, 'shared' against a quantizer built without the argument, ring mode's refusal, and train.py.
The gradients are finite, so every comparison is on all 32 bits.
(zz: behind the other GPU tests, like tests/test_gpu_zz_rot_step_api.py, whose helpers these are.)"""
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
import rot_user_contract as ru  # noqa: E402
from test_gpu_zz_drive_api import BIG, SHAPES, _ef_scale, _grads, _mean_rows  # noqa: E402
from test_gpu_zz_rot_step_api import SEED, _compressor, _kw, _run, _same_as_model  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
KINDS = ["drive", "eden2", "eden4"]
USERS = 4


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _own(kind, rotation="fixed", scale="unbiased"):
    kw = _kw(kind, scale, rotation)
    kw[("drive" if kind == "drive" else "eden") + "_user_rotation"] = "own"
    return kw


def _model(kind, grads, mode, ef=False, two_phase=False, stepped=False):
    """The parameter server stepped in numpy: user u of every round compresses under stream u at (SEED, the round's step -- 0
    throughout under the fixed rotation), the mean is DECODE-MEAN, PER STREAM from stream 0, and the two-phase re-compress, ONE
    payload, runs under stream 0."""
    users = len(grads[0])
    err = [[np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG] for _ in range(users)]
    serr = [np.zeros(int(np.prod(SHAPES[i])), f32) for i in BIG]
    aggs, secs_all = [], []
    for epoch, step in enumerate(grads):
        t = epoch if stepped else 0
        secs = [[None] * len(BIG) for _ in range(users)]
        for u, gs in enumerate(step):
            for k, i in enumerate(BIG):
                r = ru.compress(kind, gs[i].reshape(-1), mode, SEED, t, u, err[u][k] if ef else None, f32(_ef_scale(epoch)) if ef else None)
                secs[u][k] = r[0]
                if ef:
                    err[u][k] = r[3]
        out = [None] * len(SHAPES)
        for k, i in enumerate(BIG):
            n = int(np.prod(SHAPES[i]))
            m = ru.decode_mean(kind, [secs[u][k] for u in range(users)], n, SEED, t)
            if two_phase:
                r = ru.compress(kind, m, mode, SEED, t, 0, serr[k] if ef else None, f32(1.0) if ef else None)
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


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase"])
@pytest.mark.parametrize("kind", KINDS)
def test_four_users_four_rounds(kind, variant, graph):
    from gq_amd.codecs import BatchedDrive, BatchedEden
    ef, tp = variant == "ef", variant == "two_phase"
    grads = _grads(1, USERS, 4)
    q, aggs, wires = _run(kind, grads, keep_addresses=True, ef=ef, two_phase=tp, gq_graph=graph, **_own(kind))
    assert [g[0] for g in q._groups] == [BatchedDrive if kind == "drive" else BatchedEden]
    grp = q._groups[0][2]
    assert grp.own and not grp.stepped and grp.rotation is q._own_pair and q._rng_state is None
    assert q._own_pair.cpu().tolist() == [[SEED, 0]]      # (under the fixed rotation nothing steps the pair)
    want, secs = _model(kind, grads, dc.UNBIASED, ef, tp)
    _same_as_model(q, aggs, wires, want, secs)
    paths = q.record_paths
    assert sum(paths.values()) == 4 * USERS
    if not graph:
        assert paths["eager"] == 4 * USERS
    elif not ef:      # (under error feedback a record graph's key holds the round's ef scale, which changes every round here)
        assert paths["graph"] + paths["graph_any_address"] >= USERS, paths      # (a record is captured at its second sighting: the later rounds replay)


@pytest.mark.parametrize("kind", ["drive", "eden2"])
def test_equal_gradients_the_users_payloads_differ_and_the_mean_is_closer(kind):
    """Four users with the SAME gradient: under 'shared' the four payloads are the same bytes and the mean is one user's decode;
    under 'own' they differ and the mean's error is about half of it (1 / sqrt(4); tests/test_rot_user_contract.py asserts the law
    within 10%, 0.75 lies between that and 1)."""
    one = _grads(3, 1, 1)[0][0]
    grads = [[one] * USERS]
    q, aggs, wires = _run(kind, grads, **_own(kind))
    want, secs = _model(kind, grads, dc.UNBIASED)
    _same_as_model(q, aggs, wires, want, secs)
    qs, aggs_s, wires_s = _run(kind, grads, **_kw(kind, rotation="fixed"))
    i = BIG[0]
    n = int(np.prod(SHAPES[i]))
    sec = slice(q.offsets[i], q.offsets[i] + ru.section_bytes(kind, n))
    assert all(np.array_equal(wires_s[0][u][sec], wires_s[0][0][sec]) for u in range(USERS))
    assert np.array_equal(wires[0][0][sec], wires_s[0][0][sec])      # (user 0 is stream 0: the shared rotation's payload)
    assert all(not np.array_equal(wires[0][u][sec], wires[0][0][sec]) for u in range(1, USERS))
    e_own, e_shared = dc.rel_l2(aggs[0][i].reshape(-1), one[i].reshape(-1)), dc.rel_l2(aggs_s[0][i].reshape(-1), one[i].reshape(-1))
    print(kind, "equal gradients, %d users: shared %.4f own %.4f" % (USERS, e_shared, e_own))
    assert e_own < 0.75 * e_shared


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("kind", ["drive", "eden4"])
def test_own_rotations_with_the_stepped_rotation(kind, graph):
    grads = _grads(2, USERS, 3)
    q, aggs, wires = _run(kind, grads, keep_addresses=True, gq_graph=graph, **_own(kind, rotation="step"))
    grp = q._groups[0][2]
    assert grp.own and grp.stepped and grp.rotation is q._rng_state and q._own_pair is None
    want, secs = _model(kind, grads, dc.UNBIASED, stepped=True)
    _same_as_model(q, aggs, wires, want, secs)
    assert q.rotation_step() == 3


@pytest.mark.parametrize("variant", ["plain", "ef_two_phase"])
@pytest.mark.parametrize("kind", ["drive", "eden4"])
def test_per_tensor_route(kind, variant):
    """gq_no_batch: no groups, every tensor through its codec -- the pair and the record's stream reach the one-tensor launches, and
    the per-tensor re-compress of the second phase runs under stream 0."""
    ef, tp = "ef" in variant, "two_phase" in variant
    grads = _grads(2, USERS, 2)
    q, aggs, wires = _run(kind, grads, ef=ef, two_phase=tp, gq_no_batch=True, **_own(kind))
    assert not q._groups and all(q.codecs[i].rotation is q._own_pair and q.codecs[i].stream == 0 for i in BIG)
    want, secs = _model(kind, grads, dc.UNBIASED, ef, tp)
    _same_as_model(q, aggs, wires, want, secs)


@pytest.mark.parametrize("kind", ["drive", "eden4"])
def test_one_user_whole_step_graphs(kind):
    """One user, eight rounds with graphs: the whole-step graph replays, stream 0 throughout -- the stepped rotation's own values (the
    wire byte for byte, the mean but for the sign of a zero)."""
    grads = _grads(7, 1, 8)
    q, aggs, wires = _run(kind, grads, keep_addresses=True, gq_graph=True, **_own(kind, rotation="step"))
    want, secs = _model(kind, grads, dc.UNBIASED, stepped=True)
    _same_as_model(q, aggs, wires, want, secs)
    qs, aggs_s, wires_s = _run(kind, grads, keep_addresses=True, gq_graph=True, **_kw(kind, rotation="step"))
    assert all(np.array_equal(a, b) for a, b in zip(wires, wires_s))
    for a, b in zip(aggs, aggs_s):
        for x, y in zip(a, b):      # (+0 + D turns a -0 of the decode into +0; the shared order adds before the sign flip and keeps it)
            assert ((mx.bits_of(x) == mx.bits_of(y)) | ((x == 0) & (y == 0))).all()
    assert q.record_paths["whole_step"] >= 1, q.record_paths


@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase"])
@pytest.mark.parametrize("kind", ["drive", "eden2"])
def test_shared_is_a_quantizer_built_without_the_argument(kind, variant):
    ef, tp = variant == "ef", variant == "two_phase"
    grads = _grads(5, USERS, 2)
    name = ("drive" if kind == "drive" else "eden") + "_user_rotation"
    for rotation in ("fixed", "step"):
        qa, aggs_a, wires_a = _run(kind, grads, ef=ef, two_phase=tp, **dict(_kw(kind, rotation=rotation), **{name: "shared"}))
        qb, aggs_b, wires_b = _run(kind, grads, ef=ef, two_phase=tp, **_kw(kind, rotation=rotation))
        assert not qa._groups[0][2].own and qa._own_pair is None
        for a, b in zip(wires_a, wires_b):
            assert np.array_equal(a, b)
        for a, b in zip(aggs_a, aggs_b):
            for x, y in zip(a, b):
                assert np.array_equal(mx.bits_of(x), mx.bits_of(y))


def test_ring_mode_is_refused():
    from gq_amd.quantizers import Quantizer
    from test_gpu_zz_drive_api import make_args
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
    for kind in ("drive", "eden4"):
        with pytest.raises(ValueError, match="ring mode"):
            Quantizer(_compressor(kind), params, make_args(num_users=USERS, mode="ring", **_own(kind)))


@pytest.mark.timeout(600)
def test_train_py_runs_drive_with_own_rotations():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "drive", "--drive-user-rotation", "own", "--network", "fcn",
           "--dataset", "mnist", "--num-users", "4", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
