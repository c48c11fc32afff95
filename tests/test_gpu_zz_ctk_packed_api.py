"""ChunkTopKCompressor with ctk_values = "packed16" through the public interface on the MI355X, on test_gpu_zz_ctk_api.py's shapes, gradients
and stepping: Quantizer(ChunkTopKCompressor, ...) with one and three users against the numpy contract (tests/ctk_packed_contract.py) over
three records -- plain, ef, two_phase --, graph replay against eager launches byte for byte, the per-tensor calls, the wire's size, the
refusal of another format and one short train.py run.  The gradients are finite: all 32 bits are compared."""
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
import ctk_packed_contract as pc  # noqa: E402
import topk_contract as tc  # noqa: E402
from test_gpu_zz_ctk_api import BIG, CR, SHAPES, STEPS, _run, grads, make_args  # noqa: E402, F401  (grads: the module's fixture)

pytestmark = pytest.mark.gpu

f32 = np.float32
PACKED = dict(ctk_values="packed16")


def _compress(v, err, s):
    """-> (section, dense decode, the new err)"""
    w, D, e = pc.error_feedback(v, err, s, CR) if err is not None else (v, pc.dense(v, CR), None)
    return pc.section_bytes(w, CR), D, e


@pytest.mark.parametrize("users", [1, 3])
@pytest.mark.parametrize("variant", ["plain", "ef", "two_phase"])
def test_psquantizer_against_the_contract(grads, variant, users):
    from gq_amd.codecs import BatchedChunkTopK
    ef, tp = variant == "ef", variant == "two_phase"
    q, aggs, wires = _run(grads, users, ef=ef, two_phase=tp, **PACKED)
    assert [g[0] for g in q._groups] == [BatchedChunkTopK] and all(q.codecs[i].values == "packed16" for i in BIG)
    err = {(u, i): np.zeros(int(np.prod(SHAPES[i])), f32) if ef else None for u in range(users + 1) for i in BIG}      # (user `users`: the server)
    for epoch, step in enumerate(grads):
        for i in BIG:
            n, secs = int(np.prod(SHAPES[i])), []
            for u in range(users):
                sec, _, err[u, i] = _compress(step[u][i].reshape(-1), err[u, i], f32(2 / (math.exp(-epoch) + 1) - 1))
                secs.append(sec)
                assert np.array_equal(wires[epoch][u][q.offsets[i]:q.offsets[i] + sec.size], sec), "step %d, user %d, tensor %d: the wire" % (epoch, u, i)
            want = pc.decode_mean(secs, n, CR)
            if tp:
                _, want, err[users, i] = _compress(want, err[users, i], f32(1.0))
            assert np.array_equal(tc.bits(aggs[epoch][i]), tc.bits(want)), "step %d, tensor %d: the aggregate" % (epoch, i)


def test_graphs_equal_eager_launches(grads):
    """Gradients in storage that stays: the same bytes and the same gradients with graphs on and off over six steps under error feedback."""
    from gq_amd.compressors import ChunkTopKCompressor
    from gq_amd.quantizers import PSQuantizer

    def run(graph):
        params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
        q = PSQuantizer(ChunkTopKCompressor, params, make_args(num_users=1, gq_graph=graph, ef=True, **PACKED))
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


def test_per_tensor_compress_wire_size_and_refusal():
    from gq_amd.compressors import ChunkTopKCompressor
    from gq_amd.driver import build_parser
    from gq_amd.quantizers import PSQuantizer
    v = tc.heavy_tailed(5000, 31)
    t = torch.from_numpy(v).cuda().view(50, 100)
    c = ChunkTopKCompressor(5000, t.shape, make_args(**PACKED))
    assert np.array_equal(tc.bits(c.decompress(c.compress(t)).cpu().numpy()), tc.bits(pc.dense(v, CR)))
    sizes = {}
    for values in ("f32", "packed16"):
        params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in SHAPES]
        sizes[values] = PSQuantizer(ChunkTopKCompressor, params, make_args(ctk_values=values)).wire_bytes_per_user()
    dense = 4 * sum(int(np.prod(SHAPES[i])) for i in range(len(SHAPES)) if i not in BIG)
    assert sizes["packed16"] < sizes["f32"] and sizes["packed16"] >= sum(pc.section_size(int(np.prod(SHAPES[i])), CR) for i in BIG) + dense
    assert build_parser().parse_args(["--quantizer", "chunktopk", "--ctk-values", "packed16"]).ctk_values == "packed16"
    assert build_parser().parse_args(["--quantizer", "chunktopk"]).ctk_values == "f32"
    for bad in ("fp16", None, 16):
        with pytest.raises(ValueError, match="ctk_values"):
            ChunkTopKCompressor(5000, (5000,), make_args(ctk_values=bad))


@pytest.mark.timeout(600)
def test_train_py_runs_packed16_with_error_feedback():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "chunktopk", "--ctk-values", "packed16", "--cr", "64", "--ef", "--network", "fcn",
           "--dataset", "mnist", "--num-users", "2", "--epochs", "1", "--train-size", "512", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [json.loads(ln).get("loss") for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert [v for v in losses if v is not None] and all(math.isfinite(v) for v in losses if v is not None), r.stdout[-2000:]
