"""CountSketchCompressor through the public interface on the MI355X: Quantizer(CountSketchCompressor, ...) on the FCN shapes with three
users, with and without sketch_ef, against the numpy contract (tests/sketch_contract.py) over three steps; a replayed graph against
eager launches; the refusals; the parser's flags.
(zz: the file runs behind the other GPU tests, like the test_gpu_z_* files.)"""
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import sketch_contract as sc  # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
FCN = [(256, 784), (256,), (10, 256), (10,)]      # driver.FCN: one sketched tensor (the per-tensor route), three that travel as they are
WIDE = [(256, 784), (256,), (128, 256), (10,)]    # two sketched tensors: one group, whose launches replay from graphs
USERS, CR, C, SEED = 3, 64, 4, 5


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=USERS, mode="ps", cr=CR,
                sketch_rows=3, sketch_cr=C, sketch_seed=SEED, sketch_ef=False)
    base.update(kw)
    return Namespace(**base)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(u32), np.ascontiguousarray(b, f32).view(u32))


def mean_rows(rows):
    acc = np.zeros_like(rows[0])
    for r in rows:
        acc = (acc + r).astype(f32)
    return (acc / f32(len(rows))).astype(f32)


@pytest.mark.parametrize("shapes", [FCN, WIDE], ids=["fcn", "wide"])
@pytest.mark.parametrize("ef", [False, True])
def test_quantizer_against_the_contract(shapes, ef):
    from gq_amd.compressors import CountSketchCompressor
    from gq_amd.quantizers import Quantizer
    rs = np.random.RandomState(3)
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes]
    q = Quantizer(CountSketchCompressor, params, make_args(sketch_ef=ef))
    big = [i for i, s in enumerate(shapes) if sc.sketched(int(np.prod(s)), 3, C)]
    assert big == ([0] if shapes is FCN else [0, 2]) and len(q._groups) == (0 if shapes is FCN else 1)
    E = {i: (np.zeros(sc.section_bytes(int(np.prod(shapes[i])), 3, C) // 4 - 4, f32) if ef else None) for i in big}
    for step in range(3):
        grads = [[rs.standard_normal(s).astype(f32) for s in shapes] for _ in range(USERS)]
        for u in range(USERS):
            for p, g in zip(params, grads[u]):
                p.grad = torch.from_numpy(g.copy()).cuda()
            q.record(u, step)
        q.apply()
        torch.cuda.synchronize()
        for i, s in enumerate(shapes):
            n = int(np.prod(s))
            if i in big:
                tabs = [sc.sketch(grads[u][i].reshape(-1), SEED, 3, sc.layout(n, 3, C)[1]) for u in range(USERS)]
                want, E[i] = sc.decode_mean(tabs, n, n // CR, SEED, E[i])
            else:
                want = mean_rows([grads[u][i].reshape(-1) for u in range(USERS)])
            assert same(params[i].grad.cpu().numpy().reshape(-1), want), (step, i)
        if ef:
            got = q.sketch_errors()
            assert sorted(got) == big and all(same(got[i].numpy(), E[i]) for i in big), step
    if ef:
        q.set_sketch_errors({i: torch.from_numpy(E[i] * 2) for i in big})
        assert all(same(q.sketch_errors()[i].numpy(), E[i] * 2) for i in big)
    else:
        assert q.sketch_errors() == {}


def test_graphs_equal_eager_launches():
    from gq_amd.compressors import CountSketchCompressor
    from gq_amd.quantizers import PSQuantizer
    rs = np.random.RandomState(4)
    gs = [[rs.standard_normal(s).astype(f32) for s in WIDE] for _ in range(6)]

    def run(graph):
        params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in WIDE]
        q = PSQuantizer(CountSketchCompressor, params, make_args(num_users=1, gq_graph=graph, sketch_ef=True))
        fixed = [torch.zeros(s, device="cuda") for s in WIDE]
        outs = []
        for step in range(6):
            for p, a, t in zip(params, gs[step], fixed):
                t.copy_(torch.from_numpy(a))
                p.grad = t
            q.record(0, 1)
            q.apply()
            torch.cuda.synchronize()
            outs.append([p.grad.detach().cpu().numpy().copy() for p in params] + [e.numpy() for e in q.sketch_errors().values()])
        return q, outs

    qe, oe = run(False)
    qg, og = run(True)
    assert qe.record_paths["eager"] == 6 and qg.record_paths["eager"] < 6, qg.record_paths      # (some step replayed from a graph)
    for st in range(6):
        assert all(same(a, b) for a, b in zip(oe[st], og[st])), st


@pytest.mark.parametrize("kw,text", [(dict(ef=True), "ef is not available"), (dict(two_phase=True), "two_phase is not available"),
                                     (dict(momentum_correction=0.9), "momentum_correction is not available with the sketch"),
                                     (dict(mode="ring"), "not available in ring mode"), (dict(sketch_rows=2), "sketch_rows")])
def test_refusals(kw, text):
    from gq_amd.compressors import CountSketchCompressor
    from gq_amd.quantizers import PSQuantizer, RingQuantizer
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in FCN]
    with pytest.raises(ValueError, match=text):
        (RingQuantizer if kw.get("mode") == "ring" else PSQuantizer)(CountSketchCompressor, params, make_args(**kw))


def test_bfloat16_other_layouts_exchange_modes_and_flags(monkeypatch):
    from gq_amd import driver
    from gq_amd.compressors import CountSketchCompressor
    from gq_amd.quantizers import PSQuantizer
    with pytest.raises(ValueError, match="float32 parameters only"):
        PSQuantizer(CountSketchCompressor, [torch.nn.Parameter(torch.zeros(256, 784, device="cuda", dtype=torch.bfloat16))], make_args())
    # a payload sketched under another layout (here: as if with five rows) is refused where the payloads of one mean meet
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in FCN]
    q = PSQuantizer(CountSketchCompressor, params, make_args(num_users=2))
    for u in range(2):
        for p in params:
            p.grad = torch.ones_like(p)
        q.record(u, 0)
    q._wire[1, q.offsets[0] + 4:q.offsets[0] + 8] = torch.tensor([5, 0, 0, 0], dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="must share the shapes, the rows"):
        q.apply()
    monkeypatch.setenv("GQ_EXCHANGE", "split")
    with pytest.raises(ValueError, match="GQ_EXCHANGE must be allgather or direct"):
        PSQuantizer(CountSketchCompressor, params, make_args())
    assert driver.quantizer_choices["sketch"] is CountSketchCompressor
    a = driver.build_parser().parse_args(["--quantizer", "sketch", "--sketch-rows", "5", "--sketch-cr", "8", "--sketch-seed", "7", "--sketch-ef"])
    assert (a.sketch_rows, a.sketch_cr, a.sketch_seed, a.sketch_ef) == (5, 8, 7, True)
    d = driver.build_parser().parse_args(["--quantizer", "sketch"])
    assert (d.sketch_rows, d.sketch_cr, d.sketch_seed, d.sketch_ef) == (3, 32, 0, False)
