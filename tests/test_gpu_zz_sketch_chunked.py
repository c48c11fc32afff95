"""--sketch-recover chunked on the MI355X through Quantizer against tests/sketch_chunked_contract.py, BIT FOR BIT as
tests/test_gpu_zz_sketch_contract.py holds the global recovery -- but where an estimate is a NaN the test asks for a NaN, not for its
sign and payload (an Inf and a NaN are among the inputs: csrc/sparse_kernels.hpp states key_of's rule for them; the host and the
device name the NaN of inf - inf differently).  (zz: the file runs behind the other GPU tests.)"""
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sketch_chunked_contract as scc  # noqa: E402
import sketch_contract as sc  # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32, SEED, C = np.float32, np.uint32, 5, 32


def quantizer(ns, cls=None, **kw):
    from gq_amd.compressors import CountSketchCompressor
    from gq_amd.quantizers import Quantizer
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=1, mode="ps", cr=64,
                sketch_rows=3, sketch_cr=C, sketch_seed=SEED, sketch_ef=False)
    params = [torch.nn.Parameter(torch.zeros(n, device="cuda")) for n in ns]
    return (cls or Quantizer)(CountSketchCompressor, params, Namespace(**dict(base, **kw))), params


def sizes(rows):      # two sketched tensors (2 r items, the fewest, the last ragged; 13 items + 17 elements), one that travels as it is
    return [4096 * (2 * rows - 1) + 1234, 4096 * 13 + 17, 2000]


def same(got, want):
    got, want = (np.ascontiguousarray(a, f32).reshape(-1) for a in (got, want))
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got.view(u32)[~np.isnan(want)], want.view(u32)[~np.isnan(want)])


def inputs(kind, n, rs):      # equal: every cell a multiple of 1.5, the items' threshold keys tie; zero: every key 0, the first len // cr kept as +-0
    w = {"gauss": rs.standard_normal(n), "equal": np.full(n, 1.5), "zero": np.where(rs.rand(n) < 0.5, -0.0, 0.0)}[kind].astype(f32)
    if kind == "gauss":
        w[[100, n - 7]] = [np.inf, np.nan]
    return w


def apply(q, params, grads):
    for u, user in enumerate(grads):
        for p, g in zip(params, user):
            p.grad = torch.from_numpy(g.copy()).cuda()
        q.record(u, 0)
    q.apply()
    return [p.grad.cpu().numpy() for p in params]


@pytest.mark.parametrize("cr", [2, 7, 256, 4096])      # (256: the 17-element tail keeps nothing; 4096: neither ragged tail does)
@pytest.mark.parametrize("R,ef", [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize("rows", [1, 3, 5])
def test_chunked_recovery_against_the_restatement(rows, R, ef, cr):
    """Three applies: Gaussian, all equal, all +-0 -- with --sketch-ef (no Inf / NaN then) the restatement's three rounds of E."""
    ns, rs = sizes(rows), np.random.RandomState(rows * 100 + cr)
    q, params = quantizer(ns, num_users=R, sketch_rows=rows, cr=cr, sketch_recover="chunked", sketch_ef=ef)
    E = [np.zeros(sc.section_bytes(n, rows, C) // 4 - 4, f32) if ef else None for n in ns[:2]]
    for kind in ("equal", "zero", "equal") if ef else ("gauss", "equal", "zero"):
        grads = [[inputs(kind, n, rs) for n in ns] for _ in range(R)]
        got = apply(q, params, grads)
        for i, n in enumerate(ns[:2]):
            want, E[i] = scc.decode_mean([sc.sketch(g[i], SEED, rows, 1) for g in grads], n, cr, SEED, E[i])
            assert same(got[i], want) and (not ef or same(q.sketch_errors()[i].numpy(), E[i])), (kind, i)
        assert same(got[2], sc.mean_table([g[2] for g in grads])), kind
    assert len(q._groups) == 1 and not {"est", "hist", "state", "counts", "dec_table"} & set(q._groups[0][2]._tables)      # (n floats saved)


def test_default_is_the_global_recovery_and_chunked_refuses_cr_outside_an_item():
    ns = sizes(3)
    g = [np.random.RandomState(n).standard_normal(n).astype(f32) for n in ns]
    for kw in ({}, {"sketch_recover": "global"}, {"cr": 4097}):
        q, params = quantizer(ns, **kw)
        got = apply(q, params, [g])
        for i, n in enumerate(ns[:2]):
            assert same(got[i], sc.decode_mean([sc.sketch(g[i], SEED, 3, 1)], n, n // kw.get("cr", 64), SEED)[0]), (kw, i)
    for cr in (1, 4097):
        with pytest.raises(ValueError, match="cr must be in 2 ... 4096"):
            quantizer(ns, cr=cr, sketch_recover="chunked")


def test_graph_replays_equal_eager_launches():
    from gq_amd.quantizers import PSQuantizer
    ns, rs = [sizes(3)[0], 256, sizes(3)[1], 10], np.random.RandomState(4)      # (the small ones: the packed dense region, which a graph takes along)
    gs = [[rs.standard_normal(n).astype(f32) for n in ns] for _ in range(6)]
    outs = {}
    for graph in (False, True):
        q, params = quantizer(ns, PSQuantizer, gq_graph=graph, cr=7, sketch_recover="chunked", sketch_ef=True)
        fixed = [torch.zeros(n, device="cuda") for n in ns]
        for step in range(6):
            for p, a, t in zip(params, gs[step], fixed):
                t.copy_(torch.from_numpy(a))
                p.grad = t
            q.record(0, 1)
            q.apply()
            outs[graph, step] = [p.grad.detach().cpu().numpy().copy() for p in params] + [e.numpy() for e in q.sketch_errors().values()]
        assert q.record_paths["eager"] == 6 if not graph else q.record_paths["eager"] <= 4, q.record_paths      # (two replays at least)
    assert all(same(a, b) for st in range(6) for a, b in zip(outs[False, st], outs[True, st]))
