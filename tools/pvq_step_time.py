#!/usr/bin/env python3
"""Timing of the probabilistic vector compressor's parameter-server step and of its multi-tensor encode (MI355X).

    python tools/pvq_step_time.py [--out profiles/pvq_step_time.jsonl] [--steps 40] [--rounds 5]

One process, the paths alternated round by round (the clock of the box drifts within a run), medians over the rounds:
  * ResNet-50 list, one user, record + apply, d16 k8 n6, gq_rng = "device": the path before this codec existed (GenericCodec
    forced through codec_factory: per-tensor compress, decompress, dense f32 on the wire) against PVQCodec / BatchedPVQ,
    eager launches and replayed graphs; wall time per step around a device synchronisation, wire bytes per user.
  * the multi-tensor encode alone over the ResNet-50 list against gq_pvq_encode on ONE tensor of the same element count, HIP
    events around single launches, inputs rotated so that nothing is read from a warm cache -- and, to say where the difference
    sits, the same multi-tensor kernel over other tables of the same element count: ONE tensor (the per-tile look-up and fold
    without any raggedness), 76 equal tensors (tensor changes without small tensors), and the list sorted by size.
Writes one JSON line per measurement (the file is rewritten)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))

import torch  # noqa: E402

from gq_amd import native  # noqa: E402
from gq_amd.codecs import DenseCodec, GenericCodec  # noqa: E402
from gq_amd.compressors import IdenticalCompressor, ProbabilisticVectorCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402


def make_args(**kw):
    from argparse import Namespace
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=1, ef=False, two_phase=False, scale="exp", num_users=1, mode="ps",
                cr=256, gq_rng="device")
    base.update(kw)
    return Namespace(**base)


def generic_factory(comp, numel, shape, packed6=False):
    return DenseCodec(comp, numel, shape) if isinstance(comp, IdenticalCompressor) else GenericCodec(comp, numel, shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvq_step_time.jsonl"))
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    cus, arch = native.device_info(0)
    box = {"arch": arch, "cus": cus, "torch": torch.__version__}
    rows = []

    # ---- the step
    paths = {}
    for name, kw, factory in (("generic_eager", dict(gq_graph=False), generic_factory), ("pvq_eager", dict(gq_graph=False), None),
                              ("pvq_replayed", dict(), None)):
        params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
        g = torch.Generator(device=dev).manual_seed(1)
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-2
        q = PSQuantizer(ProbabilisticVectorCompressor, params, make_args(**kw), **({"codec_factory": factory} if factory else {}))
        grads = [p.grad for p in params]

        def rebind(params=params, grads=grads):
            # apply() rebinds the DATA of the tensor object in p.grad to the mean: a fresh alias of the pristine gradient per step, so
            # that every step compresses the same numbers at the same addresses (the aliases' cost is in every path: rebind_us)
            for p, t in zip(params, grads):
                p.grad = t.detach()
        paths[name] = (q, params, rebind)
    times = {k: [] for k in paths}
    for rnd in range(a.rounds + 1):
        for name, (q, params, rebind) in paths.items():
            n = max(4, a.steps // (8 if name == "generic_eager" else 1))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                rebind()
                q.record(0, 1)
                q.apply()
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / n * 1e6
            if rnd:      # round 0 warms up (graph captures, allocations)
                times[name].append(us)
    t0 = time.perf_counter()
    for _ in range(50):
        paths["pvq_replayed"][2]()
    rebind_us = (time.perf_counter() - t0) / 50 * 1e6
    for name, (q, params, _) in paths.items():
        rows.append(dict(what="resnet50_step_record_apply", path=name, us_per_step_median=round(statistics.median(times[name]), 2),
                         us_per_step_all=[round(t, 2) for t in times[name]], wire_bytes_per_user=q.wire_bytes_per_user(),
                         record_paths=dict(q.record_paths), rebind_us=round(rebind_us, 2), **box))

    # ---- the encode alone
    q = paths["pvq_eager"][0]
    grp = q._groups[0][2]
    total = sum(c.numel for c in grp.codecs)
    M = total // 16
    cd0 = grp.codecs[0]
    _, cdag = cd0.c._on(dev)
    NSETS = 3
    sets = [[torch.randn(c.numel, device=dev) * 1e-2 for c in grp.codecs] for _ in range(NSETS)]
    flats = [torch.randn(total, device=dev) * 1e-2 for _ in range(NSETS)]
    wire = torch.zeros(q.wire_bytes_per_user(), dtype=torch.uint8, device=dev)
    codes = torch.empty(M, dtype=torch.uint8, device=dev)
    u = torch.empty(M, dtype=torch.float32, device=dev)
    ws = native.new_workspace(dev, M)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"batched": [], "flat": []}
    for it in range(3 + 6 * a.rounds):
        k = it % NSETS
        assert grp._upload(sets[k], 0, grp.align)
        torch.cuda.synchronize()
        ev[0].record()
        grp._batch.encode(wire, None, native.RANDOM_DEVICE, 12345 + it)
        ev[1].record()
        torch.cuda.synchronize()
        tb = ev[0].elapsed_time(ev[1]) * 1e3
        ev[0].record()
        native.pvq_encode(flats[k], cdag, codes, u, ws, native.RANDOM_DEVICE, None, 12345 + it)
        ev[1].record()
        torch.cuda.synchronize()
        tf = ev[0].elapsed_time(ev[1]) * 1e3
        if it >= 3:
            res["batched"].append(tb)
            res["flat"].append(tf)
    # the same kernel over other tables of (about) the same element count
    from gq_amd.codecs import BatchedPVQ, PVQCodec

    def group_of(sizes):
        cds = [PVQCodec(ProbabilisticVectorCompressor(n, torch.Size([n]), make_args()), n, torch.Size([n])) for n in sizes]
        offs, off = [], 0
        for cd in cds:
            offs.append(off)
            off += (cd.nbytes + 15) // 16 * 16
        return BatchedPVQ(cds, offs, list(range(len(cds))), dev, 1, off), off

    list_sizes = [c.numel for c in grp.codecs]
    each = total // 76 // 1024 * 1024
    variants = {"one_tensor": [total], "76_equal_tensors": [each] * 76, "list_sorted_descending": sorted(list_sizes, reverse=True),
                "list_as_it_is": list_sizes}
    var_res = {}
    for vname, sizes in variants.items():
        g2, nbytes = group_of(sizes)
        w2 = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        ins = [[torch.randn(n, device=dev) * 1e-2 for n in sizes] for _ in range(NSETS)]
        ts = []
        for it in range(3 + 4 * a.rounds):
            assert g2._upload(ins[it % NSETS], 0, g2.align)
            torch.cuda.synchronize()
            ev[0].record()
            g2._batch.encode(w2, None, native.RANDOM_DEVICE, 999 + it)
            ev[1].record()
            torch.cuda.synchronize()
            if it >= 3:
                ts.append(ev[0].elapsed_time(ev[1]) * 1e3)
        var_res[vname] = dict(elements=sum(sizes), tiles=int(g2.ntiles), us_median=round(statistics.median(ts), 2), us_min=round(min(ts), 2))
        del g2, w2, ins
    mb, mf = statistics.median(res["batched"]), statistics.median(res["flat"])
    rows.append(dict(what="pvq_encode_alone_resnet50_list_vs_flat", elements=total, tensors=len(grp.codecs), us_batched_median=round(mb, 2),
                     us_flat_median=round(mf, 2), batched_over_flat=round(mb / mf, 4), us_batched_min=round(min(res["batched"]), 2),
                     us_flat_min=round(min(res["flat"]), 2), same_kernel_other_tables=var_res, timing="hip events around one launch, inputs rotated over %d sets" % NSETS, **box))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
