#!/usr/bin/env python3
"""Timing of the residual compressor's parameter-server step and of its two own launches (MI355X).

    python tools/rq_step_time.py [--out profiles/rq_step_time.jsonl] [--steps 40] [--rounds 5]

One process, the paths alternated round by round (the clock of the box drifts within a run), medians over the rounds:
  * ResNet-50 list, one user, record + apply, d16 k8 n6, gq_rng = "device": the path before this codec existed (GenericCodec
    forced through codec_factory: ResidualCompressor.compress / decompress per tensor, dense f32 on the wire) against
    ResidualCodec / BatchedResidual, eager launches and replayed graphs; a fresh alias of every gradient per step in all paths;
    wall time per step around a device synchronisation, wire bytes per user.
  * stage 2's multi-tensor encode alone against gq_pvq_encode_batched over the same elements (it reads stage 1's codes, levels
    and (lb, ub) from the wire besides), HIP events around single launches, inputs rotated;
  * the two-stage decode-mean at R = 1 and R = 8 against gq_hsq_decode_sum_batched over one stage's sections (half the bytes).
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
from gq_amd.codecs import BatchedPVQ, DenseCodec, GenericCodec, PVQCodec  # noqa: E402
from gq_amd.compressors import IdenticalCompressor, ProbabilisticVectorCompressor, ResidualCompressor  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rq_step_time.jsonl"))
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
    for name, kw, factory in (("generic_eager", dict(gq_graph=False), generic_factory), ("rq_eager", dict(gq_graph=False), None),
                              ("rq_replayed", dict(), None)):
        params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
        g = torch.Generator(device=dev).manual_seed(1)
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-2
        q = PSQuantizer(ResidualCompressor, params, make_args(**kw), **({"codec_factory": factory} if factory else {}))
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
        paths["rq_replayed"][2]()
    rebind_us = (time.perf_counter() - t0) / 50 * 1e6
    for name, (q, params, _) in paths.items():
        rows.append(dict(what="resnet50_step_record_apply", path=name, us_per_step_median=round(statistics.median(times[name]), 2),
                         us_per_step_all=[round(t, 2) for t in times[name]], wire_bytes_per_user=q.wire_bytes_per_user(),
                         record_paths=dict(q.record_paths), rebind_us=round(rebind_us, 2), **box))

    # ---- stage 2's encode alone, against the PVQ group's encode over the same elements
    q = paths["rq_eager"][0]
    grp = q._groups[0][2]
    sizes = [c.numel for c in grp.codecs]
    total = sum(sizes)
    NSETS = 3
    sets = [[torch.randn(n, device=dev) * 1e-2 for n in sizes] for _ in range(NSETS)]
    R = 8
    wires = torch.zeros((R, q.wire_bytes_per_user()), dtype=torch.uint8, device=dev)
    for r in range(R):      # real payloads in all R rows (stage 1 + stage 2)
        assert grp.encode(sets[r % NSETS], wires[r], 0, 1000 + r)
    pv = [PVQCodec(ProbabilisticVectorCompressor(n, torch.Size([n]), make_args()), n, torch.Size([n])) for n in sizes]
    offs, off = [], 0
    for cd in pv:
        offs.append(off)
        off += (cd.nbytes + 15) // 16 * 16
    pgrp = BatchedPVQ(pv, offs, list(range(len(pv))), dev, 1, off)
    pwire = torch.zeros(off, dtype=torch.uint8, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    res = {"rq": [], "pvq": []}
    for it in range(3 + 6 * a.rounds):
        k = it % NSETS
        assert grp._upload(sets[k], 0, grp.align)
        grp._batch.b1.encode(wires[0], None)
        grp._batch.b1.levels(wires[0], native.RANDOM_DEVICE, 77 + it)
        t_rq = timed(lambda: grp._batch.encode2(wires[0], native.RANDOM_DEVICE, 12345 + it))
        assert pgrp._upload(sets[k], 0, pgrp.align)
        t_pv = timed(lambda: pgrp._batch.encode(pwire, None, native.RANDOM_DEVICE, 12345 + it))
        if it >= 3:
            res["rq"].append(t_rq)
            res["pvq"].append(t_pv)
    m_rq, m_pv = statistics.median(res["rq"]), statistics.median(res["pvq"])
    rows.append(dict(what="rq_stage2_encode_alone_resnet50_list_vs_pvq_encode_batched", elements=total, tensors=len(sizes),
                     us_rq_median=round(m_rq, 2), us_pvq_median=round(m_pv, 2), rq_over_pvq=round(m_rq / m_pv, 4),
                     us_rq_min=round(min(res["rq"]), 2), us_pvq_min=round(min(res["pvq"]), 2),
                     timing="hip events around one launch, inputs rotated over %d sets" % NSETS, **box))

    # ---- the decode-mean against the HSQ decode-mean over stage 1's sections alone
    out = torch.empty(total, dtype=torch.float32, device=dev)
    for Rn in (1, 8):
        t_rq, t_hs = [], []
        for it in range(3 + 6 * a.rounds):
            t_rq.append(timed(lambda: grp._batch.decode(wires[:Rn], Rn, out)))
            t_hs.append(timed(lambda: grp._batch.b1.decode(wires[:Rn], Rn, out)))
        t_rq, t_hs = t_rq[3:], t_hs[3:]
        rows.append(dict(what="rq_decode_mean_vs_hsq_decode_mean", R=Rn, elements=total, us_rq_median=round(statistics.median(t_rq), 2),
                         us_hsq_median=round(statistics.median(t_hs), 2),
                         rq_over_hsq=round(statistics.median(t_rq) / statistics.median(t_hs), 4), us_rq_min=round(min(t_rq), 2),
                         us_hsq_min=round(min(t_hs), 2), timing="hip events around one launch", **box))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
