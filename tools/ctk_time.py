"""Time chunked top-k's two launches (libgq_ctk.so) on one MI355X against the launches of an older build -- say the parent commit's
libgq_topk.so, libgq_thr.so and libgq_stc.so -- loaded into the same process:

    python tools/ctk_time.py --parent-lib DIR [--out FILE]      (DIR holds the three files; default FILE: profiles/ctk_time.jsonl)

Rows (one JSON line each), cr = 256, N(0, 1) gradients: single_25m (one 25 M-element tensor) and resnet50_list (the 76 tensors over
1,000 elements of tests/golden/resnet50_cifar_shapes.json as ONE group), the launches alone.
  compress        gq_ctk_compress_batched over the parent's gq_topk_compress_batched: bar 0.5.  Also its ratio to the parent's
                  fixed-threshold gq_thr_compress_batched (eta with P(|N(0, 1)| > eta) = 1 / 256), the other one-read sparsifier: no bar.
  decode_mean_R1 / _R8
                  gq_ctk_decode_sum_batched over the parent's gq_stc_decode_sum_batched, each on R copies of the wire its own compress
                  wrote: bar 1.25.
`missed` lists every ratio above its bar.  *_gradient_reads_equiv: a compress time as reads of the gradient at 6.3 TB/s.
--values packed16 (DIR also holds the parent's libgq_ctk.so) writes the one row `packed16` instead and leaves the others: on both
workloads gq_ctk_compress_packed_batched and gq_ctk_decode_sum_packed_batched at R = 1 and 8 over the PARENT's f32-valued launches,
bar 1.05 each, this build's f32-valued launches over the same beside them, and the ResNet-50 list's record + apply in both formats
with and without error feedback (no bar).
Times: tools/mx_time.py's method -- ten calls captured into one HIP graph, HIP events around windows of replays, the median window; the
paths alternated round by round, the minimum over three rounds next to every round."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mx_time import _args, graphed, other_library, timed, write_rows  # noqa: E402
from stc_time import _group  # noqa: E402
from thr_time import ETA_FIXED  # noqa: E402
from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedChunkTopK, BatchedSTC, BatchedThr, BatchedTopK, ChunkTopKCodec, STCCodec, ThrCodec, TopKCodec  # noqa: E402
from gq_amd.compressors import (ChunkTopKCompressor, SparseTernaryCompressor, ThresholdSparsificationCompressor,  # noqa: E402
                                TopKSparsificationCompressor)
from gq_amd.quantizers import PSQuantizer  # noqa: E402

CR = 256
BARS = {"compress": 0.5, "decode_mean_R1": 1.25, "decode_mean_R8": 1.25}
# path -> (group, codec, compressor, further arguments, the parent's file and what loads it: None = this build)
PATHS = {
    "ctk": (BatchedChunkTopK, ChunkTopKCodec, ChunkTopKCompressor, {}, None),
    "parent_topk": (BatchedTopK, TopKCodec, TopKSparsificationCompressor, {}, (native.TopKBatch, "libgq_topk.so", "gq_topk_", native.TOPK_EXPORTS)),
    "parent_thr_fixed": (BatchedThr, ThrCodec, ThresholdSparsificationCompressor, dict(thr_stages=0, thr_value=ETA_FIXED),
                         (native.ThrBatch, "libgq_thr.so", "gq_thr_", native.THR_EXPORTS)),
    "parent_stc": (BatchedSTC, STCCodec, SparseTernaryCompressor, {}, (native.STCBatch, "libgq_stc.so", "gq_stc_", native.STC_EXPORTS)),
}


def launches_row(name, sizes, dev, parent_dir):
    torch.manual_seed(1)
    ts = [torch.randn(n, device=dev) for n in sizes]
    elems = sum(sizes)
    groups, wires = {}, {}
    for path, (group, codec, comp, kw, lib) in PATHS.items():
        codecs = [codec(comp(n, (n,), _args(cr=CR, **kw)), n, (n,)) for n in sizes]
        if lib is None:
            groups[path], ub = _group(group, codecs, dev)
        else:
            with other_library(os.path.join(parent_dir, lib[1]), *lib):
                groups[path], ub = _group(group, codecs, dev)
        wires[path] = torch.zeros((8, ub), dtype=torch.uint8, device=dev)
        assert groups[path].encode(ts, wires[path][0], 0, 0)
        for r in range(1, 8):
            wires[path][r].copy_(wires[path][0])
    torch.cuda.synchronize()
    row = {"case": name, "tensors": len(sizes), "elements": elems, "cr": CR, "bars": BARS, "wire_bytes": {p: int(w.shape[1]) for p, w in wires.items()}}
    out = torch.empty(max(g.out_floats for g in groups.values()), device=dev)
    times = {}
    for rnd in range(3):
        for path in ("ctk", "parent_topk", "parent_thr_fixed"):
            g, w = groups[path], wires[path]
            times.setdefault(path + "_compress", []).append(graphed(lambda: g.encode(ts, w[0], 0, 0)))
        for R in (1, 8):
            for path in ("ctk", "parent_stc"):
                g, w = groups[path], wires[path]
                times.setdefault("%s_decode_mean_R%d" % (path, R), []).append(graphed(lambda: g._batch.decode(w[:R], R, out)))
    for key, tt in times.items():
        row[key + "_us_rounds"] = [round(x, 2) for x in tt]
        row[key + "_us"] = round(min(tt), 2)
    row["ctk_compress_over_parent_topk"] = round(row["ctk_compress_us"] / row["parent_topk_compress_us"], 3)
    row["ctk_compress_over_parent_thr_fixed"] = round(row["ctk_compress_us"] / row["parent_thr_fixed_compress_us"], 3)
    for R in (1, 8):
        row["ctk_decode_mean_R%d_over_parent_stc" % R] = round(row["ctk_decode_mean_R%d_us" % R] / row["parent_stc_decode_mean_R%d_us" % R], 3)
    for path in ("ctk", "parent_topk", "parent_thr_fixed"):
        row[path + "_compress_gradient_reads_equiv"] = round(row[path + "_compress_us"] * 1e-6 * 6.3e12 / (elems * 4), 2)
    row["missed"] = [f for f, bar in (("ctk_compress_over_parent_topk", BARS["compress"]),
                                      ("ctk_decode_mean_R1_over_parent_stc", BARS["decode_mean_R1"]),
                                      ("ctk_decode_mean_R8_over_parent_stc", BARS["decode_mean_R8"])) if row[f] > bar]
    return row


PACKED_BAR = 1.05      # a launch that moves no more bytes than the f32 format's and adds a little arithmetic
F32_EXPORTS = native.CTK_EXPORTS[:4]      # what a build from before the PACKED16 entry points exports


def packed_workload(name, sizes, dev, parent_dir):
    """The PACKED16 launches of this build over the f32-valued launches of the parent's libgq_ctk.so (never this build's, which are timed
    beside them), each decode on R copies of the wire its own compress wrote."""
    torch.manual_seed(1)
    ts = [torch.randn(n, device=dev) for n in sizes]
    groups, wires = {}, {}
    for path, values, lib in (("packed16", "packed16", None), ("f32", "f32", None), ("parent_f32", "f32", os.path.join(parent_dir, "libgq_ctk.so"))):
        codecs = [ChunkTopKCodec(ChunkTopKCompressor(n, (n,), _args(cr=CR, ctk_values=values)), n, (n,)) for n in sizes]
        if lib is None:
            groups[path], ub = _group(BatchedChunkTopK, codecs, dev)
        else:
            with other_library(lib, native.CTKBatch, "libgq_ctk.so", "gq_ctk_", F32_EXPORTS):
                groups[path], ub = _group(BatchedChunkTopK, codecs, dev)
        wires[path] = torch.zeros((8, ub), dtype=torch.uint8, device=dev)
        assert groups[path].encode(ts, wires[path][0], 0, 0)
        for r in range(1, 8):
            wires[path][r].copy_(wires[path][0])
    torch.cuda.synchronize()
    assert torch.equal(wires["f32"], wires["parent_f32"]), "this build's f32 wire is not the parent's"
    out = torch.empty(max(g.out_floats for g in groups.values()), device=dev)
    w = {"tensors": len(sizes), "elements": sum(sizes), "wire_bytes": {p: int(x.shape[1]) for p, x in wires.items()}}
    times = {}
    for rnd in range(3):
        for path, g in groups.items():
            times.setdefault(path + "_compress", []).append(graphed(lambda: g.encode(ts, wires[path][0], 0, 0)))
        for R in (1, 8):
            for path, g in groups.items():
                times.setdefault("%s_decode_mean_R%d" % (path, R), []).append(graphed(lambda: g._batch.decode(wires[path][:R], R, out)))
    for key, tt in times.items():
        w[key + "_us_rounds"] = [round(x, 2) for x in tt]
        w[key + "_us"] = round(min(tt), 2)
    for kind in ("compress", "decode_mean_R1", "decode_mean_R8"):
        for path in ("packed16", "f32"):
            w["%s_%s_over_parent_f32" % (path, kind)] = round(w["%s_%s_us" % (path, kind)] / w["parent_f32_%s_us" % kind], 3)
    w["missed"] = ["%s: packed16_%s_over_parent_f32" % (name, k) for k in ("compress", "decode_mean_R1", "decode_mean_R8")
                   if w["packed16_%s_over_parent_f32" % k] > PACKED_BAR]
    return w


def step_times(shapes, dev):
    """The ResNet-50 list's record + apply (one user, every parameter, graphs as the quantizer replays them) in both formats, with and
    without error feedback, alternated round by round: the minimum of three rounds.  No bar."""
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    variants = {}
    for values in ("f32", "packed16"):
        for ef in (False, True):
            params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
            variants["%s%s" % (values, "_ef" if ef else "")] = (PSQuantizer(ChunkTopKCompressor, params, _args(cr=CR, ctk_values=values, ef=ef)), params)
    rounds = {}
    for rnd in range(3):
        for name, (q, params) in variants.items():
            fixed = [g.clone() for g in src]

            def step():
                for p, g in zip(params, fixed):
                    p.grad = g
                q.record(0, 0)
                q.apply()
            rounds.setdefault(name, []).append(timed(step, iters=100, warm=30, windows=3))
    return {name + "_record_apply_us": round(min(tt), 1) for name, tt in rounds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctk_time.jsonl"))
    ap.add_argument("--parent-lib", required=True, help="a directory with an older libgq_topk.so, libgq_thr.so and libgq_stc.so: the yardsticks "
                                                        "(--values packed16: with an older libgq_ctk.so)")
    ap.add_argument("--values", default="f32", choices=["f32", "packed16"],
                    help="packed16: the one row `packed16` -- the PACKED16 launches over the parent's f32-valued ones, bar 1.05 each, and the list's "
                         "record + apply in both formats; the file's other rows stay")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    r50 = [n for n in (int(torch.Size(s).numel()) for s in shapes) if n > 1000]
    parent = os.path.abspath(a.parent_lib)
    if a.values == "packed16":
        row = {"case": "packed16", "cr": CR, "bar": PACKED_BAR, "single_25m": packed_workload("single_25m", [25_000_000], dev, parent),
               "resnet50_list": packed_workload("resnet50_list", r50, dev, parent), "resnet50_step": step_times(shapes, dev)}
        row["missed"] = row["single_25m"].pop("missed") + row["resnet50_list"].pop("missed")
        return write_rows(a.out, [row], replace_case="packed16")
    write_rows(a.out, [launches_row("single_25m", [25_000_000], dev, parent), launches_row("resnet50_list", r50, dev, parent)])


if __name__ == "__main__":
    main()
