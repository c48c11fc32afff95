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

from mx_time import _args, graphed, other_library, write_rows  # noqa: E402
from stc_time import _group  # noqa: E402
from thr_time import ETA_FIXED  # noqa: E402
from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedChunkTopK, BatchedSTC, BatchedThr, BatchedTopK, ChunkTopKCodec, STCCodec, ThrCodec, TopKCodec  # noqa: E402
from gq_amd.compressors import (ChunkTopKCompressor, SparseTernaryCompressor, ThresholdSparsificationCompressor,  # noqa: E402
                                TopKSparsificationCompressor)

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctk_time.jsonl"))
    ap.add_argument("--parent-lib", required=True, help="a directory with an older libgq_topk.so, libgq_thr.so and libgq_stc.so: the yardsticks")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    r50 = [n for n in (int(torch.Size(s).numel()) for s in shapes) if n > 1000]
    parent = os.path.abspath(a.parent_lib)
    write_rows(a.out, [launches_row("single_25m", [25_000_000], dev, parent), launches_row("resnet50_list", r50, dev, parent)])


if __name__ == "__main__":
    main()
