"""Time the count sketch's launches (libgq_sketch.so) on one MI355X against the top-k launches of an older build (say the parent
commit's libgq_topk.so) loaded into the same process:

    python tools/sketch_time.py --parent-lib libgq_topk.so [--out FILE]      (default: profiles/sketch_time.jsonl)

Rows (one JSON line each), cr = 256, N(0, 1) gradients, sketch_cr = 32:
  single_25m, resnet50_list
                  one 25 M-element tensor, and the tensors of the ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json)
                  that are sketched at five rows (and so at one and three), as ONE group -- the same tensors for both sides.  compress:
                  gq_sketch_compress_batched at 1, 3 and 5 rows (sketch_r1 / _r3 / _r5: the sketch launch and the fold launch)
                  against the yardstick's gq_topk_compress_batched (parent_topk: eight launches).  decode_mean_R1 / _R8:
                  gq_sketch_decode_sum_batched at three rows (eleven launches) against the yardstick's gq_topk_decode_sum_batched
                  (one launch), each on its own payloads.  Ten calls replayed from one HIP graph (the device's own time), and
                  eager.  *_over_parent_topk: the ratio of the graphed times; `bars`: 1.0 for the compress at three rows, none for
                  the decode-means; `missed` lists every ratio above its bar.  decode_mean_R8_over_R1: the ratio the issue of this
                  compressor is about, for both sides.  *_gradient_reads_equiv: the graphed time in reads of the gradient at
                  6.3 TB/s, topk_time.py's figure.
  resnet50_step   PSQuantizer record + apply over the whole ResNet-50 parameter list, one user, default launches (graph replay),
                  gradients at fixed addresses: --quantizer sketch (three rows; --sketch-ef) next to --quantizer topk, alternated,
                  three rounds each.  --launches-only leaves these rows out.
  --recover chunked --parent-lib DIR
                  single_25m_recover, resnet50_list_recover: the chunked recovery's decode-mean (two launches), this build's global
                  decode-mean and its compress, each over the same launches of the parent commit's libgq_sketch.so in DIR; bars: 0.5 for
                  the chunked decode-mean, the band 0.99 - 1.01 for what compiles from the parent's kernels.  resnet50_step_recover:
                  record + apply under both recoveries, with and without --sketch-ef.  The file's other rows stay.
Times: tools/mx_time.py's method (HIP events around windows of back-to-back calls, the median window; paths alternated round by
round, the minimum over the rounds next to every round)."""
import argparse
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mx_time import _args, graphed, other_library, timed, write_rows  # noqa: E402
from thr_time import _group  # noqa: E402
from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedSketch, BatchedTopK, SketchCodec, TopKCodec  # noqa: E402
from gq_amd.compressors import CountSketchCompressor, TopKSparsificationCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402

CR, C = 256, 32
BARS = {"sketch_r3_compress": 1.0}
ROWS = (1, 3, 5)


def launches_row(name, sizes, dev, parent_topk):
    torch.manual_seed(1)
    ts = [torch.randn(n, device=dev) for n in sizes]
    elems = sum(sizes)
    groups, wires = {}, {}
    tk_codecs = [TopKCodec(TopKSparsificationCompressor(n, (n,), _args(cr=CR)), n, (n,)) for n in sizes]
    yard = "parent_topk" if parent_topk else "topk"
    with (other_library(parent_topk, native.TopKBatch, "libgq_topk.so", "gq_topk_", native.TOPK_EXPORTS) if parent_topk
          else contextlib.nullcontext()):
        groups[yard], _, ub = _group(BatchedTopK, tk_codecs, dev)
    wires[yard] = torch.zeros((8, ub), dtype=torch.uint8, device=dev)
    for r in ROWS:
        codecs = [SketchCodec(CountSketchCompressor(n, (n,), _args(cr=CR, sketch_rows=r, sketch_cr=C, sketch_seed=1)), n, (n,)) for n in sizes]
        groups["sketch_r%d" % r], _, ub = _group(BatchedSketch, codecs, dev)
        wires["sketch_r%d" % r] = torch.zeros((8, ub), dtype=torch.uint8, device=dev)
    for gname, g in groups.items():
        assert g.encode(ts, wires[gname][0], 0, 0)
        for r in range(1, 8):
            wires[gname][r].copy_(wires[gname][0])
    torch.cuda.synchronize()
    row = {"case": name, "tensors": len(sizes), "elements": elems, "cr": CR, "sketch_cr": C, "parent_topk": bool(parent_topk), "bars": BARS,
           "wire_bytes": {gname: int(w.shape[1]) for gname, w in wires.items()},
           "units": {gname: g.nunits for gname, g in groups.items() if gname != yard},
           "windows": {gname: g.nwindows for gname, g in groups.items() if gname != yard}}
    out = torch.empty(max(g.out_floats for g in groups.values()), device=dev)
    deco = [(yard, groups[yard]), ("sketch_r3", groups["sketch_r3"])]
    times = {}
    for rnd in range(3):
        for gname, g in groups.items():
            w = wires[gname]
            times.setdefault(gname + "_compress_eager", []).append(timed(lambda: g.encode(ts, w[0], 0, 0)))
            times.setdefault(gname + "_compress", []).append(graphed(lambda: g.encode(ts, w[0], 0, 0)))
        for R in (1, 8):
            for gname, g in deco:
                w = wires[gname]
                times.setdefault("%s_decode_mean_R%d_eager" % (gname, R), []).append(timed(lambda: g._batch.decode(w[:R], R, out)))
                times.setdefault("%s_decode_mean_R%d" % (gname, R), []).append(graphed(lambda: g._batch.decode(w[:R], R, out)))
    for key, tt in times.items():
        row[key + "_us_rounds"] = [round(x, 2) for x in tt]
        row[key + "_us"] = round(min(tt), 2)
    missed = []
    for path, kinds in [("sketch_r%d" % r, ("compress",)) for r in ROWS] + [("sketch_r3", ("decode_mean_R1", "decode_mean_R8"))]:
        for kind in kinds:
            for eager in ("", "_eager"):
                field = "%s_%s%s_over_%s" % (path, kind, eager, yard)
                row[field] = round(row["%s_%s%s_us" % (path, kind, eager)] / row["%s_%s%s_us" % (yard, kind, eager)], 3)
                if not eager and row[field] > BARS.get("%s_%s" % (path, kind), float("inf")):
                    missed.append(field)
    for gname, _ in deco:
        row[gname + "_decode_mean_R8_over_R1"] = round(row[gname + "_decode_mean_R8_us"] / row[gname + "_decode_mean_R1_us"], 3)
    for path in groups:
        row[path + "_compress_gradient_reads_equiv"] = round(row[path + "_compress_us"] * 1e-6 * 6.3e12 / (elems * 4), 2)
    row["missed"] = missed
    return row


RECOVER_BAR, BAND = 0.5, (0.99, 1.01)


def recover_row(name, sizes, dev, parent_dir):
    """--recover chunked: this build's chunked decode-mean (two launches) and its global one and compress, over the decode-mean and the
    compress of the parent commit's libgq_sketch.so in `parent_dir`, three rows.  The parent reads the version-1 descriptor: the same
    bytes without { recover, cr }, so its groups are built as usual and say the old size."""
    torch.manual_seed(1)
    ts = [torch.randn(n, device=dev) for n in sizes]
    groups, wires = {}, {}

    def group(recover):
        codecs = [SketchCodec(CountSketchCompressor(n, (n,), _args(cr=CR, sketch_rows=3, sketch_cr=C, sketch_seed=1, sketch_recover=recover)), n, (n,))
                  for n in sizes]
        g, _, ub = _group(BatchedSketch, codecs, dev)
        return g, torch.zeros((8, ub), dtype=torch.uint8, device=dev)

    with other_library(os.path.join(parent_dir, "libgq_sketch.so"), native.SketchBatch, "libgq_sketch.so", "gq_sketch_", native.SKETCH_EXPORTS):
        groups["parent"], wires["parent"] = group("global")
    groups["parent"]._batch.s.struct_bytes = 168
    groups["global"], wires["global"] = group("global")
    groups["chunked"], wires["chunked"] = group("chunked")
    for gname, g in groups.items():
        assert g.encode(ts, wires[gname][0], 0, 0)
        for r in range(1, 8):
            wires[gname][r].copy_(wires[gname][0])
    outs = {gname: torch.empty(g.out_floats, device=dev) for gname, g in groups.items()}
    for gname, g in groups.items():
        g._batch.decode(wires[gname][:8], 8, outs[gname])
    torch.cuda.synchronize()
    row = {"case": name + "_recover", "tensors": len(sizes), "elements": sum(sizes), "cr": CR, "sketch_cr": C, "rows": 3,
           "global_equals_parent": bool(torch.equal(outs["global"].view(torch.int32), outs["parent"].view(torch.int32))
                                        and torch.equal(wires["global"], wires["parent"])),
           "kept": {gname: int((o != 0).sum()) for gname, o in outs.items()}, "bars": {"chunked_decode_mean": RECOVER_BAR, "global_band": BAND}}
    times = {}
    for rnd in range(3):
        for gname, g in groups.items():
            w, o = wires[gname], outs[gname]
            times.setdefault(gname + "_compress", []).append(graphed(lambda: g.encode(ts, w[0], 0, 0)))
            for R in (1, 8):
                times.setdefault("%s_decode_mean_R%d" % (gname, R), []).append(graphed(lambda: g._batch.decode(w[:R], R, o)))
    for key, tt in times.items():
        row[key + "_us_rounds"] = [round(x, 2) for x in tt]
        row[key + "_us"] = round(min(tt), 2)
    missed = []
    for R in (1, 8):
        kind = "decode_mean_R%d" % R
        row["chunked_%s_over_parent" % kind] = round(row["chunked_%s_us" % kind] / row["parent_%s_us" % kind], 3)
        if row["chunked_%s_over_parent" % kind] > RECOVER_BAR:
            missed.append("chunked_%s_over_parent" % kind)
    for kind in ("compress", "decode_mean_R1", "decode_mean_R8"):
        field = "global_%s_over_parent" % kind
        row[field] = round(row["global_%s_us" % kind] / row["parent_%s_us" % kind], 3)
        if not BAND[0] <= row[field] <= BAND[1]:
            missed.append(field)
    row["missed"] = missed
    return row


def resnet50_rows(dev, shapes, recover=False):
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    variants = {}
    for name, comp, kw in [("sketch_r3", CountSketchCompressor, dict(sketch_rows=3, sketch_cr=C, sketch_seed=1)),
                           ("sketch_r3_ef", CountSketchCompressor, dict(sketch_rows=3, sketch_cr=C, sketch_seed=1, sketch_ef=True))] + (
                           [("sketch_r3_chunked", CountSketchCompressor, dict(sketch_rows=3, sketch_cr=C, sketch_seed=1, sketch_recover="chunked")),
                            ("sketch_r3_chunked_ef", CountSketchCompressor,
                             dict(sketch_rows=3, sketch_cr=C, sketch_seed=1, sketch_recover="chunked", sketch_ef=True))] if recover else
                           [("topk", TopKSparsificationCompressor, {})]):
        params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
        variants[name] = (PSQuantizer(comp, params, _args(cr=CR, **kw)), params)
    rows = {}
    for rnd in range(3):
        for name, (q, params) in variants.items():
            fixed = [g.clone() for g in src]

            def step():
                for p, g in zip(params, fixed):
                    p.grad = g
                q.record(0, 0)
                q.apply()
            rows.setdefault(name, []).append(timed(step, iters=100, warm=30, windows=3))
    out = []
    for name, tt in rows.items():
        q = variants[name][0]
        out.append({"case": "resnet50_step_recover" if recover else "resnet50_step", "path": name, "us_per_step_rounds": [round(t, 2) for t in tt], "us_per_step_min": round(min(tt), 2),
                    "wire_bytes_per_user": q.wire_bytes_per_user(), "record_paths": dict(q.record_paths)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sketch_time.jsonl"))
    ap.add_argument("--parent-lib", default=None, help="an older libgq_topk.so: its launches are the yardstick; without it the in-tree one")
    ap.add_argument("--launches-only", action="store_true", help="the two launch rows, no resnet50_step rows")
    ap.add_argument("--recover", default=None, choices=["chunked"],
                    help="the rows of --sketch-recover chunked instead (single_25m_recover, resnet50_list_recover, resnet50_step_recover; the "
                         "file's other rows stay): --parent-lib is then the DIRECTORY of the parent commit's libgq_sketch.so")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    r50 = [n for n in (int(torch.Size(s).numel()) for s in shapes) if CountSketchCompressor.layout(n, 5, C)[0] >= 10 * CountSketchCompressor.layout(n, 5, C)[1]]
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    if a.recover:
        assert parent and os.path.isdir(parent), "--recover needs --parent-lib DIR"
        write_rows(a.out, [recover_row("single_25m", [25_000_000], dev, parent)], replace_case="single_25m_recover")
        write_rows(a.out, [recover_row("resnet50_list", r50, dev, parent)], replace_case="resnet50_list_recover")
        if not a.launches_only:
            write_rows(a.out, resnet50_rows(dev, shapes, recover=True), replace_case="resnet50_step_recover")
        return
    write_rows(a.out, [launches_row("single_25m", [25_000_000], dev, parent), launches_row("resnet50_list", r50, dev, parent)]
               + ([] if a.launches_only else resnet50_rows(dev, shapes)))


if __name__ == "__main__":
    main()
