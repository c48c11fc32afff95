"""Time sparse ternary compression's kernels (libgq_stc.so) on one MI355X against the top-k launches of an older build (say the parent
commit's libgq_topk.so) loaded into the same process:

    python tools/stc_time.py --parent-lib libgq_topk.so [--out FILE]      (default: profiles/stc_time.jsonl)
    python tools/stc_time.py --parent-lib libgq_topk.so --parent-own-lib libgq_stc.so --launches-only --out FILE

Rows (one JSON line each), cr = 256, N(0, 1) gradients:
  single_25m, resnet50_list
                  one 25 M-element tensor, and the ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json: the 76 tensors
                  over 1,000 elements as ONE group), the launches alone.  compress: gq_stc_compress_batched (stc) and this build's
                  gq_topk_compress_batched (topk) against the yardstick's gq_topk_compress_batched (parent_topk).  decode_mean_R1 /
                  _R8: gq_stc_decode_sum_batched on the wire its own compress wrote against the yardstick's
                  gq_topk_decode_sum_batched on its own -- the same kept set, R copies of one payload.  Ten calls replayed from one HIP
                  graph (the device's own time), and eager.  *_over_parent_topk: the ratio of the graphed times; `bars`: 1.05 for
                  stc's compress and its two decode-means, the band 0.99 ... 1.01 for this build's top-k launches; `missed` lists
                  every ratio outside.
  resnet50_step   PSQuantizer record + apply over the whole ResNet-50 parameter list, one user, default launches (graph replay),
                  gradients at fixed addresses: --quantizer stc and stc --ef next to --quantizer topk and topk --ef (the in-tree
                  library), alternated, three rounds each.
--parent-own-lib: an older libgq_stc.so as well (a refactor of both libraries against its parent commit).  The two launch rows then
also time parent_stc, and a second load of either parent file (parent_topk_again, parent_stc_again: the A/A ratios), and carry
`refactor`: stc over parent_stc and topk over parent_topk per launch, the A/A ratios, the case's bar (its largest A/A ratio + 0.01)
and what missed it.  --launches-only leaves the resnet50_step rows out.
Times: tools/mx_time.py's method (HIP events around windows of back-to-back calls, the median window; paths alternated round by
round, the minimum over the rounds next to every round)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mx_time import _args, graphed, other_library, refactor_ratios, refactor_verdict, second_load, timed, write_rows  # noqa: E402
from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedSTC, BatchedTopK, STCCodec, TopKCodec, _up  # noqa: E402
from gq_amd.compressors import SparseTernaryCompressor, TopKSparsificationCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402

CR = 256
BAR, BAND = 1.05, (0.99, 1.01)
KINDS = ("compress", "decode_mean_R1", "decode_mean_R8")


def _group(cls, codecs, dev):
    offs, off = [], 0
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes)
    ub = max(16, _up(off))
    return cls(codecs, offs, list(range(len(codecs))), dev, 1, ub), ub


def launches_row(name, sizes, dev, parent_topk, parent_stc=None):
    torch.manual_seed(1)
    ts = [torch.randn(n, device=dev) for n in sizes]
    elems = sum(sizes)
    tk = lambda: [TopKCodec(TopKSparsificationCompressor(n, (n,), _args(cr=CR)), n, (n,)) for n in sizes]
    stc = lambda: [STCCodec(SparseTernaryCompressor(n, (n,), _args(cr=CR)), n, (n,)) for n in sizes]
    groups, wires = {}, {}
    yard = "parent_topk" if parent_topk else "topk"
    olds = [(yard, parent_topk, BatchedTopK, tk)] if parent_topk else []
    if parent_stc:
        olds += [("parent_topk_again", second_load(parent_topk), BatchedTopK, tk), ("parent_stc", parent_stc, BatchedSTC, stc),
                 ("parent_stc_again", second_load(parent_stc), BatchedSTC, stc)]
    for gname, path, cls, codecs in olds:
        with (other_library(path, native.TopKBatch, "libgq_topk.so", "gq_topk_", native.TOPK_EXPORTS) if cls is BatchedTopK
              else other_library(path, native.STCBatch, "libgq_stc.so", "gq_stc_", native.STC_EXPORTS)):
            groups[gname], ub = _group(cls, codecs(), dev)
        wires[gname] = torch.zeros((8, ub), dtype=torch.uint8, device=dev)
    groups["topk"], ub = _group(BatchedTopK, tk(), dev)
    wires["topk"] = torch.zeros((8, ub), dtype=torch.uint8, device=dev)
    groups["stc"], ub = _group(BatchedSTC, stc(), dev)
    wires["stc"] = torch.zeros((8, ub), dtype=torch.uint8, device=dev)
    for gname, g in groups.items():
        assert g.encode(ts, wires[gname][0], 0, 0)
        for r in range(1, 8):
            wires[gname][r].copy_(wires[gname][0])
    torch.cuda.synchronize()
    row = {"case": name, "tensors": len(sizes), "elements": elems, "cr": CR, "k_total": sum(n // CR for n in sizes),
           "parent_topk": bool(parent_topk), "bars": {"stc": BAR, "topk": list(BAND)},
           "wire_bytes": {gname: int(w.shape[1]) for gname, w in wires.items()}}
    out = torch.empty(max(g.out_floats for g in groups.values()), device=dev)
    times = {}
    for rnd in range(3):
        for gname, g in groups.items():
            w = wires[gname]
            times.setdefault(gname + "_compress_eager", []).append(timed(lambda: g.encode(ts, w[0], 0, 0)))
            times.setdefault(gname + "_compress", []).append(graphed(lambda: g.encode(ts, w[0], 0, 0)))
        for R in (1, 8):
            for gname, g in groups.items():
                w = wires[gname]
                times.setdefault("%s_decode_mean_R%d_eager" % (gname, R), []).append(timed(lambda: g._batch.decode(w[:R], R, out)))
                times.setdefault("%s_decode_mean_R%d" % (gname, R), []).append(graphed(lambda: g._batch.decode(w[:R], R, out)))
    for key, tt in times.items():
        row[key + "_us_rounds"] = [round(x, 2) for x in tt]
        row[key + "_us"] = round(min(tt), 2)
    missed = []
    for path in ("topk", "stc") if parent_topk else ("stc",):
        for kind in KINDS:
            for eager in ("", "_eager"):
                field = "%s_%s%s_over_%s" % (path, kind, eager, yard)
                row[field] = round(row["%s_%s%s_us" % (path, kind, eager)] / row["%s_%s%s_us" % (yard, kind, eager)], 3)
                outside = row[field] > BAR if path == "stc" else not BAND[0] <= row[field] <= BAND[1]
                if not eager and outside:
                    missed.append(field)
    for path in groups:
        row[path + "_compress_gradient_reads_equiv"] = round(row[path + "_compress_us"] * 1e-6 * 6.3e12 / (elems * 4), 2)
    row["missed"] = missed
    if parent_stc:
        refactor_verdict(row, {"topk": refactor_ratios(row, "topk", "parent_topk"), "stc": refactor_ratios(row, "stc", "parent_stc")})
    return row


def resnet50_rows(dev, shapes):
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    variants = {}
    for name, comp, kw in [("stc", SparseTernaryCompressor, {}), ("stc_ef", SparseTernaryCompressor, dict(ef=True)),
                           ("topk", TopKSparsificationCompressor, {}), ("topk_ef", TopKSparsificationCompressor, dict(ef=True))]:
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
        out.append({"case": "resnet50_step", "path": name, "us_per_step_rounds": [round(t, 2) for t in tt], "us_per_step_min": round(min(tt), 2),
                    "wire_bytes_per_user": q.wire_bytes_per_user(), "record_paths": dict(q.record_paths)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stc_time.jsonl"))
    ap.add_argument("--parent-lib", default=None, help="an older libgq_topk.so: its launches are the yardstick; without it the in-tree one")
    ap.add_argument("--parent-own-lib", default=None, help="an older libgq_stc.so (needs --parent-lib): the rows' `refactor` field")
    ap.add_argument("--launches-only", action="store_true", help="the two launch rows, no resnet50_step rows")
    a = ap.parse_args()
    if a.parent_own_lib and not a.parent_lib:
        ap.error("--parent-own-lib needs --parent-lib")
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    r50 = [n for n in (int(torch.Size(s).numel()) for s in shapes) if n > 1000]
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    own = os.path.abspath(a.parent_own_lib) if a.parent_own_lib else None
    write_rows(a.out, [launches_row("single_25m", [25_000_000], dev, parent, own), launches_row("resnet50_list", r50, dev, parent, own)]
               + ([] if a.launches_only else resnet50_rows(dev, shapes)))


if __name__ == "__main__":
    main()
