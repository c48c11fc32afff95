"""Time the threshold sparsifier's kernels (libgq_thr.so) on one MI355X against the top-k launches of an older build (say the parent
commit's libgq_topk.so) loaded into the same process:

    python tools/thr_time.py --parent-lib libgq_topk.so [--out FILE]      (default: profiles/thr_time.jsonl)
    python tools/thr_time.py --parent-lib libgq_topk.so --parent-own-lib libgq_thr.so --launches-only --out FILE

Rows (one JSON line each), cr = 256, N(0, 1) gradients:
  single_25m, resnet50_list
                  one 25 M-element tensor, and the ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json: the 76 tensors
                  over 1,000 elements as ONE group), the launches alone.  compress: gq_thr_compress_batched with three stages at fit
                  stride 1 (thr_s3_m1), three stages at --thr-fit-stride 8 (thr_s3_m8) and a fixed threshold (thr_fixed: eta =
                  the N(0, 1) quantile that 1 / 256 of the magnitudes exceed) against the yardstick's gq_topk_compress_batched
                  (parent_topk).  decode_mean_R1 / _R8: gq_thr_decode_sum_batched against the yardstick's
                  gq_topk_decode_sum_batched on payloads that carry the SAME pairs -- the threshold wire is built on the host
                  from the top-k wire: kept = found = k, top-k's indices and values, pad slots up to cap.  Ten calls replayed
                  from one HIP graph (the device's own time), and eager.  *_over_parent_topk: the ratio of the graphed times;
                  `bars`: 1.0 for the compress of thr_s3_m1 and thr_fixed, 1.05 for the two decode-means; `missed` lists every
                  ratio above its bar.  thr_s3_m8 has no bar.  *_gradient_reads_equiv: the graphed time in reads of the
                  gradient at 6.3 TB/s, topk_time.py's figure.  kept_over_k: what the estimate kept, summed over the tensors.
  resnet50_step   PSQuantizer record + apply over the whole ResNet-50 parameter list, one user, default launches (graph replay),
                  gradients at fixed addresses: --quantizer threshold (three stages; --thr-fit-stride 8; a fixed threshold; --ef)
                  next to --quantizer topk and topk --ef (the in-tree library), alternated, three rounds each.
--parent-own-lib: an older libgq_thr.so as well (a refactor of the library against its parent commit).  The two launch rows then also
time parent_thr (three stages at fit stride 1, and the decode-means on thr's payloads) and a second load of the same file
(parent_thr_again: the A/A ratios), and carry `refactor`: thr over parent_thr per launch, the A/A ratios, the case's bar (its
largest A/A ratio + 0.01) and what missed it.  --launches-only leaves the resnet50_step rows out.
Times: tools/mx_time.py's method (HIP events around windows of back-to-back calls, the median window; paths alternated round by
round, the minimum over the rounds next to every round)."""
import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mx_time import _args, graphed, other_library, refactor_ratios, refactor_verdict, second_load, timed, write_rows  # noqa: E402
from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedThr, BatchedTopK, ThrCodec, TopKCodec, _up  # noqa: E402
from gq_amd.compressors import ThresholdSparsificationCompressor, TopKSparsificationCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402

CR = 256
BARS = {"thr_s3_m1_compress": 1.0, "thr_fixed_compress": 1.0, "thr_decode_mean_R1": 1.05, "thr_decode_mean_R8": 1.05}
ETA_FIXED = 2.8856349      # P(|N(0, 1)| > eta) = 1 / 256
MODES = {"thr_s3_m1": dict(thr_stages=3), "thr_s3_m8": dict(thr_stages=3, thr_fit_stride=8), "thr_fixed": dict(thr_stages=0, thr_value=ETA_FIXED)}


def _group(cls, codecs, dev):
    offs, off = [], 0
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes)
    ub = max(16, _up(off))
    return cls(codecs, offs, list(range(len(codecs))), dev, 1, ub), offs, ub


def _thr_wire_of(topk_wire, topk_codecs, topk_offs, thr_codecs, thr_offs, ub):
    """One user's threshold wire carrying the pairs of a top-k wire: kept = found = k, eta = 0, pad slots behind the pairs."""
    src = topk_wire.cpu().numpy()
    dst = np.zeros(ub, dtype=np.uint8)
    for tk, to, th, ho in zip(topk_codecs, topk_offs, thr_codecs, thr_offs):
        k, cap = tk.k, th.cap
        assert k <= cap
        words = dst[ho:ho + 16 + 8 * cap].view("<u4")
        words[0], words[1] = k, k
        words[4:4 + cap] = 0xffffffff
        words[4:4 + k] = src[to:to + 4 * k].view("<u4")
        words[4 + cap:4 + cap + k] = src[to + 4 * k:to + 8 * k].view("<u4")
    return torch.from_numpy(dst)


def launches_row(name, sizes, dev, parent_topk, parent_thr=None):
    torch.manual_seed(1)
    ts = [torch.randn(n, device=dev) for n in sizes]
    elems = sum(sizes)
    groups, wires = {}, {}
    tk_codecs = [TopKCodec(TopKSparsificationCompressor(n, (n,), _args(cr=CR)), n, (n,)) for n in sizes]
    yard = "parent_topk" if parent_topk else "topk"
    with (other_library(parent_topk, native.TopKBatch, "libgq_topk.so", "gq_topk_", native.TOPK_EXPORTS) if parent_topk
          else contextlib.nullcontext()):
        groups[yard], tk_offs, ub = _group(BatchedTopK, tk_codecs, dev)
    wires[yard] = torch.zeros((8, ub), dtype=torch.uint8, device=dev)
    thr_codecs = {}
    for mode, kw in MODES.items():
        thr_codecs[mode] = [ThrCodec(ThresholdSparsificationCompressor(n, (n,), _args(cr=CR, **kw)), n, (n,)) for n in sizes]
        groups[mode], thr_offs, ub = _group(BatchedThr, thr_codecs[mode], dev)
        wires[mode] = torch.zeros((8, ub), dtype=torch.uint8, device=dev)
    olds = [("parent_thr", parent_thr), ("parent_thr_again", second_load(parent_thr))] if parent_thr else []
    for gname, path in olds:
        with other_library(path, native.ThrBatch, "libgq_thr.so", "gq_thr_", native.THR_EXPORTS):
            codecs = [ThrCodec(ThresholdSparsificationCompressor(n, (n,), _args(cr=CR, **MODES["thr_s3_m1"])), n, (n,)) for n in sizes]
            groups[gname], _, ub = _group(BatchedThr, codecs, dev)
        wires[gname] = torch.zeros((8, ub), dtype=torch.uint8, device=dev)
    for gname, g in groups.items():
        assert g.encode(ts, wires[gname][0], 0, 0)
    torch.cuda.synchronize()
    k_total = sum(cd.k for cd in tk_codecs)
    row = {"case": name, "tensors": len(sizes), "elements": elems, "cr": CR, "k_total": k_total, "parent_topk": bool(parent_topk), "bars": BARS,
           "wire_bytes": {gname: int(w.shape[1]) for gname, w in wires.items()}}
    for mode in MODES:
        counts = groups[mode].kept_counts(wires[mode][0])
        row[mode + "_kept_over_k"] = round(sum(c[0] for c in counts) / k_total, 4)
        row[mode + "_found_over_k"] = round(sum(c[1] for c in counts) / k_total, 4)
    # the decode-mean's payloads: the top-k wire's pairs in the threshold wire's layout, the same rows for R = 8
    dec = wires["thr_s3_m1"].clone()
    dec[0].copy_(_thr_wire_of(wires[yard][0], tk_codecs, tk_offs, thr_codecs["thr_s3_m1"], thr_offs, ub))
    for w in (wires[yard], dec):
        for r in range(1, 8):
            w[r].copy_(w[0])
    g_tk, g_thr = groups[yard], groups["thr_s3_m1"]
    out = torch.empty(max(g_tk.out_floats, g_thr.out_floats), device=dev)
    out2 = torch.empty_like(out)
    g_tk._batch.decode(wires[yard][:8], 8, out)
    g_thr._batch.decode(dec[:8], 8, out2)
    torch.cuda.synchronize()
    row["decode_means_equal"] = (g_tk.out_floats == g_thr.out_floats
                                 and torch.equal(out[:g_tk.out_floats].view(torch.int32), out2[:g_tk.out_floats].view(torch.int32)))
    times = {}
    for rnd in range(3):
        for gname, g in groups.items():
            w = wires[gname]
            times.setdefault(gname + "_compress_eager", []).append(timed(lambda: g.encode(ts, w[0], 0, 0)))
            times.setdefault(gname + "_compress", []).append(graphed(lambda: g.encode(ts, w[0], 0, 0)))
        for R in (1, 8):
            for gname, g, w in [(yard, g_tk, wires[yard]), ("thr", g_thr, dec)] + [(gname, groups[gname], dec) for gname, _ in olds]:
                times.setdefault("%s_decode_mean_R%d_eager" % (gname, R), []).append(timed(lambda: g._batch.decode(w[:R], R, out)))
                times.setdefault("%s_decode_mean_R%d" % (gname, R), []).append(graphed(lambda: g._batch.decode(w[:R], R, out)))
    for key, tt in times.items():
        row[key + "_us_rounds"] = [round(x, 2) for x in tt]
        row[key + "_us"] = round(min(tt), 2)
    missed = []
    for path in list(MODES) + ["thr"]:
        for kind in (("compress",) if path in MODES else ("decode_mean_R1", "decode_mean_R8")):
            for eager in ("", "_eager"):
                field = "%s_%s%s_over_%s" % (path, kind, eager, yard)
                row[field] = round(row["%s_%s%s_us" % (path, kind, eager)] / row["%s_%s%s_us" % (yard, kind, eager)], 3)
                if not eager and row[field] > BARS.get("%s_%s" % (path, kind), float("inf")):
                    missed.append(field)
    for path in list(MODES) + [yard]:
        row[path + "_compress_gradient_reads_equiv"] = round(row[path + "_compress_us"] * 1e-6 * 6.3e12 / (elems * 4), 2)
    row["missed"] = missed
    if parent_thr:
        row["thr_compress_us"] = row["thr_s3_m1_compress_us"]      # (the new side of the refactor's compress: the parent's mode)
        refactor_verdict(row, {"thr": refactor_ratios(row, "thr", "parent_thr")})
    return row


def resnet50_rows(dev, shapes):
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    variants = {}
    for name, comp, kw in [("threshold_s3", ThresholdSparsificationCompressor, dict(thr_stages=3)),
                           ("threshold_s3_stride8", ThresholdSparsificationCompressor, dict(thr_stages=3, thr_fit_stride=8)),
                           ("threshold_fixed", ThresholdSparsificationCompressor, dict(thr_stages=0, thr_value=ETA_FIXED * 1e-2)),
                           ("threshold_s3_ef", ThresholdSparsificationCompressor, dict(thr_stages=3, ef=True)),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thr_time.jsonl"))
    ap.add_argument("--parent-lib", default=None, help="an older libgq_topk.so: its launches are the yardstick; without it the in-tree one")
    ap.add_argument("--parent-own-lib", default=None, help="an older libgq_thr.so (needs --parent-lib): the rows' `refactor` field")
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
