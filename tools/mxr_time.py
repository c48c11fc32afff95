"""Time the rotated microscaling kernels (libgq_mxr.so) against the plain ones (libgq_mx.so) on one MI355X, in one process:

    python tools/mxr_time.py [--out FILE] [--dtype bf16 [--parent-lib libgq_mxr.so]]      (default: profiles/mxr_time.jsonl)

Rows (one JSON line each):
  resnet50_step   PSQuantizer record + apply over the ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json), one
                  user, default launches (graph replay), gradients at fixed addresses: --quantizer mx with and without
                  --mx-rotate hadamard, alternated, three rounds each.
  single_25m      one 25 M-element tensor: the compress launch alone, gq_mxr_compress_batched against gq_mx_compress_batched,
                  fp4 / fp6_e2m3 / fp6_e3m2 / fp8, stochastic (device generator) and nearest, eager and as ten launches replayed from one HIP graph;
                  the decode-mean at R = 1 and R = 8.  *_over_plain: the ratio to the plain MX launch of the same run -- the
                  plain launch is the yardstick, not this code.
  bf16_25m        (--dtype bf16) tools/mx_time.py's row of that name over libgq_mxr.so: the rotated launches over bf16 tensors, over
                  float32 tensors and (--parent-lib, an older libgq_mxr.so) the parent's float32 and, where it has them, bf16 launches;
                  only this row is measured, and it replaces the row of that case in FILE.
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

from mx_time import FORMATS, _args, dtype_rows, graphed, timed, write_rows  # noqa: E402
from gq_amd.codecs import BatchedMX, BatchedMXR, MXCodec, MXRCodec  # noqa: E402
from gq_amd.compressors import MXCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402


def resnet50_rows(dev):
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    variants = {}
    for name, kw in [("mx_fp4", {}), ("mxr_fp4", {"mx_rotate": "hadamard"})] + [
            (kind + "_" + f, dict({"mx_format": f}, **({"mx_rotate": "hadamard"} if kind == "mxr" else {})))
            for f in FORMATS[1:] for kind in ("mx", "mxr")]:
        params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
        variants[name] = (PSQuantizer(MXCompressor, params, _args(**kw)), params)
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
    for name, ts in rows.items():
        q = variants[name][0]
        out.append({"case": "resnet50_step", "path": name, "us_per_step_rounds": [round(t, 2) for t in ts], "us_per_step_min": round(min(ts), 2),
                    "wire_bytes_per_user": q.wire_bytes_per_user(), "record_paths": dict(q.record_paths)})
    for fmt in FORMATS:
        out.append({"case": "resnet50_step", "path": "mxr_%s_over_plain" % fmt,
                    "ratio_min": round(min(rows["mxr_" + fmt]) / min(rows["mx_" + fmt]), 3),
                    "ratio_rounds": [round(a / b, 3) for a, b in zip(rows["mxr_" + fmt], rows["mx_" + fmt])]})
    return out


def single_rows(dev, n=25_000_000):
    torch.manual_seed(1)
    t = torch.randn(n, device=dev)
    groups, wires, paths = {}, {}, {}
    for fmt in FORMATS:
        for random in (1, 0):
            for rot in (False, True):
                name = "%s_%s_%s" % ("mxr" if rot else "mx", fmt, "stochastic" if random else "nearest")
                comp = MXCompressor(n, (n,), _args(mx_format=fmt, random=random, mx_rotate="hadamard" if rot else "none"))
                cd = (MXRCodec if rot else MXCodec)(comp, n, (n,))
                g = (BatchedMXR if rot else BatchedMX)([cd], [0], [0], dev, 1, cd.nbytes)
                wire = torch.zeros((8, cd.nbytes), dtype=torch.uint8, device=dev)
                assert g.encode([t], wire[0], 0, 0)
                for r in range(1, 8):
                    wire[r].copy_(wire[0])
                groups[name], wires[name] = g, wire
    for rnd in range(3):
        for name, g in groups.items():
            w = wires[name]
            paths.setdefault(name, []).append(timed(lambda: g.encode([t], w[0], 0, 0)))
    row = {"case": "single_25m", "elements": n}
    for name, ts in paths.items():
        row[name + "_compress_us_rounds"] = [round(x, 2) for x in ts]
        row[name + "_compress_us"] = round(min(ts), 2)
    for name, g in groups.items():
        w = wires[name]
        row[name + "_compress_graphed_us"] = round(graphed(lambda: g.encode([t], w[0], 0, 0)), 2)
    out = torch.empty(groups["mx_fp4_nearest"].out_floats, device=dev)
    for fmt in FORMATS:
        for R in (1, 8):
            for rnd in range(3):
                for kind in ("mx", "mxr"):
                    name = "%s_%s_stochastic" % (kind, fmt)
                    g, w = groups[name], wires[name]
                    paths.setdefault("%s_%s_decode_R%d" % (kind, fmt, R), []).append(timed(lambda: g._batch.decode(w[:R], R, out)))
            for kind in ("mx", "mxr"):
                ts = paths["%s_%s_decode_R%d" % (kind, fmt, R)]
                row["%s_%s_decode_mean_R%d_us_rounds" % (kind, fmt, R)] = [round(x, 2) for x in ts]
                row["%s_%s_decode_mean_R%d_us" % (kind, fmt, R)] = round(min(ts), 2)
            row["mxr_%s_decode_mean_R%d_over_plain" % (fmt, R)] = round(
                row["mxr_%s_decode_mean_R%d_us" % (fmt, R)] / row["mx_%s_decode_mean_R%d_us" % (fmt, R)], 3)
        for mode in ("stochastic", "nearest"):
            a, b = "mxr_%s_%s" % (fmt, mode), "mx_%s_%s" % (fmt, mode)
            row[a + "_compress_over_plain"] = round(row[a + "_compress_us"] / row[b + "_compress_us"], 3)
            row[a + "_compress_over_plain_rounds"] = [round(x / y, 3) for x, y in zip(paths[a], paths[b])]
            row[a + "_compress_graphed_over_plain"] = round(row[a + "_compress_graphed_us"] / row[b + "_compress_graphed_us"], 3)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxr_time.jsonl"))
    ap.add_argument("--parent-lib", default=None, help="--dtype bf16: an older libgq_mxr.so whose launches are the yardstick")
    ap.add_argument("--dtype", default=None, choices=["bf16"], help="the bf16_25m row alone: bf16 launches next to the float32 ones")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.dtype == "bf16":
        write_rows(a.out, dtype_rows(dev, a.parent_lib, rotated=True), replace_case="bf16_25m")
        return
    write_rows(a.out, single_rows(dev) + resnet50_rows(dev))


if __name__ == "__main__":
    main()
