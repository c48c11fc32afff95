"""Time the rotated 1-bit kernels (libgq_drive.so) on one MI355X against the rotated microscaling launches of an older libgq_mxr.so
(say the parent commit's) loaded into the same process:

    python tools/drive_time.py --parent-lib libgq_mxr.so [--out FILE]      (default: profiles/drive_time.jsonl)

Rows (one JSON line each):
  resnet50_step   PSQuantizer record + apply over the ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json), one
                  user, default launches (graph replay), gradients at fixed addresses: --quantizer drive with both scales next to
                  --quantizer mx --mx-rotate hadamard (fp4, nearest), alternated, three rounds each; wire bytes per user.
  single_25m      one 25 M-element tensor, the launches alone: gq_drive_compress_batched (both scales) and
                  gq_drive_decode_sum_batched at R = 1 and R = 8, against the parent library's fp4 round-to-nearest
                  gq_mxr_compress_batched and its fp4 decode-mean at R = 1 and R = 8 -- the yardstick: the same 4 B per element
                  read and the same transform, about four times the wire bytes, no block reductions.  Eager, and as ten launches
                  replayed from one HIP graph (the device's own time).  *_over_parent_mxr_fp4: the ratio of the graphed times;
                  `bar` is 1.05 for each of the three launches and `missed` lists every ratio above it.
--rotation step: the rot_step rows alone -- the stepped launches against the fixed ones of --parent-lib, then an older libgq_drive.so
(tools/rot_step_time.py).
--user-rotation own: the rot_user rows alone -- the *_streams launches (per-user rotations) against the stepped and fixed ones of
--parent-lib, then an older libgq_drive.so (tools/rot_user_time.py).
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

from mx_time import _args, graphed, other_library, timed, write_rows  # noqa: E402
from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedDrive, BatchedMXR, DriveCodec, MXRCodec  # noqa: E402
from gq_amd.compressors import DriveCompressor, MXCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402

BAR = 1.05      # the margin of "the same stream, slightly different packing"
SCALES = ("unbiased", "mse")


def resnet50_rows(dev):
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    variants = {}
    for name, comp, kw in [("drive_" + s, DriveCompressor, {"drive_scale": s}) for s in SCALES] + [
            ("mxr_fp4_nearest", MXCompressor, {"mx_rotate": "hadamard", "random": 0})]:
        params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
        variants[name] = (PSQuantizer(comp, params, _args(**kw)), params)
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
    return out


def single_rows(dev, parent_lib, n=25_000_000):
    torch.manual_seed(1)
    t = torch.randn(n, device=dev)
    groups, wires = {}, {}

    def one(name, cls, cd):
        g = cls([cd], [0], [0], dev, 1, cd.nbytes)
        wire = torch.zeros((8, cd.nbytes), dtype=torch.uint8, device=dev)
        assert g.encode([t], wire[0], 0, 0)
        for r in range(1, 8):
            wire[r].copy_(wire[0])
        groups[name], wires[name] = g, wire

    for s in SCALES:
        one("drive_" + s, BatchedDrive, DriveCodec(DriveCompressor(n, (n,), _args(drive_scale=s)), n, (n,)))
    cd = MXRCodec(MXCompressor(n, (n,), _args(mx_format="fp4", random=0, mx_rotate="hadamard")), n, (n,))
    one("mxr_fp4", BatchedMXR, cd)
    if parent_lib:
        with other_library(parent_lib, native.MXRBatch, "libgq_mxr.so", "gq_mxr_", native.MXR_EXPORTS):
            one("parent_mxr_fp4", BatchedMXR, cd)
    out = torch.empty(groups["drive_unbiased"].out_floats, device=dev)
    times = {}
    for rnd in range(3):
        for name, g in groups.items():
            w = wires[name]
            times.setdefault(name + "_compress_eager", []).append(timed(lambda: g.encode([t], w[0], 0, 0)))
            times.setdefault(name + "_compress", []).append(graphed(lambda: g.encode([t], w[0], 0, 0)))
            for R in (1, 8):
                times.setdefault("%s_decode_mean_R%d_eager" % (name, R), []).append(timed(lambda: g._batch.decode(w[:R], R, out)))
                times.setdefault("%s_decode_mean_R%d" % (name, R), []).append(graphed(lambda: g._batch.decode(w[:R], R, out)))
    row = {"case": "single_25m", "elements": n, "bar": BAR, "parent_lib": bool(parent_lib),
           "wire_bytes": {name: int(w.shape[1]) for name, w in wires.items()}}
    for key, ts in times.items():
        row[key + "_us_rounds"] = [round(x, 2) for x in ts]
        row[key + "_us"] = round(min(ts), 2)
    yard = "parent_mxr_fp4" if parent_lib else "mxr_fp4"
    missed = []
    for s in SCALES:
        for kind in ("compress", "decode_mean_R1", "decode_mean_R8"):
            for eager in ("", "_eager"):
                field = "drive_%s_%s%s_over_%s" % (s, kind, eager, yard)
                row[field] = round(row["drive_%s_%s%s_us" % (s, kind, eager)] / row["%s_%s%s_us" % (yard, kind, eager)], 3)
                if not eager and row[field] > BAR:
                    missed.append(field)
    row["missed"] = missed
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drive_time.jsonl"))
    ap.add_argument("--parent-lib", default=None, help="an older libgq_mxr.so whose fp4 launches are the yardstick (without it: the in-tree one)")
    ap.add_argument("--rotation", default=None, choices=["step"],
                    help="the rot_step rows alone (tools/rot_step_time.py): the stepped launches against the fixed ones of --parent-lib, here "
                         "an older libgq_drive.so")
    ap.add_argument("--user-rotation", default=None, choices=["own"],
                    help="the rot_user rows alone (tools/rot_user_time.py): the *_streams launches against the stepped and fixed ones of "
                         "--parent-lib, here ONE older libgq_drive.so")
    a = ap.parse_args()
    if a.user_rotation == "own":
        import rot_user_time
        parent = a.parent_lib[0] if isinstance(a.parent_lib, list) and a.parent_lib else a.parent_lib
        return rot_user_time.main("drive", a.out, os.path.abspath(parent) if parent else None)
    if a.rotation == "step":
        import rot_step_time
        return rot_step_time.main("drive", a.out, a.parent_lib)
    dev = torch.device("cuda:0")
    write_rows(a.out, single_rows(dev, a.parent_lib) + resnet50_rows(dev))


if __name__ == "__main__":
    main()
