"""Time the rotated 2- / 3- / 4-bit kernels (libgq_eden.so) on one MI355X against the rotated microscaling and the rotated 1-bit
launches of older builds (say the parent commit's libgq_mxr.so and libgq_drive.so) loaded into the same process:

    python tools/eden_time.py --parent-lib libgq_mxr.so libgq_drive.so [--out FILE]      (default: profiles/eden_time.jsonl)

Rows (one JSON line each):
  single_25m      one 25 M-element tensor, the launches alone: gq_eden_compress_batched for b = 2, 3, 4 with the unbiased scale
                  (and b = 4 with the mse scale) and gq_eden_decode_sum_batched at R = 1 and R = 8, against the yardstick -- the
                  parent library's fp4 round-to-nearest gq_mxr_compress_batched and its fp4 decode-mean at R = 1 and R = 8: the
                  same 4 B per element read, the same transform, 3 % more wire bytes than b = 4 -- and, as a bracket without a
                  bar, the parent's libgq_drive.so launches.  Ten launches replayed from one HIP graph (the device's own time),
                  and eager.  *_over_parent_mxr_fp4: the ratio of the graphed times; `bar` is 1.05 for each of the nine
                  unbiased-scale ratios and `missed` lists every one above it.  *_over_parent_drive: informational.
  resnet50_step   PSQuantizer record + apply over the ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json), one
                  user, default launches (graph replay), gradients at fixed addresses: --quantizer eden at b = 2, 3, 4 next to
                  --quantizer drive and --quantizer mx --mx-rotate hadamard (fp4, nearest), alternated, three rounds each.
--user-rotation own: the rot_user rows alone -- the *_streams launches (per-user rotations) against the stepped and fixed ones of
--parent-lib, then an older libgq_eden.so (tools/rot_user_time.py).
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
from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedDrive, BatchedEden, BatchedMXR, DriveCodec, EdenCodec, MXRCodec  # noqa: E402
from gq_amd.compressors import DriveCompressor, EdenCompressor, MXCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402

BAR = 1.05      # the margin the drive row uses for box-to-box and run-to-run spread
BITS = (2, 3, 4)
KINDS = ("compress", "decode_mean_R1", "decode_mean_R8")


def resnet50_rows(dev):
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    variants = {}
    for name, comp, kw in [("eden_b%d" % b, EdenCompressor, {"eden_bits": b}) for b in BITS] + [
            ("drive", DriveCompressor, {}), ("mxr_fp4_nearest", MXCompressor, {"mx_rotate": "hadamard", "random": 0})]:
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


def single_rows(dev, parent_mxr, parent_drive, n=25_000_000):
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

    for b, s in [(b, "unbiased") for b in BITS] + [(4, "mse")]:
        one("eden_b%d_%s" % (b, s), BatchedEden, EdenCodec(EdenCompressor(n, (n,), _args(eden_bits=b, eden_scale=s)), n, (n,)))
    mxr_cd = MXRCodec(MXCompressor(n, (n,), _args(mx_format="fp4", random=0, mx_rotate="hadamard")), n, (n,))
    drive_cd = DriveCodec(DriveCompressor(n, (n,), _args()), n, (n,))
    with (other_library(parent_mxr, native.MXRBatch, "libgq_mxr.so", "gq_mxr_", native.MXR_EXPORTS) if parent_mxr else contextlib.nullcontext()):
        one("parent_mxr_fp4" if parent_mxr else "mxr_fp4", BatchedMXR, mxr_cd)
    with (other_library(parent_drive, native.DriveBatch, "libgq_drive.so", "gq_drive_", native.DRIVE_EXPORTS) if parent_drive
          else contextlib.nullcontext()):
        one("parent_drive" if parent_drive else "drive", BatchedDrive, drive_cd)
    out = torch.empty(max(g.out_floats for g in groups.values()), device=dev)
    times = {}
    for rnd in range(3):
        for name, g in groups.items():
            w = wires[name]
            times.setdefault(name + "_compress_eager", []).append(timed(lambda: g.encode([t], w[0], 0, 0)))
            times.setdefault(name + "_compress", []).append(graphed(lambda: g.encode([t], w[0], 0, 0)))
            for R in (1, 8):
                times.setdefault("%s_decode_mean_R%d_eager" % (name, R), []).append(timed(lambda: g._batch.decode(w[:R], R, out)))
                times.setdefault("%s_decode_mean_R%d" % (name, R), []).append(graphed(lambda: g._batch.decode(w[:R], R, out)))
    row = {"case": "single_25m", "elements": n, "bar": BAR, "parent_mxr": bool(parent_mxr), "parent_drive": bool(parent_drive),
           "wire_bytes": {name: int(w.shape[1]) for name, w in wires.items()}}
    for key, ts in times.items():
        row[key + "_us_rounds"] = [round(x, 2) for x in ts]
        row[key + "_us"] = round(min(ts), 2)
    yard = "parent_mxr_fp4" if parent_mxr else "mxr_fp4"
    bracket = "parent_drive" if parent_drive else "drive"
    missed = []
    for name in [n_ for n_ in groups if n_.startswith("eden_")]:
        for kind in KINDS:
            for eager in ("", "_eager"):
                field = "%s_%s%s_over_%s" % (name, kind, eager, yard)
                row[field] = round(row["%s_%s%s_us" % (name, kind, eager)] / row["%s_%s%s_us" % (yard, kind, eager)], 3)
                if not eager and name.endswith("_unbiased") and row[field] > BAR:
                    missed.append(field)
            row["%s_%s_over_%s" % (name, kind, bracket)] = round(row["%s_%s_us" % (name, kind)] / row["%s_%s_us" % (bracket, kind)], 3)
    row["missed"] = missed
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eden_time.jsonl"))
    ap.add_argument("--parent-lib", nargs="*", default=[],
                    help="an older libgq_mxr.so (its fp4 launches are the yardstick) and an older libgq_drive.so (the bracket), told apart "
                         "by their file names; without them the in-tree ones")
    ap.add_argument("--rotation", default=None, choices=["step"],
                    help="the rot_step rows alone (tools/rot_step_time.py): the stepped launches against the fixed ones of --parent-lib, here "
                         "ONE older libgq_eden.so")
    ap.add_argument("--user-rotation", default=None, choices=["own"],
                    help="the rot_user rows alone (tools/rot_user_time.py): the *_streams launches against the stepped and fixed ones of "
                         "--parent-lib, here ONE older libgq_eden.so")
    ap.add_argument("--scale", default=None, choices=["mse"], help="with --rotation step: the compress launch under the mse scale")
    ap.add_argument("--ef", action="store_true", help="with --rotation step: the compress launch with error feedback")
    a = ap.parse_args()
    if a.user_rotation == "own":
        import rot_user_time
        parent = a.parent_lib[0] if isinstance(a.parent_lib, list) and a.parent_lib else a.parent_lib
        return rot_user_time.main("eden", a.out, os.path.abspath(parent) if parent else None)
    if a.rotation == "step":
        import rot_step_time
        if len(a.parent_lib) > 1:
            ap.error("--rotation step takes one --parent-lib, an older libgq_eden.so")
        return rot_step_time.main("eden", a.out, os.path.abspath(a.parent_lib[0]) if a.parent_lib else None, a.scale, a.ef)
    parent = {"mxr": None, "drive": None}
    for p in a.parent_lib:
        kind = [k for k in parent if k in os.path.basename(p)]
        if len(kind) != 1 or parent[kind[0]]:
            ap.error("--parent-lib: %s is neither a libgq_mxr.so nor a libgq_drive.so, or named twice" % p)
        parent[kind[0]] = os.path.abspath(p)
    dev = torch.device("cuda:0")
    write_rows(a.out, single_rows(dev, parent["mxr"], parent["drive"]) + resnet50_rows(dev))


if __name__ == "__main__":
    main()
