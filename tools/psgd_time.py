"""Time the low-rank compressor's kernels (libgq_psgd.so, rank 4) on one MI355X against launches of an older build (say the parent
commit's libgq_sign.so and libgq_drive.so) loaded into the same process:

    python tools/psgd_time.py --parent-lib DIR [--out FILE]      (default: profiles/psgd_time.jsonl)

DIR holds the yardsticks' libgq_sign.so and libgq_drive.so; without it the in-tree ones are the yardsticks.
Rows (one JSON line each), N(0, 1) gradients:
  single_25m, resnet50_list
                  one 4096 x 6144 tensor (25,165,824 elements), and the ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json:
                  the 54 tensors rank 4 compresses as ONE group; the yardsticks get the same tensors flat), the launches alone.
                  compress: gq_psgd_compress_batched without error feedback and without the dense decode (four launches) against the
                  yardstick's gq_sign_compress_batched, a 4 B per element streaming read -- bar 2.5 (M is read twice: 2.0 from the code).
                  compress_ef: with error feedback (five launches; no bar: the ratio next to the bytes per element from the code).
                  decode_mean_R1 / _R8: gq_psgd_decode_sum_batched on R copies of the wire its own compress wrote against the
                  yardstick's gq_drive_decode_sum_batched (the shared rotation) on its own -- bar 1.05.
                  Ten calls replayed from one HIP graph (the device's own time), and eager.  `missed` lists every graphed ratio over
                  its bar.
  resnet50_step   PSQuantizer record + apply over the whole ResNet-50 parameter list, one user, default launches (graph replay),
                  gradients at fixed addresses: --quantizer powersgd --psgd-rank 4 and the same with --ef next to --quantizer sign
                  and --quantizer stc (the in-tree libraries), alternated, three rounds each.  No bar.
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
from gq_amd.codecs import BatchedDrive, BatchedPowerSGD, BatchedSign, DriveCodec, PowerSGDCodec, SignCodec, _up  # noqa: E402
from gq_amd.compressors import DriveCompressor, PowerSGDCompressor, SignSGDCompressor, SparseTernaryCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402

RANK = 4
BARS = {"compress": 2.5, "decode_mean_R1": 1.05, "decode_mean_R8": 1.05}
YARD = {"compress": "sign", "decode_mean_R1": "drive", "decode_mean_R8": "drive"}


def _group(cls, codecs, dev):
    offs, off = [], 0
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes)
    ub = max(16, _up(off))
    return cls(codecs, offs, list(range(len(codecs))), dev, 1, ub), ub


def launches_row(name, shapes, dev, parent_dir):
    torch.manual_seed(1)
    sizes = [int(torch.Size(s).numel()) for s in shapes]
    ts = [torch.randn(n, device=dev) for n in sizes]
    elems = sum(sizes)
    pargs = _args(psgd_rank=RANK, psgd_seed=1)
    pcodecs = [PowerSGDCodec(PowerSGDCompressor(n, tuple(s), pargs), n, tuple(s), param_index=i) for i, (n, s) in enumerate(zip(sizes, shapes))]
    psgd, ub = _group(BatchedPowerSGD, pcodecs, dev)
    qs = [cd.warm_start(i, 0, dev) for i, cd in enumerate(pcodecs)]
    errs = [torch.zeros(n, device=dev) for n in sizes]
    pwire = torch.zeros((8, ub), dtype=torch.uint8, device=dev)

    def yardstick(cls, batch_cls, lib, prefix, exports, codecs):
        if parent_dir:
            with other_library(os.path.join(parent_dir, lib), batch_cls, lib, prefix, exports):
                g, b = _group(cls, codecs, dev)
        else:
            g, b = _group(cls, codecs, dev)
        w = torch.zeros((8, b), dtype=torch.uint8, device=dev)
        assert g.encode(ts, w[0], 0, 0)
        for r in range(1, 8):
            w[r].copy_(w[0])
        return g, w

    sign, swire = yardstick(BatchedSign, native.SignBatch, "libgq_sign.so", "gq_sign_", native.SIGN_EXPORTS,
                            [SignCodec(SignSGDCompressor(n, (n,), _args()), n, (n,)) for n in sizes])
    drive, dwire = yardstick(BatchedDrive, native.DriveBatch, "libgq_drive.so", "gq_drive_", native.DRIVE_EXPORTS,
                             [DriveCodec(DriveCompressor(n, (n,), _args(drive_scale="unbiased")), n, (n,)) for n in sizes])
    state = (None, qs, 0)
    assert psgd.encode(ts, pwire[0], 0, 0, state, None)
    for r in range(1, 8):
        pwire[r].copy_(pwire[0])
    torch.cuda.synchronize()
    out = torch.empty(max(psgd.out_floats, drive.out_floats), device=dev)
    paths = {
        "psgd_compress": lambda: psgd.encode(ts, pwire[0], 0, 0, state, None),
        "psgd_compress_ef": lambda: psgd.encode(ts, pwire[0], 0, 0, (errs, qs, 0), 1.0),
        "sign_compress": lambda: sign.encode(ts, swire[0], 0, 0),
    }
    for R in (1, 8):
        paths["psgd_decode_mean_R%d" % R] = lambda R=R: psgd._batch.decode(pwire[:R], R, out)
        paths["drive_decode_mean_R%d" % R] = lambda R=R: drive._batch.decode(dwire[:R], R, out)
    times = {}
    for rnd in range(3):
        for key, fn in paths.items():
            times.setdefault(key + "_eager", []).append(timed(fn))
            times.setdefault(key, []).append(graphed(fn))
            if key == "psgd_compress_ef":      # (the residual grows with every call: back to zero between the measurements)
                for e in errs:
                    e.zero_()
    nm = [(cd.n, cd.m) for cd in pcodecs]
    factors = 4 * RANK * sum(n + m for n, m in nm)
    back = 4 * RANK * sum(-(-n // native.PSGD_ROW_BLOCK) * m for n, m in nm)      # the row blocks' partial sums, written and read
    row = {"case": name, "tensors": len(sizes), "elements": elems, "rank": RANK, "parent_lib": bool(parent_dir), "bars": BARS,
           "yardsticks": {"compress": "gq_sign_compress_batched", "decode_mean": "gq_drive_decode_sum_batched (shared rotation)"},
           "wire_bytes": {"psgd": int(pwire.shape[1]), "sign": int(swire.shape[1]), "drive": int(dwire.shape[1])},
           "bytes_per_element_from_the_code": {
               "psgd_compress": round((8 * elems + 2 * back + 3 * factors) / elems, 3),             # M twice
               "psgd_compress_ef": round((24 * elems + 2 * back + 4 * factors) / elems, 3),         # M, e read + written, e, e read + written
               "psgd_decode_mean_R1": round((4 * elems + factors) / elems, 3), "sign_compress": 4.125}}
    for key, tt in times.items():
        row[key + "_us_rounds"] = [round(x, 2) for x in tt]
        row[key + "_us"] = round(min(tt), 2)
    missed = []
    for kind, bar in BARS.items():
        for eager in ("", "_eager"):
            field = "psgd_%s%s_over_parent_%s" % (kind, eager, YARD[kind])
            row[field] = round(row["psgd_%s%s_us" % (kind, eager)] / row["%s_%s%s_us" % (YARD[kind], kind, eager)], 3)
            if not eager and row[field] > bar:
                missed.append(field)
    for eager in ("", "_eager"):
        row["psgd_compress_ef%s_over_parent_sign" % eager] = round(row["psgd_compress_ef%s_us" % eager] / row["sign_compress%s_us" % eager], 3)
    row["psgd_compress_gradient_reads_equiv"] = round(row["psgd_compress_us"] * 1e-6 * 6.3e12 / (elems * 4), 2)
    row["missed"] = missed
    return row


def resnet50_rows(dev, shapes):
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    variants = {}
    for name, comp, kw in [("powersgd", PowerSGDCompressor, {}), ("powersgd_ef", PowerSGDCompressor, dict(ef=True)),
                           ("sign", SignSGDCompressor, {}), ("stc", SparseTernaryCompressor, {})]:
        params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
        variants[name] = (PSQuantizer(comp, params, _args(psgd_rank=RANK, psgd_seed=1, **kw)), params)
    rows = {}
    for rnd in range(3):
        for name, (q, params) in variants.items():
            fixed = [g.clone() for g in src]

            def step():
                for p, g in zip(params, fixed):
                    p.grad = g
                q.record(0, 1)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psgd_time.jsonl"))
    ap.add_argument("--parent-lib", default=None,
                    help="a directory with an older libgq_sign.so and libgq_drive.so: their launches are the yardsticks; without it the in-tree ones")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = [tuple(s) for s in json.load(f)["parameter_shapes"]]
    args = _args(psgd_rank=RANK)
    r50 = [s for s in shapes if PowerSGDCompressor(int(torch.Size(s).numel()), s, args).compresses]
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    write_rows(a.out, [launches_row("single_25m", [(4096, 6144)], dev, parent), launches_row("resnet50_list", r50, dev, parent)]
               + resnet50_rows(dev, shapes))


if __name__ == "__main__":
    main()
