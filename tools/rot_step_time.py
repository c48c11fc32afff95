"""Time the stepped launches of libgq_drive.so / libgq_eden.so (include/gq_drive.h: SIGNS, STEPPED) on one MI355X against the fixed-word
launches of an older build of the same library (say the parent commit's) loaded into the same process.  Run through

    python tools/drive_time.py --rotation step --parent-lib libgq_drive.so [--out FILE]      (default: profiles/drive_time.jsonl)
    python tools/eden_time.py --rotation step --parent-lib libgq_eden.so [--out FILE]        (default: profiles/eden_time.jsonl)

Rows (case rot_step, one JSON line each; the file's other rows stay):
  single_25m      one 25 M-element tensor, the launches alone, ten launches replayed from one HIP graph: compress and decode-mean at
                  R = 1 and R = 8 -- the stepped launch, this build's fixed launch and the parent's fixed launch, alternated, three
                  rounds, the minimum.  step_*_over_parent_fixed: the ratio; `bar` is 1.05 and `missed` lists every ratio above it.
  resnet50_step   PSQuantizer record + apply over the ResNet-50 parameter list, one user, graph replay, gradients at fixed addresses:
                  rotation 'step' next to 'fixed', alternated, three rounds; the entry-point calls of one EAGER step of either
                  (launches_per_eager_step: the list has identity tensors, so gq_mean_rows carries the step move and the two agree).
--scale mse / --ef (with --rotation step): the compress launch alone under EDEN's mse scale and / or with error feedback in the
launch (ef_scale 0, so the tensor stays as it is from launch to launch) -- the instantiations the rows above do not reach; case
rot_step_<scale>[_ef], single_25m rows only.
Times: tools/mx_time.py's method."""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mx_time import _args, graphed, timed, write_rows  # noqa: E402
from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedDrive, BatchedEden, DriveCodec, EdenCodec  # noqa: E402
from gq_amd.compressors import DriveCompressor, EdenCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402

BAR = 1.05      # a launch variant against its parent


def variants(kind):
    """name -> (compressor class, codec class, group class, batch class, compressor arguments)"""
    if kind == "drive":
        return {"drive_" + s: (DriveCompressor, DriveCodec, BatchedDrive, native.DriveBatch, {"drive_scale": s}) for s in ("unbiased", "mse")}
    return {"eden_b%d" % b: (EdenCompressor, EdenCodec, BatchedEden, native.EdenBatch, {"eden_bits": b}) for b in (2, 3, 4)}


class parent_library(object):
    """Descriptors built inside bind to the build at `path`, which need not have the stepped entry points."""

    def __init__(self, path, batch_cls):
        self.batch_cls, lib = batch_cls, batch_cls.LIBRARY
        version = getattr(ctypes.CDLL(path), lib.prefix + "abi_version")
        version.restype = ctypes.c_int
        self.other = native.Library(lib.name, "GQ_NO_SUCH_VARIABLE", lib.prefix, version(), [e for e in lib.exports if not e.endswith("_stepped")])
        self.other.path = path

    def __enter__(self):
        self.saved, self.batch_cls.LIBRARY = self.batch_cls.LIBRARY, self.other

    def __exit__(self, *exc):
        self.batch_cls.LIBRARY = self.saved


def single_rows(kind, dev, parent_lib, n=25_000_000, scale=None, ef=False, case="rot_step"):
    torch.manual_seed(1)
    t = torch.randn(n, device=dev)
    pair = torch.tensor([[1, 3]], dtype=torch.int64).to(dev)
    enc = {"errs": [torch.zeros(n, device=dev)], "ef_scale": 0.0} if ef else {}
    rows = []
    for name, (comp_cls, codec_cls, group_cls, batch_cls, kw) in variants(kind).items():
        if scale and kind == "eden":
            kw = dict(kw, eden_scale=scale)
        cd = codec_cls(comp_cls(n, (n,), _args(**kw)), n, (n,))
        groups = {}

        def one(tag, rotation=None):
            g = group_cls([cd], [0], [0], dev, 1, cd.nbytes)
            g.rotation = rotation
            wire = torch.zeros((8, cd.nbytes), dtype=torch.uint8, device=dev)
            assert g.encode([t], wire[0], 0, 0, **enc)
            for r in range(1, 8):
                wire[r].copy_(wire[0])
            groups[tag] = (g, wire)

        one("fixed")
        one("step", pair)
        if parent_lib:
            with parent_library(parent_lib, batch_cls):
                one("parent_fixed")
        out = torch.empty(groups["fixed"][0].out_floats, device=dev)
        times = {}
        for rnd in range(3):
            for tag, (g, w) in groups.items():
                kwd = {"rotation": g.rotation} if g.rotation is not None else {}
                times.setdefault(tag + "_compress", []).append(graphed(lambda: g.encode([t], w[0], 0, 0, **enc)))
                for R in (1, 8) if case == "rot_step" else ():      # (the decode-mean has neither a scale mode nor error feedback)
                    times.setdefault("%s_decode_mean_R%d" % (tag, R), []).append(graphed(lambda: g._batch.decode(w[:R], R, out, **kwd)))
        row = {"case": case, "row": "single_25m", "path": name, "elements": n, "bar": BAR, "parent_lib": bool(parent_lib)}
        for key, ts in times.items():
            row[key + "_us_rounds"] = [round(x, 2) for x in ts]
            row[key + "_us"] = round(min(ts), 2)
        yard = "parent_fixed" if parent_lib else "fixed"
        row["missed"] = []
        for launch in ("compress", "decode_mean_R1", "decode_mean_R8") if case == "rot_step" else ("compress",):
            field = "step_%s_over_%s" % (launch, yard)
            row[field] = round(row["step_%s_us" % launch] / row["%s_%s_us" % (yard, launch)], 3)
            if row[field] > BAR:
                row["missed"].append(field)
            if parent_lib:
                row["fixed_%s_over_parent_fixed" % launch] = round(row["fixed_%s_us" % launch] / row["parent_fixed_%s_us" % launch], 3)
        rows.append(row)
    return rows


def resnet50_rows(kind, dev):
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    name, (comp_cls, _, _, _, kw) = list(variants(kind).items())[0 if kind == "drive" else 2]
    qs = {}
    for rot in ("fixed", "step"):
        for graph in (True, False):
            params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
            qs[(rot, graph)] = (PSQuantizer(comp_cls, params, _args(gq_graph=graph, **dict(kw, **{kind + "_rotation": rot}))), params)

    def stepper(q, params):
        fixed = [g.clone() for g in src]

        def step():
            for p, g in zip(params, fixed):
                p.grad = g.detach()
            q.record(0, 0)
            q.apply()
        return step

    launches = {}
    for rot in ("fixed", "step"):
        step = stepper(*qs[(rot, False)])
        step()
        torch.cuda.synchronize()
        before = native.CALLS[0]
        step()
        torch.cuda.synchronize()
        launches[rot] = native.CALLS[0] - before
    times = {}
    for rnd in range(3):
        for rot in ("fixed", "step"):
            times.setdefault(rot, []).append(timed(stepper(*qs[(rot, True)]), iters=100, warm=30, windows=3))
    row = {"case": "rot_step", "row": "resnet50_step", "path": name, "launches_per_eager_step": launches,
           "no_launch_added": launches["fixed"] == launches["step"]}
    for rot, ts in times.items():
        row[rot + "_us_per_step_rounds"] = [round(x, 2) for x in ts]
        row[rot + "_us_per_step"] = round(min(ts), 2)
        row[rot + "_record_paths"] = dict(qs[(rot, True)][0].record_paths)
    row["step_over_fixed"] = round(row["step_us_per_step"] / row["fixed_us_per_step"], 3)
    row["rotation_step_afterwards"] = qs[("step", True)][0].rotation_step()
    return [row]


def main(kind, out, parent_lib, scale=None, ef=False):
    dev = torch.device("cuda:0")
    if scale or ef:
        case = "rot_step" + ("_" + scale if scale else "") + ("_ef" if ef else "")
        return write_rows(out, single_rows(kind, dev, parent_lib, scale=scale, ef=ef, case=case), replace_case=case)
    write_rows(out, single_rows(kind, dev, parent_lib) + resnet50_rows(kind, dev), replace_case="rot_step")
