"""Time the *_streams launches of libgq_drive.so / libgq_eden.so (include/gq_drive.h: SIGNS, PER STREAM) on one MI355X against the
launches of an older build of the same library (say the parent commit's) loaded into the same process.  Run through

    python tools/drive_time.py --user-rotation own --parent-lib libgq_drive.so [--out FILE]      (default: profiles/drive_time.jsonl)
    python tools/eden_time.py --user-rotation own --parent-lib libgq_eden.so [--out FILE]        (default: profiles/eden_time.jsonl)

Rows (case rot_user, one JSON line each; the file's other rows stay):
  single_25m      one 25 M-element tensor, the launches alone, ten launches replayed from one HIP graph, alternated, three rounds, the
                  minimum.  compress: the *_streams launch at stream 5 over the parent's stepped launch (bar 1.05).  decode-mean at
                  R = 1: *_streams over the parent's stepped launch (bar 1.05).  decode-mean at R = 8: *_streams over what a user of
                  the parent has to run for the same result -- eight stepped R = 1 decode-means into eight buffers and gq_mean_rows
                  over them (bar 1.0; gq_mean_rows is libgq_hsq.so's, which this library does not touch) -- and, without a bar, over
                  the parent's shared-rotation R = 8 launch.  This build's fixed and stepped launches over the parent's (0.99 - 1.01).
                  `missed` lists every ratio outside its bar.
  resnet50_step   PSQuantizer record + apply over the ResNet-50 parameter list, one user, graph replay, gradients at fixed addresses:
                  user rotation 'own' next to 'shared', alternated, three rounds (no bar: one user is stream 0, R = 1).
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
from rot_step_time import variants  # noqa: E402
from gq_amd import native  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402

BAR, BAR_FUSED, SAME = 1.05, 1.0, (0.99, 1.01)
STREAM = 5


class parent_library(object):
    """Descriptors built inside bind to the build at `path`, which need not have the *_streams entry points."""

    def __init__(self, path, batch_cls):
        self.batch_cls, lib = batch_cls, batch_cls.LIBRARY
        version = getattr(ctypes.CDLL(path), lib.prefix + "abi_version")
        version.restype = ctypes.c_int
        self.other = native.Library(lib.name, "GQ_NO_SUCH_VARIABLE", lib.prefix, version(), [e for e in lib.exports if not e.endswith("_streams")])
        self.other.path = path

    def __enter__(self):
        self.saved, self.batch_cls.LIBRARY = self.batch_cls.LIBRARY, self.other

    def __exit__(self, *exc):
        self.batch_cls.LIBRARY = self.saved


def single_rows(kind, dev, parent_lib, n=25_000_000):
    torch.manual_seed(1)
    t = torch.randn(n, device=dev)
    pair = torch.tensor([[1, 3]], dtype=torch.int64).to(dev)
    rows = []
    for name, (comp_cls, codec_cls, group_cls, batch_cls, kw) in variants(kind).items():
        cd = codec_cls(comp_cls(n, (n,), _args(**kw)), n, (n,))
        groups = {}

        def one(tag, rotation=None, own=False):
            g = group_cls([cd], [0], [0], dev, 1, cd.nbytes)
            g.rotation, g.own, g.stream_base = rotation, own, STREAM if own else 0
            wire = torch.zeros((8, cd.nbytes), dtype=torch.uint8, device=dev)
            assert g.encode([t], wire[0], 0, 0)
            for r in range(1, 8):
                wire[r].copy_(wire[0])
            groups[tag] = (g, wire)

        one("streams", pair, own=True)
        one("step", pair)
        one("fixed")
        yard_step, yard_fixed = "step", "fixed"
        if parent_lib:
            with parent_library(parent_lib, batch_cls):
                one("parent_step", pair)
                one("parent_fixed")
            yard_step, yard_fixed = "parent_step", "parent_fixed"
        floats = groups["fixed"][0].out_floats
        out = torch.empty(floats, device=dev)
        eight = torch.empty((8, floats), device=dev)      # what the unfused yardstick decodes into

        def decode(tag, R):
            g, w = groups[tag]
            if g.own:
                return lambda: g._batch.decode(w[:R], R, out, rotation=pair, first_stream=0)
            kwd = {"rotation": g.rotation} if g.rotation is not None else {}
            return lambda: g._batch.decode(w[:R], R, out, **kwd)

        def unfused():
            g, w = groups[yard_step]
            for r in range(8):
                g._batch.decode(w[r:r + 1], 1, eight[r], rotation=pair)
            native.mean_rows(eight, out)

        times = {}
        for rnd in range(3):
            for tag, (g, w) in groups.items():
                times.setdefault(tag + "_compress", []).append(graphed(lambda: g.encode([t], w[0], 0, 0)))
                for R in (1, 8):
                    times.setdefault("%s_decode_mean_R%d" % (tag, R), []).append(graphed(decode(tag, R)))
            times.setdefault("unfused_decode_mean_R8", []).append(graphed(unfused))
        row = {"case": "rot_user", "row": "single_25m", "path": name, "elements": n, "stream": STREAM, "parent_lib": bool(parent_lib),
               "bars": {"streams_over_step": BAR, "streams_R8_over_unfused": BAR_FUSED, "this_build_over_parent": list(SAME)}}
        for key, ts in times.items():
            row[key + "_us_rounds"] = [round(x, 2) for x in ts]
            row[key + "_us"] = round(min(ts), 2)
        missed = []

        def ratio(field, a, b, lo, hi):
            row[field] = round(row[a + "_us"] / row[b + "_us"], 3)
            if hi is not None and not (lo <= row[field] <= hi):
                missed.append(field)

        ratio("streams_compress_over_%s" % yard_step, "streams_compress", yard_step + "_compress", 0.0, BAR)
        ratio("streams_decode_mean_R1_over_%s" % yard_step, "streams_decode_mean_R1", yard_step + "_decode_mean_R1", 0.0, BAR)
        ratio("streams_decode_mean_R8_over_unfused", "streams_decode_mean_R8", "unfused_decode_mean_R8", 0.0, BAR_FUSED)
        ratio("streams_decode_mean_R8_over_%s_shared" % yard_step, "streams_decode_mean_R8", yard_step + "_decode_mean_R8", 0.0, None)
        if parent_lib:
            for launch in ("compress", "decode_mean_R1", "decode_mean_R8"):
                ratio("fixed_%s_over_parent_fixed" % launch, "fixed_" + launch, "parent_fixed_" + launch, *SAME)
                ratio("step_%s_over_parent_step" % launch, "step_" + launch, "parent_step_" + launch, *SAME)
        row["missed"] = missed
        rows.append(row)
    return rows


def resnet50_rows(kind, dev):
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    name, (comp_cls, _, _, _, kw) = list(variants(kind).items())[0 if kind == "drive" else 2]
    qs = {}
    for mode in ("shared", "own"):
        params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
        qs[mode] = (PSQuantizer(comp_cls, params, _args(gq_graph=True, **dict(kw, **{kind + "_user_rotation": mode}))), params)

    def stepper(q, params):
        fixed = [g.clone() for g in src]

        def step():
            for p, g in zip(params, fixed):
                p.grad = g.detach()
            q.record(0, 0)
            q.apply()
        return step

    times = {}
    for rnd in range(3):
        for mode in ("shared", "own"):
            times.setdefault(mode, []).append(timed(stepper(*qs[mode]), iters=100, warm=30, windows=3))
    row = {"case": "rot_user", "row": "resnet50_step", "path": name}
    for mode, ts in times.items():
        row[mode + "_us_per_step_rounds"] = [round(x, 2) for x in ts]
        row[mode + "_us_per_step"] = round(min(ts), 2)
        row[mode + "_record_paths"] = dict(qs[mode][0].record_paths)
    row["own_over_shared"] = round(row["own_us_per_step"] / row["shared_us_per_step"], 3)
    return [row]


def main(kind, out, parent_lib):
    dev = torch.device("cuda:0")
    write_rows(out, single_rows(kind, dev, parent_lib) + resnet50_rows(kind, dev), replace_case="rot_user")
