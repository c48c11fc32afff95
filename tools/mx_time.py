"""Time the microscaling kernels (libgq_mx.so) on one MI355X, next to signSGD and QSGD in the same process:

    python tools/mx_time.py [--out FILE] [--parent-lib libgq_mx.so] [--dtype bf16]      (default: profiles/mx_time.jsonl)

Rows (one JSON line each):
  resnet50_step   PSQuantizer record + apply over the ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json), one
                  user, default launches (graph replay), gradients at fixed addresses: --quantizer mx with fp4, fp6_e2m3,
                  fp6_e3m2 and fp8,
                  --quantizer sign, and QSGD --c-dim 32 --n-bit 2 (the same 4-bit codes, the same draw per element), alternated
                  in this process, three rounds each; wire bytes per user against the dense 94,083,376.
  single_25m      one 25 M-element tensor: the compress launch alone (fp4 / fp6_e2m3 / fp6_e3m2 / fp8, stochastic rounding from the device generator
                  and deterministic) and the decode-mean at R = 1 and 8, next to the QSGD c_dim 32 bucketed compress launch
                  (the same bytes moved, one draw per element) and the sign compress; mx_fp4_over_qsgd is the ratio the README
                  quotes.  *_given_*: the draws handed in (no hash); *_graphed_*: ten launches replayed from one HIP graph (the
                  device's time without the host's share of an eager launch).
                  --parent-lib: an older build of libgq_mx.so (say the parent commit's) loaded next to the in-tree one, its fp4 /
                  fp8 launches alternated with the in-tree ones in the same rounds (parent_mx_*); *_over_parent_fp8: a launch of
                  this build over the parent's fp8 launch of the same kind, *_over_parent: over the parent's same launch.
  bf16_25m        (--dtype bf16: this row alone is measured, and replaces the row of that case in FILE, whose other rows stay) one
                  25 M-element tensor, fp4 and fp8: the four launches -- compress stochastic, compress nearest, decode-mean R = 1 and
                  R = 8 -- over bf16 tensors, over float32 tensors, and (--parent-lib) the parent build's float32 launches and, where
                  it exports the _bf16 entry points, its bf16 launches (tag parent_bf16), alternated round by round in this
                  process; eager and as ten launches replayed from one HIP graph.  *_bf16_over_parent and *_f32_over_parent: the
                  ratio to the PARENT's float32 launch of the same format and kind (graphed; *_eager_* the eager ones);
                  *_bf16_over_parent_bf16: a bf16 launch over the parent's bf16 launch of the same format and kind; `bar` is 1.03
                  and `missed` lists every ratio above it.
Times: HIP events around a window of back-to-back calls after untimed ones, median of the windows, microseconds per call; the
paths of a row are alternated round by round and the minimum over the rounds is reported next to every round."""
import argparse
import contextlib
import ctypes
import json
import os
import shutil
import sys
import tempfile
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))

from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedMX, BatchedQSGD, BatchedSign, MXCodec, QSGDCodec, SignCodec  # noqa: E402
from gq_amd.compressors import MXCompressor, QSGDCompressor, SignSGDCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402

DENSE_RESNET50_BYTES = 94083376


def timed(fn, iters=50, warm=20, windows=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        res.append(s.elapsed_time(e) / iters * 1e3)
    return sorted(res)[len(res) // 2]


def graphed(fn, reps=10):
    """Microseconds per call of `fn` with `reps` calls captured into one HIP graph and the graph replayed."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    return timed(graph.replay, iters=20, warm=5) / reps


def _args(**kw):
    base = dict(no_cuda=False, random=1, ef=False, two_phase=False, scale="exp", num_users=1, mode="ps", c_dim=32, k_bit=8, n_bit=2,
                cr=256, mx_format="fp4")
    base.update(kw)
    return Namespace(**base)


def resnet50_rows(dev):
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    variants = {}
    for name, comp, kw in (("mx_fp4", MXCompressor, {}), ("mx_fp6_e2m3", MXCompressor, {"mx_format": "fp6_e2m3"}),
                           ("mx_fp6_e3m2", MXCompressor, {"mx_format": "fp6_e3m2"}), ("mx_fp8", MXCompressor, {"mx_format": "fp8"}),
                           ("sign", SignSGDCompressor, {"random": 0}), ("qsgd_c32_n2", QSGDCompressor, {})):
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
        wb = q.wire_bytes_per_user()
        out.append({"case": "resnet50_step", "path": name, "us_per_step_rounds": [round(t, 2) for t in ts], "us_per_step_min": round(min(ts), 2),
                    "wire_bytes_per_user": wb, "dense_bytes_per_user": DENSE_RESNET50_BYTES,
                    "wire_over_dense": round(wb / DENSE_RESNET50_BYTES, 4), "record_paths": dict(q.record_paths)})
    return out


FORMATS = ("fp4", "fp6_e2m3", "fp6_e3m2", "fp8")


@contextlib.contextmanager
def library(path):
    """Groups built inside bind their launches to another build of libgq_mx.so (whatever ABI number it reports: the two entry
    points and the descriptor's layout have not changed since version 1); path None: the in-tree library."""
    if path is None:
        yield
        return
    with other_library(path, native.MXBatch, "libgq_mx.so", "gq_mx_", native.MX_EXPORTS):
        yield


@contextlib.contextmanager
def other_library(path, batch_cls, name, prefix, exports):
    """library() for either descriptor class (native.MXBatch / native.MXRBatch).  An older build may have no bf16 entry points:
    only those it exports are asked of it (the loader would otherwise refuse it), and no environment variable overrides its path
    -- the one difference to what library() did before the bf16 entry points were listed in native.MX_EXPORTS."""
    probe = ctypes.CDLL(path)
    version = getattr(probe, prefix + "abi_version")
    version.restype = ctypes.c_int
    other = native.Library(name, "GQ_NO_SUCH_VARIABLE", prefix, version(), [e for e in exports if not e.endswith("_bf16") or exports_bf16(path, prefix)])
    other.path = path
    saved, batch_cls.LIBRARY = batch_cls.LIBRARY, other      # (a descriptor takes its library when it is built)
    try:
        yield
    finally:
        batch_cls.LIBRARY = saved


def second_load(path):
    """A copy of the library at `path` under another directory: loading it gives the process a second code object of the same
    instruction text -- the A/A yardstick of a refactor's timing (the loader hands out ONE handle per file, however often asked)."""
    return shutil.copy(path, os.path.join(tempfile.mkdtemp(prefix="gq_second_load_"), os.path.basename(path)))


def refactor_ratios(row, new, parent, kinds=("compress", "decode_mean_R1", "decode_mean_R8")):
    """This build's launches (`new`) over the parent's (`parent`) next to the parent's second load over its first (A/A), graphed
    times of `row`.  The bar of a case: its largest A/A ratio + 0.01 (the half-width of stc_time.py's BAND)."""
    out = {"new_over_parent": {}, "aa": {}}
    for kind in kinds:
        base = row["%s_%s_us" % (parent, kind)]
        out["new_over_parent"][kind] = round(row["%s_%s_us" % (new, kind)] / base, 3)
        out["aa"][kind] = round(row["%s_again_%s_us" % (parent, kind)] / base, 3)
    return out


def refactor_verdict(row, ratios):
    """ratios: library -> refactor_ratios(...).  One bar for the case; `missed`: the launches above it."""
    bar = round(max(r for lib in ratios.values() for r in lib["aa"].values()) + 0.01, 3)
    row["refactor"] = dict(ratios, bar=bar, missed=["%s_%s" % (lib, kind) for lib, rr in ratios.items()
                                                     for kind, r in rr["new_over_parent"].items() if r > bar])


def exports_bf16(path, prefix):
    """Does the build of the library at `path` have the bf16 entry points?"""
    return hasattr(ctypes.CDLL(path), prefix + "compress_batched_bf16")


BAR = 1.03      # a launch of this build over the parent's launch: the spread between identical instruction streams in one run


def dtype_rows(dev, parent_lib=None, rotated=False, n=25_000_000):
    """The bf16_25m row (see the module's text); rotated: libgq_mxr.so's launches (tools/mxr_time.py)."""
    from gq_amd.codecs import BatchedMXR, MXRCodec
    torch.manual_seed(1)
    t16 = torch.randn(n, device=dev).to(torch.bfloat16)
    t32 = t16.float()      # the same values: the wire of the two is the same, byte for byte
    group_cls, codec_cls, batch_cls = (BatchedMXR, MXRCodec, native.MXRBatch) if rotated else (BatchedMX, MXCodec, native.MXBatch)
    lib_name, prefix, exports = (("libgq_mxr.so", "gq_mxr_", native.MXR_EXPORTS) if rotated else ("libgq_mx.so", "gq_mx_", native.MX_EXPORTS))
    parent_bf16 = bool(parent_lib) and exports_bf16(parent_lib, prefix)
    groups, wires, src = {}, {}, {}
    for fmt in ("fp4", "fp8"):
        for random in (1, 0):
            comp = MXCompressor(n, (n,), _args(mx_format=fmt, random=random, mx_rotate="hadamard" if rotated else "none"))
            for tag, dt, lib in (("bf16", torch.bfloat16, None), ("f32", torch.float32, None), ("parent_f32", torch.float32, parent_lib),
                                 ("parent_bf16", torch.bfloat16, parent_lib)):
                if lib is None and tag.startswith("parent_") or tag == "parent_bf16" and not parent_bf16:
                    continue
                name = "%s_%s_%s" % (fmt, "stochastic" if random else "nearest", tag)
                cd = codec_cls(comp, n, (n,), dt)
                with (other_library(lib, batch_cls, lib_name, prefix, exports) if lib else contextlib.nullcontext()):
                    g = group_cls([cd], [0], [0], dev, 1, cd.nbytes)
                wire = torch.zeros((8, cd.nbytes), dtype=torch.uint8, device=dev)
                src[name] = t16 if dt == torch.bfloat16 else t32
                assert g.encode([src[name]], wire[0], 0, 0, seed=7)
                for r in range(1, 8):
                    wire[r].copy_(wire[0])
                groups[name], wires[name] = g, wire
    for fmt in ("fp4", "fp8"):      # (the claim the ratios rest on: the same bytes leave all of them)
        for mode in ("stochastic", "nearest"):
            same = [wires["%s_%s_%s" % (fmt, mode, tag)][0] for tag in ("bf16", "f32", "parent_f32", "parent_bf16") if "%s_%s_%s" % (fmt, mode, tag) in wires]
            assert all(torch.equal(same[0], w) for w in same[1:]), "the wires of %s %s differ" % (fmt, mode)
    times, outs = {}, {}
    for rnd in range(3):
        for name, g in groups.items():
            w, t = wires[name], src[name]
            times.setdefault(name + "_compress_eager", []).append(timed(lambda: g.encode([t], w[0], 0, 0)))
            times.setdefault(name + "_compress", []).append(graphed(lambda: g.encode([t], w[0], 0, 0)))
            if "_stochastic_" in name:
                for R in (1, 8):
                    key = name.replace("_stochastic_", "_") + "_decode_mean_R%d" % R
                    out = outs.setdefault(name, torch.empty(g.out_floats, dtype=g.dtype, device=dev))
                    times.setdefault(key + "_eager", []).append(timed(lambda: g._batch.decode(w[:R], R, out)))
                    times.setdefault(key, []).append(graphed(lambda: g._batch.decode(w[:R], R, out)))
    row = {"case": "bf16_25m", "library": lib_name, "elements": n, "bar": BAR, "parent_lib": bool(parent_lib), "parent_bf16": parent_bf16}
    for key, ts in times.items():
        row[key + "_us_rounds"] = [round(x, 2) for x in ts]
        row[key + "_us"] = round(min(ts), 2)
    missed = []
    if parent_lib:
        for fmt in ("fp4", "fp8"):
            for kind in ("stochastic_%s_compress", "nearest_%s_compress", "%s_decode_mean_R1", "%s_decode_mean_R8"):
                for eager in ("", "_eager"):
                    base = row["%s_%s%s_us" % (fmt, kind % "parent_f32", eager)]
                    for tag in ("bf16", "f32"):
                        field = "%s_%s%s_over_parent" % (fmt, kind % tag, eager)
                        row[field] = round(row["%s_%s%s_us" % (fmt, kind % tag, eager)] / base, 3)
                        if not eager and row[field] > BAR:
                            missed.append(field)
                    if parent_bf16:      # bf16 against the parent's OWN bf16 launch
                        field = "%s_%s%s_over_parent_bf16" % (fmt, kind % "bf16", eager)
                        row[field] = round(row["%s_%s%s_us" % (fmt, kind % "bf16", eager)] / row["%s_%s%s_us" % (fmt, kind % "parent_bf16", eager)], 3)
                        if not eager and row[field] > BAR:
                            missed.append(field)
        row["missed"] = missed
    return [row]


def write_rows(path, rows, replace_case=None):
    """rows as JSON lines into `path`; replace_case: the file's other rows stay, only the rows of that case are replaced."""
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    kept = []
    if replace_case is not None and os.path.exists(path):
        with open(path) as f:
            kept = [ln.rstrip("\n") for ln in f if ln.strip() and json.loads(ln).get("case") != replace_case]
    with open(path, "w") as f:
        f.write("\n".join(kept + lines) + "\n")


def single_rows(dev, n=25_000_000, parent_lib=None):
    torch.manual_seed(1)
    t = torch.randn(n, device=dev)
    paths, groups, wires = {}, {}, {}

    def one(cls, cd):
        g = cls([cd], [0], [0], dev, 1, cd.nbytes)
        wire = torch.zeros((8, cd.nbytes), dtype=torch.uint8, device=dev)
        assert g.encode([t], wire[0], 0, 0)
        for r in range(1, 8):
            wire[r].copy_(wire[0])
        return g, wire

    for fmt in FORMATS:
        for random in (1, 0):
            name = "mx_%s_%s" % (fmt, "stochastic" if random else "nearest")
            cd = MXCodec(MXCompressor(n, (n,), _args(mx_format=fmt, random=random)), n, (n,))
            groups[name], wires[name] = one(BatchedMX, cd)
            if parent_lib and fmt in ("fp4", "fp8"):
                with library(parent_lib):
                    groups["parent_" + name], wires["parent_" + name] = one(BatchedMX, cd)
    qc = QSGDCodec(QSGDCompressor(n, (n,), _args()), n, (n,))
    BatchedQSGD.place_lone_buckets([qc])
    assert qc.bits == 4 and qc.d == 32 and not BatchedQSGD.is_wide(qc)
    groups["qsgd_c32_n2"], wires["qsgd_c32_n2"] = one(BatchedQSGD, qc)
    groups["sign"], wires["sign"] = one(BatchedSign, SignCodec(None, n, (n,)))
    for rnd in range(3):
        for name, g in groups.items():
            w = wires[name]
            paths.setdefault(name, []).append(timed(lambda: g.encode([t], w[0], 0, 0)))
    row = {"case": "single_25m", "elements": n}
    for name, ts in paths.items():
        row[name + "_compress_us_rounds"] = [round(x, 2) for x in ts]
        row[name + "_compress_us"] = round(min(ts), 2)
        row[name + "_wire_bytes"] = int(wires[name].shape[1])
    # what the stochastic path costs beside the hash: the same launch with the draws handed in (GQ_RANDOM_GIVEN: 4 B more read per
    # element, no hash, the same fraction rebuild and comparison)
    r = torch.rand(n, device=dev)
    for fmt in ("fp4", "fp8"):
        g, w = groups["mx_%s_stochastic" % fmt], wires["mx_%s_stochastic" % fmt]
        row["mx_%s_given_compress_us" % fmt] = round(timed(lambda: g.encode([t], w[0], 0, 0, draws=(r, {0: 0}))), 2)
    # the device's own time: ten launches captured into one HIP graph and replayed (no host work between them), per launch --
    # against the eager figures above, which cannot go below what the host needs to issue a launch
    for name, g in groups.items():
        w = wires[name]
        row[name + "_compress_graphed_us"] = round(graphed(lambda: g.encode([t], w[0], 0, 0)), 2)
    g, w = groups["mx_fp4_stochastic"], wires["mx_fp4_stochastic"]
    row["mx_fp4_given_compress_graphed_us"] = round(graphed(lambda: g.encode([t], w[0], 0, 0, draws=(r, {0: 0}))), 2)
    row["mx_fp4_over_qsgd_graphed"] = round(row["mx_fp4_stochastic_compress_graphed_us"] / row["qsgd_c32_n2_compress_graphed_us"], 3)
    row["mx_fp4_over_qsgd"] = round(row["mx_fp4_stochastic_compress_us"] / row["qsgd_c32_n2_compress_us"], 3)
    row["mx_fp4_over_qsgd_rounds"] = [round(a / b, 3) for a, b in zip(paths["mx_fp4_stochastic"], paths["qsgd_c32_n2"])]
    dec = ["mx_%s_stochastic" % f for f in FORMATS] + [k for k in groups if k.startswith("parent_") and k.endswith("stochastic")]
    dec += ["qsgd_c32_n2", "sign"]
    for R in (1, 8):
        for rnd in range(3):
            for name in dec:
                g, w = groups[name], wires[name]
                paths.setdefault("%s_decode_R%d" % (name, R), []).append(timed(lambda: g.decode_mean(w[:R], R)))
        for name in dec:
            ts = paths["%s_decode_R%d" % (name, R)]
            row["%s_decode_mean_R%d_us_rounds" % (name, R)] = [round(x, 2) for x in ts]
            row["%s_decode_mean_R%d_us" % (name, R)] = round(min(ts), 2)
    if parent_lib:
        for fmt in FORMATS:
            ref = "fp8" if fmt.startswith("fp6") else fmt
            tag = "_over_parent_fp8" if fmt.startswith("fp6") else "_over_parent"
            for kind in ("stochastic_compress", "nearest_compress", "stochastic_compress_graphed", "nearest_compress_graphed",
                         "stochastic_decode_mean_R1", "stochastic_decode_mean_R8"):
                a, b = row["mx_%s_%s_us" % (fmt, kind)], row["parent_mx_%s_%s_us" % (ref, kind)]
                row["mx_%s_%s%s" % (fmt, kind, tag)] = round(a / b, 3)
    nb = row["mx_fp4_stochastic_wire_bytes"]
    row["mx_fp4_compress_TBps"] = round((4 * n + nb) / (row["mx_fp4_stochastic_compress_us"] * 1e-6) / 1e12, 2)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_time.jsonl"))
    ap.add_argument("--parent-lib", default=None, help="an older libgq_mx.so to time next to the in-tree one (parent_mx_* fields)")
    ap.add_argument("--dtype", default=None, choices=["bf16"], help="the bf16_25m row alone: bf16 launches next to the float32 ones")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.dtype == "bf16":
        write_rows(a.out, dtype_rows(dev, a.parent_lib), replace_case="bf16_25m")
        return
    write_rows(a.out, single_rows(dev, parent_lib=a.parent_lib) + resnet50_rows(dev))


if __name__ == "__main__":
    main()
