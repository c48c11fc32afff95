"""Time the bf16 QSGD launches (gq_qsgd_batch.tensor_type = GQ_QSGD_TENSOR_BF16) on one MI355X against the parent build's float32
launches loaded into the same process:

    python tools/qsgd_bf16_time.py --parent-lib PATH/libgq_hsq.so [--out FILE]      (default: profiles/qsgd_bf16_time.jsonl)

Rows (one JSON line each):
  bf16_25m        one 25 M-element tensor, ten launches replayed from one HIP graph, the minimum of three alternated rounds, us per
                  launch: compress stochastic (GQ_RANDOM_DEVICE) and random = 0, for c_dim 128 n_bit 2 and for c_dim 0 (one wide
                  bucket, n_bit 1), and the decode-mean at R = 1 and R = 8 -- over bf16 tensors (this build), over float32 tensors
                  (this build) and over float32 tensors with the PARENT's library.  *_bf16_over_parent: bar 1.03; *_f32_over_parent:
                  band 0.99 - 1.01; `missed` lists every ratio outside.  *_parent_again_over_parent: a second load of the parent's file
                  (the same instruction text at other addresses) over the first, the A/A spread of the comparison.
  resnet50_step   PSQuantizer record + apply over the ResNet-50 parameter list, one user, replayed from the step graphs, c_dim 128
                  n_bit 2 random 0: bf16 parameters, against float32 parameters plus the two torch casts a bf16 model needs around
                  them (bf16 -> float32 of every gradient in front, float32 -> bf16 of every mean behind)."""
import argparse
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
from gq_amd.compressors import QSGDCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402

N = 128 * 195313      # 25,000,064 elements
BAR, BAND = 1.03, (0.99, 1.01)
NAN = float("nan")


def timed(fn, iters=20, warm=5, windows=5):
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
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    return graph, reps


def up16(x):
    return (x + 15) // 16 * 16


class Case(object):
    """One tensor of N elements under one library and one tensor-side type: its descriptor, wire, gathered payloads and `out`."""

    def __init__(self, lib, dtype, d, n_bit, mode, dev):
        wide = d == 0
        d = N if wide else d
        nb = N // d
        self.lib, self.mode, self.n_bit = lib, mode, n_bit
        bits = native.qsgd_code_bits(n_bit, mode)
        torch.manual_seed(1)
        self.grad = (torch.randn(N, device=dev) * 1e-2).to(dtype)
        codes_off = up16(4 * nb)
        self.ub = codes_off + up16(N * bits // 8)
        items = -(-N // native.QSGD_WIDE_CHUNK) if wide else nb
        table = torch.tensor([[self.grad.data_ptr(), d, 0, 0, codes_off, 0, 0 if wide else nb, 0]], dtype=torch.int64).to(dev)
        self.keep = (table, torch.zeros(items, dtype=torch.int32, device=dev), torch.zeros(32, dtype=torch.int32, device=dev))
        self.s = native._QSGDBatchStruct(ctypes.sizeof(native._QSGDBatchStruct), n_bit, bits, 1 if wide else 0, 1, 0 if wide else d, items,
                                         table.data_ptr(), self.keep[1].data_ptr(), self.keep[2].data_ptr() if wide else None, None, 0,
                                         1 if dtype == torch.bfloat16 else 0)
        self.wire = torch.zeros(self.ub, dtype=torch.uint8, device=dev)
        self.out = torch.empty(N, dtype=dtype, device=dev)
        self.compress()
        torch.cuda.synchronize()
        self.gathered = self.wire.view(1, -1).repeat(8, 1).contiguous()

    def _ok(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d)" % (what, rc))

    def compress(self):
        self._ok(self.lib.gq_qsgd_compress_batched(ctypes.byref(self.s), ctypes.c_void_p(self.wire.data_ptr()), ctypes.c_int(self.mode),
                                                   ctypes.c_uint64(0x1234567), ctypes.c_float(NAN), native._stream()), "compress")

    def decode(self, R):
        self._ok(self.lib.gq_qsgd_decode_sum_batched(ctypes.byref(self.s), ctypes.c_void_p(self.gathered.data_ptr()), ctypes.c_int64(self.ub),
                                                     ctypes.c_int(R), ctypes.c_void_p(self.out.data_ptr()), ctypes.c_int(0), native._stream()),
                 "decode")


def bf16_25m(parent, again, dev):
    libs = {"bf16": (native.lib(), torch.bfloat16), "f32": (native.lib(), torch.float32), "parent": (parent, torch.float32),
            "parent_again": (again, torch.float32)}
    row = {"case": "bf16_25m", "elements": N, "bar": BAR, "f32_band": list(BAND), "missed": []}
    for cfg, d, n_bit in (("c128_n2", 128, 2), ("c0_n1", 0, 1)):
        for kind, mode in (("compress_stochastic", native.RANDOM_DEVICE), ("compress_nearest", native.RANDOM_OFF),
                           ("decode_mean_R1", native.RANDOM_OFF), ("decode_mean_R8", native.RANDOM_OFF)):
            graphs = {}
            for tag, (lib, dtype) in libs.items():
                c = Case(lib, dtype, d, n_bit, mode, dev)
                fn = c.compress if kind.startswith("compress") else (lambda c=c, R=int(kind[-1]): c.decode(R))
                graphs[tag] = (c,) + graphed(fn)
            rounds = {tag: [] for tag in libs}
            for _ in range(3):
                for tag, (c, g, reps) in graphs.items():
                    rounds[tag].append(timed(g.replay) / reps)
            key = "%s_%s" % (cfg, kind)
            for tag in libs:
                row["%s_%s_us" % (key, tag)] = round(min(rounds[tag]), 2)
                row["%s_%s_us_rounds" % (key, tag)] = [round(t, 2) for t in rounds[tag]]
            rb = row["%s_bf16_over_parent" % key] = round(min(rounds["bf16"]) / min(rounds["parent"]), 3)
            rf = row["%s_f32_over_parent" % key] = round(min(rounds["f32"]) / min(rounds["parent"]), 3)
            row["%s_parent_again_over_parent" % key] = round(min(rounds["parent_again"]) / min(rounds["parent"]), 3)      # A/A
            if rb > BAR:
                row["missed"].append("%s_bf16_over_parent" % key)
            if not BAND[0] <= rf <= BAND[1]:
                row["missed"].append("%s_f32_over_parent" % key)
            del graphs
            torch.cuda.empty_cache()
    return row


def resnet50_step(dev):
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    args = Namespace(no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=1, mode="ps", c_dim=128, k_bit=8, n_bit=2, cr=256)
    torch.manual_seed(0)
    src = [(torch.randn(s, device=dev) * 1e-2).to(torch.bfloat16) for s in shapes]
    variants = {}
    for name, dtype in (("bf16", torch.bfloat16), ("f32_plus_casts", torch.float32)):
        params = [torch.nn.Parameter(torch.zeros(s, device=dev, dtype=dtype)) for s in shapes]
        variants[name] = (PSQuantizer(QSGDCompressor, params, args), params)
    f32_fixed = [torch.empty(s, device=dev) for s in shapes]
    bf16_means = [torch.empty(s, device=dev, dtype=torch.bfloat16) for s in shapes]

    def step(name):
        q, params = variants[name]
        if name == "bf16":
            for p, g in zip(params, src):
                p.grad = g
        else:
            torch._foreach_copy_(f32_fixed, src)      # the cast in front: bf16 -> float32 of every gradient
            for p, g in zip(params, f32_fixed):
                p.grad = g
        q.record(0, 0)
        q.apply()
        if name != "bf16":
            torch._foreach_copy_(bf16_means, [p.grad for p in params])      # the cast behind every decode

    rounds = {name: [] for name in variants}
    for _ in range(3):
        for name in variants:
            rounds[name].append(timed(lambda: step(name), iters=100, warm=30, windows=3))
    row = {"case": "resnet50_step", "config": "c_dim 128 n_bit 2 random 0, one user, graph replay"}
    for name, ts in rounds.items():
        row["%s_us_per_step" % name] = round(min(ts), 2)
        row["%s_us_per_step_rounds" % name] = [round(t, 2) for t in ts]
        row["%s_record_paths" % name] = dict(variants[name][0].record_paths)
    row["bf16_over_f32_plus_casts"] = round(row["bf16_us_per_step"] / row["f32_plus_casts_us_per_step"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="the parent commit's libgq_hsq.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qsgd_bf16_time.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
    # the A/A yardstick: a copy of the parent's file is a second code object of the same instruction text at other addresses
    again = ctypes.CDLL(shutil.copy(a.parent_lib, os.path.join(tempfile.mkdtemp(prefix="gq_second_load_"), "libgq_hsq.so")))
    rows = [bf16_25m(parent, again, dev), resnet50_step(dev)]
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
