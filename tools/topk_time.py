"""Time the top-k kernels (libgq_topk.so) next to the torch path they replace, on one MI355X:

    python tools/topk_time.py [--out FILE]

Two shapes at cr 256: one tensor of 25 M elements, and the ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json:
the 76 tensors over 1,000 elements as ONE group).  Rows:
  compress        gq_topk_compress_batched (eight launches) writing the sparse wire
  compress_dense  the same + the dense decoded tensors (what error feedback / two-phase use)
  decode_mean_R   gq_topk_decode_sum_batched over R payloads (R = 1, 8)
  torch_compress  the reference's expression per tensor on the device: abs, topk, zeros_like, scatter_, mul
                  (topk_sparsification_compressor.py:17-22) -- what went on the wire as dense f32 before
  torch_mean_R    torch.stack(decoded).mean(0) of R dense payloads per tensor
Each row: the median over 5 windows of HIP events around 50 back-to-back calls (after 20 untimed ones), in microseconds per call."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))

from gq_amd.codecs import BatchedTopK, TopKCodec, _up  # noqa: E402


class _Comp(object):
    def __init__(self, k):
        self.k = k


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


def case(name, sizes, cr, dev):
    torch.manual_seed(1)
    ts = [torch.randn(n, device=dev) for n in sizes]
    ks = [n // cr for n in sizes]
    codecs = [TopKCodec(_Comp(k), n, (n,)) for n, k in zip(sizes, ks)]
    offs, off = [], 0
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes)
    ub = max(16, _up(off))
    g = BatchedTopK(codecs, offs, list(range(len(codecs))), dev, 1, ub)
    wire = torch.zeros((8, ub), dtype=torch.uint8, device=dev)
    out = torch.empty(g.out_floats, dtype=torch.float32, device=dev)
    elems = sum(sizes)
    row = {"case": name, "tensors": len(sizes), "elements": elems, "cr": cr, "k_total": sum(ks), "wire_bytes": ub,
           "dense_wire_bytes": sum(_up(4 * n) for n in sizes)}
    assert g.encode(ts, wire[0], 0, 0)
    for r in range(1, 8):
        wire[r].copy_(wire[0])
    row["compress_us"] = timed(lambda: g.encode(ts, wire[0], 0, 0))
    row["compress_dense_us"] = timed(lambda: g.encode(ts, wire[0], 0, 0, out=out))
    for R in (1, 8):
        row["decode_mean_R%d_us" % R] = timed(lambda: g.decode_mean(wire[:R], R))

    def torch_compress():
        res = []
        for v, k in zip(ts, ks):
            vec = v.view(1, -1)
            keep = torch.zeros_like(vec)
            idx = torch.topk(torch.abs(vec), k=k, dim=1)[1]
            keep.scatter_(1, idx, 1)
            res.append(vec * keep)
        return res
    row["torch_compress_us"] = timed(torch_compress, iters=10 if elems > 5e6 else 50, warm=5)
    dec = torch_compress()
    for R in (1, 8):
        stacks = [[d] * R for d in dec]
        row["torch_mean_R%d_us" % R] = timed(lambda: [torch.stack(s).mean(0) for s in stacks], iters=10, warm=3)
    gb = elems * 4 / 1e9
    row["compress_gradient_reads_equiv"] = round(row["compress_us"] * 1e-6 * 6.3e12 / (elems * 4), 2)    # at ~6.3 TB/s
    row["compress_GBps_of_gradient"] = round(gb / (row["compress_us"] * 1e-6), 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    r50 = [n for n in (int(torch.Size(s).numel()) for s in shapes) if n > 1000]
    rows = [case("single_25m", [25_000_000], 256, dev), case("resnet50_list", r50, 256, dev)]
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
