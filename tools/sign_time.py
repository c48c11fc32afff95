"""Time the signSGD kernels (libgq_sign.so) against the dense-f32 path they replace, on one MI355X:

    python tools/sign_time.py [--out FILE]

Rows (one JSON line each):
  resnet50_step   PSQuantizer record + apply over the ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json), one
                  user, default launches (graph replay), for the 2-bit wire ("sign": one BatchedSign group) and for the
                  GenericCodec path over torch.sign ("dense": what `--quantizer sign` ran before), alternated in this process,
                  three rounds each.  grads "fixed": the same gradient tensors every step; "moving": a fresh clone every step.
  single_25m      one 25 M-element tensor: gq_sign_compress_batched (wire only / + the dense signs), gq_sign_decode_sum_batched
                  for R = 1 and 8, next to torch.sign and gq_mean_rows over R dense payloads.
Times: HIP events around a window of back-to-back calls after untimed ones, median of the windows, microseconds per call."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))

from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedSign, GenericCodec, SignCodec, _up, default_codec_factory  # noqa: E402
from gq_amd.compressors import SignSGDCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402


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


class _TorchSign(object):
    def compress(self, vec):
        return torch.sign(vec)

    def decompress(self, signature):
        return signature


def _dense_factory(compressor, numel, shape, packed6=False):
    if isinstance(compressor, SignSGDCompressor):
        return GenericCodec(_TorchSign(), numel, shape)
    return default_codec_factory(compressor, numel, shape, packed6)


def resnet50_rows(dev):
    from argparse import Namespace
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    args = Namespace(no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=1, mode="ps")
    variants = {}
    for name, factory in (("sign", None), ("dense", _dense_factory)):
        params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
        q = PSQuantizer(SignSGDCompressor, params, args, codec_factory=factory)
        variants[name] = (q, params)
    rows = {}
    for rnd in range(3):
        for name, (q, params) in variants.items():
            for grads in ("fixed", "moving"):
                fixed = [g.clone() for g in src]

                def step():
                    for p, g0, g1 in zip(params, src, fixed):
                        p.grad = g1 if grads == "fixed" else g0.clone()
                    q.record(0, 0)
                    q.apply()
                us = timed(step, iters=100, warm=30, windows=3)
                rows.setdefault((name, grads), []).append(us)
    out = []
    for (name, grads), ts in sorted(rows.items()):
        q = variants[name][0]
        out.append({"case": "resnet50_step", "path": name, "grads": grads, "us_per_step_rounds": [round(t, 2) for t in ts],
                    "us_per_step_min": round(min(ts), 2), "wire_bytes_per_user": q.wire_bytes_per_user(),
                    "record_paths": dict(q.record_paths)})
    return out


def single_rows(dev, n=25_000_000):
    torch.manual_seed(1)
    t = torch.randn(n, device=dev)
    cd = SignCodec(None, n, (n,))
    g = BatchedSign([cd], [0], [0], dev, 1, cd.nbytes)
    wire = torch.zeros((8, cd.nbytes), dtype=torch.uint8, device=dev)
    out = torch.empty(g.out_floats, dtype=torch.float32, device=dev)
    assert g.encode([t], wire[0], 0, 0)
    for r in range(1, 8):
        wire[r].copy_(wire[0])
    row = {"case": "single_25m", "elements": n, "wire_bytes": cd.nbytes, "dense_wire_bytes": _up(4 * n)}
    row["compress_us"] = timed(lambda: g.encode([t], wire[0], 0, 0))
    row["compress_dense_us"] = timed(lambda: g.encode([t], wire[0], 0, 0, out=out))
    for R in (1, 8):
        row["decode_mean_R%d_us" % R] = timed(lambda: g.decode_mean(wire[:R], R))
    row["torch_sign_us"] = timed(lambda: torch.sign(t))
    dense = torch.sign(t).expand(8, n).contiguous()
    mean = torch.empty(n, dtype=torch.float32, device=dev)
    for R in (1, 8):
        row["dense_mean_rows_R%d_us" % R] = timed(lambda: native.mean_rows(dense[:R], mean))
    # bytes the compress moves (4 B read per element + the 2-bit wire) and the decode (R wires + 4 B written per element)
    row["compress_TBps"] = round((4 * n + cd.nbytes) / (row["compress_us"] * 1e-6) / 1e12, 2)
    row["decode_R1_TBps"] = round((4 * n + cd.nbytes) / (row["decode_mean_R1_us"] * 1e-6) / 1e12, 2)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = single_rows(dev) + resnet50_rows(dev)
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
