"""Time the Maurey kernels (libgq_maurey.so) against the dense-f32 path they replace, on one MI355X:

    python tools/maurey_time.py [--out FILE]      (default: profiles/maurey_time.jsonl)

Rows (one JSON line each):
  resnet50_step   PSQuantizer record + apply over the ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json), one
                  user, default launches (graph replay, gq_rng "device"), for the sparse wire ("maurey": one BatchedMaurey
                  group) and for the GenericCodec path over the torch class ("dense": torch.multinomial per tensor, the decoded
                  dense f32 on the wire -- what the class ran before), alternated in this process, three rounds each.
  single_25m      one 25 M-element tensor, k = n // 37: the compress sequence alone (wire only / + the dense decode), the
                  decode-mean for R = 1 and 8, next to torch.multinomial + sign on the same tensor.
Times: HIP events around a window of back-to-back calls after untimed ones, median of the windows, microseconds per call."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))

from gq_amd.codecs import BatchedMaurey, GenericCodec, MaureyCodec, _up, default_codec_factory  # noqa: E402
from gq_amd.compressors import MaureySparsification  # noqa: E402
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


class _TorchMaurey(object):
    """The class's torch expressions (what a CUDA tensor took before the kernels): torch.multinomial on the device."""

    def __init__(self, c):
        self.k, self.size, self.shape = c.k, c.size, c.shape

    def compress(self, vec):
        flat = vec.reshape(-1)
        mag = flat.abs()
        l1_norm = mag.sum()
        codes = torch.multinomial(mag / l1_norm, self.k, replacement=True)
        return [l1_norm / self.k, codes, torch.sign(flat[codes])]

    def decompress(self, signature):
        scale, codes, signs = signature
        out = torch.zeros(self.size, dtype=signs.dtype, device=signs.device)
        out.index_add_(0, codes.reshape(-1).long(), signs.reshape(-1))
        return (scale * out).view(self.shape)


def _dense_factory(compressor, numel, shape, packed6=False):
    if isinstance(compressor, MaureySparsification):
        return GenericCodec(_TorchMaurey(compressor), numel, shape)
    return default_codec_factory(compressor, numel, shape, packed6)


def resnet50_rows(dev):
    from argparse import Namespace
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    torch.manual_seed(0)
    src = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    args = Namespace(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=1,
                     mode="ps", gq_rng="device")
    variants = {}
    for name, factory in (("maurey", None), ("dense", _dense_factory)):
        params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
        variants[name] = (PSQuantizer(MaureySparsification, params, args, codec_factory=factory), params)
    rows = {}
    for rnd in range(3):
        for name, (q, params) in variants.items():
            fixed = [g.clone() for g in src]

            def step():
                for p, g1 in zip(params, fixed):
                    p.grad = g1
                q.record(0, 0)
                q.apply()
            fast = name == "maurey"
            rows.setdefault(name, []).append(timed(step, iters=100 if fast else 5, warm=30 if fast else 2, windows=3))
    out = []
    for name, ts in sorted(rows.items()):
        q = variants[name][0]
        out.append({"case": "resnet50_step", "path": name, "us_per_step_rounds": [round(t, 2) for t in ts],
                    "us_per_step_min": round(min(ts), 2), "wire_bytes_per_user": q.wire_bytes_per_user(),
                    "draws_per_user": sum(c.k for c in q.codecs if isinstance(c, MaureyCodec)) or None,
                    "record_paths": dict(q.record_paths)})
    return out


def single_rows(dev, n=25_000_000):
    class _K(object):
        k = n // 37
    torch.manual_seed(1)
    t = torch.randn(n, device=dev) * 1e-2
    cd = MaureyCodec(_K(), n, (n,))
    g = BatchedMaurey([cd], [0], [0], dev, 1, cd.nbytes)
    wire = torch.zeros((8, cd.nbytes), dtype=torch.uint8, device=dev)
    out = torch.empty(g.out_floats, dtype=torch.float32, device=dev)
    for r in range(8):
        assert g.encode([t], wire[r], 0, 0, seed=r)
    row = {"case": "single_25m", "elements": n, "k": cd.k, "wire_bytes": cd.nbytes, "dense_wire_bytes": _up(4 * n)}
    row["compress_us"] = round(timed(lambda: g.encode([t], wire[0], 0, 0, seed=0)), 2)
    row["compress_dense_us"] = round(timed(lambda: g.encode([t], wire[0], 0, 0, seed=0, out=out)), 2)
    for R in (1, 8):
        row["decode_mean_R%d_us" % R] = round(timed(lambda: g.decode_mean(wire[:R], R)), 2)
    ref = _TorchMaurey(MaureySparsification(n, (n,), argparse.Namespace(c_dim=16, k_bit=8, n_bit=6, no_cuda=False)))
    row["torch_compress_us"] = round(timed(lambda: ref.compress(t), iters=5, warm=2, windows=3), 2)
    row["compress_read_TBps"] = round(2 * 4 * n / (row["compress_us"] * 1e-6) / 1e12, 2)      # the gradient is read twice
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maurey_time.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = single_rows(dev) + resnet50_rows(dev)
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
