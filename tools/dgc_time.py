"""Time a step with momentum correction (--quantizer topk --momentum-correction M) next to the step it extends (--quantizer topk
--ef), in ONE process and alternated, on one MI355X:

    python tools/dgc_time.py [--out FILE] [--cr 256] [--windows 7]

The ResNet-50 parameter list (tests/golden/resnet50_cifar_shapes.json), one rank, one user.  Rows (JSON lines):
  step      PSQuantizer.record + apply as a training loop calls them (gradients at fixed addresses: the whole step replays from
            a graph), both quantizers in turn within every window: dgc_us, topk_ef_us, their ratio
  launches  the group's launches on their own, eager, over the 76 compressed tensors: the three of a record with momentum
            correction (accumulate, select in its error-feedback form at scale 1, mask), top-k's record with error feedback, and
            the accumulate and mask launches alone with the bytes they move and the rate that gives
Each figure: the median over the windows of HIP events around 40 back-to-back calls (after 20 untimed ones), in microseconds."""
import argparse
import json
import os
import sys
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))

from gq_amd.compressors import TopKSparsificationCompressor  # noqa: E402
from gq_amd.quantizers import PSQuantizer  # noqa: E402


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def median(xs):
    return sorted(xs)[len(xs) // 2]


def alternated(fns, iters=40, warm=20, windows=7):
    """{name: median us per call}; every window times every fn once, in turn."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            res[k].append(window(fn, iters))
    return {k: median(v) for k, v in res.items()}


def make(shapes, dev, cr, **kw):
    params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="1.0", num_users=1, mode="ps", cr=cr)
    base.update(kw)
    args = Namespace(**base)
    q = PSQuantizer(TopKSparsificationCompressor, params, args)
    grads = [torch.randn(s, device=dev) * 1e-2 for s in shapes]

    def step():
        for p, g in zip(params, grads):
            p.grad = g.detach()
        q.record(0, 1)
        q.apply()
    return q, params, grads, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cr", type=int, default=256)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--momentum", type=float, default=0.9)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    with open(os.path.join(ROOT, "tests", "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = [tuple(s) for s in json.load(f)["parameter_shapes"]]
    qd, pd, gd, step_d = make(shapes, dev, a.cr, momentum_correction=a.momentum)
    qe, pe, ge, step_e = make(shapes, dev, a.cr, ef=True)      # (error feedback adds into the gradient in place: small gradients stay finite)
    t = alternated({"dgc_us": step_d, "topk_ef_us": step_e}, windows=a.windows)
    elems = sum(p.numel() for p in pd if p.numel() > 1000)
    rows = [dict(row="step", model="resnet50_list", cr=a.cr, momentum=a.momentum, compressed_elements=elems, ratio=round(t["dgc_us"] / t["topk_ef_us"], 3),
                 dgc_paths=qd.record_paths, topk_ef_paths=qe.record_paths, **{k: round(v, 2) for k, v in t.items()})]

    # the launches on their own
    gdg, geg = qd._groups[0][2], qe._groups[0][2]
    idxs = qd._groups[0][1]
    grads = [gd[i] for i in idxs]
    us, vs = [pd[i].dgc_u[0] for i in idxs], [pd[i].dgc_v[0] for i in idxs]
    errs = [pe[i].error[0] for i in idxs]
    egrads = [ge[i] for i in idxs]
    wire = torch.zeros(qd.user_bytes, dtype=torch.uint8, device=dev)
    assert gdg.encode(grads, wire, 0, 0, errs=(us, vs), ef_scale=a.momentum) and geg.encode(egrads, wire, 0, 0, errs=errs, ef_scale=1.0)
    b = gdg._batch
    out = gdg._ef_buffer(dev)
    t = alternated({"dgc_record_us": lambda: gdg.encode(grads, wire, 0, 0, errs=(us, vs), ef_scale=a.momentum),
                    "topk_ef_record_us": lambda: geg.encode(egrads, wire, 0, 0, errs=errs, ef_scale=1.0),
                    "accumulate_us": lambda: b.accumulate(a.momentum),
                    "select_us": lambda: b.select.compress(wire, out, 1.0),
                    "mask_us": lambda: b.mask(wire)}, windows=a.windows)
    k_total = sum(cd.k for cd in gdg.codecs)
    acc_bytes, mask_bytes = 16 * elems, 8 * k_total      # g and u read, u and the scratch written | index read, u written
    rows.append(dict(row="launches", tensors=len(idxs), compressed_elements=elems, k_total=k_total,
                     accumulate_bytes=acc_bytes, accumulate_GBps=round(acc_bytes / t["accumulate_us"] / 1e3, 1),
                     mask_bytes=mask_bytes, **{k: round(v, 2) for k, v in t.items()}))
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
