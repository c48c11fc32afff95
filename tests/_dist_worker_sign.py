"""Worker for the two-rank sign test (tests/test_gpu_sign.py): both ranks drive libgq_sign.so on cuda:0 and exchange the 2-bit
wire over gloo (two ranks cannot share one GPU under RCCL).  TEST-ONLY."""
import os
import sys
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "gradient-quantization_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(96, 112), (96,), (64, 64, 3, 3), (12,), (40, 128), (1024,)]
STEPS = 3


def grads_for(global_user, step):
    g = torch.Generator().manual_seed(1000 * step + global_user)
    out = []
    for s in SHAPES:
        t = torch.randn(s, generator=g) * 1e-2
        t.view(-1)[::9] = 0.0
        out.append(t)
    return out


def build(users, mode, ef):
    from gq_amd.compressors import SignSGDCompressor
    from gq_amd.quantizers import Quantizer
    params = [torch.nn.Parameter(torch.zeros(*s, device="cuda")) for s in SHAPES]
    args = Namespace(no_cuda=False, random=0, ef=ef, two_phase=False, scale="exp", num_users=users, mode=mode)
    return Quantizer(SignSGDCompressor, params, args), params


def run(quantizer, params, local_users, first_global_user):
    out = {}
    for st in range(STEPS):
        for u in range(local_users):
            for p, gr in zip(params, grads_for(first_global_user + u, st)):
                p.grad = gr.cuda()
            quantizer.record(u, epoch=st)
        quantizer.apply()
        for i, p in enumerate(params):
            out["s%d_p%d" % (st, i)] = p.grad.data.cpu().numpy().copy()
    return out


def run_single_process(total_users, mode, ef):
    q, params = build(total_users, mode, ef)
    return run(q, params, total_users, 0)


if __name__ == "__main__":
    rank, world, out, mode, ef = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5] == "1"
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    q, params = build(2, mode, ef)
    np.savez(out + "_rank%d.npz" % rank, **run(q, params, 2, rank * 2))
    dist.barrier()
    dist.destroy_process_group()
