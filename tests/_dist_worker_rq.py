"""Worker for the two-rank test of the residual compressor (tests/test_gpu_rq.py): both ranks drive the kernels on cuda:0 and
exchange the two-section wire over gloo (two ranks cannot share one GPU under RCCL).  gq_rng = "reference" with the CPU generator
re-seeded per (global user, step) in front of every record, so that two processes and one process draw the same numbers for the
same user.  TEST-ONLY."""
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
    return [torch.randn(s, generator=g) * 1e-2 for s in SHAPES]


def build(users, mode, ef):
    from gq_amd.compressors import ResidualCompressor
    from gq_amd.quantizers import Quantizer
    params = [torch.nn.Parameter(torch.zeros(*s, device="cuda")) for s in SHAPES]
    args = Namespace(no_cuda=False, c_dim=16, k_bit=8, n_bit=6, random=1, ef=ef, two_phase=False, scale="exp", num_users=users, mode=mode,
                     cr=256, gq_rng="reference")
    return Quantizer(ResidualCompressor, params, args), params


def run(quantizer, params, local_users, first_global_user):
    from gq_amd.codecs import BatchedResidual
    out = {}
    for st in range(STEPS):
        for u in range(local_users):
            for p, gr in zip(params, grads_for(first_global_user + u, st)):
                p.grad = gr.cuda()
            torch.manual_seed(77000 + 100 * st + first_global_user + u)      # this user's draws, whichever process records it
            quantizer.record(u, epoch=st)
        quantizer.apply()
        for i, p in enumerate(params):
            out["s%d_p%d" % (st, i)] = p.grad.data.cpu().numpy().copy()
    assert [g[0] for g in quantizer._groups] == [BatchedResidual] and quantizer._groups[0][2] is not None
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
