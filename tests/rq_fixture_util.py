"""TEST-ONLY: runs this project's quantizers over a rqpsq_* / rqring_* fixture (tests/golden/make_golden_rq.py: the reference's
own PSQuantizer / RingQuantizer over ResidualCompressor, CPU draws from the stored seed) and lists everything that differs --
both stages' codes, levels and (lb, ub) of every user on the wire, the aggregate of every step, the residuals."""
import hashlib
import json
import os
from argparse import Namespace

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FCN_FIXTURES = ["rqpsq_fcn_u3_plain", "rqpsq_fcn_u3_ef", "rqpsq_fcn_u3_twophase", "rqpsq_fcn_u3_ef_twophase", "rqpsq_fcn_u3_random0",
                "rqring_fcn_u3"]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def grads_of(seed, shapes, users, steps, scale):
    rs = np.random.RandomState(seed)
    return [[[(rs.standard_normal(int(np.prod(s))) * scale).astype(np.float32).reshape(s) for s in shapes]
             for _ in range(users)] for _ in range(steps)]


def run_fixture(name, device, codec_factory=None, **extra):
    """-> (list of differences, the quantizer)."""
    from gq_amd.compressors import ResidualCompressor
    from gq_amd.quantizers import PSQuantizer, RingQuantizer
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    argkw = json.loads(str(fx["args"]))
    shapes = [tuple(s) for s in json.loads(str(fx["shapes"]))]
    users, steps, seed = int(fx["users"]), int(fx["steps"]), int(fx["seed"])
    grads = grads_of(seed, shapes, users, steps, float(fx["scale"]))
    assert sha(np.concatenate([g.reshape(-1) for st in grads for us in st for g in us])) == str(fx["grads_sha"])
    ring = argkw["mode"] == "ring"
    args = Namespace(no_cuda=device.type != "cuda", scale="exp", num_users=users, gq_rng="reference", cr=256, **dict(argkw, **extra))
    params = [torch.nn.Parameter(torch.zeros(s, device=device)) for s in shapes]
    q = (RingQuantizer if ring else PSQuantizer)(ResidualCompressor, params, args, **({"codec_factory": codec_factory} if codec_factory else {}))
    coded = [i for i, p in enumerate(params) if p.numel() > 1000]
    call_param = fx["call_param"]
    per_step = users * len(coded) + (len(coded) if argkw["two_phase"] else 0)
    assert len(call_param) == steps * per_step
    diffs = []

    def check_payload(k, wire_user, what):
        i = int(call_param[k])
        cd, off = q.codecs[i], q.offsets[i]
        for stage, st, o in ((1, cd.s1, off), (2, cd.s2, off + cd.stage2_off)):
            codes, levels, lb_ub = st._views(wire_user, o)
            if sha(codes.cpu().numpy().astype(np.uint8)) != str(fx["codes%d_sha" % stage][k]):
                diffs.append("%s parameter %d: stage %d codes" % (what, i, stage))
            if not np.array_equal(lb_ub.cpu().numpy().view(np.uint32), fx["lbub%d" % stage][k].view(np.uint32)):
                diffs.append("%s parameter %d: stage %d (lb, ub) %s against %s" % (what, i, stage, lb_ub.cpu().numpy(), fx["lbub%d" % stage][k]))
            if sha(levels.cpu().numpy().astype(np.uint8)) != str(fx["levels%d_sha" % stage][k]):
                diffs.append("%s parameter %d: stage %d levels" % (what, i, stage))

    torch.manual_seed(seed)
    for step in range(steps):
        for u, gs in enumerate(grads[step]):
            for p, g in zip(params, gs):
                p.grad = torch.from_numpy(g.copy()).to(device)
            q.record(u, step)
            if ring:
                for j in range(len(coded)):
                    check_payload(step * per_step + u * len(coded) + j, q._wire[0], "step %d user %d" % (step, u))
        if not ring:
            for u in range(users):
                for j in range(len(coded)):
                    check_payload(step * per_step + u * len(coded) + j, q._wire[u], "step %d user %d" % (step, u))
        q.apply()
        for i, p in enumerate(params):
            if sha(p.grad.detach().cpu().numpy().astype(np.float32)) != str(fx["agg_sha"][step][i]):
                diffs.append("step %d parameter %d: aggregate" % (step, i))
    if "err_sha" in fx.files:
        for i, p in enumerate(params):
            for u in range(users):
                if sha(p.error[u].detach().cpu().numpy()) != str(fx["err_sha"][i][u]):
                    diffs.append("parameter %d user %d: residual" % (i, u))
    if "serr_sha" in fx.files:
        for i, p in enumerate(params):
            if sha(p.server_error.detach().cpu().numpy()) != str(fx["serr_sha"][i]):
                diffs.append("parameter %d: server residual" % i)
    return diffs, q
