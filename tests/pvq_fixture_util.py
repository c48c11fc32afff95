"""TEST-ONLY: runs this project's quantizers over a pvqpsq_* / pvqring_* / pvqpsqd_* fixture (tests/golden/make_golden_pvqpsq.py:
the reference's own PSQuantizer / RingQuantizer over ProbabilisticVectorCompressor, CPU draws from the stored seed) and lists
everything that differs -- every user's codes, levels and (lb, ub) on the wire, the aggregate of every step, the residuals."""
import hashlib
import json
import os
from argparse import Namespace

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FCN_FIXTURES = ["pvqpsq_fcn_u3_plain", "pvqpsq_fcn_u3_ef", "pvqpsq_fcn_u3_twophase", "pvqpsq_fcn_u3_ef_twophase", "pvqring_fcn_u3",
                "pvqpsq_fcn_u3_n32", "pvqpsq_fcn_u3_random0"]
RESNET_FIXTURE = "pvqpsqd_resnet50_u2"


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def grads_of(seed, shapes, users, steps, scale):
    rs = np.random.RandomState(seed)
    return [[[(rs.standard_normal(int(np.prod(s))) * scale).astype(np.float32).reshape(s) for s in shapes]
             for _ in range(users)] for _ in range(steps)]


def run_fixture(name, device, codec_factory=None, **extra):
    """-> (list of differences, the quantizer)."""
    from gq_amd.compressors import ProbabilisticVectorCompressor
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
    q = (RingQuantizer if ring else PSQuantizer)(ProbabilisticVectorCompressor, params, args,
                                                 **({"codec_factory": codec_factory} if codec_factory else {}))
    coded = [i for i, p in enumerate(params) if p.numel() > 1000]
    n32 = argkw["n_bit"] == 32
    digests = "codes_sha" in fx.files
    call_param = fx["call_param"]
    Ms = [params[i].numel() // 16 for i in call_param]
    starts = np.concatenate([[0], np.cumsum(Ms)])
    per_step = users * len(coded) + (len(coded) if argkw["two_phase"] else 0)
    assert len(call_param) == steps * per_step
    diffs = []

    def check_payload(k, wire_user, what):
        i = int(call_param[k])
        cd, off = q.codecs[i], q.offsets[i]
        codes, levels, lb_ub = cd._views(wire_user, off)
        codes, levels = codes.cpu().numpy(), levels.cpu().numpy()
        if digests:
            if sha(codes.astype(np.uint8)) != str(fx["codes_sha"][k]):
                diffs.append("%s parameter %d: codes" % (what, i))
        elif not np.array_equal(codes, fx["codes"][starts[k]:starts[k + 1]]):
            diffs.append("%s parameter %d: codes (%d of %d differ)" % (what, i, int((codes != fx["codes"][starts[k]:starts[k + 1]]).sum()), codes.size))
        if n32:
            if sha(levels.astype(np.float32)) != str(fx["u_sha"][k]):
                diffs.append("%s parameter %d: u" % (what, i))
            return
        if not np.array_equal(lb_ub.cpu().numpy().view(np.uint32), fx["lbub"][k].view(np.uint32)):
            diffs.append("%s parameter %d: (lb, ub) %s against %s" % (what, i, lb_ub.cpu().numpy(), fx["lbub"][k]))
        if digests:
            if sha(levels.astype(np.uint8)) != str(fx["levels_sha"][k]):
                diffs.append("%s parameter %d: levels" % (what, i))
        elif not np.array_equal(levels, fx["levels"][starts[k]:starts[k + 1]]):
            diffs.append("%s parameter %d: levels" % (what, i))

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
