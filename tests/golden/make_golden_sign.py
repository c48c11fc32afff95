#!/usr/bin/env python3
"""Generate the signSGD golden vectors under tests/golden/ (sign_*, signpsq_*, signring_*, signd_*) by IMPORTING the reference.

Run from a checkout of the reference (it is imported from the current directory, or from $GQ_REFERENCE_DIR):

    cd <reference checkout> && python -B <this repository>/tests/golden/make_golden_sign.py [--verify] [name-prefix ...]

--verify writes NOTHING: the reference is re-run on the inputs the committed fixtures hold (large cases: on their regenerated
inputs) and every stored array / digest is compared with what it produces now; exit code 1 if anything differs.

Every case's input comes from a NumPy RandomState seeded by the case's name (zlib.crc32), so a partial run writes what a full
run writes.  The reference runs on the CPU; torch.sign gives the same tensor on an MI355X (include/gq_sign.h).

What is written (data only -- inputs, and the reference's outputs or their sha256 digests):
* sign_<case>.npz           one SignSGDCompressor: x and the decoded tensor (large inputs: seed / n / x_sha / dec_sha)
* signpsq_fcn_u3_*.npz      PSQuantizer on the FCN parameter shapes, 3 users, 3 steps at epochs 0, 1, 2 with --scale exp (plain,
                            --ef, --two-phase, both): digests of every parameter's aggregate per step and of the final residuals
* signring_fcn_u3.npz       RingQuantizer, the same shapes and users, --ef, 3 steps: digests as above
* signd_resnet50_u2.npz     PSQuantizer on the ResNet-50 parameter list, 2 users, one step: digest per parameter
"""
import hashlib
import json
import os
import sys
import zlib
from argparse import Namespace

import numpy as np
import torch

REF = os.environ.get("GQ_REFERENCE_DIR") or os.getcwd()
OUT = os.path.dirname(os.path.abspath(__file__))

if not os.path.exists(os.path.join(REF, "compressors", "signsgd_compressor.py")):
    sys.exit("%s is not a checkout of the reference (see the module docstring)" % REF)
sys.path.insert(0, REF)

from compressors.signsgd_compressor import SignSGDCompressor  # noqa: E402
from quantizers.ps_quantizer import PSQuantizer  # noqa: E402
from quantizers.ring_quantizer import RingQuantizer  # noqa: E402

FCN_SHAPES = [(256, 784), (256,), (10, 256), (10,)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


def ref_sign(x):
    n = x.size
    c = SignSGDCompressor(n, (n,), Namespace(no_cuda=True))
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return c.decompress(c.compress(t)).numpy().astype(np.float32)


# ---- inputs ------------------------------------------------------------------------------------------------------------
EDGE_BITS = [0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800123, 0x7fbfffff, 0x7fc0beef, 0x7f800000,
             0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x7f7fffff, 0xff7fffff,
             0x3f800000, 0xbf800000]


def input_of(kind, n, rs):
    if kind == "randn":
        return rs.standard_normal(n).astype(np.float32)
    if kind == "edges":         # every special value at random places among normal ones
        x = rs.standard_normal(n).astype(np.float32)
        bits = np.array(EDGE_BITS, np.uint32)
        pos = rs.choice(n, n // 3, replace=False)
        x[pos] = bits[rs.randint(0, bits.size, pos.size)].view(np.float32)
        return x
    if kind == "zeros":         # mostly signed zeros
        x = np.zeros(n, np.float32)
        x[rs.rand(n) < 0.5] = np.float32(-0.0)
        nz = rs.rand(n) < 0.1
        x[nz] = rs.standard_normal(int(nz.sum())).astype(np.float32)
        return x
    raise ValueError(kind)


SINGLE = [      # name, kind, n, stored in full
    ("sign_edges", "edges", 10_007, True),
    ("sign_zeros_4097", "zeros", 4_097, True),
    ("sign_randn_1001", "randn", 1_001, True),
    ("sign_randn_1m", "randn", 1_000_000, False),
]


def single_case(name, kind, n, full):
    seed = seed_of(name)
    x = input_of(kind, n, np.random.RandomState(seed))
    dec = ref_sign(x)
    d = dict(kind=kind, n=n, seed=seed, x_sha=sha(x), dec_sha=sha(dec))
    if full:
        d.update(x=x, dec=dec)
    return d


# ---- quantizers ----------------------------------------------------------------------------------------------------------
def grads_of(seed, shapes, users, steps, scale):
    """[step][user][param] float32 arrays, drawn in that order from one RandomState; 5 % +0 and 5 % -0 entries."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        st = []
        for _ in range(users):
            us = []
            for s in shapes:
                n = int(np.prod(s))
                a = (rs.standard_normal(n) * scale).astype(np.float32)
                z = rs.rand(n)
                a[z < 0.05] = np.float32(0.0)
                a[(z >= 0.05) & (z < 0.1)] = np.float32(-0.0)
                us.append(a.reshape(s))
            st.append(us)
        out.append(st)
    return out


def run_quantizer(cls, shapes, grads, ef, two_phase, mode):
    users = len(grads[0])
    args = Namespace(no_cuda=True, ef=ef, two_phase=two_phase, scale="exp", num_users=users, mode=mode)
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    q = cls(SignSGDCompressor, params, args)
    agg = []
    for epoch, step in enumerate(grads):
        for u, gs in enumerate(step):
            for p, g in zip(params, gs):
                p.grad = torch.from_numpy(g.copy())
            q.record(u, epoch)
        q.apply()
        agg.append([p.grad.detach().numpy().astype(np.float32).copy() for p in params])
    errs = [[e.detach().numpy() for e in p.error] for p in params] if ef else None
    serr = [p.server_error.detach().numpy() for p in params] if (ef and two_phase) else None
    return agg, errs, serr


def quantizer_case(name, cls, shapes, users, steps, scale, ef, two_phase, mode="ps"):
    seed = seed_of(name)
    grads = grads_of(seed, shapes, users, steps, scale)
    agg, errs, serr = run_quantizer(cls, shapes, grads, ef, two_phase, mode)
    d = dict(seed=seed, users=users, steps=steps, scale=scale, ef=int(ef), two_phase=int(two_phase), mode=mode,
             shapes=json.dumps([list(s) for s in shapes]),
             grads_sha=sha(np.concatenate([g.reshape(-1) for st in grads for us in st for g in us])),
             agg_sha=np.array([[sha(a) for a in step] for step in agg]))
    if errs is not None:
        d["err_sha"] = np.array([[sha(e) for e in es] for es in errs])
    if serr is not None:
        d["serr_sha"] = np.array([sha(e) for e in serr])
    return d


def resnet50_shapes():
    with open(os.path.join(OUT, "resnet50_cifar_shapes.json")) as f:
        return [tuple(s) for s in json.load(f)["parameter_shapes"]]


CASES = {}
for _name, _kind, _n, _full in SINGLE:
    CASES[_name] = (lambda nm=_name, kd=_kind, n=_n, fu=_full: single_case(nm, kd, n, fu))
for _tag, _ef, _tp in (("plain", False, False), ("ef", True, False), ("twophase", False, True), ("ef_twophase", True, True)):
    _nm = "signpsq_fcn_u3_" + _tag
    CASES[_nm] = (lambda nm=_nm, ef=_ef, tp=_tp: quantizer_case(nm, PSQuantizer, FCN_SHAPES, 3, 3, 0.01, ef, tp))
CASES["signring_fcn_u3"] = lambda: quantizer_case("signring_fcn_u3", RingQuantizer, FCN_SHAPES, 3, 3, 0.01, True, False, "ring")
CASES["signd_resnet50_u2"] = lambda: quantizer_case("signd_resnet50_u2", PSQuantizer, resnet50_shapes(), 2, 1, 0.01, False, False)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f" and b.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                     b.view(np.uint32) if b.dtype == np.float32 else b)
    return a.shape == b.shape and np.array_equal(a, b)


def main(argv):
    verify = "--verify" in argv
    prefixes = [a for a in argv if not a.startswith("--")]
    bad = 0
    for name, make in CASES.items():
        if prefixes and not any(name.startswith(p) for p in prefixes):
            continue
        path = os.path.join(OUT, name + ".npz")
        d = make()
        if verify:
            g = np.load(path)
            diff = [k for k in d if k not in g.files or not same(g[k], d[k])]
            print("%-28s %s" % (name, "ok" if not diff else "DIFFERS: %s" % diff))
            bad += bool(diff)
        else:
            np.savez_compressed(path, **d)
            print("%-28s %7d bytes" % (name, os.path.getsize(path)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
