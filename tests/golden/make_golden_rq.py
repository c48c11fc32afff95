#!/usr/bin/env python3
"""Generate the quantizer-level golden vectors of the ResidualCompressor under tests/golden/ (rqpsq_*, rqring_*) by IMPORTING the
reference.

Run from a checkout of the reference (it is imported from the current directory, or from $GQ_REFERENCE_DIR):

    cd <reference checkout> && python -B <this repository>/tests/golden/make_golden_rq.py [--verify] [name-prefix ...]

--verify writes NOTHING: the reference is re-run on the regenerated inputs and every stored array / digest is compared with what
it produces now; exit code 1 if anything differs.

The class's second stage runs under the same two provisions make_golden.py states for the vector compressor: (a) a scratch cwd in
which ./codebook is a link to the reference's codebooks/learned_codebook (the constructor opens ./codebook/..., the tree has
./codebooks/learned_codebook/), (b) torch.argmin DEFINED for bool input as (index of the first True) - 1, K-1 when none is True
(probabilistic_vector_compressor.py:58).  Every other line is the reference's own.

Inputs come from a NumPy RandomState seeded by the case's name (zlib.crc32); the reference's CPU draws (torch.rand, per tensor:
stage 1's level draws -- with args.random and n_bit != 32 --, stage 2's codeword draws, stage 2's level draws) from
torch.manual_seed(the same seed), set once before the first record.  What is written (data only), per case: for every compress
call in call order (the second phase's calls included) the parameter, (lb, ub) of both stages and sha256 of both stages' codes
and levels; sha256 of every parameter's aggregate per step, of the residuals and the server residuals.
* rqpsq_fcn_u3_{plain,ef,twophase,ef_twophase}.npz   PSQuantizer over FCN-shaped gradients (256x784, 256, 10x256, 10), 3 users,
                            2 steps at epochs 0, 1 (--scale exp), d16 k8 n6 random=1
* rqpsq_fcn_u3_random0.npz  random=0: deterministic levels, only stage 2's sampler draws
* rqring_fcn_u3.npz         the same through RingQuantizer (--ef)
"""
import hashlib
import json
import os
import shutil
import sys
import tempfile
import zlib
from argparse import Namespace

import numpy as np
import torch

REF = os.environ.get("GQ_REFERENCE_DIR") or os.getcwd()
OUT = os.path.dirname(os.path.abspath(__file__))

if not os.path.exists(os.path.join(REF, "compressors", "residual_compressor.py")):
    sys.exit("%s is not a checkout of the reference (see the module docstring)" % REF)
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from compressors.residual_compressor import ResidualCompressor  # noqa: E402
from quantizers.ps_quantizer import PSQuantizer  # noqa: E402
from quantizers.ring_quantizer import RingQuantizer  # noqa: E402

torch.set_num_threads(8)
FCN_SHAPES = [(256, 784), (256,), (10, 256), (10,)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


class rq_environment(object):
    """The two provisions of the module docstring."""

    def __enter__(self):
        self.tmp = tempfile.mkdtemp(prefix="gq_rq_")
        os.symlink(os.path.join(REF, "codebooks", "learned_codebook"), os.path.join(self.tmp, "codebook"))
        os.symlink(os.path.join(REF, "codebooks"), os.path.join(self.tmp, "codebooks"))      # (stage 1 opens the tree's own path)
        self.cwd = os.getcwd()
        os.chdir(self.tmp)
        self.argmin = torch.argmin

        def argmin_defined_for_bool(t, dim=None, keepdim=False):
            if t.dtype != torch.bool:
                return self.argmin(t, dim=dim, keepdim=keepdim)
            assert dim == 1 and not keepdim
            first = t.to(torch.int32).argmax(dim=1)                     # first True (0 when none is True)
            first = torch.where(t.any(dim=1), first, torch.full_like(first, t.shape[1] - 1))
            return first - 1
        torch.argmin = argmin_defined_for_bool
        return self

    def __exit__(self, *exc):
        torch.argmin = self.argmin
        os.chdir(self.cwd)
        shutil.rmtree(self.tmp)


def grads_of(seed, shapes, users, steps, scale):
    """[step][user][param] float32 arrays, drawn in that order from one RandomState."""
    rs = np.random.RandomState(seed)
    return [[[(rs.standard_normal(int(np.prod(s))) * scale).astype(np.float32).reshape(s) for s in shapes]
             for _ in range(users)] for _ in range(steps)]


def run_quantizer(cls, shapes, grads, seed, argkw):
    """-> (calls, aggregates, residuals, server residuals); calls = [(parameter, [stage 1's signature, stage 2's])] in call order."""
    users = len(grads[0])
    args = Namespace(no_cuda=True, scale="exp", num_users=users, **argkw)
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    q = cls(ResidualCompressor, params, args)
    calls = []
    for i, c in enumerate(q.compressors):
        if isinstance(c, ResidualCompressor):
            def compress(vec, i=i, inner=c.compress):
                sigs = inner(vec)
                calls.append((i, sigs))
                return sigs
            c.compress = compress
    torch.manual_seed(seed)
    agg = []
    for epoch, step in enumerate(grads):
        for u, gs in enumerate(step):
            for p, g in zip(params, gs):
                p.grad = torch.from_numpy(g.copy())
            q.record(u, epoch)
        q.apply()
        agg.append([p.grad.detach().numpy().astype(np.float32).copy() for p in params])
    errs = [[e.detach().numpy() for e in p.error] for p in params] if args.ef else None
    serr = [p.server_error.detach().numpy() for p in params] if (args.ef and args.two_phase) else None
    return calls, agg, errs, serr


def quantizer_case(name, cls, shapes, users, steps, scale, mode="ps", **kw):
    argkw = dict(c_dim=16, k_bit=8, n_bit=6, random=1, ef=False, two_phase=False, mode=mode)
    argkw.update(kw)
    seed = seed_of(name)
    grads = grads_of(seed, shapes, users, steps, scale)
    with rq_environment():
        calls, agg, errs, serr = run_quantizer(cls, shapes, grads, seed, argkw)
    d = dict(seed=seed, users=users, steps=steps, scale=scale, args=json.dumps(argkw), shapes=json.dumps([list(s) for s in shapes]),
             grads_sha=sha(np.concatenate([g.reshape(-1) for st in grads for us in st for g in us])),
             call_param=np.array([i for i, _ in calls], np.int32),
             agg_sha=np.array([[sha(a) for a in step] for step in agg]))
    for k in (0, 1):      # the two stages: [(lb, ub, levels), codes] each
        sigs = [s[k] for _, s in calls]
        assert all(int(sig[0][2].max()) <= 255 and int(sig[0][2].min()) >= 0 for sig in sigs)
        d["codes%d_sha" % (k + 1)] = np.array([sha(sig[1].numpy().astype(np.uint8)) for sig in sigs])
        d["levels%d_sha" % (k + 1)] = np.array([sha(sig[0][2].numpy().astype(np.uint8)) for sig in sigs])
        d["lbub%d" % (k + 1)] = np.array([[np.float32(sig[0][0].item()), np.float32(sig[0][1].item())] for sig in sigs], np.float32)
    if errs is not None:
        d["err_sha"] = np.array([[sha(e) for e in es] for es in errs])
    if serr is not None:
        d["serr_sha"] = np.array([sha(e) for e in serr])
    return d


CASES = {}
for _tag, _kw in (("plain", {}), ("ef", dict(ef=True)), ("twophase", dict(two_phase=True)), ("ef_twophase", dict(ef=True, two_phase=True))):
    _nm = "rqpsq_fcn_u3_" + _tag
    CASES[_nm] = (lambda nm=_nm, kw=_kw: quantizer_case(nm, PSQuantizer, FCN_SHAPES, 3, 2, 0.01, **kw))
CASES["rqpsq_fcn_u3_random0"] = lambda: quantizer_case("rqpsq_fcn_u3_random0", PSQuantizer, FCN_SHAPES, 3, 2, 0.01, random=0)
CASES["rqring_fcn_u3"] = lambda: quantizer_case("rqring_fcn_u3", RingQuantizer, FCN_SHAPES, 3, 2, 0.01, mode="ring", ef=True)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32 and b.dtype == np.float32:
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
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
            print("%-28s %s" % (name, "identical" if not diff else "DIFFERS: %s" % diff))
            bad += bool(diff)
        else:
            np.savez_compressed(path, **d)
            print("%-28s %7d bytes" % (name, os.path.getsize(path)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
