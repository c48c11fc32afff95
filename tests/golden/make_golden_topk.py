#!/usr/bin/env python3
"""Generate the top-k golden vectors under tests/golden/ (topk_*, topkd_*, topkpsq_*) by IMPORTING the reference.

Run from a checkout of the reference (it is imported from the current directory, or from $GQ_REFERENCE_DIR):

    cd <reference checkout> && python -B <this repository>/tests/golden/make_golden_topk.py [--verify] [name-prefix ...]

--verify writes NOTHING: the reference is re-run on the inputs the committed fixtures hold (large cases: on their regenerated
inputs) and every stored array / digest is compared with what it produces now; exit code 1 if anything differs.

Every case's input comes from a NumPy RandomState seeded by the case's name (zlib.crc32), so a partial run writes what a full
run writes.  The kernels break ties at the boundary by the lowest index; torch.topk may pick others among EQUAL nonzero
magnitudes, and then v * 1 and v * 0 differ.  So the generator checks every compress the reference makes (the two-phase
re-compress of the aggregate included) and RE-SEEDS a case (seed + 1, ...) when a nonzero tie straddles the boundary.  Ties
on a zero magnitude (v * 1 == v * 0, sign included) and among NaNs (NaN either way) are harmless and kept.

What is written (data only -- inputs, and the reference's outputs or their sha256 digests):
* topk_<case>.npz          one TopKSparsificationCompressor: x, k, the decoded tensor (large inputs: seed / n / x_sha, the
                           kept indices and the decoded tensor's digest)
* topkd_25m.npz            25 M elements at cr 256: digests of the input, the decoded tensor and the kept indices
* topkpsq_fcn_u3_*.npz     PSQuantizer on the FCN parameter shapes, 3 users, 2 steps (plain, --ef, --two-phase, both):
                           digests of every parameter's aggregate per step and of the final residuals
* topkd_resnet50_u2.npz    PSQuantizer on the ResNet-50 parameter list, 2 users, one step: digest per parameter
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

if not os.path.exists(os.path.join(REF, "compressors", "topk_sparsification_compressor.py")):
    sys.exit("%s is not a checkout of the reference (see the module docstring)" % REF)
sys.path.insert(0, REF)

from compressors.topk_sparsification_compressor import TopKSparsificationCompressor  # noqa: E402
from quantizers.ps_quantizer import PSQuantizer  # noqa: E402

FCN_SHAPES = [(256, 784), (256,), (10, 256), (10,)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def keys_of(x):
    """bits(v) & 0x7fffffff with every NaN mapped to 0x7fffffff, as int64."""
    k = (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0x7fffffff)).astype(np.int64)
    k[k > 0x7f800000] = 0x7fffffff
    return k


class Straddle(Exception):
    pass


def check_no_straddle(x, k):
    """Raise Straddle if elements with the k-th largest key are partly kept and partly dropped and that key is neither 0 nor
    NaN's (there the reference's choice among the ties decides the decoded tensor)."""
    if k == 0 or k == x.size:
        return
    key = keys_of(x.reshape(-1))
    T = np.partition(key, key.size - k)[key.size - k]
    above, ties = int((key > T).sum()), int((key == T).sum())
    if ties > k - above and T not in (0, 0x7fffffff):
        raise Straddle("key %#x: %d ties, %d of them kept" % (T, ties, k - above))


class CheckedTopK(TopKSparsificationCompressor):
    """The reference's class; every compress first checks its input for a straddling tie."""

    def compress(self, vec):
        check_no_straddle(vec.detach().cpu().numpy(), self.k)
        return super().compress(vec)


def ref_topk(x, cr):
    n = x.size
    c = CheckedTopK(n, (n,), Namespace(cr=cr, no_cuda=True))
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    dec = c.decompress(c.compress(t)).numpy().astype(np.float32)
    kept = np.sort(torch.topk(torch.abs(t.view(1, -1)), k=c.k, dim=1)[1].numpy().reshape(-1)).astype(np.uint32)
    return c.k, dec, kept


def seed_of(name, attempt):
    return (zlib.crc32(name.encode()) + 7919 * attempt) & 0x7fffffff


# ---- inputs ------------------------------------------------------------------------------------------------------------
def input_of(kind, n, rs):
    if kind == "randn":
        return rs.standard_normal(n).astype(np.float32)
    if kind == "heavytail":
        return (rs.standard_cauchy(n) * 1e-3).astype(np.float32)
    if kind == "fewnz":         # fewer nonzeros than k: the boundary key is 0; half the zeros are -0
        x = np.zeros(n, np.float32)
        nz = rs.choice(n, 3000, replace=False)
        x[nz] = rs.standard_normal(3000).astype(np.float32)
        zeros = np.setdiff1d(np.arange(n), nz)
        x[zeros[rs.rand(zeros.size) < 0.5]] = np.float32(-0.0)
        return x
    if kind == "nonfinite":     # 40 NaN, 30 +inf, 20 -inf: 90 <= k = 100
        x = rs.standard_normal(n).astype(np.float32)
        pos = rs.choice(n, 90, replace=False)
        x[pos[:40]] = np.nan
        x[pos[40:70]] = np.inf
        x[pos[70:]] = -np.inf
        return x
    raise ValueError(kind)


SINGLE = [      # name, kind, n, cr, stored in full
    ("topk_randn_1m_cr256", "randn", 1_000_000, 256, False),
    ("topk_heavytail_cr256", "heavytail", 50_000, 256, True),
    ("topk_fewnz_negzero_cr4", "fewnz", 20_000, 4, True),
    ("topk_nonfinite_cr100", "nonfinite", 10_007, 100, True),
    ("topk_k1", "randn", 5_000, 5_000, True),
    ("topk_cr1", "randn", 3_000, 1, True),
    ("topk_k0", "randn", 1_500, 2_000, True),
]


def single_case(name, kind, n, cr, full):
    for attempt in range(50):
        seed = seed_of(name, attempt)
        x = input_of(kind, n, np.random.RandomState(seed))
        try:
            k, dec, kept = ref_topk(x, cr)
        except Straddle:
            continue
        d = dict(kind=kind, n=n, cr=cr, k=k, seed=seed, x_sha=sha(x), dec_sha=sha(dec), kept=kept)
        if full:
            d.update(x=x, dec=dec)
        return d
    raise RuntimeError("%s: no seed without a straddling tie" % name)


def digest_25m(name):
    n, cr = 25_000_000, 256
    for attempt in range(50):
        seed = seed_of(name, attempt)
        x = np.random.RandomState(seed).standard_normal(n).astype(np.float32)
        try:
            k, dec, kept = ref_topk(x, cr)
        except Straddle:
            continue
        return dict(kind="randn", n=n, cr=cr, k=k, seed=seed, x_sha=sha(x), dec_sha=sha(dec), kept_sha=sha(kept))
    raise RuntimeError("%s: no seed without a straddling tie" % name)


# ---- PSQuantizer -------------------------------------------------------------------------------------------------------
def grads_of(seed, shapes, users, steps, scale):
    """[step][user][param] float32 arrays, drawn in that order from one RandomState."""
    rs = np.random.RandomState(seed)
    return [[[(rs.standard_normal(int(np.prod(s))) * scale).astype(np.float32).reshape(s) for s in shapes]
             for _ in range(users)] for _ in range(steps)]


def run_psq(shapes, grads, cr, ef, two_phase):
    users = len(grads[0])
    args = Namespace(cr=cr, no_cuda=True, ef=ef, two_phase=two_phase, scale="1.0", num_users=users, mode="ps")
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    q = PSQuantizer(CheckedTopK, params, args)
    agg = []
    for step in grads:
        for u, gs in enumerate(step):
            for p, g in zip(params, gs):
                p.grad = torch.from_numpy(g.copy())
            q.record(u, 0)
        q.apply()
        agg.append([p.grad.detach().numpy().astype(np.float32).copy() for p in params])
    errs = [[e.detach().numpy() for e in p.error] for p in params] if ef else None
    serr = [p.server_error.detach().numpy() for p in params] if (ef and two_phase) else None
    return agg, errs, serr


def psq_case(name, shapes, users, steps, scale, cr, ef, two_phase):
    for attempt in range(50):
        seed = seed_of(name, attempt)
        grads = grads_of(seed, shapes, users, steps, scale)
        try:
            agg, errs, serr = run_psq(shapes, grads, cr, ef, two_phase)
        except Straddle:
            continue
        d = dict(seed=seed, users=users, steps=steps, scale=scale, cr=cr, ef=int(ef), two_phase=int(two_phase),
                 shapes=json.dumps([list(s) for s in shapes]),
                 grads_sha=sha(np.concatenate([g.reshape(-1) for st in grads for us in st for g in us])),
                 agg_sha=np.array([[sha(a) for a in step] for step in agg]))
        if errs is not None:
            d["err_sha"] = np.array([[sha(e) for e in es] for es in errs])
        if serr is not None:
            d["serr_sha"] = np.array([sha(e) for e in serr])
        return d
    raise RuntimeError("%s: no seed without a straddling tie" % name)


def resnet50_shapes():
    with open(os.path.join(OUT, "resnet50_cifar_shapes.json")) as f:
        return [tuple(s) for s in json.load(f)["parameter_shapes"]]


CASES = {}
for _name, _kind, _n, _cr, _full in SINGLE:
    CASES[_name] = (lambda nm=_name, kd=_kind, n=_n, cr=_cr, fu=_full: single_case(nm, kd, n, cr, fu))
CASES["topkd_25m"] = lambda: digest_25m("topkd_25m")
for _tag, _ef, _tp in (("plain", False, False), ("ef", True, False), ("twophase", False, True), ("ef_twophase", True, True)):
    _nm = "topkpsq_fcn_u3_" + _tag
    CASES[_nm] = (lambda nm=_nm, ef=_ef, tp=_tp: psq_case(nm, FCN_SHAPES, 3, 2, 0.01, 256, ef, tp))
CASES["topkd_resnet50_u2"] = lambda: psq_case("topkd_resnet50_u2", resnet50_shapes(), 2, 1, 0.01, 256, False, False)


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
