"""Subvectors whose projection is a SIGNED zero, for the HSQ encode kernels that pad the sub-dimension (csrc/hsq_encode_pf.hip: 12 in
16, 24 in 32; csrc/hsq_encode.hip: d rounded up to 8 in LDS, odd d in the last MFMA k-step).  TEST INFRASTRUCTURE ONLY; numpy and
the CPU oracle, nothing from a GPU kernel.  On top of hsq_encode_contract (ec), rq_contract and oracle.hsq_encode_scalar.

The contract: u is the literal fmaf chain from +0, ascending over the subvector's d REAL elements.  A product that underflows
rounds to -0: with g = -+min-subnormal at a column j where every |c[k][j]| < 0.5, every row's product at j is a zero, row 0's
is -0, and fmaf(c, g, +0) = -0.  Zeros behind j signed so that row 0's products are -0 keep the chain there (-0 + -0 = -0).  Every
|p| is zero, so the code is 0 and u = p[0] = -0 (0x80000000).  One more step over a zero-padded element gives fmaf(0, 0, -0) = +0:
`padded` below is that restatement -- rows and codebook padded with zeros to D columns, the same oracle -- NOT the contract.

Row kinds (`catalog`): neg_last / pos_last (min-subnormal at d - 1, row 0's product negative / positive), neg_mid@j / pos_mid@j (at
a column j < d - 1, the elements behind j zeros whose products with row 0 are -0), neg_last2 (twice the min-subnormal at d - 1,
where every |c| < 0.25).  pos_* rows are the controls: u = +0 either way.
tests/test_hsq_zero_contract.py checks without a GPU what is claimed here.

What the CPU proof does NOT cover: at shapes without padding -- (16, 250) on the exact LDS kernel, d = 16 on the d16 MFMA kernel,
every shape of the VALU kernel -- the padded restatement IS the contract, so it distinguishes nothing there.  Those kernels could
lose the sign another way, a running best that starts from +0 and is only replaced by a strictly larger |p|; only the GPU cases
tell (the same expectations: u of every neg_* row is 0x80000000)."""
import collections
import functools
import os

import numpy as np

import hsq_dequant_contract as hc
import hsq_encode_contract as ec
import rq_contract as rc

F = np.float32
TINY = np.array([1], np.uint32).view(np.float32)[0]          # the smallest subnormal, 2^-149
NEG0, POS0 = 0x80000000, 0x00000000
SHIPPED = {(24, 256): "codebook_d24_k256_normalized.npy", (24, 64): "codebook_d24_k64_normalized.npy"}
COLUMN_SCALE = F(2.0 ** -5)                                   # test codebooks: columns (d - 1) // 2 and d - 1 times this
# (a): ec.SMALL_MS-like tensors and one of five tiles; (b): tensor 5, only the new rows; (c): tensor 6, only neg_* rows
MS = (67, 1, 130, 64, 320, 70, 70)
ONLY_NEW, ONLY_NEG = 5, 6
EF_SCALES = ec.EF_SCALES


def pad_to(d, path):
    """The columns a kernel's exact chain would run over if it went on over its padding."""
    if path == ec.PREFILTER:
        return {12: 16, 24: 32}.get(d, d)
    return (d + 7) // 8 * 8           # lds_plan's dpad (the generic kernel, impl 2 and d > 128, pads an odd d to d + 1: any zero
    #                                   column behind d - 1 gives the same restatement)


@functools.lru_cache(maxsize=None)
def codebook(d, K, shipped=False):
    if shipped:
        cb = rc.f32(np.load(os.path.join(rc.GOLDEN, SHIPPED[(d, K)])))
        assert cb.shape == (K, d)
    else:
        cb = ec.codebook(d, K).copy()
        cols = sorted({d - 1} | ({(d - 1) // 2} if d >= 3 else set()))
        cb[:, cols] *= COLUMN_SCALE                            # (a power of two: exact, and ec's ties stay ties)
    cb.setflags(write=False)
    return cb


def small_columns(cb, bound=0.5):
    return [j for j in range(cb.shape[1]) if np.abs(cb[:, j]).max() < bound and cb[0, j] != 0]


@functools.lru_cache(maxsize=None)
def catalog(d, K, shipped=False):
    """-> tuple of (name, row f32[d]).  Every kind the codebook has columns for; at most two mid columns."""
    return catalog_of(codebook(d, K, shipped))


def catalog_of(cb):
    """catalog for any codebook f32[K, d] (the quantizer-level test: the compressor's own codewords)."""
    cb = rc.f32(cb)
    K, d = cb.shape
    s0 = np.where(np.signbit(cb[0]), F(-1.0), F(1.0)).astype(np.float32)      # signs of row 0
    assert (cb[0] != 0).all()
    zeros_neg = rc.f32(-s0 * F(0.0))                          # zeros whose products with row 0 are -0
    small = small_columns(cb)
    out = []

    def row(j, sign, mult=1):
        g = zeros_neg.copy()
        g[j] = F(sign) * s0[j] * F(mult) * TINY
        return g

    for j in [c for c in small if c < d - 1][:2]:
        out += [("neg_mid@%d" % j, row(j, -1)), ("pos_mid@%d" % j, row(j, +1))]
    if d - 1 in small:
        out += [("neg_last", row(d - 1, -1)), ("pos_last", row(d - 1, +1))]
    if d - 1 in small_columns(cb, 0.25):
        out += [("neg_last2", row(d - 1, -1, 2))]
    assert out, "no column of the (%d, %d) codebook has max |c| < 0.5" % (d, K)
    return tuple(out)


def is_neg(name):
    return name.startswith("neg")


def layout_kinds(d, K, shipped=False):
    """Per tensor of MS: int16[M], -1 = an ordinary Gaussian row, else an index into catalog.  Deterministic."""
    cat = catalog(d, K, shipped)
    negs = [i for i, (n, _) in enumerate(cat) if is_neg(n)]
    out = []
    for s, M in enumerate(MS):
        k = np.full(M, -1, np.int16)
        for r in range(M):
            if s == ONLY_NEW:
                k[r] = r % len(cat)
            elif s == ONLY_NEG:
                k[r] = negs[r % len(negs)]
            elif M == 1 or (r + s) % 4 == 0:
                k[r] = (r // 4 + s) % len(cat)
        out.append(k)
    return out


def _ef_split(v, ef_scale, r):
    """(grad, err) with grad + RN(ef_scale * err) == v bit for bit for a catalog row v.  Even r: err is v's zeros (x + (+-0) of
    its own sign is x); odd r: the subnormal comes out of the error buffer (grad a zero of its sign there)."""
    zero = rc.f32(np.copysign(F(0.0), v))
    if r % 2 == 0:
        return v.copy(), zero
    j = int(np.nonzero(v)[0][0])
    g, e = v.copy(), zero.copy()
    g[j] = zero[j]
    for n in range(1, 64):
        e[j] = np.copysign(F(n) * TINY, v[j])
        if rc.bits(ec.ef_add(g, e, ef_scale))[j] == rc.bits(v)[j]:
            return g, e
    raise AssertionError("no error value gives the row under ef_scale %r" % ef_scale)


ZCase = collections.namedtuple("ZCase", "d K shipped ef level")      # ef: None or an index into EF_SCALES; level: ec.Layout's form


def zcase_id(c):
    return "d%d-K%d-%s-%s-l%d" % (c.d, c.K, "shipped" if c.shipped else "test", "plain" if c.ef is None else "ef%g" % EF_SCALES[c.ef], c.level)


class Zero(object):
    """The tensors MS of a shape: gradients (and error buffers), the layout, and what an encode must leave.  Has the attributes
    ec.chain_want reads (want, lay, cb, errs, v, ebuf)."""

    def __init__(self, c):
        self.c, self.Ms = c, MS
        self.cb, self.cat = codebook(c.d, c.K, c.shipped), catalog(c.d, c.K, c.shipped)
        self.code_bytes = 1 if c.K <= 256 else 4
        self.path = ec.batch_path(c.d, c.K, self.code_bytes, len(MS))
        self.lay = ec.Layout(MS, c.d, self.code_bytes, c.level)
        self.ef_scale = None if c.ef is None else EF_SCALES[c.ef]
        self.kinds = layout_kinds(c.d, c.K, c.shipped)
        self.v, self.grads, self.errs = [], [], []
        for s, M in enumerate(MS):
            rs = np.random.RandomState(131 * c.d + c.K + 7919 * s)
            v = rc.f32(rs.standard_normal((M, c.d)) * 1e-2)
            has = self.ef_scale is not None and s % 3 != 1          # every third tensor has no error buffer
            e = rc.f32(rs.standard_normal((M, c.d)) * 1e-2) if has else None
            g = v.copy()
            for r in np.nonzero(self.kinds[s] >= 0)[0]:
                row = self.cat[self.kinds[s][r]][1]
                if has:
                    g[r], e[r] = _ef_split(row, self.ef_scale, int(r))
                else:
                    g[r] = row
            self.grads.append(g)
            self.errs.append(e)
            self.v.append(g if e is None else ec.ef_add(g, e, self.ef_scale))
        self.gbuf, self.ebuf = self.lay.floats_of(self.grads), self.lay.floats_of(self.errs)

    def special(self, s):
        """-> (rows of tensor s that are catalog rows, their names)."""
        rows = np.nonzero(self.kinds[s] >= 0)[0]
        return rows, [self.cat[self.kinds[s][r]][0] for r in rows]

    def encode(self, padded=False):
        """Per tensor (codes, u): ONE oracle call.  padded: NOT the contract -- the chain goes on over zero padding."""
        v, cb = np.concatenate(self.v), self.cb
        if padded:
            D = pad_to(self.c.d, self.path)
            v = np.concatenate([v, np.zeros((v.shape[0], D - self.c.d), np.float32)], axis=1)
            cb = np.concatenate([cb, np.zeros((cb.shape[0], D - self.c.d), np.float32)], axis=1)
        codes, u = ec.encode_ref(v, cb)
        cut = np.cumsum(MS)[:-1]
        return list(zip(np.split(codes, cut), np.split(u, cut)))

    @functools.lru_cache(maxsize=None)
    def want(self, padded=False):
        enc = self.encode(padded)
        wire = self.lay.new_wire()
        for s, (codes, _) in enumerate(enc):
            self.lay.put(wire, s, "codes", codes.astype(self.lay.code_np()))
        mm = np.array([rc.fold_minmax(u) for _, u in enc], np.uint32)
        out = dict(wire=wire, u_flat=self.lay.flat_of([u for _, u in enc]), minmax=mm, gbuf=self.lay.floats_of(self.v), ebuf=self.ebuf,
                   codes=[c_ for c_, _ in enc], u=[u for _, u in enc])
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return out


@functools.lru_cache(maxsize=None)
def zero_of(c):
    return Zero(c)


def chain_want(z, n_bit, padded=False):
    """Behind an encode: gq_hsq_levels_batched (rounding off, write_error) and the PLAIN decode of the one payload (R = 1: the
    decompress as it is, a -0 stays -0) -> dict wire, ebuf, out.  ec.chain_want for every level form: form 0 (n_bit 32) carries
    u itself and leaves the (lb, ub) bytes unwritten."""
    enc, lay = z.want(padded), z.lay
    wire, errs, outs = enc["wire"].copy(), [], []
    for s in range(lay.nseg):
        lb, ub = ec.order_unmap(enc["minmax"][s, 0]), ec.order_unmap(enc["minmax"][s, 1])
        if lay.level == 0:
            levels = enc["u"][s]
        else:
            levels = hc.quantise(enc["u"][s], lb, ub, n_bit, None)
            lay.put(wire, s, "lbub", np.array([lb, ub], np.float32))
        lay.put(wire, s, "levels", lay.level_section(levels))
        dec = rc.stage_decode(enc["codes"][s], lay.norms(levels, n_bit, lb, ub), z.cb)
        with np.errstate(all="ignore"):
            errs.append(None if z.errs[s] is None else z.v[s] - dec)
        outs.append(hc.mean(dec, 1, True))
    buf = z.ebuf.copy()
    for s, x in enumerate(errs):
        if x is not None:
            buf[lay.span(s)] = rc.f32(x).reshape(-1)
    return dict(wire=wire, ebuf=buf, out=lay.floats_of(outs))


# ---- the shapes of tests/test_gpu_zz_hsq_zero_contract.py ------------------------------------------------------------------------
PF_PADDED = ((12, 256, False), (12, 32, False), (24, 256, True), (24, 64, True))
PF_CONTROLS = ((8, 256, False), (16, 256, False), (32, 256, False))
EXACT_SHAPES = ((5, 5, False), (3, 32, False), (10, 33, False), (33, 300, False), (100, 512, False), (12, 101, False), (16, 250, False))
PAGED_CONTROL = ((16, 512, False),)                          # csrc/hsq_encode_pfd.hip has no padding (d = 8, 16, 32 only): a pin
GENERIC_AUTO = ((130, 8, False),)                            # d > 128: lds_plan declines, the dispatcher takes the generic kernel
GENERIC_FORCED = ((12, 101, False), (5, 5, False))           # impl 2; d = 5: the last MFMA k-step holds one real and one padded element
D16_FORCED = ((16, 256, False),)                             # impl 1
VALU_FORCED = ((12, 256, False), (16, 256, False), (24, 256, True))      # impl 3
# (shape, impl): 0 = ENCODE_AUTO, 1 = ENCODE_MFMA_D16K256, 2 = ENCODE_MFMA_GENERIC, 3 = ENCODE_VALU, 5 = ENCODE_MFMA_LDS
FLAT = ([(s, 0) for s in PF_PADDED + EXACT_SHAPES + PF_CONTROLS + PAGED_CONTROL + GENERIC_AUTO] + [(s, 5) for s in PF_PADDED]
        + [(s, 2) for s in GENERIC_FORCED] + [(s, 1) for s in D16_FORCED] + [(s, 3) for s in VALU_FORCED])
BATCHED = ([ZCase(d, K, sh, ef, 1) for d, K, sh in ((12, 256, False), (24, 256, True)) for ef in (None, 0, 1)]
           + [ZCase(d, K, False, ef, 1) for d, K, e in ((12, 101, 0), (5, 5, 1), (33, 300, 0)) for ef in (None, e)])
CHAINS = [(ZCase(d, K, sh, ef, lv), nb) for d, K, sh in ((12, 256, False), (24, 256, True), (12, 101, False))
          for ef, lv, nb in ((0, 0, 32), (None, 0, 32), (1, 1, 8))]
STEADY = [ZCase(12, 256, False, 0, 1), ZCase(24, 256, True, None, 1), ZCase(12, 101, False, 1, 1), ZCase(33, 300, False, None, 1)]


@functools.lru_cache(maxsize=None)
def flat_case(d, K, shipped):
    """One tensor for gq_hsq_encode: the tensors of Zero (no error feedback) one behind the other -> (grad, names per row or
    None, codes, u)."""
    z = zero_of(ZCase(d, K, shipped, None, 1))
    names = [None if k < 0 else z.cat[k][0] for ks in z.kinds for k in ks]
    g = np.concatenate(z.v)
    codes, u = ec.encode_ref(g, z.cb)
    return g, names, codes, u


# ---- PVQ: csrc/pvq.hip recomputes the selected projection over the d real elements -----------------------------------------------
PVQ_SHAPE = (12, 100)


@functools.lru_cache(maxsize=None)
def pvq_case():
    """(c_dagger, grad, names, r): the catalog rows of a (12, 100) matrix whose last and middle columns are scaled like the test
    codebooks', between Gaussian rows."""
    d, K = PVQ_SHAPE
    rs = np.random.RandomState(12100)
    cd = rc.f32(rs.standard_normal((K, d)) / np.sqrt(d))
    cd[:, [(d - 1) // 2, d - 1]] *= COLUMN_SCALE
    s0 = np.where(np.signbit(cd[0]), F(-1.0), F(1.0)).astype(np.float32)
    M = 200
    g = rc.f32(rs.standard_normal((M, d)) * 1e-2)
    names = [None] * M
    for r in range(0, M, 3):
        j = (d - 1, (d - 1) // 2)[(r // 3) % 2]
        sign = (-1, +1)[(r // 6) % 2]
        g[r] = -s0 * F(0.0)
        g[r, j] = F(sign) * s0[j] * TINY
        names[r] = ("neg" if sign < 0 else "pos") + "@%d" % j
    return cd, g, names, rc.f32(rs.rand(M))


# ---- the quantizer: NearestNeighborCompressor c_dim 24 / k_bit 8 / n_bit 32 through PSQuantizer -----------------------------------
Q_SHAPES = ((130 * 24,), (67, 24), (70, 24), (43, 24))      # tensor 2: only neg_mid rows (all above 1000 elements: compressed)


def quantizer_grads(cb):
    """Per tensor of Q_SHAPES (grad f32 of that shape, names per subvector or None): Gaussian rows with the neg_mid / pos_mid rows
    of the compressor's own codebook `cb` (f32[256, 24]) at every third subvector; tensor 2 holds neg_mid rows only."""
    cat = [(n, r) for n, r in catalog_of(cb) if "mid" in n]
    negs = [(n, r) for n, r in cat if is_neg(n)]
    assert negs and len(cat) > len(negs)
    out = []
    for t, shape in enumerate(Q_SHAPES):
        M = int(np.prod(shape)) // 24
        g = rc.f32(np.random.RandomState(2400 + t).standard_normal((M, 24)) * 1e-2)
        names = [None] * M
        for r in range(M):
            if t == 2:
                names[r], g[r] = negs[r % len(negs)]
            elif r % 3 == 1:
                names[r], g[r] = cat[(r // 3 + t) % len(cat)]
        out.append((g.reshape(shape), names))
    return out


def quantizer_args(cuda):
    from argparse import Namespace
    return Namespace(c_dim=24, k_bit=8, n_bit=32, no_cuda=not cuda, random=0, ef=False, two_phase=False, scale="exp", num_users=1,
                     mode="ps", cr=256)


def quantizer_run(cuda, steps=3):
    """`steps` steps of one user through PSQuantizer: on the HIP kernels (cuda) or, on the CPU, with tests/oracle_codec.py's codecs
    (the product's wire layout, the compute by the CPU oracle).  -> dict: names (per tensor), cb, and per step wire (uint8, the
    user's payload), codes / norms (per tensor, as the wire holds them) and grads (the aggregate per parameter)."""
    import torch
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import PSQuantizer
    os.environ["GQ_CODEBOOK_DIR"] = os.path.join(rc.GOLDEN, "codebooks")
    args = quantizer_args(cuda)
    probe = NearestNeighborCompressor(int(np.prod(Q_SHAPES[0])), Q_SHAPES[0], quantizer_args(False))
    assert probe.dim == 24 and probe.K == 256
    cb = rc.f32(probe.codewords.cpu().numpy())
    data = quantizer_grads(cb)
    dev = "cuda:0" if cuda else "cpu"
    params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in Q_SHAPES]
    kw = {}
    if not cuda:
        from oracle_codec import oracle_codec_factory
        kw["codec_factory"] = oracle_codec_factory
    q = PSQuantizer(NearestNeighborCompressor, params, args, **kw)
    out = dict(names=[n for _, n in data], cb=cb, wire=[], codes=[], norms=[], grads=[])
    for _ in range(steps):
        for p, (g, _) in zip(params, data):
            p.grad = torch.from_numpy(g.copy()).to(dev)
        q.record(0, epoch=1)
        if cuda:
            torch.cuda.synchronize()
        wire = q._wire[0].detach().cpu()
        views = [c._views(wire, q.offsets[i]) for i, c in enumerate(q.codecs)]
        out["wire"].append(wire.numpy().copy())
        out["codes"].append([v[0].numpy().astype(np.int32) for v in views])
        out["norms"].append([rc.f32(v[1].numpy()) for v in views])
        q.apply()
        if cuda:
            torch.cuda.synchronize()
        out["grads"].append([p.grad.detach().cpu().numpy().copy() for p in params])
    return out
