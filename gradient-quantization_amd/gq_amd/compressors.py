"""Compressor classes with the reference's names, constructor and method contract
(SURVEY.md 8b), backed by the HIP kernels in libgq_hsq.so.

    Compressor(size, shape, args).compress(vec) -> signature
    Compressor(...).decompress(signature)       -> tensor of `shape`

Signatures have the reference's structure and dtypes, so code that inspects them keeps
working:  HSQ  [ (lb, ub, levels int32[M]) | u f32[M] , codes uint8|int32 [M] ]
          QSGD [ norm f32[Mb,1], signs bool(shape), levels int32(shape) ].

No CPU path: `compress` / `decompress` raise if the tensor is not in MI355X HBM or the
HIP library is missing.  Construction (sub-dimension choice, codebook load) is host-side
NumPy exactly as in the reference and works anywhere.

Stochastic rounding (`args.random`, default True in the reference's CLI) needs uniform
draws.  The reference draws them with the CPU generator and copies them to the GPU every
call (probabilistic_scalar_compressor.py:23-25).  `args.gq_rng` (or $GQ_RNG) selects:
    "device"     (default) counter-based generator inside the kernel: same distribution,
                 no host round trip, different draws than the reference;
    "reference"  torch.rand on the CPU generator + H2D copy: bit-identical to the
                 reference for the same torch seed;
    "keyed"      as "device", but in the multi-tensor level kernels the stream of a tensor is keyed by the bits of
                 its (lb, ub) instead of a per-call seed: nothing in the launch changes from step to step, which is
                 what lets a quantizer step replay from a HIP graph (gq_graph, quantizers.py).
"""
import math
import os

import numpy as np
import torch

from . import native
from .codebook import load_codebook, repaired_dim

_seed_counter = [0]


def _rng_mode(args):
    mode = getattr(args, "gq_rng", None) or os.environ.get("GQ_RNG", "device")
    if mode not in ("device", "reference", "keyed"):
        raise ValueError("gq_rng must be 'device', 'reference' or 'keyed', got %r" % (mode,))
    return mode


_seed_source = [None]      # a callable that replaces the process-local stream below while it is set (shared_seeds)


def _next_seed():
    """A fresh 63-bit seed per call for the in-kernel generator, derived from torch's CPU
    seed so that torch.manual_seed() makes runs reproducible."""
    if _seed_source[0] is not None:
        return _seed_source[0]()
    _seed_counter[0] += 1
    return (torch.initial_seed() * 0x9E3779B97F4A7C15 + _seed_counter[0] * 0xD1B54A32D192ED03) & (2 ** 63 - 1)


class shared_seeds(object):
    """with shared_seeds(source): every _next_seed() inside comes from `source()` instead of this process's torch seed and call
    count.  The parameter-server quantizer wraps the replicated second phase (ps_quantizer.py:52-61) in it with a source all ranks
    share, so that whatever path the re-compress takes (multi-tensor launches without device step words, per-tensor codecs, any
    compressor object) the ranks round identically -- whatever their own torch seeds are."""

    def __init__(self, source):
        self.source = source

    def __enter__(self):
        self.prev, _seed_source[0] = _seed_source[0], self.source

    def __exit__(self, *exc):
        _seed_source[0] = self.prev


def _require_device(t, what):
    if t.device.type != "cuda":
        raise native.GQNativeError(
            "%s: tensor is on %s; gq_amd runs on MI355X only (no CPU fallback). "
            "Run without --no-cuda on a GPU box." % (what, t.device))


class IdenticalCompressor(object):
    """Pass-through for small tensors and `--quantizer sgd` (identical_compressor.py:1-11)."""

    def __init__(self, size=None, shape=None, args=None):
        pass

    @staticmethod
    def compress(vec):
        return vec.clone()

    @staticmethod
    def decompress(signature):
        return signature


class ProbabilisticScalarCompressor(object):
    """Uniform 2^n_bit-level quantiser of a vector between its global min and max
    (probabilistic_scalar_compressor.py:4-33)."""

    def __init__(self, n_bit, args):
        self.n_bit = n_bit
        self.s = 2 ** n_bit
        self.cuda = not args.no_cuda
        self.code_dtype = torch.int32
        self.random = args.random
        self._rng = _rng_mode(args)

    # -- shared with NearestNeighborCompressor ---------------------------------------
    def _levels_from_partials(self, u, partials, levels, lb_ub):
        M = u.numel()
        if not self.random:
            native.hsq_levels(u, self.n_bit, native.RANDOM_OFF, None, 0, partials, lb_ub, levels)
        elif self._rng == "reference":
            r = torch.rand(M)  # CPU generator, as prob_scalar:23
            native.hsq_levels(u, self.n_bit, native.RANDOM_GIVEN, r.to(u.device), 0, partials, lb_ub, levels)
        else:
            native.hsq_levels(u, self.n_bit, native.RANDOM_DEVICE, None, _next_seed(), partials, lb_ub, levels)

    def compress(self, vec):
        _require_device(vec, "ProbabilisticScalarCompressor.compress")
        flat = vec.contiguous().view(-1)
        partials = native.new_workspace(flat.device, 0)
        native.minmax_partials(flat, partials)
        lb_ub = torch.empty(2, dtype=torch.float32, device=flat.device)
        levels = torch.empty(flat.numel(), dtype=self.code_dtype, device=flat.device)
        self._levels_from_partials(flat, partials, levels, lb_ub)
        return lb_ub[0], lb_ub[1], levels.view(vec.shape)

    def decompress(self, signature):
        """probabilistic_scalar_compressor.py:29-33 on the library's decode: float(l) * (ub - lb) / 2^n + lb, each step rounded on
        its own, is what gq_hsq_decode_sum computes for the norm of a subvector -- here times a one-by-one codebook holding 1.0
        (exact).  (Until round 6: three torch elementwise launches.)"""
        lower_bound, upper_bound, l = signature
        _require_device(l, "ProbabilisticScalarCompressor.decompress")
        dev = l.device
        flat = l.contiguous().view(-1)
        if flat.dtype not in (torch.uint8, torch.int16, torch.int32):
            flat = flat.to(torch.int32)
        M = flat.numel()
        unit = getattr(self, "_unit", None)
        if unit is None or unit[0].device != dev or unit[1].numel() < M:
            unit = self._unit = (torch.ones((1, 1), dtype=torch.float32, device=dev), torch.zeros(M, dtype=torch.uint8, device=dev))
        lb_ub = torch.stack([torch.as_tensor(lower_bound, dtype=torch.float32, device=dev).reshape(()),
                             torch.as_tensor(upper_bound, dtype=torch.float32, device=dev).reshape(())])
        out = torch.empty(M, dtype=torch.float32, device=dev)
        native.hsq_decode_sum(unit[1][:M], flat, lb_ub, unit[0], self.n_bit, out, R=1)
        return out.view(l.shape)


class NearestNeighborCompressor(object):
    """HSQ: per d-float subvector, the codeword with the largest |<c, v>| and the signed
    projection, then the scalar quantiser (nearest_neighbor_compressor.py:9-90)."""

    def __init__(self, size, shape, args):
        c_dim = args.c_dim
        k_bit = args.k_bit
        n_bit = args.n_bit
        assert c_dim > 0
        assert k_bit >= 0
        assert n_bit > 0

        self.cuda = not args.no_cuda
        self.size = size
        self.shape = shape
        self.dim = repaired_dim(size, c_dim)
        if c_dim != self.dim:
            print("alternate dimension form {} to {}, size {} shape {}".format(c_dim, self.dim, size, shape))
        assert size % self.dim == 0, \
            "not divisible size {}  c_dim {} self.dim {}".format(size, c_dim, self.dim)

        self.K = self.dim if k_bit <= 0 else 2 ** k_bit
        if self.K == self.dim:
            # random orthogonal codebook from NumPy's global generator, as :46
            from scipy import stats
            codewords = stats.ortho_group.rvs(self.dim).astype(np.float32)
        else:
            codewords = load_codebook(self.dim, self.K)
        self.codewords = torch.from_numpy(np.ascontiguousarray(codewords))
        self.code_dtype = torch.uint8 if k_bit <= 8 else torch.int32
        self.n_bit = n_bit
        self.compressed_norm = n_bit != 32
        if self.compressed_norm:
            self.norm_compressor = ProbabilisticScalarCompressor(n_bit, args)
        self.M = size // self.dim
        if self.cuda and torch.cuda.is_available():
            self.codewords = self.codewords.cuda()

    def _codebook_on(self, device):
        if self.codewords.device != device:
            self.codewords = self.codewords.to(device)
        return self.codewords

    # ---- reference protocol -----------------------------------------------------------
    def compress(self, vec):
        _require_device(vec, "NearestNeighborCompressor.compress")
        dev = vec.device
        flat = vec.contiguous().view(-1)
        assert flat.numel() == self.size
        cb = self._codebook_on(dev)
        M = self.M
        codes = torch.empty(M, dtype=self.code_dtype, device=dev)
        u = torch.empty(M, dtype=torch.float32, device=dev)
        partials = native.new_workspace(dev, M)
        native.hsq_encode(flat, cb, codes, u, partials)
        if not self.compressed_norm:
            return [u, codes]
        lb_ub = torch.empty(2, dtype=torch.float32, device=dev)
        levels = torch.empty(M, dtype=torch.int32, device=dev)
        self.norm_compressor._levels_from_partials(u, partials, levels, lb_ub)
        return [(lb_ub[0], lb_ub[1], levels), codes]

    def decompress(self, signature):
        norms, codes = signature
        _require_device(codes, "NearestNeighborCompressor.decompress")
        dev = codes.device
        cb = self._codebook_on(dev)
        codes = codes.contiguous().view(-1)
        if codes.dtype not in (torch.uint8, torch.int32):
            codes = codes.to(torch.int32)
        out = torch.empty(self.size, dtype=torch.float32, device=dev)
        if self.compressed_norm:
            lb, ub, levels = norms
            lb_ub = torch.stack([lb.reshape(()), ub.reshape(())]).to(device=dev, dtype=torch.float32)
            levels = levels.contiguous().view(-1)
            if levels.dtype not in (torch.uint8, torch.int16, torch.int32):
                levels = levels.to(torch.int32)
            native.hsq_decode_sum(codes, levels, lb_ub, cb, self.n_bit, out, R=1)
        else:
            native.hsq_decode_sum(codes, norms.contiguous().view(-1).float(), None, cb, 32, out, R=1)
        return out.view(self.shape)

    # ---- fused paths used by the quantizers (same results, fewer bytes / launches) ------
    def wire_level_dtype(self):
        """Narrowest level type that holds [0, 2^n_bit] (stochastic) / [0, 2^n_bit - 1]."""
        top = 2 ** self.n_bit - (0 if self.norm_compressor.random else 1)
        return torch.uint8 if top <= 255 else (torch.int16 if top <= 32767 else torch.int32)

    def compress_into(self, vec, codes, levels, lb_ub, u=None, partials=None):
        """compress() writing into caller-owned (wire) buffers; levels may be uint8."""
        _require_device(vec, "NearestNeighborCompressor.compress_into")
        assert self.compressed_norm
        dev = vec.device
        flat = vec.contiguous().view(-1)
        cb = self._codebook_on(dev)
        if u is None:
            u = torch.empty(self.M, dtype=torch.float32, device=dev)
        if partials is None:
            partials = native.new_workspace(dev, self.M)
        native.hsq_encode(flat, cb, codes, u, partials)
        self.norm_compressor._levels_from_partials(u, partials, levels, lb_ub)

    def roundtrip(self, vec):
        """decompress(compress(vec)) without the int32 signature round trip."""
        _require_device(vec, "NearestNeighborCompressor.roundtrip")
        if not self.compressed_norm:
            return self.decompress(self.compress(vec))
        dev = vec.device
        codes = torch.empty(self.M, dtype=self.code_dtype, device=dev)
        levels = torch.empty(self.M, dtype=self.wire_level_dtype(), device=dev)
        lb_ub = torch.empty(2, dtype=torch.float32, device=dev)
        self.compress_into(vec, codes, levels, lb_ub)
        out = torch.empty(self.size, dtype=torch.float32, device=dev)
        native.hsq_decode_sum(codes, levels, lb_ub, self._codebook_on(dev), self.n_bit, out, R=1)
        return out.view(self.shape)


class QSGDCompressor(object):
    """Bucketed max-norm stochastic quantiser (qsgd_compressor.py:4-71)."""

    def __init__(self, size, shape, args):
        self.random = args.random
        self.bit = args.n_bit
        c_dim = args.c_dim
        assert self.bit > 0
        self.cuda = not args.no_cuda
        self.s = 2 ** self.bit
        self.size = size
        self.shape = shape
        self.dim = repaired_dim(size, c_dim)
        if c_dim != self.dim:
            print("alternate dimension form {} to {}, size {} shape {}".format(c_dim, self.dim, size, shape))
        assert self.dim != 0, "0 sub dimension size {}  c_dim {} self.dim {}".format(size, c_dim, self.dim)
        assert size % self.dim == 0, "not divisible size {}  c_dim {} self.dim {}".format(size, c_dim, self.dim)
        self.M = size // self.dim
        self.code_dtype = torch.int32
        self._rng = _rng_mode(args)

    def compress(self, vec):
        _require_device(vec, "QSGDCompressor.compress")
        dev = vec.device
        flat = vec.contiguous().view(-1)
        norm = torch.empty(self.M, dtype=torch.float32, device=dev)
        signs = torch.empty(self.size, dtype=torch.bool, device=dev)
        levels = torch.empty(self.size, dtype=self.code_dtype, device=dev)
        if not self.random:
            native.qsgd_compress(flat, self.dim, self.bit, native.RANDOM_OFF, None, 0, norm, signs, levels)
        elif self._rng == "reference":
            r = torch.rand(self.M, self.dim)  # CPU generator, as qsgd_compressor.py:58
            native.qsgd_compress(flat, self.dim, self.bit, native.RANDOM_GIVEN, r.to(dev).view(-1), 0, norm, signs,
                                 levels)
        else:
            native.qsgd_compress(flat, self.dim, self.bit, native.RANDOM_DEVICE, None, _next_seed(), norm, signs,
                                 levels)
        return [norm.view(self.M, 1), signs.view(self.shape), levels.view(self.shape)]

    def decompress(self, signature):
        norm, signs, l = signature
        assert l.shape == signs.shape
        _require_device(l, "QSGDCompressor.decompress")
        out = torch.empty(self.size, dtype=torch.float32, device=l.device)
        lv = l.contiguous().view(-1)
        if lv.dtype not in (torch.uint8, torch.int32):
            lv = lv.to(torch.int32)
        native.qsgd_decode_sum(norm.contiguous().view(-1), signs.contiguous().view(-1), lv, self.dim, self.bit, out,
                               R=1)
        return out.view(self.shape)

    def roundtrip(self, vec):
        return self.decompress(self.compress(vec))


class ProbabilisticVectorCompressor(object):
    """Unbiased vector quantiser (probabilistic_vector_compressor.py:8-77): sample the codeword with probability
    |p_k| / ||p||_1, p = pinv(C^T) v, magnitude sign(p_k) * ||p||_1, so that E[decode] = v.
    Pinned by the reference's own output (tests/golden/pvq_*.npz, residual_*.npz): the class as it
    stands opens ./codebook/... (the tree has ./codebooks/learned_codebook/..., which is what is used here) and calls
    torch.argmin on a bool tensor (:58), which no torch with bool tensors implements; the fixtures were produced with
    that one operation defined as (index of the first True) - 1 -- the inverse-CDF sample the line's `+ 1` is written
    for -- and every other line running unedited.  gq_pvq_encode reproduces them bit for bit, including torch.cumsum's
    double accumulation of the cumulative probabilities."""

    def __init__(self, size, shape, args):
        c_dim, k_bit, n_bit = args.c_dim, args.k_bit, args.n_bit
        assert c_dim > 0
        assert k_bit > 0
        assert n_bit > 0
        self.cuda = not args.no_cuda
        self.size, self.shape = size, shape
        self.dim = c_dim if c_dim < size else size
        assert size % self.dim == 0, "not divisible size {} dim {}".format(size, self.dim)
        self.K = 2 ** k_bit
        if self.K == self.dim:
            from scipy import stats
            codewords = stats.ortho_group.rvs(self.dim).astype(np.float32)
        else:
            codewords = load_codebook(self.dim, self.K)
        self.codewords = torch.from_numpy(np.ascontiguousarray(codewords))
        self.c_dagger = torch.from_numpy(np.ascontiguousarray(np.linalg.pinv(codewords.T).astype(np.float32)))
        self.code_dtype = torch.uint8 if k_bit <= 8 else torch.int32
        self.n_bit = n_bit
        self.compressed_norm = n_bit != 32
        if self.compressed_norm:
            self.norm_compressor = ProbabilisticScalarCompressor(n_bit, args)
        self.M = size // self.dim
        self._rng = _rng_mode(args)

    def _on(self, device):
        if self.codewords.device != device:
            self.codewords = self.codewords.to(device)
            self.c_dagger = self.c_dagger.to(device)
        return self.codewords, self.c_dagger

    def _codebook_on(self, device):
        """The DECODE codebook, as NearestNeighborCompressor names it (the wire codecs decode both classes the same way)."""
        return self._on(device)[0]

    wire_level_dtype = NearestNeighborCompressor.wire_level_dtype

    def compress(self, vec, minus=None):
        """minus = (codes1, norm1, codebook1): compress  vec - codebook1[codes1] * norm1  -- the residual of a first
        stage (ResidualCompressor) -- computed inside the kernel's tile staging instead of as a tensor."""
        _require_device(vec, "ProbabilisticVectorCompressor.compress")
        dev = vec.device
        flat = vec.contiguous().view(-1)
        _, cdag = self._on(dev)
        codes = torch.empty(self.M, dtype=self.code_dtype, device=dev)
        u = torch.empty(self.M, dtype=torch.float32, device=dev)
        ws = native.new_workspace(dev, 0)
        r, mode, seed = None, native.RANDOM_DEVICE, 0
        if self._rng == "reference":
            r, mode = torch.rand(self.M).to(dev), native.RANDOM_GIVEN       # CPU generator, as :52
        else:
            seed = _next_seed()
        if minus is None:
            native.pvq_encode(flat, cdag, codes, u, ws, mode, r, seed)
        else:
            codes1, norm1, cb1 = minus
            native.pvq_encode_residual(flat, codes1.contiguous().view(-1), norm1.contiguous().view(-1).float(), cb1, cdag,
                                       codes, u, ws, mode, r, seed)
        if not self.compressed_norm:
            return [u, codes]
        lb_ub = torch.empty(2, dtype=torch.float32, device=dev)
        levels = torch.empty(self.M, dtype=torch.int32, device=dev)
        self.norm_compressor._levels_from_partials(u, ws, levels, lb_ub)
        return [(lb_ub[0], lb_ub[1], levels), codes]

    def decompress(self, signature):
        norms, codes = signature
        _require_device(codes, "ProbabilisticVectorCompressor.decompress")
        dev = codes.device
        cb, _ = self._on(dev)
        codes = codes.contiguous().view(-1)
        if codes.dtype not in (torch.uint8, torch.int32):
            codes = codes.to(torch.int32)
        out = torch.empty(self.size, dtype=torch.float32, device=dev)
        if self.compressed_norm:
            lb, ub, levels = norms
            lb_ub = torch.stack([lb.reshape(()), ub.reshape(())]).to(device=dev, dtype=torch.float32)
            native.hsq_decode_sum(codes, levels.contiguous().view(-1), lb_ub, cb, self.n_bit, out, R=1)
        else:
            native.hsq_decode_sum(codes, norms.contiguous().view(-1).float(), None, cb, 32, out, R=1)
        return out.view(self.shape)


class ResidualCompressor(object):
    """Two stages (residual_compressor.py:7-32): NearestNeighbor on the gradient, the probabilistic vector
    compressor on what stage 1 leaves; decode = sum of the stage decodes.  The residual is never a tensor here:
    stage 2's kernel stages its tiles as  v - codebook1[code1] * norm1  (gq_pvq_encode_residual), so compress is
    stage 1's two launches + stage 2's, with two reads of the gradient instead of a clone, a decode, an in-place
    subtraction and a second encode over a materialised residual.  Pinned against the reference's own output
    (tests/golden/residual_*.npz)."""

    FUSED_MAX_DIM = 104      # the LDS-staged second-stage kernel; wider subvectors take the tensor path

    def __init__(self, size, shape, args):
        self.compressors = [
            NearestNeighborCompressor(size, shape, args),
            ProbabilisticVectorCompressor(size, shape, args),
        ]

    def compress(self, vec):
        first, second = self.compressors
        sig1 = first.compress(vec)
        if first.dim > self.FUSED_MAX_DIM or first.dim != second.dim:
            residuals = vec.clone()
            residuals -= first.decompress(sig1)
            return [sig1, second.compress(residuals)]
        norms, codes1 = sig1
        norm1 = first.norm_compressor.decompress(norms) if first.compressed_norm else norms     # probabilistic_scalar_compressor.py:31-32
        return [sig1, second.compress(vec, minus=(codes1, norm1, first._codebook_on(vec.device)))]

    def decompress(self, signatures):
        decoded = [c.decompress(sig) for sig, c in zip(signatures, self.compressors)]
        # the reference's reduction, not `a + b`: sum() starts from +0, so two -0 entries give +0 (:26-32)
        return torch.stack(decoded, dim=0).sum(dim=0)


# ---- exported for `from compressors import *` in the reference's main.py ----------------
# SignSGD, TopK and Maurey run on HIP kernels for device float32 tensors (libgq_sign.so, libgq_topk.so, libgq_maurey.so; the
# quantizers ship them on a 2-bit and two sparse wires, gq_amd.codecs.SignCodec / TopKCodec / MaureyCodec) and keep torch
# expressions for CPU tensors.

class SignSGDCompressor(object):
    """sign(v) (signsgd_compressor.py:4-12)."""

    def __init__(self, size, shape, args):
        pass

    def compress(self, vec):
        if vec.device.type == "cuda" and vec.dtype == torch.float32:
            # the sign kernels (libgq_sign.so, gq_amd.codecs.SignCodec): torch.sign's tensor bit for bit
            return self._device_roundtrip(vec)
        return torch.sign(vec)

    def decompress(self, signature):
        return signature

    def _device_roundtrip(self, vec):
        from .codecs import SignCodec      # (codecs imports this module)
        n = vec.numel()
        if n == 0:
            return torch.sign(vec)
        codecs = self.__dict__.setdefault("_codecs", {})
        codec = codecs.get(n)
        if codec is None:
            codec = codecs[n] = SignCodec(self, n, (n,))
        return codec.roundtrip(vec.reshape(-1), 0).view(vec.shape)


class TopKSparsificationCompressor(object):
    """Keep the size//cr largest-magnitude entries (topk_sparsification_compressor.py:9-26)."""

    def __init__(self, size, shape, args):
        self.cuda = not args.no_cuda
        self.size = size
        self.shape = shape
        self.users = 1
        self.k = size // args.cr

    def compress(self, vec):
        if vec.device.type == "cuda":
            # the top-k kernels (libgq_topk.so, gq_amd.codecs.TopKCodec): the same dense tensor bit for bit
            return self._device_roundtrip(vec).view(self.users, -1)
        vec = vec.view(self.users, -1)
        keep = torch.zeros_like(vec)
        idx = torch.topk(torch.abs(vec), k=self.k, dim=1)[1]
        keep.scatter_(1, idx, 1)
        return vec * keep

    def decompress(self, signature):
        return signature.view(self.shape)

    def _device_roundtrip(self, vec):
        from .codecs import TopKCodec      # (codecs imports this module)
        if vec.dtype != torch.float32:
            raise TypeError("TopKSparsificationCompressor: the device kernels take float32 tensors, got %s" % (vec.dtype,))
        n = vec.numel()
        if self.k > n:
            raise RuntimeError("TopKSparsificationCompressor: k = %d is larger than the tensor (%d elements)" % (self.k, n))
        codecs = self.__dict__.setdefault("_codecs", {})
        codec = codecs.get(n)
        if codec is None:
            codec = codecs[n] = TopKCodec(self, n, (n,))
        return codec.roundtrip(vec.reshape(-1), 0)


class MaureySparsification(object):
    """Maurey sampling (maurey_sparsification.py:4-50): k coordinates drawn with probability |v_i| / ||v||_1, each
    carrying sign(v_i) * ||v||_1 / k; same constructor arithmetic for cr and k, the same signature [scale, codes, signs] and
    the same decompress.  The reference compares cumsum(p) with a k x size matrix of independent uniforms on the CPU, which is
    not an inverse-CDF sample and cannot run at size; here the draws are i.i.d. samples of that distribution.  A CUDA float32
    tensor is sampled by the HIP kernels (libgq_maurey.so, gq_amd.codecs.MaureyCodec: an inverse-CDF sample of one uniform per
    draw over the f64 running sum of |v|; codes ascending; a tensor whose l1 norm is zero or not finite gives k times index 0
    with a plus sign -- include/gq_maurey.h), every other tensor by torch.multinomial on the tensor's device."""

    def __init__(self, size, shape, args):
        self.cr = 32 * args.c_dim // (args.k_bit + args.n_bit)
        bit_for_idx = 32 if size > 65536 else 16
        self.k = max(1, 32 * size // ((bit_for_idx + 1) * self.cr))
        self.cuda = not args.no_cuda
        self.size, self.shape = size, shape
        self._rng = _rng_mode(args)      # where the kernels' uniforms come from (MaureyCodec)

    def compress(self, vec):
        if vec.device.type == "cuda" and vec.dtype == torch.float32 and vec.numel() > 0:
            return self._device_compress(vec)
        flat = vec.reshape(-1)
        mag = flat.abs()
        l1_norm = mag.sum()
        codes = torch.multinomial(mag / l1_norm, self.k, replacement=True)
        return [l1_norm / self.k, codes, torch.sign(flat[codes])]

    def _device_compress(self, vec):
        """The signature read back from the sparse wire of the kernels: scale (0-dim f32), codes int64[k] ascending, signs f32[k]."""
        from .codecs import MaureyCodec      # (codecs imports this module)
        n = vec.numel()
        codecs = self.__dict__.setdefault("_codecs", {})
        codec = codecs.get(n)
        if codec is None:
            codec = codecs[n] = MaureyCodec(self, n, (n,))
        wire = torch.empty(codec.nbytes, dtype=torch.uint8, device=vec.device)
        codec.encode_into(vec.reshape(-1), wire, 0, 0)
        words = wire[native.MAUREY_HEADER_BYTES:native.MAUREY_HEADER_BYTES + 4 * codec.k].view(torch.int32)
        signs = torch.where(words < 0, -1.0, 1.0).to(torch.float32)
        return [wire[:4].view(torch.float32)[0].clone(), (words & 0x7fffffff).to(torch.int64), signs]

    def decompress(self, signature):
        scale, codes, signs = signature
        out = torch.zeros(self.size, dtype=signs.dtype, device=signs.device)
        out.index_add_(0, codes.reshape(-1).long(), signs.reshape(-1))
        return (scale * out).view(self.shape)


class MXCompressor(object):
    """Block-scaled small floats (OCP Microscaling; no counterpart in the reference's catalogue): 32 consecutive elements share a
    power-of-two scale byte, every element is an FP4 (E2M1), FP6 (E2M3 or E3M2) or FP8 (E4M3) value -- 4.25, 6.25 or 8.25 bits
    per element, unbiased under stochastic rounding, relative precision inside a block (include/gq_mx.h defines it to the bit).
    args.mx_format: 'fp4' (the default), 'fp6_e2m3', 'fp6_e3m2' or 'fp8' ('fp6' alone names no format); args.random: stochastic rounding (otherwise to nearest, ties to the even code); gq_rng: where
    the draws come from (MXCodec).  compress returns the decoded tensor -- the wire carries it exactly -- and decompress is the
    identity, as for SignSGDCompressor.  HIP kernels only (libgq_mx.so): a float32 or bfloat16 tensor on the device (a bfloat16
    tensor is widened exactly, compressed to the same wire, and returned as bfloat16).
    args.mx_rotate: None / 'none' (the default) or 'hadamard' -- a randomized 256-point Hadamard rotation in front of the
    quantiser and its inverse behind the decode (include/gq_mxr.h, libgq_mxr.so): one large entry no longer sets the grid of its
    31 neighbours, at the same bits on the same wire.  args.mx_rotate_seed (default 1) gives the four sign words, outputs
    0 ... 3 of splitmix64 started at the seed, computed here in Python integers: every rank with the same arguments has the same
    signs.  With rotation compress returns the inverse-rotated dense decode."""

    FORMATS = ("fp4", "fp6_e2m3", "fp6_e3m2", "fp8")

    @staticmethod
    def sign_words(seed):
        """Outputs 0 ... 3 of splitmix64 started at `seed` (include/gq_mxr.h writes the recurrence out)."""
        M = (1 << 64) - 1
        state, words = int(seed) & M, []
        for _ in range(4):
            state = (state + 0x9E3779B97F4A7C15) & M
            z = state
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            words.append(z ^ (z >> 31))
        return tuple(words)

    def __init__(self, size, shape, args):
        fmt = getattr(args, "mx_format", None) or "fp4"
        if fmt not in self.FORMATS:
            raise ValueError("mx_format must be one of %s, got %r" % (", ".join(repr(f) for f in self.FORMATS), fmt))
        self.format = fmt
        self.random = bool(getattr(args, "random", True))
        self.size, self.shape = size, shape
        self._rng = _rng_mode(args)
        rotate = getattr(args, "mx_rotate", None)
        if rotate not in (None, "none", "hadamard"):
            raise ValueError("mx_rotate must be 'none' or 'hadamard', got %r" % (rotate,))
        self.rotate = "hadamard" if rotate == "hadamard" else None
        seed = getattr(args, "mx_rotate_seed", None)
        self.rotate_seed = 1 if seed is None else int(seed)
        self.rotate_signs = self.sign_words(self.rotate_seed) if self.rotate else None

    def compress(self, vec):
        from .codecs import MXCodec, MXRCodec      # (codecs imports this module)
        if vec.device.type != "cuda" or vec.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("MXCompressor: the kernels take float32 or bfloat16 tensors on the HIP device (there is no CPU path), got %s on %s"
                            % (vec.dtype, vec.device))
        n = vec.numel()
        if n == 0:
            return vec.clone()
        codecs = self.__dict__.setdefault("_codecs", {})
        codec = codecs.get((n, vec.dtype))
        if codec is None:      # (a bfloat16 tensor comes back as bfloat16: include/gq_mx.h, TENSOR-SIDE TYPE)
            codec = codecs[(n, vec.dtype)] = (MXRCodec if self.rotate else MXCodec)(self, n, (n,), vec.dtype)
        return codec.roundtrip(vec.reshape(-1), 0).view(vec.shape)

    def decompress(self, signature):
        return signature


def _rotation_mode(args, name):
    """args.drive_rotation / args.eden_rotation: 'fixed' (also when absent) or 'step'."""
    mode = getattr(args, name, None)
    mode = "fixed" if mode is None else mode
    if mode not in ("fixed", "step"):
        raise ValueError("%s must be 'fixed' or 'step', got %r" % (name, mode))
    return mode


def _user_rotation_mode(args, name):
    """args.drive_user_rotation / args.eden_user_rotation: 'shared' (also when absent) or 'own'."""
    mode = getattr(args, name, None)
    mode = "shared" if mode is None else mode
    if mode not in ("shared", "own"):
        raise ValueError("%s must be 'shared' or 'own', got %r" % (name, mode))
    return mode


class DriveCompressor(object):
    """The rotated 1-bit compressor (DRIVE, Vargaftik et al. 2021; no counterpart in the reference's catalogue): a block of 256
    elements is rotated by a randomized Hadamard matrix, the sign of every rotated coordinate is kept and one f32 scale per block --
    1.125 bits per element, no draws (include/gq_drive.h defines it to the bit).
    args.drive_scale: 'unbiased' (the default) -- S = |x|^2 / |Rx|_1: the decode is unbiased over the rotation's randomness and
    exact in the direction of x, so the mean over users averages out -- or 'mse' -- S = |Rx|_1 / 256: the least single-shot error,
    what error feedback wants.  args.drive_seed (default 1) gives the four sign words (MXCompressor.sign_words: every rank with
    the same arguments has the same signs; one decode-mean needs every payload under the same signs).
    args.drive_rotation: 'fixed' (the default, also when absent) -- the sign words of the seed at every step: over a run the
    compressor is a deterministic function of the gradient -- or 'step' -- the words of step t are outputs 4t ... 4t + 3 of the
    seed's splitmix64 stream (rotation_words; include/gq_drive.h: SIGNS, STEPPED), a fresh rotation every round, which is what
    makes the 'unbiased' decodes average out over ROUNDS.  The step is a device { seed, step } pair that a quantizer owns and moves
    once per apply(); a bare DriveCompressor(...).compress() outside a quantizer has no pair and stays at step 0, which is the fixed
    rotation of the seed.
    args.drive_user_rotation: 'shared' (the default, also when absent) -- every user of one mean rotates by the same words, the
    payloads are added in the rotated domain and rotated back ONCE -- or 'own' -- every user rotates by a stream of sign words of
    their own (include/gq_drive.h: SIGNS, PER STREAM; stream_seed), every payload is rotated back by ITS words and the mean is taken
    in the gradient's domain, one launch still: R inverse transforms against one, which is why 'shared' stays the default.  'own' is
    what makes the 'unbiased' decodes average out over USERS (the error of the mean of R users with equal gradients falls as
    1 / sqrt(R); under 'shared' it is one user's).  The wire does not change.  The stream of a payload is its place in the mean,
    which a quantizer assigns; a bare compress() is stream 0.
    compress returns the dense decode and decompress is the identity, as for MXCompressor.  HIP kernels only (libgq_drive.so): a
    float32 tensor on the device."""

    SCALES = ("unbiased", "mse")
    ROTATIONS = ("fixed", "step")
    USER_ROTATIONS = ("shared", "own")

    @staticmethod
    def stream_seed(seed, stream):
        """The seed of a stream (include/gq_drive.h: SIGNS, PER STREAM): stream 0 keeps the seed, stream s >= 1 is the splitmix64
        finaliser of seed + s * 0xD6E8FEB86659FD93.  The words of (seed, step, stream) are rotation_words(stream_seed(seed, stream),
        step)."""
        M = (1 << 64) - 1
        seed, stream = int(seed) & M, int(stream)
        if stream < 0:
            raise ValueError("a stream is a non-negative integer, got %d" % stream)
        if stream == 0:
            return seed
        z = (seed + stream * 0xD6E8FEB86659FD93) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    @staticmethod
    def rotation_words(seed, step):
        """The four sign words of (seed, step): outputs 4 step ... 4 step + 3 of splitmix64 started at seed, i.e. sign_words of the
        seed moved on by 4 step increments.  Step 0: MXCompressor.sign_words(seed)."""
        M = (1 << 64) - 1
        return MXCompressor.sign_words(((int(seed) & M) + 4 * (int(step) & M) * 0x9E3779B97F4A7C15) & M)

    def __init__(self, size, shape, args):
        scale = getattr(args, "drive_scale", None) or "unbiased"
        if scale not in self.SCALES:
            raise ValueError("drive_scale must be 'unbiased' or 'mse', got %r" % (scale,))
        self.scale = scale
        self.rotation = _rotation_mode(args, "drive_rotation")
        self.user_rotation = _user_rotation_mode(args, "drive_user_rotation")
        seed = getattr(args, "drive_seed", None)
        self.seed = 1 if seed is None else int(seed)
        self.signs = MXCompressor.sign_words(self.seed)
        self.size, self.shape = size, shape

    def compress(self, vec):
        from .codecs import DriveCodec      # (codecs imports this module)
        if vec.device.type != "cuda" or vec.dtype != torch.float32:
            raise TypeError("DriveCompressor: the kernels take float32 tensors on the HIP device (there is no CPU path), got %s on %s"
                            % (vec.dtype, vec.device))
        n = vec.numel()
        if n == 0:
            return vec.clone()
        codecs = self.__dict__.setdefault("_codecs", {})
        codec = codecs.get(n)
        if codec is None:
            codec = codecs[n] = DriveCodec(self, n, (n,))
        return codec.roundtrip(vec.reshape(-1), 0).view(vec.shape)

    def decompress(self, signature):
        return signature


class EdenCompressor(object):
    """The rotated 2-, 3- or 4-bit compressor (EDEN, Vargaftik et al. 2022, DRIVE's sequel; no counterpart in the reference's
    catalogue): a block of 256 elements is rotated by a randomized Hadamard matrix, every rotated coordinate is replaced by the
    nearest of the 2^bits Lloyd-Max centroids of N(0, 1) times the block's spread, and one f32 scale per block is kept --
    bits + 0.125 bits per element, no draws (include/gq_eden.h defines it to the bit).
    args.eden_bits: 2, 3 or 4 (the default; one bit is DriveCompressor).  args.eden_scale: 'unbiased' (the default) -- the decode
    is unbiased over the rotation's randomness and exact in the direction of x -- or 'mse' -- the least-squares scale.
    args.eden_seed (default 1) gives the four sign words (MXCompressor.sign_words: every rank with the same arguments has the same
    signs; one decode-mean needs every payload under the same signs).
    args.eden_rotation: 'fixed' (the default, also when absent) or 'step' -- DriveCompressor's drive_rotation, word for word: a
    fresh rotation every round from a { seed, step } pair the quantizer owns; a bare EdenCompressor(...).compress() stays at step 0.
    args.eden_user_rotation: 'shared' (the default, also when absent) or 'own' -- DriveCompressor's drive_user_rotation, word for
    word: every user of one mean under a stream of sign words of their own (include/gq_eden.h: SIGNS, PER STREAM).
    compress returns the dense decode and decompress is the identity, as for DriveCompressor.  HIP kernels only (libgq_eden.so): a
    float32 tensor on the device."""

    SCALES = ("unbiased", "mse")
    BITS = (2, 3, 4)
    ROTATIONS = DriveCompressor.ROTATIONS
    USER_ROTATIONS = DriveCompressor.USER_ROTATIONS
    rotation_words = staticmethod(DriveCompressor.rotation_words)
    stream_seed = staticmethod(DriveCompressor.stream_seed)

    def __init__(self, size, shape, args):
        bits = getattr(args, "eden_bits", None)
        bits = 4 if bits is None else bits
        if isinstance(bits, bool) or bits not in self.BITS:
            raise ValueError("eden_bits must be 2, 3 or 4 (one bit is --quantizer drive), got %r" % (bits,))
        self.bits = int(bits)
        scale = getattr(args, "eden_scale", None) or "unbiased"
        if scale not in self.SCALES:
            raise ValueError("eden_scale must be 'unbiased' or 'mse', got %r" % (scale,))
        self.scale = scale
        self.rotation = _rotation_mode(args, "eden_rotation")
        self.user_rotation = _user_rotation_mode(args, "eden_user_rotation")
        seed = getattr(args, "eden_seed", None)
        self.seed = 1 if seed is None else int(seed)
        self.signs = MXCompressor.sign_words(self.seed)
        self.size, self.shape = size, shape

    def compress(self, vec):
        from .codecs import EdenCodec      # (codecs imports this module)
        if vec.device.type != "cuda" or vec.dtype != torch.float32:
            raise TypeError("EdenCompressor: the kernels take float32 tensors on the HIP device (there is no CPU path), got %s on %s"
                            % (vec.dtype, vec.device))
        n = vec.numel()
        if n == 0:
            return vec.clone()
        codecs = self.__dict__.setdefault("_codecs", {})
        codec = codecs.get(n)
        if codec is None:
            codec = codecs[n] = EdenCodec(self, n, (n,))
        return codec.roundtrip(vec.reshape(-1), 0).view(vec.shape)

    def decompress(self, signature):
        return signature


class ThresholdSparsificationCompressor(object):
    """Keep what exceeds a threshold (no counterpart in the reference's catalogue): the elements with |w| > eta, at most
    cap = min(n, ceil(k * thr_cap_percent / 100)) of them in index order, k = size // cr.  eta is fitted to the tail of |w| in
    args.thr_stages passes over the tensor (the default 3; a count-adaptive multi-stage exponential fit after SIDCo) or, with
    thr_stages = 0, is args.thr_value -- a hard threshold (include/gq_thr.h defines both to the bit).  args.thr_fit_stride M fits on
    every m-th item of 4,096 elements, m the largest power of two <= M that leaves a tensor at least 16 fit items (else 1).
    compress returns the dense decode and decompress is the identity, as for TopKSparsificationCompressor's device path.  HIP kernels
    only (libgq_thr.so): a float32 tensor on the device."""

    MIN_FIT_ITEMS = 16
    FLT_MAX = 3.4028234663852886e38

    def __init__(self, size, shape, args):
        cr = getattr(args, "cr", None)
        if isinstance(cr, bool) or not isinstance(cr, int) or cr < 1:
            raise ValueError("cr must be a positive integer, got %r" % (cr,))
        stages = getattr(args, "thr_stages", None)
        stages = 3 if stages is None else stages
        if isinstance(stages, bool) or not isinstance(stages, int) or not 0 <= stages <= 8:
            raise ValueError("thr_stages must be 0 (a fixed threshold, thr_value) or 1 ... 8, got %r" % (stages,))
        value = getattr(args, "thr_value", None)
        if stages == 0:
            if value is None:
                raise ValueError("thr_stages = 0 needs thr_value (the fixed threshold)")
            value = float(value)
            if value != value or math.copysign(1.0, value) < 0 or value > self.FLT_MAX:
                raise ValueError("thr_value must lie in [+0, FLT_MAX], got %r" % (value,))
            value = torch.tensor(value, dtype=torch.float32).item()      # (the f32 the launches are handed)
        percent = getattr(args, "thr_cap_percent", None)
        percent = 150 if percent is None else percent
        if isinstance(percent, bool) or not isinstance(percent, int) or percent < 1:
            raise ValueError("thr_cap_percent must be a positive integer, got %r" % (percent,))
        M = getattr(args, "thr_fit_stride", None)
        M = 1 if M is None else M
        if isinstance(M, bool) or not isinstance(M, int) or M < 1:
            raise ValueError("thr_fit_stride must be a positive integer, got %r" % (M,))
        self.size, self.shape = size, shape
        self.cr, self.stages, self.eta, self.percent, self.fit_stride = cr, stages, (value if stages == 0 else 0.0), percent, M
        self.k = size // cr

    @staticmethod
    def capacity(numel, k, percent):
        """cap = min(n, (k * P + 99) // 100) (include/gq_thr.h)."""
        return min(numel, (k * percent + 99) // 100)

    @classmethod
    def stride_for(cls, numel, M):
        """The tensor's fit stride m: the largest power of two <= M that leaves it at least MIN_FIT_ITEMS fit items, else 1."""
        items = -(-numel // 4096)
        m = 1
        while 2 * m <= M and -(-items // (2 * m)) >= cls.MIN_FIT_ITEMS:
            m *= 2
        return m

    def compress(self, vec):
        from .codecs import ThrCodec      # (codecs imports this module)
        if vec.device.type != "cuda" or vec.dtype != torch.float32:
            raise TypeError("ThresholdSparsificationCompressor: the kernels take float32 tensors on the HIP device (there is no CPU "
                            "path), got %s on %s" % (vec.dtype, vec.device))
        n = vec.numel()
        codecs = self.__dict__.setdefault("_codecs", {})
        codec = codecs.get(n)
        if codec is None:
            codec = codecs[n] = ThrCodec(self, n, (n,))
        return codec.roundtrip(vec.reshape(-1), 0).view(vec.shape)

    def decompress(self, signature):
        return signature


class SparseTernaryCompressor(object):
    """Sparse ternary compression (Sattler et al. 2019; no counterpart in the reference's catalogue): top-k's kept set (k = size // cr,
    the largest |w|, ties to the lowest indices), every kept value replaced by sign(w) * mu, mu the mean |w| of the kept set --
    include/gq_stc.h defines the sum's order and every rounding.  compress returns the dense decode and decompress is the identity, as
    for TopKSparsificationCompressor's device path.  HIP kernels only (libgq_stc.so): a float32 tensor on the device."""

    def __init__(self, size, shape, args):
        cr = getattr(args, "cr", None)
        if isinstance(cr, bool) or not isinstance(cr, int) or cr < 1:
            raise ValueError("cr must be a positive integer, got %r" % (cr,))
        self.size, self.shape, self.cr = size, shape, cr
        self.k = size // cr

    def compress(self, vec):
        from .codecs import STCCodec      # (codecs imports this module)
        if vec.device.type != "cuda" or vec.dtype != torch.float32:
            raise TypeError("SparseTernaryCompressor: the kernels take float32 tensors on the HIP device (there is no CPU path), "
                            "got %s on %s" % (vec.dtype, vec.device))
        n = vec.numel()
        codecs = self.__dict__.setdefault("_codecs", {})
        codec = codecs.get(n)
        if codec is None:
            codec = codecs[n] = STCCodec(self, n, (n,))
        return codec.roundtrip(vec.reshape(-1), 0).view(vec.shape)

    def decompress(self, signature):
        return signature


class PowerSGDCompressor(object):
    """Low-rank compression (PowerSGD: Vogels, Karimireddy, Jaggi 2019; no counterpart in the reference's catalogue): the tensor as
    the matrix M of shape[0] rows, one power iteration M Q -> orthogonalise -> M^T Ph from a warm start Q the caller of the kernels
    owns, rank psgd_rank = 1, 2 or 4 -- include/gq_psgd.h defines every operation's order and rounding.  A tensor that is not a matrix,
    has a side below the rank, or whose factors would be no smaller than the tensor itself, travels uncompressed (`compresses`).
    compress returns the dense decode Ph Q'^T and steps this object's own warm start (user 0, parameter 0); decompress is the
    identity.  HIP kernels only (libgq_psgd.so): a float32 tensor on the device."""

    def __init__(self, size, shape, args):
        r = getattr(args, "psgd_rank", 2)
        if isinstance(r, bool) or r not in (1, 2, 4):
            raise ValueError("psgd_rank must be 1, 2 or 4, got %r" % (r,))
        seed = getattr(args, "psgd_seed", 0)
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise ValueError("psgd_seed must be an integer in [0, 2^64), got %r" % (seed,))
        self.size, self.shape, self.rank, self.seed = size, tuple(shape), r, seed

    @staticmethod
    def matrix(size, shape):
        """(n, m) of the matrix a tensor of this shape is, or None for what is not one."""
        if len(shape) < 2 or size < 1 or shape[0] < 1:
            return None
        return int(shape[0]), int(size) // int(shape[0])

    @property
    def compresses(self):
        """Whether a tensor of this size and shape is compressed at all (include/gq_psgd.h; otherwise it travels as it is)."""
        nm = self.matrix(self.size, self.shape)
        if nm is None or self.size <= 1000 or self.size >= 2 ** 31 or min(nm) < self.rank:
            return False
        return (16 + 4 * self.rank * (nm[0] + nm[1]) + 15) // 16 * 16 < 4 * self.size

    def compress(self, vec):
        from .codecs import BatchedPowerSGD, PowerSGDCodec      # (codecs imports this module)
        if vec.device.type != "cuda" or vec.dtype != torch.float32:
            raise TypeError("PowerSGDCompressor: the kernels take float32 tensors on the HIP device (there is no CPU path), "
                            "got %s on %s" % (vec.dtype, vec.device))
        if vec.numel() != self.size or not self.compresses:
            return vec.clone()
        st = self.__dict__.get("_single")
        if st is None or st[0].device != vec.device:
            codec = PowerSGDCodec(self, self.size, self.shape)
            st = self._single = (BatchedPowerSGD([codec], [0], [0], vec.device, 1, codec.nbytes), codec.warm_start(0, 0, vec.device))
        grp, q = st
        views = grp.roundtrip([vec.contiguous().view(-1)], 0, 0, (None, [q], 0))
        if views is None:
            raise TypeError("PowerSGDCompressor: the tensor must be 4-byte aligned float32 memory on the current HIP device")
        return views[0].clone().view(vec.shape)

    def decompress(self, signature):
        return signature


__all__ = ["IdenticalCompressor", "QSGDCompressor", "NearestNeighborCompressor", "ProbabilisticScalarCompressor",
           "ProbabilisticVectorCompressor", "ResidualCompressor", "SignSGDCompressor", "TopKSparsificationCompressor",
           "MaureySparsification", "MXCompressor", "DriveCompressor", "EdenCompressor", "ThresholdSparsificationCompressor", "SparseTernaryCompressor",
           "PowerSGDCompressor"]
