"""Codecs: how one parameter tensor -- or all tensors of a model that share a compressor -- is written to and read
from the wire (gq_amd.quantizers owns the wire, the exchange and the step; the codecs are the only objects that touch
device memory, through gq_amd.native).

    DenseCodec                 IdenticalCompressor tensors (<= 1000 elements, ps_quantizer.py:18-19): raw f32
    HSQCodec / QSGDCodec       one tensor per launch (the reference's per-tensor loop, nearest_neighbor_compressor.py:63-90,
                               qsgd_compressor.py:42-71)
    PVQCodec                   ProbabilisticVectorCompressor: HSQCodec's wire, the sampled encode (gq_pvq_encode)
    ResidualCodec              ResidualCompressor: two HSQ sections back to back, stage 1's and stage 2's
    TopKCodec                  TopKSparsificationCompressor: k ascending uint32 indices, then their k f32 values
    SignCodec                  SignSGDCompressor: one 2-bit code per element (+0, +1, -1), 16 to a uint32 word
    MaureyCodec                MaureySparsification: a 16-byte header (scale), then k ascending uint32 words index | sign << 31
    MXCodec                    MXCompressor: a scale byte per block of 32 elements, then one FP4 / FP6 / FP8 code per element
    DriveCodec                 DriveCompressor: one sign bit per element of the rotated 256-element blocks, then an f32 scale per block
    EdenCodec                  EdenCompressor: a 2-, 3- or 4-bit Lloyd-Max code per element of the rotated blocks, then an f32 scale per block
    ThrCodec                   ThresholdSparsificationCompressor: a 16-byte header (kept, found, threshold), then cap ascending uint32 indices and cap f32 values
    BatchedHSQ / BatchedPVQ / BatchedResidual / BatchedQSGD / BatchedTopK / BatchedDGC / BatchedSign / BatchedMaurey / BatchedMX / BatchedMXR /
    STCCodec                   SparseTernaryCompressor: a 16-byte header (k, the magnitude), a uint32 start per item of 4,096 elements, then k 16-bit words
    PowerSGDCodec              PowerSGDCompressor: a 16-byte header (n, m, r), then the factors Ph (n x r) and Q' (m x r) as f32
    BatchedDrive / BatchedEden / BatchedThr / BatchedSTC / BatchedPowerSGD
                               every tensor of a model in one launch per stage (descriptor tables, HIP-graph friendly)
    GenericCodec               any other compressor object: its own compress / decompress, tensors on the wire as they are

`codec_factory` arguments of the quantizers exist so that the host logic can be exercised without a GPU by the tests
(with the CPU oracle as the checker codec: tests/oracle_codec.py).
"""
import itertools
import operator
import os

import torch

from . import exchange, native
from .compressors import (DriveCompressor, EdenCompressor, IdenticalCompressor, MaureySparsification, MXCompressor, NearestNeighborCompressor, ProbabilisticVectorCompressor,
                          PowerSGDCompressor, QSGDCompressor, ResidualCompressor, SignSGDCompressor, SparseTernaryCompressor, ThresholdSparsificationCompressor, TopKSparsificationCompressor, _next_seed,
                          _require_device)


def _up(x, a=16):
    return (x + a - 1) // a * a


# --------------------------------------------------------------------------------------
# Codecs: how one parameter tensor is written to / read from the wire
# --------------------------------------------------------------------------------------
class DenseCodec(object):
    """IdenticalCompressor tensors (<=1000 elements, ps_quantizer.py:18-19): raw f32 on the wire."""

    align = 4       # dense sections are packed back to back so that ONE cat / ONE mean serves them all

    def __init__(self, compressor, numel, shape):
        self.numel, self.shape = numel, shape
        self.nbytes = numel * 4

    def encode_into(self, grad, wire_user, off, salt):
        wire_user[off:off + self.numel * 4].view(torch.float32).copy_(grad.reshape(-1))

    def roundtrip(self, grad, salt):
        return grad.clone()

    def encode_decode_into(self, grad, wire_user, off, salt, out):
        """encode_into + the decode of what was written (error feedback, ps_quantizer.py:37: the residual is zero)."""
        self.encode_into(grad, wire_user, off, salt)
        out.copy_(grad.reshape(-1))

    def decode_mean(self, gathered, off, R, plain=False):
        # [R, numel] view of the gathered wire; stack().mean(0) of the reference (plain: the one payload as it is)
        rows = gathered[:, off:off + self.numel * 4].view(torch.float32)
        if plain and R == 1:
            return rows[0].clone().view(self.shape)
        if rows.device.type == "cuda":      # torch's GPU mean multiplies by 1/R and sums in its own order
            out = torch.empty(self.numel, dtype=torch.float32, device=rows.device)
            native.mean_rows(rows, out)
            return out.view(self.shape)
        return rows.mean(dim=0).view(self.shape)


def _kernel_copy(dst, src):
    """dst <- src (int64 device tensors of one size) by an elementwise KERNEL, for use under stream capture: a memcpy node in a
    replayed HIP graph costs ~15 us of every step whether its source is pinned host memory or device memory (84.9 / 83.4 us
    against 69.7 without the node, tools/graph_pieces.py -- the copy engine's hand-over), a kernel node ~2."""
    torch.bitwise_or(src, 0, out=dst)


def _esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


class GenericCodec(object):
    """Any other compressor class (sign, top-k, user supplied): ships the DECODED tensor.
    Keeps the reference semantics (mean of decompress(compress(g))) without a compact format."""

    def __init__(self, compressor, numel, shape):
        self.c, self.numel, self.shape = compressor, numel, shape
        self.nbytes = _up(numel * 4)

    def roundtrip(self, grad, salt):
        return self.c.decompress(self.c.compress(grad)).reshape(self.shape)

    def encode_into(self, grad, wire_user, off, salt):
        wire_user[off:off + self.numel * 4].view(torch.float32).copy_(self.roundtrip(grad, salt).reshape(-1))

    def encode_decode_into(self, grad, wire_user, off, salt, out):
        """ONE decompress(compress(grad)) (ps_quantizer.py:37): it is both what travels and what the residual is taken against
        (a compressor that rounds stochastically must not be asked twice)."""
        self.encode_into(grad, wire_user, off, salt)
        out.copy_(wire_user[off:off + self.numel * 4].view(torch.float32))

    def decode_mean(self, gathered, off, R, plain=False):
        rows = gathered[:, off:off + self.numel * 4].view(torch.float32)
        if plain and R == 1:
            return rows[0].clone().view(self.shape)
        if rows.device.type == "cuda":      # torch's GPU mean multiplies by 1/R and sums in its own order
            out = torch.empty(self.numel, dtype=torch.float32, device=rows.device)
            native.mean_rows(rows, out)
            return out.view(self.shape)
        return rows.mean(dim=0).view(self.shape)


def aggregate_fma(args=None):
    """Opt-in (args.gq_aggregate = "fma" / $GQ_AGGREGATE=fma): the decode-mean over R >= 2 payloads accumulates with fused
    multiply-adds (GQ_AGGREGATE_FMA: half the arithmetic per payload, aggregate within 1e-6 relative L2 of the bit-exact one;
    the north star grants 1e-5).  Default "exact": the reference's separately rounded product and sum."""
    mode = getattr(args, "gq_aggregate", None) or os.environ.get("GQ_AGGREGATE", "exact")
    if mode not in ("exact", "fma"):
        raise ValueError("gq_aggregate / GQ_AGGREGATE must be 'exact' or 'fma', got %r" % (mode,))
    return mode == "fma"


def wire_levels_mode(args=None, world=1):
    """How byte-sized levels travel: "bytes" (one per level) or "packed6" (four 6-bit levels per three bytes, for the
    configurations whose top level is <= 63 with d = 16, K <= 256).  args.gq_wire_levels, else $GQ_WIRE_LEVELS, else
    "auto": packed6 when there is an exchange to shorten (more than one rank), bytes on a single rank -- the packed form is
    bit-identical in its result and costs < 1 % of a single-rank step."""
    mode = getattr(args, "gq_wire_levels", None) or os.environ.get("GQ_WIRE_LEVELS", "auto")
    if mode not in ("bytes", "packed6", "auto"):
        raise ValueError("gq_wire_levels / GQ_WIRE_LEVELS must be 'bytes', 'packed6' or 'auto', got %r" % (mode,))
    if mode == "auto":
        mode = "packed6" if world > 1 else "bytes"
    return mode


class HSQCodec(object):
    """NearestNeighborCompressor on the HIP kernels.  Wire per user:
    codes[M] (uint8 | int32) | levels[M] (uint8/int16/int32, or f32 u when n_bit == 32; packed6: 3 * ceil(M/4) bytes) | lb, ub."""

    def __init__(self, compressor, numel, shape, packed6=False):
        self.c, self.numel, self.shape = compressor, numel, shape
        M = compressor.M
        self.M = M
        self.code_dtype = compressor.code_dtype
        self.level_dtype = compressor.wire_level_dtype() if compressor.compressed_norm else torch.float32
        self.packed6 = bool(packed6) and self.can_pack6(compressor)
        cb = torch.empty(0, dtype=self.code_dtype).element_size()
        self._level_bytes = native.packed6_bytes(M) if self.packed6 else M * torch.empty(0, dtype=self.level_dtype).element_size()
        self.codes_off = 0
        self.levels_off = _up(M * cb)
        self.lbub_off = self.levels_off + _up(self._level_bytes)
        self.nbytes = self.lbub_off + 16
        self._u = None
        self._partials = None

    @staticmethod
    def can_pack6(compressor):
        """The packed form is used for d = 16, K <= 256 (what the multi-tensor level / decode kernels with packed levels are
        built for; the per-tensor entry points would take any K <= 256) when no level exceeds 63: n_bit <= 6 without
        stochastic rounding (probabilistic_scalar_compressor.py:18: levels up to 2^n_bit - 1), n_bit <= 5 with it (:25: up
        to 2^n_bit).  Every other configuration keeps one byte (or more) per level."""
        if not compressor.compressed_norm or compressor.dim != 16 or compressor.K > 256:
            return False
        nc = compressor.norm_compressor
        return (1 << nc.n_bit) - (0 if nc.random else 1) <= 63

    def wire_level_kind(self):
        """What the native calls take as the level type of this codec's wire."""
        return native.PACKED6 if self.packed6 else self.level_dtype

    def _views(self, wire_user, off):
        M = self.M
        cb = torch.empty(0, dtype=self.code_dtype).element_size()
        codes = wire_user[off + self.codes_off:off + self.codes_off + M * cb].view(self.code_dtype)
        levels = wire_user[off + self.levels_off:off + self.levels_off + self._level_bytes]
        if not self.packed6:
            levels = levels.view(self.level_dtype)
        lb_ub = wire_user[off + self.lbub_off:off + self.lbub_off + 8].view(torch.float32)
        return codes, levels, lb_ub

    def _scratch(self, dev):
        if self._u is None or self._u.device != dev:
            self._u = torch.empty(self.M, dtype=torch.float32, device=dev)
            self._partials = native.new_workspace(dev, self.M)
        return self._u, self._partials

    def uses_reference_draws(self):
        """True if compress draws r = torch.rand(M) from the CPU generator as the reference does
        (probabilistic_scalar_compressor.py:23-25; args.random with gq_rng = "reference")."""
        nc = getattr(self.c, "norm_compressor", None)
        return bool(self.c.compressed_norm and nc is not None and nc.random and nc._rng == "reference")

    def draw_count(self):
        """Reference draws per compress (uses_reference_draws): the quantizer's one torch.rand per record gives the codec a
        slice of this length."""
        return self.M

    def _levels(self, u, partials, levels, lb_ub, salt, r=None):
        nc = self.c.norm_compressor
        if not nc.random:
            native.hsq_levels(u, nc.n_bit, native.RANDOM_OFF, None, 0, partials, lb_ub, levels, self.packed6)
        elif nc._rng == "reference":
            if r is None:       # the quantizer hands over its slice of ONE torch.rand per record (same stream)
                r = torch.rand(self.M).to(u.device)
            native.hsq_levels(u, nc.n_bit, native.RANDOM_GIVEN, r, 0, partials, lb_ub, levels, self.packed6)
        else:
            native.hsq_levels(u, nc.n_bit, native.RANDOM_DEVICE, None, _next_seed() ^ salt, partials, lb_ub, levels, self.packed6)

    def encode_into(self, grad, wire_user, off, salt, r=None):
        _require_device(grad, "HSQCodec.encode_into")
        dev = grad.device
        flat = grad.contiguous().view(-1)
        codes, levels, lb_ub = self._views(wire_user, off)
        cbk = self.c._codebook_on(dev)
        if self.c.compressed_norm:
            u, partials = self._scratch(dev)
            nc = self.c.norm_compressor
            if nc.random and nc._rng == "reference":
                native.hsq_encode(flat, cbk, codes, u, partials)
                self._levels(u, partials, levels, lb_ub, salt, r)
            else:   # encode + levels in one library call (gq_hsq_compress)
                mode = native.RANDOM_DEVICE if nc.random else native.RANDOM_OFF
                native.hsq_compress(flat, cbk, codes, u, partials, nc.n_bit, mode, None,
                                    (_next_seed() ^ salt) if nc.random else 0, lb_ub, levels, self.packed6)
        else:
            _, partials = self._scratch(dev)
            native.hsq_encode(flat, cbk, codes, levels, partials)  # `levels` section holds f32 u

    def decode_wire(self, wire_user, off, out):
        """Decode this user's own payload (error feedback residual)."""
        self._decode(wire_user.view(1, -1), off, 1, out)

    def encode_decode_into(self, grad, wire_user, off, salt, out, r=None):
        """encode_into + decode_wire: decompress(compress(grad)) with the payload left in the wire (ps_quantizer.py:37).
        Where the library serves it (d = 16, byte codes, byte or packed levels) the level quantiser and the decode are ONE
        launch (gq_hsq_levels_decode); same bits either way."""
        nc = getattr(self.c, "norm_compressor", None)
        if self.c.compressed_norm and self.c.dim == 16 and self.code_dtype == torch.uint8 and grad.device.type == "cuda":
            dev = grad.device
            flat = grad.contiguous().view(-1)
            codes, levels, lb_ub = self._views(wire_user, off)
            if self.packed6 or levels.dtype == torch.uint8:
                cbk = self.c._codebook_on(dev)
                u, partials = self._scratch(dev)
                if not nc.random:
                    mode, rr, seed = native.RANDOM_OFF, None, 0
                elif nc._rng == "reference":
                    mode, rr, seed = native.RANDOM_GIVEN, (r if r is not None else torch.rand(self.M).to(dev)), 0
                else:
                    mode, rr, seed = native.RANDOM_DEVICE, None, _next_seed() ^ salt
                native.hsq_encode(flat, cbk, codes, u, partials)
                if native.hsq_levels_decode(u, nc.n_bit, mode, rr, seed, partials, lb_ub, levels, codes, cbk, out, self.packed6):
                    return
                native.hsq_levels(u, nc.n_bit, mode, rr, seed, partials, lb_ub, levels, self.packed6)
                self.decode_wire(wire_user, off, out)
                return
        self.encode_into(grad, wire_user, off, salt, r)
        self.decode_wire(wire_user, off, out)

    def _decode(self, gathered, off, R, out):
        P = gathered.shape[1]
        cbk = self.c._codebook_on(gathered.device)
        n_bit = self.c.n_bit if self.c.compressed_norm else 32
        if getattr(self, "fma", False) and R >= 2 and self.c.compressed_norm:
            n_bit |= native.AGGREGATE_FMA
        native.hsq_decode_sum_packed(gathered, self.M, cbk, n_bit, out, R,
                                     codes_off=off + self.codes_off, levels_off=off + self.levels_off,
                                     lbub_off=off + self.lbub_off, code_dtype=self.code_dtype,
                                     level_dtype=self.wire_level_kind())
        assert P == gathered.stride(0)

    def roundtrip(self, grad, salt, r=None):
        dev = grad.device
        tmp = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(self.numel, dtype=torch.float32, device=dev)
        self.encode_decode_into(grad, tmp, 0, salt, out, r)
        return out.view(self.shape)

    def decode_mean(self, gathered, off, R, plain=False):
        out = torch.empty(self.numel, dtype=torch.float32, device=gathered.device)
        self._decode(gathered, off, R, out)
        if R == 1 and not plain:
            out.add_(0.0)   # one payload is the plain decompress (-0 kept); the aggregate is a sum that starts from +0
        return out.view(self.shape)


class PVQCodec(HSQCodec):
    """ProbabilisticVectorCompressor on the HIP kernels: HSQCodec's wire layout, packed6 rule and decode (the compressor's
    decode IS HSQ's: codewords[codes] * norms, probabilistic_vector_compressor.py:67-77); the encode samples the codeword
    (gq_pvq_encode).  Reference draws: torch.rand(M) for the codewords (:52, always), then torch.rand(M) for the levels
    (probabilistic_scalar_compressor.py:23, with args.random and n_bit != 32) -- `r` is the two slices back to back.
    gq_rng = "keyed" draws like "device" here (a fresh seed per call, as HSQCodec): only the multi-tensor launches key their
    streams, so keyed runs with and without gq_no_batch give different bits."""

    def _level_draws_wanted(self):
        nc = getattr(self.c, "norm_compressor", None)
        return bool(self.c.compressed_norm and nc is not None and nc.random)

    def uses_reference_draws(self):
        return self.c._rng == "reference"      # the sampler always draws

    def draw_count(self):
        return self.M * (2 if self._level_draws_wanted() else 1)

    def encode_into(self, grad, wire_user, off, salt, r=None):
        _require_device(grad, "PVQCodec.encode_into")
        dev = grad.device
        flat = grad.contiguous().view(-1)
        codes, levels, lb_ub = self._views(wire_user, off)
        _, cdag = self.c._on(dev)
        u, partials = self._scratch(dev)
        if not self.c.compressed_norm:
            u = levels      # the `levels` section holds f32 u
        r_levels = None
        if self.c._rng == "reference":
            if r is None:       # the compressor's own order: the codeword draws, then the level draws (HSQCodec._levels)
                r_code = torch.rand(self.M).to(dev)
            else:
                r_code, r_levels = r[:self.M], (r[self.M:2 * self.M] if self._level_draws_wanted() else None)
            native.pvq_encode(flat, cdag, codes, u, partials, native.RANDOM_GIVEN, r_code, 0)
        else:
            native.pvq_encode(flat, cdag, codes, u, partials, native.RANDOM_DEVICE, None, _next_seed() ^ salt)
        if self.c.compressed_norm:
            self._levels(u, partials, levels, lb_ub, salt, r_levels)

    def encode_decode_into(self, grad, wire_user, off, salt, out, r=None):
        """ONE compress: what travels is what the residual is taken against (ps_quantizer.py:37)."""
        self.encode_into(grad, wire_user, off, salt, r)
        self.decode_wire(wire_user, off, out)


class ResidualCodec(object):
    """ResidualCompressor on the HIP kernels.  Wire per user: stage 1's HSQ section (NearestNeighbor on the gradient), then --
    16-byte aligned -- stage 2's (the probabilistic vector compressor on what stage 1 leaves), each laid out as HSQCodec lays
    out codes | levels (or f32 u when n_bit == 32) | lb, ub.  The encode is the launches ResidualCompressor.compress makes,
    writing into wire views: gq_hsq_encode + levels, stage 1's norms de-quantised, gq_pvq_encode's stage1 form + levels.  The
    decode is the two-stage decode-mean of libgq_rq.so over a one-row table: per payload (0 + d1) + d2, rounded before it
    enters the sum over the payloads -- torch.stack([d1, d2]).sum(0) per user, then stack(users).mean(0).
    Reference draws per compress, in the reference's call order: stage 1's level draws (with args.random and n_bit != 32),
    stage 2's codeword draws (always), stage 2's level draws (as the first) -- `r` is the runs back to back.
    Levels travel as bytes or wider, never as packed6 (the stage-2 kernel reads stage 1's levels as they are on the wire).
    Shapes: the ones libgq_rq.so serves (serves()); every other ResidualCompressor keeps GenericCodec."""

    @staticmethod
    def serves(compressor):
        first, second = compressor.compressors
        return bool(first.dim == second.dim and first.K == second.K and first.code_dtype == second.code_dtype
                    and native.rq_batched_serves(first.dim, first.K, first.code_dtype))

    def __init__(self, compressor, numel, shape, packed6=False):
        self.c, self.numel, self.shape = compressor, numel, shape
        first, second = compressor.compressors
        self.s1 = HSQCodec(first, numel, shape)
        self.s2 = PVQCodec(second, numel, shape)
        assert self.s1.M == self.s2.M and self.s1.level_dtype == self.s2.level_dtype
        self.M = self.s1.M
        self.code_dtype, self.level_dtype = self.s1.code_dtype, self.s1.level_dtype
        self.stage2_off = _up(self.s1.nbytes)
        self.nbytes = self.stage2_off + self.s2.nbytes
        self._single = None

    def _level_draws_wanted(self):
        return self.s2._level_draws_wanted()

    def uses_reference_draws(self):
        return self.s2.uses_reference_draws()      # stage 2's sampler always draws

    def draw_runs(self):
        """Which run of M reference draws each consumer takes: (stage 1's levels, stage 2's codewords, stage 2's levels);
        None: that consumer does not draw."""
        return (0, 1, 2) if self._level_draws_wanted() else (None, 0, None)

    def draw_count(self):
        return self.M * (3 if self._level_draws_wanted() else 1)

    def wire_level_kind(self):
        return self.level_dtype

    def _batched1(self, dev, off):
        """The launch descriptor of this one tensor at byte `off` of a payload (a one-row table)."""
        if self._single is None or self._single[0] != (dev, off):
            first, second = self.c.compressors
            ntiles = (self.M + 63) // 64
            tabs = []
            for cd, o in ((self.s1, off), (self.s2, off + self.stage2_off)):
                t = torch.zeros((1, 8), dtype=torch.int64)
                t[0, 1], t[0, 3], t[0, 4], t[0, 5] = self.M, o + cd.codes_off, o + cd.levels_off, o + cd.lbub_off
                tabs.append(t.view(-1).to(dev))
            cb1, (cb2, cdag) = first._codebook_on(dev), second._on(dev)
            n_bit = first.n_bit if first.compressed_norm else 32
            batch = native.RQBatch(tabs[0], tabs[1], torch.zeros(ntiles, dtype=torch.int32, device=dev), 1, ntiles, cb1, cb2, cdag,
                                   self.code_dtype, self.level_dtype, n_bit)
            self._single = ((dev, off), batch)
        return self._single[1]

    def encode_into(self, grad, wire_user, off, salt, r=None):
        _require_device(grad, "ResidualCodec.encode_into")
        dev = grad.device
        first, second = self.c.compressors
        flat = grad.contiguous().view(-1)
        M = self.M
        runs = self.draw_runs()
        take = lambda k: None if (r is None or runs[k] is None) else r[runs[k] * M:(runs[k] + 1) * M]
        self.s1.encode_into(flat, wire_user, off, salt, take(0))
        codes1, levels1, lb_ub1 = self.s1._views(wire_user, off)
        # stage 1's norms as the compressor de-quantises them (probabilistic_scalar_compressor.py:31-32); n_bit == 32: f32 u as it travels
        norm1 = first.norm_compressor.decompress((lb_ub1[0], lb_ub1[1], levels1)) if first.compressed_norm else levels1
        codes2, levels2, lb_ub2 = self.s2._views(wire_user, off + self.stage2_off)
        _, cdag = second._on(dev)
        u, partials = self.s2._scratch(dev)
        if not second.compressed_norm:
            u = levels2      # the `levels` section holds f32 u
        if second._rng == "reference":
            r_code = take(1)
            if r_code is None:       # the compressor's own order: its codeword draws here, its level draws in _levels
                r_code = torch.rand(M).to(dev)
            native.pvq_encode_residual(flat, codes1, norm1, first._codebook_on(dev), cdag, codes2, u, partials, native.RANDOM_GIVEN, r_code, 0)
        else:
            native.pvq_encode_residual(flat, codes1, norm1, first._codebook_on(dev), cdag, codes2, u, partials, native.RANDOM_DEVICE, None,
                                       _next_seed() ^ salt)
        if second.compressed_norm:
            self.s2._levels(u, partials, levels2, lb_ub2, salt, take(2))

    def decode_wire(self, wire_user, off, out):
        """Decode this user's own payload (error feedback residual): the plain decompress, (0 + d1) + d2."""
        self._decode(wire_user.view(1, -1), off, 1, out, plain=True)

    def encode_decode_into(self, grad, wire_user, off, salt, out, r=None):
        """ONE compress: what travels is what the residual is taken against (ps_quantizer.py:37)."""
        self.encode_into(grad, wire_user, off, salt, r)
        self.decode_wire(wire_user, off, out)

    def _decode(self, gathered, off, R, out, plain=False):
        self._batched1(gathered.device, off).decode(gathered, R, out.view(-1), plain=plain)

    def roundtrip(self, grad, salt, r=None):
        dev = grad.device
        tmp = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(self.numel, dtype=torch.float32, device=dev)
        self.encode_decode_into(grad, tmp, 0, salt, out, r)
        return out.view(self.shape)

    def decode_mean(self, gathered, off, R, plain=False):
        out = torch.empty(self.numel, dtype=torch.float32, device=gathered.device)
        self._decode(gathered, off, R, out, plain=plain)
        return out.view(self.shape)


class QSGDCodec(object):
    """QSGDCompressor on the HIP kernels.  Wire per user, packed form (even bucket size and a
    top level that fits 3, 7 or 15 bits):  norm f32[Mb] | one code per element = sign<<(bits-1) | level,
    4-bit codes two per byte.  Otherwise the plain form  norm f32[Mb] | signs u8[n] | levels u8|i32 [n]."""

    def __init__(self, compressor, numel, shape):
        self.c, self.numel, self.shape = compressor, numel, shape
        self.Mb, self.d = compressor.M, compressor.dim
        mode = native.RANDOM_DEVICE if compressor.random else native.RANDOM_OFF
        self.bits = 0
        if self.d % 2 == 0 and (not compressor.random or compressor._rng != "reference"):
            top = 2 ** compressor.bit - (0 if compressor.random else 1)
            self.bits = 4 if top <= 7 else (8 if top <= 127 else (16 if top <= 32767 else 0))
        self.norm_off = 0
        if self.bits:
            self.codes_off = _up(self.Mb * 4)
            self.nbytes = self.codes_off + _up(numel * self.bits // 8)
            self._single = None     # a one-tensor BatchedQSGD, built on first use
        else:
            top = 2 ** compressor.bit
            self.level_dtype = torch.uint8 if top <= 127 else torch.int32
            lb = torch.empty(0, dtype=self.level_dtype).element_size()
            self.signs_off = _up(self.Mb * 4)
            self.levels_off = self.signs_off + _up(numel)
            self.nbytes = self.levels_off + _up(numel * lb)
        self._mode = mode

    # ---- packed form: a single-segment instance of the batched kernels ----------------------
    def _batched1(self, dev):
        if self._single is None or self._single.device != dev:
            self._single = BatchedQSGD([self], [0], [0], dev, 1, self.nbytes)
        return self._single

    # ---- plain form --------------------------------------------------------------------------
    def _views(self, wire_user, off):
        lb = torch.empty(0, dtype=self.level_dtype).element_size()
        norm = wire_user[off + self.norm_off:off + self.norm_off + self.Mb * 4].view(torch.float32)
        signs = wire_user[off + self.signs_off:off + self.signs_off + self.numel]
        levels = wire_user[off + self.levels_off:off + self.levels_off + self.numel * lb].view(self.level_dtype)
        return norm, signs, levels

    def encode_into(self, grad, wire_user, off, salt):
        _require_device(grad, "QSGDCodec.encode_into")
        flat = grad.contiguous().view(-1)
        c = self.c
        if self.bits:
            ok = self._batched1(flat.device).encode([flat], wire_user[off:off + self.nbytes], 0, salt)
            assert ok, "QSGDCodec: gradient storage must be 8-byte aligned"
            return
        norm, signs, levels = self._views(wire_user, off)
        if not c.random:
            native.qsgd_compress(flat, self.d, c.bit, native.RANDOM_OFF, None, 0, norm, signs, levels)
        elif c._rng == "reference":
            r = torch.rand(self.Mb, self.d)
            native.qsgd_compress(flat, self.d, c.bit, native.RANDOM_GIVEN, r.to(flat.device).view(-1), 0, norm, signs,
                                 levels)
        else:
            native.qsgd_compress(flat, self.d, c.bit, native.RANDOM_DEVICE, None, _next_seed() ^ salt, norm, signs,
                                 levels)

    def _decode_rows(self, gathered, off, R, out, plain=False):
        if self.bits:
            rows = gathered[:, off:off + self.nbytes]
            if not rows.is_contiguous():
                rows = rows.contiguous()
            out.copy_(self._batched1(gathered.device).decode_mean(rows, R, plain=plain)[0].view(-1))
            return
        # the plain entry point takes dense [R][...] arrays: gather the three sections
        lb = torch.empty(0, dtype=self.level_dtype).element_size()
        norm = gathered[:, off + self.norm_off:off + self.norm_off + self.Mb * 4].contiguous().view(torch.float32)
        signs = gathered[:, off + self.signs_off:off + self.signs_off + self.numel].contiguous()
        levels = gathered[:, off + self.levels_off:off + self.levels_off + self.numel * lb].contiguous() \
            .view(self.level_dtype)
        native.qsgd_decode_sum(norm.view(-1), signs.view(-1), levels.view(-1), self.d, self.c.bit, out, R=R)

    def roundtrip(self, grad, salt):
        tmp = torch.empty(self.nbytes, dtype=torch.uint8, device=grad.device)
        self.encode_into(grad, tmp, 0, salt)
        out = torch.empty(self.numel, dtype=torch.float32, device=grad.device)
        self._decode_rows(tmp.view(1, -1), 0, 1, out, plain=True)     # decompress(compress(g)): no aggregate
        return out.view(self.shape)

    def decode_wire(self, wire_user, off, out):
        self._decode_rows(wire_user.view(1, -1), off, 1, out, plain=True)

    def decode_mean(self, gathered, off, R, plain=False):
        out = torch.empty(self.numel, dtype=torch.float32, device=gathered.device)
        self._decode_rows(gathered, off, R, out, plain=plain)
        if R == 1 and not plain:
            out.add_(0.0)   # as HSQCodec.decode_mean: torch.stack(...).mean(0) of one payload turns -0 into +0
        return out.view(self.shape)


class _SparseCodec(object):
    """What TopKCodec, SignCodec, MaureyCodec and MXCodec share: every call is a one-tensor group of the codec's multi-tensor class
    (GROUP, set below that class), and roundtrip / encode_decode_into return the compress launches' own dense decode, not a
    decode of the wire.  A subclass sets numel, shape and nbytes; `extra` are further arguments of its group's encode."""

    GROUP = None
    _single = None
    dtype = torch.float32      # of the gradients, and of what roundtrip / decode_mean return (MXCodec: float32 or bfloat16)

    def _wire_bytes(self):
        """Bytes of a wire of this tensor alone.  A launch is handed a valid address also when the section is empty, which only
        TopKCodec's can be (k = 0); every other section is at least 16 bytes at one element, so this is nbytes."""
        return max(16, self.nbytes)

    def _draws(self, r, dev):
        """The draws of a call as the group takes them: `r`, or for gq_rng "reference" torch.rand(draw_count()) (the codec on its
        own: the quantizers draw once per record and hand out slices); None where there are none."""
        if r is None and self.uses_reference_draws():
            r = torch.rand(self.draw_count()).to(dev)
        return (r, {0: 0}) if r is not None else None

    @staticmethod
    def _errs_of(grad, err, who):
        """A call's residual as the group's `errs`.  Error feedback updates the gradient in place: it must be contiguous itself."""
        if err is None:
            return None
        if not grad.is_contiguous():
            raise ValueError("%s: error feedback updates the gradient in place and needs a contiguous one" % who)
        return [err.view(-1)]

    def _batched1(self, dev):
        if self._single is None or self._single.device != dev:
            self._single = self.GROUP([self], [0], [0], dev, 1, self._wire_bytes())
        return self._single

    @staticmethod
    def _at(wire_user, off):
        return wire_user[off:]

    def encode_decode_into(self, grad, wire_user, off, salt, out, **extra):
        """The payload into the wire and decompress(compress(grad)) into `out` (ps_quantizer.py:37), one launch sequence."""
        self.encode_into(grad, wire_user, off, salt, out=out.view(-1), **extra)

    def encode_into(self, grad, wire_user, off, salt, **extra):
        name = type(self).__name__
        _require_device(grad, name + (".encode_decode_into" if extra.get("out") is not None else ".encode_into"))
        flat = grad.contiguous().view(-1)
        ok = self._batched1(flat.device).encode([flat], self._at(wire_user, off), 0, salt, **extra)
        assert ok, name + ": the gradient must be a %s tensor on the current device" % (self.dtype,)

    def roundtrip(self, grad, salt, **extra):
        out = torch.empty(self.numel, dtype=self.dtype, device=grad.device)
        tmp = torch.empty(self._wire_bytes(), dtype=torch.uint8, device=grad.device)
        self.encode_decode_into(grad, tmp, 0, salt, out, **extra)
        return out.view(self.shape)

    def decode_wire(self, wire_user, off, out):
        self._decode_rows(wire_user.view(1, -1), off, 1, out, plain=True)

    def _decode_rows(self, gathered, off, R, out, plain=False):
        self._batched1(gathered.device).decode_into(gathered[:, off:off + self.nbytes], R, out, plain=plain)

    def decode_mean(self, gathered, off, R, plain=False):
        out = torch.empty(self.numel, dtype=self.dtype, device=gathered.device)
        self._decode_rows(gathered, off, R, out, plain=plain)
        return out.view(self.shape)


class TopKCodec(_SparseCodec):
    """TopKSparsificationCompressor on the HIP kernels (libgq_topk.so).  Wire per tensor: k = numel // cr ascending uint32
    indices, then the k f32 values -- 8k bytes.  Every call is a one-tensor BatchedTopK; roundtrip / encode_decode_into return the
    compress launch's own dense decode (v * mask, the reference's signed zeros and NaNs included), not a decode of the wire."""

    def __init__(self, compressor, numel, shape):
        self.c, self.numel, self.shape = compressor, numel, shape
        self.k = int(compressor.k)
        if not 0 <= self.k <= numel:
            raise ValueError("TopKCodec: k = %d for a tensor of %d elements" % (self.k, numel))
        self.nbytes = 8 * self.k

    @staticmethod
    def _at(wire_user, off):
        # (k = 0 writes nothing: any valid address will do when the section is empty and ends the buffer)
        return wire_user[off:] if off < wire_user.numel() else wire_user

    def _decode_rows(self, gathered, off, R, out, plain=False):
        if self.k == 0:
            out.zero_()
            return
        _SparseCodec._decode_rows(self, gathered, off, R, out, plain=plain)


def thr_section_bytes(numel, cr, percent=150):
    """Bytes of one tensor's section of the threshold wire (include/gq_thr.h): a 16-byte header, cap uint32 indices, cap f32 values,
    zero bytes up to a multiple of 16; cap = min(numel, (k * percent + 99) // 100), k = numel // cr."""
    k = numel // cr
    if k < 1:
        raise ValueError("thr_section_bytes: k = %d // %d is below 1" % (numel, cr))
    return native.THR_HEADER_BYTES + _up(8 * ThresholdSparsificationCompressor.capacity(numel, k, percent))


class ThrCodec(_SparseCodec):
    """ThresholdSparsificationCompressor on the HIP kernels (libgq_thr.so).  Wire per tensor: a 16-byte header { kept, found,
    bits(eta), 0 }, cap ascending uint32 indices, cap f32 values, slots from `kept` on holding index 0xffffffff and +0 --
    thr_section_bytes.  Every call is a one-tensor BatchedThr; roundtrip / encode_decode_into return the compress launches' own
    dense decode (w * mask), not a decode of the wire."""

    def __init__(self, compressor, numel, shape):
        self.c, self.numel, self.shape = compressor, numel, shape
        self.k = numel // compressor.cr
        if self.k < 1 or not 1 <= numel < 2 ** 31:
            raise ValueError("ThrCodec: k = %d // %d = %d for a tensor of %d elements (k must be at least 1)"
                             % (numel, compressor.cr, self.k, numel))
        self.cap = compressor.capacity(numel, self.k, compressor.percent)
        self.stride = compressor.stride_for(numel, compressor.fit_stride)
        self.stages, self.eta = compressor.stages, compressor.eta
        self.nbytes = thr_section_bytes(numel, compressor.cr, compressor.percent)

    def header(self, wire_user, off):
        """(kept, found, eta) of this tensor's section of one user's wire: a read of three words, with a synchronisation."""
        w = wire_user[off:off + 12].cpu().numpy()
        kept, found = (int(x) for x in w[:8].view("<u4"))
        return kept, found, float(w[8:12].view("<f4")[0])


def stc_section_bytes(numel, cr):
    """Bytes of one tensor's section of the sparse ternary wire (include/gq_stc.h): a 16-byte header, a uint32 start per item of 4,096
    elements, k = numel // cr 16-bit words, zero bytes up to a multiple of 16."""
    return _stc_bytes(numel, numel // cr)


def _stc_bytes(numel, k):
    return _up(native.STC_HEADER_BYTES + 4 * -(-numel // native.STC_CHUNK) + 2 * k)


class STCCodec(_SparseCodec):
    """SparseTernaryCompressor on the HIP kernels (libgq_stc.so).  Wire per tensor: { k, bits(mu), items, 0 }, the items' starts, then
    k words  position inside the item | sign << 15  -- stc_section_bytes.  Every call is a one-tensor BatchedSTC; roundtrip /
    encode_decode_into return the compress launches' own dense decode (copysign(mu, w) on the kept set), not a decode of the wire."""

    def __init__(self, compressor, numel, shape, k=None):
        """k: another count than numel // cr (the launches take any 0 <= k <= numel)."""
        self.c, self.numel, self.shape = compressor, numel, shape
        self.k = numel // compressor.cr if k is None else int(k)
        if not 1 <= numel < 2 ** 31 or not 0 <= self.k <= numel:
            raise ValueError("STCCodec: k = %d for a tensor of %d elements (1 ... 2^31 - 1)" % (self.k, numel))
        self.nbytes = _stc_bytes(numel, self.k)

    def header(self, wire_user, off):
        """(k, mu) of this tensor's section of one user's wire: a read of two words, with a synchronisation."""
        w = wire_user[off:off + 8].cpu().numpy()
        return int(w[:4].view("<u4")[0]), float(w[4:8].view("<f4")[0])


def psgd_section_bytes(n, m, r):
    """Bytes of one tensor's section of the low-rank wire (include/gq_psgd.h): a 16-byte header, Ph (n x r) and Q' (m x r) as
    float32, zero bytes up to a multiple of 16."""
    return _up(native.PSGD_HEADER_BYTES + 4 * r * (n + m))


def _uniform_bits(seed, idx):
    """uniform_bits of csrc/gq_common.hpp over a uint64 array of indices (numpy, on the host)."""
    import numpy as np
    u64, m32 = np.uint64, np.uint64(0xFFFFFFFF)

    def mul(a, c):
        return (a * u64(c)) & m32

    seed = u64(seed & (2 ** 64 - 1))
    h = ((idx & m32) + mul(seed & m32, 0x9E3779B1)) & m32
    h = h ^ (h >> u64(16))
    h = mul(h, 0x7FEB352D)
    h = h ^ (h >> u64(15))
    h = mul(h, 0x846CA68B)
    h = h ^ (h >> u64(16))
    h = (h + ((seed >> u64(32)) ^ mul(idx >> u64(32), 0x85EBCA77))) & m32
    h = mul(h, 0xC2B2AE3D)
    return h ^ (h >> u64(15))


def psgd_q0(seed, param_index, user, m, r):
    """Q0 of include/gq_psgd.h, the warm start before the first record: float32 [m, r] on the host, 2 * uniform01 - 1 of the counter
    hash under (seed, (parameter index << 12 | user) << 32 | element)."""
    import numpy as np
    if not 0 <= user < native.PSGD_MAX_USERS or not 0 <= param_index < 2 ** 20 or m * r >= 2 ** 32:
        raise ValueError("psgd_q0: user %d (< %d), parameter %d (< 2^20), %d elements (< 2^32)" % (user, native.PSGD_MAX_USERS, param_index, m * r))
    idx = (np.uint64(((param_index << 12) | user) << 32) | np.arange(m * r, dtype=np.uint64))
    u = (_uniform_bits(seed, idx) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return torch.from_numpy((np.float32(2.0) * u - np.float32(1.0)).astype(np.float32).reshape(m, r))


class PowerSGDCodec(_SparseCodec):
    """PowerSGDCompressor on the HIP kernels (libgq_psgd.so).  Wire per tensor: { n, m, r, 0 }, Ph (n x r), Q' (m x r), float32 --
    psgd_section_bytes.  Every call is a one-tensor BatchedPowerSGD.  A record steps a warm start: the caller's (`q`, `user`; the
    quantizer keeps one per parameter and user) or, where none is given, one this codec owns (user 0).  roundtrip /
    encode_decode_into return the compress launches' own dense decode."""

    SERVER_USER = native.PSGD_MAX_USERS - 1      # the key of the two-phase server's warm start

    def __init__(self, compressor, numel, shape, param_index=0):
        self.c, self.numel, self.shape = compressor, numel, shape
        self.rank, self.seed, self.param_index = compressor.rank, compressor.seed, int(param_index)
        nm = compressor.matrix(numel, tuple(shape))
        if nm is None or min(nm) < self.rank or not 1 <= numel < 2 ** 31 or nm[0] * nm[1] != numel:
            raise ValueError("PowerSGDCodec: a tensor of shape %r is no matrix of at least %d rows and columns" % (tuple(shape), self.rank))
        self.n, self.m = nm
        self.nbytes = psgd_section_bytes(self.n, self.m, self.rank)
        self._q = None

    def warm_start(self, param_index, user, device):
        """Q0 of (this codec's seed, the parameter, the user) on the device: float32 [m, r]."""
        return psgd_q0(self.seed, param_index, user, self.m, self.rank).to(device)

    def encode_into(self, grad, wire_user, off, salt, out=None, err=None, ef_scale=None, q=None, user=0):
        _require_device(grad, "PowerSGDCodec" + (".encode_decode_into" if out is not None else ".encode_into"))
        flat = grad.contiguous().view(-1)
        if q is None:
            if self._q is None or self._q.device != flat.device:
                self._q = self.warm_start(self.param_index, user, flat.device)
            q = self._q
        errs = ([err.view(-1)] if err is not None else None, [q], user)
        ok = self._batched1(flat.device).encode([flat], self._at(wire_user, off), 0, salt, errs, ef_scale, out=out)
        assert ok, "PowerSGDCodec: gradient, residual and warm start must be contiguous float32 tensors on the current device"


def sign_section_bytes(numel):
    """Bytes of one tensor's section of the 2-bit sign wire (include/gq_sign.h): ceil(numel / 16) words, 16-byte aligned."""
    return _up(-(-numel // 16) * 4)


class SignCodec(_SparseCodec):
    """SignSGDCompressor on the HIP kernels (libgq_sign.so).  Wire per tensor: one 2-bit code per element, 00 = +0, 01 = +1,
    11 = -1, sixteen to a little-endian uint32 word (element i in bits 2*(i%16) of word i/16) -- _up(ceil(numel/16) * 4) bytes.
    torch.sign never returns -0 or NaN on the device, so the wire holds the decoded tensor exactly.  Every call is a one-tensor
    BatchedSign; roundtrip / encode_decode_into return the compress launch's own dense sign(grad)."""

    def __init__(self, compressor, numel, shape):
        self.c, self.numel, self.shape = compressor, numel, shape
        self.nbytes = sign_section_bytes(numel)


class MaureyCodec(_SparseCodec):
    """MaureySparsification on the HIP kernels (libgq_maurey.so).  Wire per tensor: a 16-byte header (scale = ||w||_1 / k as
    f32, 12 zero bytes), then k little-endian uint32 words  index | (w_index < 0) << 31, ascending by index (an index drawn m
    times appears m times), zero padding to 16 bytes -- 16 + _up(4k) bytes.  Every call is a one-tensor BatchedMaurey; roundtrip /
    encode_decode_into return the compress launches' own dense decode.
    The draws, by the compressor's gq_rng: "device" -- the library's counter-based generator, a fresh seed per call (the
    multi-tensor launches key theirs by the quantizer's { seed, step } words); "reference" -- torch.rand(k) per tensor from the
    CPU generator, in parameter order, handed to the kernels as given draws.  That is ONE uniform per draw, not the reference's
    k x n matrix (maurey_sparsification.py:28), so the draws are not the reference's; "keyed" draws like "device".
    `r` (float32 [k] on the device) hands a call its uniforms whatever the mode; `seed` pins the device generator's."""

    def __init__(self, compressor, numel, shape):
        self.c, self.numel, self.shape = compressor, numel, shape
        self.k = int(compressor.k)
        if self.k < 1 or not 1 <= numel < 2 ** 31:
            raise ValueError("MaureyCodec: k = %d draws for a tensor of %d elements" % (self.k, numel))
        self.nbytes = native.MAUREY_HEADER_BYTES + _up(4 * self.k)
        self._rng = getattr(compressor, "_rng", "device")

    def uses_reference_draws(self):
        return self._rng == "reference"

    def draw_count(self):
        return self.k

    def encode_into(self, grad, wire_user, off, salt, r=None, seed=None, out=None):
        _SparseCodec.encode_into(self, grad, wire_user, off, salt, draws=self._draws(r, grad.device), seed=seed, out=out)


def mx_section_bytes(numel, fmt):
    """Bytes of one tensor's section of the microscaling wire (include/gq_mx.h): ceil(numel / 32) scale bytes, 16-byte aligned,
    then 16 (fp4), 24 (fp6_e2m3 / fp6_e3m2) or 32 (fp8) code bytes per block, zero bytes up to a multiple of 16 (fp6 with an odd
    number of blocks: 8).  fmt: a name of native.MX_FORMATS or its id."""
    fmt = native.MX_FORMATS.get(fmt, fmt)
    nb = -(-numel // native.MX_BLOCK)
    return _up(nb) + _up(nb * native.MX_BLOCK * native.MX_CODE_BITS[fmt] // 8)


class MXCodec(_SparseCodec):
    """MXCompressor on the HIP kernels (libgq_mx.so).  Wire per tensor: the blocks' scale bytes (E8M0, padded to 16 bytes), then
    one FP4 code per element, element 2i in the low nibble, one FP8 byte, or one FP6 code (element i in bits 6i .. 6i+5 of its
    block's 24 bytes) -- mx_section_bytes.  The wire carries the decoded
    tensor exactly (-0, and NaN for a block that held an infinity or a NaN), so ring mode ships it as it is.  Every call is a
    one-tensor BatchedMX; roundtrip / encode_decode_into return the compress launch's own dense decode.
    The draws (compressor.random; otherwise the rounding is to nearest-even and there are none), by the compressor's gq_rng:
    "device" -- the library's counter-based generator, a fresh seed per call (the multi-tensor launch keys its stream by the
    quantizer's { seed, step } words); "reference" -- torch.rand(numel) per tensor from the CPU generator, in parameter order,
    handed to the kernels as given draws; "keyed" draws like "device".
    `r` (float32 [numel] on the device) hands a call its uniforms whatever the mode; `seed` pins the device generator's.
    dtype: torch.float32 or torch.bfloat16 -- what the gradients are and what every decode returns (include/gq_mx.h, TENSOR-SIDE
    TYPE).  The wire and its bytes do not depend on it; error buffers are float32 either way."""

    def __init__(self, compressor, numel, shape, dtype=torch.float32):
        self.c, self.numel, self.shape = compressor, numel, shape
        if numel < 1:
            raise ValueError("MXCodec: a tensor of %d elements" % numel)
        self.set_dtype(dtype)
        self.format = native.MX_FORMATS[compressor.format]
        self.random = bool(compressor.random)
        self.nbytes = mx_section_bytes(numel, self.format)
        self._rng = getattr(compressor, "_rng", "device")

    def uses_reference_draws(self):
        return self.random and self._rng == "reference"

    def draw_count(self):
        return self.numel

    def set_dtype(self, dtype):
        """(the quantizers: a codec factory is not told the parameter's dtype)"""
        if dtype not in native.MX_DTYPES:
            raise TypeError("%s: the kernels take float32 or bfloat16 tensors, got %s" % (type(self).__name__, dtype))
        self.dtype, self._single = dtype, None

    def encode_into(self, grad, wire_user, off, salt, r=None, seed=None, out=None, err=None, ef_scale=None):
        """err, ef_scale: error feedback in the same launch -- grad <- w = grad + ef_scale * err (narrowed where grad is bfloat16),
        err <- w - decoded from the unrounded w.  err: float32, contiguous, of grad's size; grad must then be contiguous itself."""
        errs = self._errs_of(grad, err, "MXCodec")      # (in front of the draws: a refused call takes none from the generator)
        _SparseCodec.encode_into(self, grad, wire_user, off, salt, draws=self._draws(r, grad.device), seed=seed, out=out, errs=errs,
                                 ef_scale=ef_scale)


class MXRCodec(MXCodec):
    """MXCompressor with mx_rotate = 'hadamard' on libgq_mxr.so (include/gq_mxr.h): MXCodec's wire, bytes and draw rules over the
    tensor rotated in blocks of 256 by H * diag(signs) / 16; every decode ends with the inverse rotation, so the wire no longer
    carries the decoded tensor itself.  Every call is a one-tensor BatchedMXR."""

    def __init__(self, compressor, numel, shape, dtype=torch.float32):
        MXCodec.__init__(self, compressor, numel, shape, dtype)
        self.signs = tuple(int(w) for w in compressor.rotate_signs)


def drive_section_bytes(numel):
    """Bytes of one tensor's section of the DRIVE wire (include/gq_drive.h): ceil(numel / 256) blocks of 32 code bytes, then one f32
    scale per block, zero bytes up to a multiple of 16."""
    nb = -(-numel // native.DRIVE_BLOCK)
    return nb * (native.DRIVE_BLOCK // 8) + _up(4 * nb)


class DriveCodec(_SparseCodec):
    """DriveCompressor on the HIP kernels (libgq_drive.so).  Wire per tensor: the sign bit of every coordinate of the rotated
    256-element blocks (the last block zero-padded), then one f32 scale per block -- drive_section_bytes, 1.125 bits per element.
    The decode ends with an inverse rotation, so the wire does not carry the decoded tensor itself.  No draws.  Every call is a
    one-tensor BatchedDrive; roundtrip / encode_decode_into return the compress launch's own dense decode.
    stepped (the compressor's rotation is 'step'): `rotation`, the device { seed, step } pair a quantizer hands the codec, goes
    to every launch (include/gq_drive.h: SIGNS, STEPPED).  Without a pair -- a codec used on its own -- the launches are the fixed
    ones under the seed's words, which is step 0.
    own (the compressor's user_rotation is 'own'; include/gq_drive.h: SIGNS, PER STREAM): the codec's launches are the *_streams
    ones -- a compress under `stream` (which the quantizer sets: the payload's place in the mean; 0 on its own), a decode-mean that
    rotates payload r back under stream r.  They need a pair in either rotation mode: the quantizer's, or on its own one the codec
    makes at (seed, step 0)."""

    rotation = None      # the { seed, step } pair (device int64 [1, 2]) of a stepped or `own` codec inside a quantizer
    stream = 0           # own: the stream of the next compress

    _SCALES = native.DRIVE_SCALES      # the compressor's `scale` -> the descriptor's scale_mode

    def __init__(self, compressor, numel, shape):
        self.c, self.numel, self.shape = compressor, numel, shape
        if numel < 1:
            raise ValueError("%s: a tensor of %d elements" % (type(self).__name__, numel))
        self.scale_mode = self._SCALES[compressor.scale]
        self._rotation_of(compressor)
        self.nbytes = self._section_bytes()

    def _section_bytes(self):
        return drive_section_bytes(self.numel)

    def _rotation_of(self, compressor):
        self.signs = tuple(int(w) for w in compressor.signs)
        self.stepped = getattr(compressor, "rotation", "fixed") == "step"
        self.own = getattr(compressor, "user_rotation", "shared") == "own"
        self.seed = getattr(compressor, "seed", None)

    def _batched1(self, dev):
        grp = _SparseCodec._batched1(self, dev)
        grp.rotation = self.rotation      # (the quantizer's pair, or None: step 0)
        grp.stream_base = self.stream     # (a one-tensor group records into slot 0)
        return grp

    def encode_into(self, grad, wire_user, off, salt, out=None, err=None, ef_scale=None):
        """err, ef_scale: error feedback in the same launch -- grad <- w = grad + ef_scale * err, err <- w - decoded.  err: float32,
        contiguous, of grad's size; grad must then be contiguous itself."""
        _SparseCodec.encode_into(self, grad, wire_user, off, salt, out=out, errs=self._errs_of(grad, err, "DriveCodec"), ef_scale=ef_scale)


def eden_section_bytes(numel, bits):
    """Bytes of one tensor's section of the EDEN wire (include/gq_eden.h): ceil(numel / 256) blocks of 32 * bits code bytes, then one
    f32 scale per block, zero bytes up to a multiple of 16."""
    if bits not in native.EDEN_BITS:
        raise ValueError("eden_bits must be 2, 3 or 4, got %r" % (bits,))
    nb = -(-numel // native.EDEN_BLOCK)
    return nb * (native.EDEN_BLOCK * bits // 8) + _up(4 * nb)


class EdenCodec(DriveCodec):
    """EdenCompressor on the HIP kernels (libgq_eden.so).  Wire per tensor: a `bits`-bit code (the nearest Lloyd-Max centroid of
    N(0, 1), sign on top) for every coordinate of the rotated 256-element blocks (the last block zero-padded), then one f32 scale per
    block -- eden_section_bytes, bits + 0.125 bits per element.  Otherwise DriveCodec: the decode ends with an inverse rotation, no
    draws, every call is a one-tensor BatchedEden."""

    _SCALES = native.EDEN_SCALES

    def __init__(self, compressor, numel, shape):
        self.bits = int(compressor.bits)
        DriveCodec.__init__(self, compressor, numel, shape)

    def _section_bytes(self):
        return eden_section_bytes(self.numel, self.bits)


_DATA_PTR = torch.Tensor.data_ptr
_IS_CONTIGUOUS = torch.Tensor.is_contiguous
_DTYPE_OF = operator.attrgetter("dtype")
_GET_DEVICE = torch.Tensor.get_device      # the device index (-1 for a CPU tensor)
_F32_ONLY = {torch.float32}


class _BatchedBase(object):
    """Shared plumbing of the multi-tensor kernels: a per-step header (segment table with the
    tensors' current device pointers, plus kernel-specific reset values) goes to the device in ONE
    pinned H2D copy; a ring of pinned buffers keeps a copy in flight from being overwritten."""

    UPLOAD_RING = 8
    # what a group's launches read and write: the gradients' (and the dense-copy sources') dtype -- `dtype`, as a set in `_dtypes`
    # for the upload's check -- and the alignment of the dense-copy sources.  Error buffers are float32 in every group.
    dtype, _dtypes, _dense_align = torch.float32, _F32_ONLY, 4

    def _setup(self, table, extra, device, slots, user_bytes, dense=None):
        """dense: [(byte offset in one user's wire, elements), ...] of the identity-compressed tensors this group's compress
        launch also copies into the wire (the quantizer gives them to its first group), or None."""
        self.nseg = table.shape[0]
        self.device = device
        self.user_bytes = user_bytes
        self._table_words = self.nseg * 8
        host = torch.cat([table.view(-1), extra.view(-1)]) if extra is not None else table.view(-1).clone()
        self.ndense = len(dense) if dense else 0
        self._dense_at = int(host.numel())      # the dense table's first word in the header
        if self.ndense:
            dt = torch.zeros((self.ndense, 3), dtype=torch.int64)
            for k, (off, numel) in enumerate(dense):
                dt[k, 1], dt[k, 2] = off, numel
            host = torch.cat([host, dt.view(-1)])
        # a ring of pinned copies of the header: an upload rewrites the OLDEST one, so the copy it has to wait for was queued
        # UPLOAD_RING uploads ago (round 6: indexed by the user slot, a one-user training loop rewrote the same buffer every step
        # and waited for the previous step's copy -- the host could never run ahead of the device)
        self._host = [host.clone().pin_memory() for _ in range(max(slots + 1, self.UPLOAD_RING))]
        self._up_turn = 0
        self._host_np = [h[:self._table_words].view(self.nseg, 8).numpy() for h in self._host]   # views of the pinned tables
        self._host_dense_np = [h[self._dense_at:].view(self.ndense, 3).numpy() for h in self._host] if self.ndense else None
        self._last_dptrs = None
        self._zeros = [0] * self.nseg
        self._resets = extra is not None    # the header also carries per-step reset values (min / max accumulators)
        self._acc_init = extra.view(-1).to(device) if extra is not None else None     # the accumulators' empty state, on the device
        self._acc_clean = False             # the device accumulators are in that state right now (see _graph_tables)
        self._last_ptrs = self._last_eptrs = None
        self._events = [None] * len(self._host)
        self._dev = torch.empty_like(host, device=device)
        self._tmp_wire = None
        self.ready = False      # the device header has been written at least once
        self._outs, self._out_views, self._out_turn = [None, None], [None, None], 0
        self._out_gen = 0               # output-buffer allocations so far (PSQuantizer._apply_key_for remembers the buffers' addresses per count)
        self._layout = table.clone()    # host copy of the segment table without pointers (decode needs no pointers)
        self._parts = {}                # (first tensor, end) -> launch descriptor of one chunk of a split / pipelined decode
        self.rng_pairs = None           # this group's { seed, step } pairs, one per user slot (PSQuantizer._rng_pairs_for)

    def _out_buffer(self, device, advance=True):
        """Decode target + its per-tensor views.  Two buffers used in turn (the mean and its two-phase
        re-decode never alias; last step's gradients stay intact for one more apply) and the 76+
        slice/view objects of a model are built once instead of every step.  advance=False: the buffer
        of the previous call again (second part of a split decode)."""
        if not advance:
            k = self._out_turn ^ 1
            return self._outs[k], self._out_views[k]
        k = self._out_turn
        self._out_turn ^= 1
        if self._outs[k] is None or self._outs[k].device != device:
            out = torch.empty(self.out_floats, dtype=self.dtype, device=device)
            self._outs[k] = out
            self._out_views[k] = [out[o:o + cd.numel].view(cd.shape) for o, cd in zip(self.out_off, self.codecs)]
            self._out_gen += 1
        return self._outs[k], self._out_views[k]

    def dense_table_dev(self):
        return self._dev[self._dense_at:].view(self.ndense, 3) if self.ndense else None

    # ---- launches under stream capture: a graph's own tables, accumulators reset behind their last reader -----------------
    # A captured record reads the segment / dense tables from a device copy that belongs to the graph (nobody rewrites
    # it), so a replay needs no header copy in front of the encode -- any node there, memcpy or kernel, cost ~7 us of every
    # step (profiles/r04_graph_pieces.txt).  What the header copy also did, resetting the accumulators the kernels fold into
    # ((min, max) per tensor; wide QSGD buckets' norms), is a small kernel BEHIND the group's last launch instead: a graph
    # leaves them clean for the next replay, an eager step leaves them used (`_acc_clean`), and whoever replays a graph
    # after an eager step cleans them first (ensure_clean).
    def _graph_tables(self, graph_header, dense):
        self._batch.set_table(graph_header[:self._table_words])
        self._batch.set_dense(graph_header[self._dense_at:].view(self.ndense, 3) if (dense is not None and self.ndense) else None,
                              self.ndense)

    def _graph_tables_done(self, defer=None):
        """defer (a list): the reset is left to the caller -- (accumulators, their empty state) is appended -- who folds it
        into a launch that runs anyway behind this group's last one (the aggregate's gq_mean_rows in a whole-step graph)."""
        if self._resets:
            if defer is not None:
                defer.append((self._dev[self._table_words:self._dense_at], self._acc_init))
            else:
                _kernel_copy(self._dev[self._table_words:self._dense_at], self._acc_init)
        self._batch.set_table(self._dev[:self._table_words])

    def _choose_header(self, tensors, slot, align, errs, dense, graph_header, table_current):
        """Where an encode's launches read their tables from.  graph_header (stream capture): a device copy of the header of
        exactly these tensors that nobody rewrites (no events, no validation: the caller has just run the same call eagerly).
        table_current (capture of an ADDRESS-FREE graph, PSQuantizer._capture_generic): the shared device header as it is, which
        the caller refreshes by upload() in front of every replay -- pointers and accumulator resets -- as an eager step does.
        Otherwise the shared header, with these tensors' pointers sent to it now; False -- nothing changed, nothing to launch
        -- when a tensor cannot be addressed that way."""
        if graph_header is not None:
            self._graph_tables(graph_header, dense)
            return True
        if table_current:
            self._batch.set_table(self._dev[:self._table_words])
        elif not self._upload(tensors, slot, align, errs, dense):
            return False
        else:
            self._acc_clean = False
        self._batch.set_dense(self.dense_table_dev() if dense is not None else None, self.ndense)
        return True

    def _launch(self, graph_header, defer_reset, launches, *args):
        """launches(*args) -- an encode's launches behind _choose_header -- with the descriptor taken back from a graph's own
        tables behind them: _graph_tables_done, or graph_tables_abort when one of them raised."""
        try:
            launches(*args)
        except BaseException:
            if graph_header is not None:
                self.graph_tables_abort()
            raise
        if graph_header is not None:
            self._graph_tables_done(defer_reset)

    def graph_tables_abort(self):
        """A launch failed between _graph_tables and _graph_tables_done (an invalidated capture, a launch error): the callers
        fall back to eager launches, which must not read their pointers from the graph's header.  The descriptor goes back to
        the shared device header and the next eager encode re-validates and re-sends it (no reset kernel: the stream may be
        in a broken capture; `_acc_clean = False` makes the next replay clean the accumulators first).  A level launch left
        for the capture's decode (encode(..., skip_levels=True)) is dropped."""
        self._batch.set_table(self._dev[:self._table_words])
        self._batch.set_dense(self.dense_table_dev(), self.ndense)
        self._last_ptrs = self._last_eptrs = self._last_dptrs = None
        self._acc_clean = False
        self._pending_levels = None

    _pending_levels = None      # (BatchedHSQ.encode(..., skip_levels=True): the launch levels_decode still has to make)

    def after_replay(self, decoded, table_replaced):
        """What a replayed graph leaves behind.  decoded: it decoded into the next output buffer.  table_replaced: it read its
        own table, not the last upload's pointers in the device header -- the next eager encode re-sends them."""
        if decoded:
            self._out_turn ^= 1
        if table_replaced:
            self._last_ptrs = None

    def set_out_turn(self, turn):      # (a capture re-issues an eager call's launches, then puts the turn back)
        self._out_turn = turn

    def ensure_clean(self):
        if self._resets and not self._acc_clean:
            _kernel_copy(self._dev[self._table_words:self._dense_at], self._acc_init)
            self._acc_clean = True

    def _upload(self, tensors, slot, align, errs=None, dense=None):
        """Column 0 of the segment table <- the tensors' device pointers; column 7 <- the error
        buffers' (error-feedback kernels) or 0.  False if any tensor cannot be addressed that way.
        A header that also carries the reset values of the kernels' min / max accumulators (HSQ, wide-bucket QSGD)
        goes to the device every time; when the pointers are the ones of the last upload (gradients that keep their storage from
        step to step) the pinned copy is sent as it is, without checking and rewriting the table."""
        ptrs = list(map(_DATA_PTR, tensors))
        eptrs = list(map(_DATA_PTR, errs)) if errs is not None else self._zeros
        dptrs = list(map(_DATA_PTR, dense)) if dense is not None else None
        # the fast path still checks what the kernels assume about every tensor: a gradient replaced by a strided view or
        # another dtype AT THE SAME ADDRESS (channels_last, the caching allocator handing the block out again) must not
        # ride on the last upload's validation.  (map() over the C-level accessors: ~6 us for 76 tensors; a Python-level
        # list of (dtype, is_contiguous) tuples cost 20.)
        if (self.ready and ptrs == self._last_ptrs and eptrs == self._last_eptrs and dptrs == self._last_dptrs
                and all(map(_IS_CONTIGUOUS, tensors)) and set(map(_DTYPE_OF, tensors)) == self._dtypes
                and (dense is None or (all(map(_IS_CONTIGUOUS, dense)) and set(map(_DTYPE_OF, dense)) == self._dtypes))):
            if not self._resets:
                return True     # nothing but the table in this header, and the device copy still holds it
            self._dev.copy_(self._host[self._last_slot], non_blocking=True)     # unchanged since its last copy
            self._events[self._last_slot].record()     # a later rewrite of this pinned buffer waits for this copy too
            return True
        # (the same facts for a new set of pointers, from the C-level accessors: a Python loop over
        # `g.device != ... or g.dtype != ...` cost 40 us for 76 tensors, most of it building torch.device objects)
        dev_index = self.device.index if self.device.index is not None else torch._C._cuda_getDevice()
        for ts, ps, al, dts in ((tensors, ptrs, align, self._dtypes), (errs or (), eptrs if errs is not None else (), max(align, 4), _F32_ONLY),
                                (dense or (), dptrs or (), self._dense_align, self._dtypes)):
            if not ts:
                continue
            if (not all(map(_IS_CONTIGUOUS, ts)) or set(map(_DTYPE_OF, ts)) != dts
                    or set(map(_GET_DEVICE, ts)) != {dev_index} or any(p % al for p in ps)):
                return False
        if dense is not None and len(dense) != self.ndense:
            return False
        if len(eptrs) != len(ptrs):
            return False
        slot = self._up_turn      # (the user slot plays no part: any pinned buffer whose last copy is done will do)
        self._up_turn = (slot + 1) % len(self._host)
        if self._events[slot] is not None:
            self._events[slot].synchronize()       # the previous copy out of this pinned buffer (UPLOAD_RING uploads ago)
        tab = self._host_np[slot]
        tab[:, 0] = ptrs
        tab[:, 7] = eptrs
        if dptrs is not None:
            self._host_dense_np[slot][:, 0] = dptrs
        self._dev.copy_(self._host[slot], non_blocking=True)
        self.ready = True
        self._last_ptrs, self._last_eptrs, self._last_slot, self._last_dptrs = ptrs, eptrs, slot, dptrs
        if self._events[slot] is None:
            self._events[slot] = torch.cuda.Event()
        self._events[slot].record()
        return True

    def upload(self, tensors, slot, errs=None, dense=None):
        """The header of these tensors to the device (pointers, accumulator resets, dense copy table), as the eager encode sends
        it -- in front of the replay of an address-free graph.  False: a tensor cannot be addressed that way."""
        if not self._upload(tensors, slot, self.align, errs, dense):
            return False
        self._acc_clean = False
        return True

    def _counter_seed(self, slot, reserved=False):
        """GQ_RANDOM_DEVICE_COUNTER: the address of this group's { seed, step } pair of user slot `slot`, or None when the
        quantizer gave the group no pairs (a codec used on its own) or not enough of them.  The LAST pair is reserved for the
        two-phase re-compress (its seed is the same on every rank): a record() of a user slot that high gets None -- a fresh
        per-call seed -- unless the caller asks for the reserved pair by name (reserved=True)."""
        if self.rng_pairs is None or not 0 <= slot < self.rng_pairs.shape[0] - (0 if reserved else 1):
            return None
        return self.rng_pairs.data_ptr() + 16 * slot

    def _range(self, lo, hi):
        """Launch descriptor of the tensors [lo, hi) of the group (one chunk of a split / pipelined decode, PSQuantizer.apply
        under GQ_EXCHANGE=split|pipelined).  lo == 0: the same device table, fewer items; otherwise a table of its own, built
        once (segment and item indices restart at zero).  None when the range is empty."""
        if lo >= hi:
            return None
        ent = self._parts.get((lo, hi))
        if ent is None:
            i_lo = int(self._layout[lo, 2])
            i_hi = int(self._layout[hi, 2]) if hi < self.nseg else self._nitems
            if lo == 0:
                ent = self._batch.part(self._dev[:self._table_words], self._item_seg, hi, i_hi)
            else:
                tab = self._layout[lo:hi].clone()
                tab[:, 2] -= i_lo
                items = (self._item_seg[i_lo:i_hi] - lo).contiguous()
                ent = self._batch.part(tab.view(-1).to(self.device), items, hi - lo, i_hi - i_lo)
            self._parts[(lo, hi)] = ent
        return ent

    def decode_mean(self, gathered, R, part=None, plain=False, tail=None):
        """Mean of the R payloads of `gathered` for every tensor of the group (views of one output buffer).
        part = (lo, hi, first): only the tensors [lo, hi) of the group -- the chunks of a split / pipelined exchange land in
        the same buffer, `first` on the first of them (it takes the next output buffer, the others write into it too).
        plain: the decompress of ONE payload as the reference returns it (a -0 stays -0) instead of the aggregate."""
        if not self.ready:      # a rank that decodes before it has encoded anything (ring hop, late joiner)
            self.upload_layout()
        out, views = self._out_buffer(gathered.device, advance=part is None or part[2])
        batch = self._batch if part is None else self._range(part[0], part[1])
        if batch is not None:
            kw = self._rotation_kw()
            if tail is not None:
                kw["tail"] = tail      # (BatchedHSQ only: see takes_tail)
            if getattr(self, "fma", False) and R >= 2 and not plain:
                batch.decode(gathered, R, out, fma=True, **kw)      # (BatchedHSQ only: the quantizer sets `fma` on its HSQ groups)
            else:
                batch.decode(gathered, R, out, plain=plain, **kw)
        return views

    takes_tail = False      # the group's decode-mean launch can take the aggregate's small per-step work along (native.StepTail)
    rotation = None         # BatchedDrive / BatchedEden in step mode: the quantizer's { seed, step } pair, read by every launch
    own = False             # BatchedDrive / BatchedEden under user_rotation = 'own': the *_streams launches (they read the pair too)

    def _rotation_kw(self):
        """The decode launch's keywords for `rotation` and `own` (two attribute reads for every other group): the pair of step
        mode, or under 'own' the pair and first stream 0 -- payload r of the gather under stream r."""
        if self.own:
            return {"rotation": self._pair(), "first_stream": 0}
        return {"rotation": self.rotation} if self.rotation is not None else {}

    def upload_layout(self):
        """Device header with the layout columns only (no tensor pointers): enough for decode_mean,
        which a ring rank may need before it has encoded anything."""
        self._last_ptrs = self._last_eptrs = self._last_dptrs = None
        self._dev.copy_(self._host[0], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._events[0] = ev
        self.ready = True

    def roundtrip(self, tensors, slot, salt, errs=None, ef_scale=None, draws=None, rng_slot=None, graph_header=None, defer_reset=None):
        """decompress(compress(t)) for every batched tensor in a few launches; None if not batchable.
        With `errs`: t <- t + ef_scale*err in place first and err <- t - decoded afterwards.
        rng_slot: the { seed, step } pair the stochastic rounding draws from (default: the one of `slot`).
        graph_header, defer_reset (stream capture of a two-phase apply): see encode."""
        if self._tmp_wire is None:
            self._tmp_wire = torch.zeros((1, self.user_bytes), dtype=torch.uint8, device=self.device)
        kw = {"graph_header": graph_header, "defer_reset": defer_reset} if graph_header is not None else {}
        if not self.encode(tensors, self._tmp_wire[0], slot, salt, errs, ef_scale, draws=draws, rng_slot=rng_slot, **kw):
            return None
        return self.decode_mean(self._tmp_wire, 1, plain=True)     # decompress(compress(t)) (ps_quantizer.py:52-61): a -0 stays -0


class BatchedHSQ(_BatchedBase):
    """All NearestNeighborCompressor tensors that share a codebook are encoded by ONE encode + ONE levels
    launch and decoded by ONE decode-mean launch (per-tensor lb / ub, identical results).  The reference
    walks the parameter list in Python (ps_quantizer.py:33,47); ResNet-50 has 76 such tensors.
    The library decides which kernels serve the group's shape (include/gq_hsq.h, gq_hsq_batched_path): K <= 256 with
    d = 8 / 16 / 32 and byte-sized codes the prefilter encode and the specialised levels / decode kernels, larger
    codebooks of those dimensions the paged prefilter, every other shape exact scoring."""

    takes_tail = True      # gq_hsq_decode_sum_batched_tail

    @staticmethod
    def eligible(codec):
        c = getattr(codec, "c", None)
        if type(codec) is not HSQCodec or c.K == c.dim:   # K == d: a random codebook per tensor
            return False
        return native.hsq_batched_path(c.dim, c.K, codec.code_dtype) != 0

    @staticmethod
    def group_key(codec):
        return (codec.c.dim, codec.c.K, _esize(codec.code_dtype), _esize(codec.level_dtype), int(codec.c.n_bit), int(codec.packed6))

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        self.idxs = list(idxs)
        self.codecs = [codecs[i] for i in self.idxs]
        c0 = self.codecs[0].c
        self.n_bit = c0.n_bit                                  # 32: the projections travel as f32 (no level quantiser)
        self.random = bool(c0.compressed_norm and c0.norm_compressor.random)
        self.keyed = bool(self.random and c0.norm_compressor._rng == "keyed")   # draws keyed by (lb, ub): a launch that never changes
        self.counter = bool(self.random and c0.norm_compressor._rng == "device")  # draws keyed by a device step word: likewise, and fresh every step
        self.reference_draws = self.codecs[0].uses_reference_draws()     # the reference's CPU draws, handed in per record
        # ... for the level quantiser.  Here the two are one fact; BatchedPVQ's sampler draws also when the levels are
        # deterministic or travel as f32, so there `reference_draws` (the record needs draws) can hold without this one
        self.level_reference = bool(self.random and c0.norm_compressor._rng == "reference")
        self._r_gather = {}
        self.codebook = c0._codebook_on(device)
        nseg = len(self.idxs)
        table = torch.zeros((nseg, 8), dtype=torch.int64)
        tile_seg = []
        tile, out_off = 0, 0
        self.out_off = []
        for s, (i, cd) in enumerate(zip(self.idxs, self.codecs)):
            ntile = (cd.M + 63) // 64
            table[s, 1], table[s, 2] = cd.M, tile
            table[s, 3] = offsets[i] + cd.codes_off
            table[s, 4] = offsets[i] + cd.levels_off
            table[s, 5] = offsets[i] + cd.lbub_off
            table[s, 6] = out_off
            tile_seg += [s] * ntile
            tile += ntile
            self.out_off.append(out_off)
            out_off += cd.numel
        self.ntiles, self.out_floats = tile, out_off
        self.tile_seg = torch.tensor(tile_seg, dtype=torch.int32, device=device)
        self._item_seg, self._nitems = self.tile_seg, tile
        init = torch.empty((nseg, 2), dtype=torch.int32)
        init[:, 0], init[:, 1] = -1, 0            # 0xFFFFFFFF / 0: identities of the mapped min / max
        self._setup(table, init.view(torch.int64), device, slots, user_bytes, dense)
        self.u_flat = torch.empty(self.ntiles * 64, dtype=torch.float32, device=device)
        cd0 = self.codecs[0]
        self.code_dtype, self.level_dtype = cd0.code_dtype, cd0.level_dtype
        self.align = 16 if c0.dim % 4 == 0 else 4
        self.ws = native.new_workspace(device, self.ntiles * 64)
        # ONE launch descriptor for the group (gq_hsq_batch): the library picks the kernels -- prefilter (K <= 256,
        # d = 8 / 12 / 16 / 24 / 32), the same with the pages of a larger codebook resident, or exact scoring for every other shape
        self._batch = self._new_batch(cd0)
        self.profile_slot = -1      # measurement hook (bench.py): the NEXT encode's dispatch is timed into this slot

    def _new_batch(self, cd0):
        return native.HSQBatch(self._dev[:self._table_words], self.tile_seg, self.nseg, self.ntiles, self.codebook,
                               self.code_dtype, cd0.wire_level_kind(), self.n_bit, self.u_flat,
                               self._dev[self._table_words:self._dense_at].view(torch.int32), self.ws)

    def _given_draws(self, draws, which=0):
        """draws = (r_all on the device, {parameter index: offset of its draws}): the reference's
        torch.rand(M) per tensor, drawn by the quantizer in ONE call per record.  Laid out like u_flat for
        the kernels (one gather through an index built once).  which: the tensor's first (0) or second (1) run of M draws
        (BatchedPVQ: the codeword draws, then the level draws)."""
        r_all, offsets = draws
        ent = self._r_gather.get(which)
        if ent is None:
            idx = torch.zeros(self.ntiles * 64, dtype=torch.int64)
            for s, (i, cd) in enumerate(zip(self.idxs, self.codecs)):
                first = int(self._layout[s, 2]) * 64
                idx[first:first + cd.M] = torch.arange(offsets[i] + which * cd.M, offsets[i] + (which + 1) * cd.M)
            ent = self._r_gather[which] = (idx.to(self.device), torch.empty(self.ntiles * 64, dtype=torch.float32, device=self.device))
        torch.index_select(r_all, 0, ent[0], out=ent[1])
        return ent[1]

    _level_draw_run = 0      # which run of a tensor's reference draws the level quantiser takes

    def _launch_encode(self, wire_user, ef, salt, counter_seed, draws):
        self._batch.encode(wire_user, ef, self.profile_slot)
        self.profile_slot = -1

    def _level_draws(self, salt, counter_seed, draws):
        """(random_mode, seed, r_flat) of the level launch."""
        if self.n_bit == 32 or not self.random:
            return native.RANDOM_OFF, 0, None
        if self.level_reference:
            return native.RANDOM_GIVEN, 0, self._given_draws(draws, self._level_draw_run)
        if self.keyed:
            return native.RANDOM_DEVICE_KEYED, (salt * 0x2545F4914F6CDD1D + 0x5851F42D4C957F2D) & (2 ** 63 - 1), None
        if self.counter and counter_seed is not None:
            return native.RANDOM_DEVICE_COUNTER, counter_seed, None
        return native.RANDOM_DEVICE, _next_seed() ^ salt, None

    def graphable(self):
        """True when nothing in this group's launches changes from record to record for fixed gradient addresses (no
        per-call seed, no host-side draws): the launches can be nodes of a HIP graph (PSQuantizer, gq_graph)."""
        return (not self.random or self.keyed or (self.counter and self.rng_pairs is not None)) and not self.reference_draws \
            and self._batch.path != 0

    def encode(self, tensors, wire_user, slot, salt, errs=None, ef_scale=None, draws=None, graph_header=None, dense=None, defer_reset=None,
               rng_slot=None, skip_levels=False, table_current=False):
        """Compress `tensors` (one per batched parameter, in order) into one user's wire.
        skip_levels (whole-step capture at one rank and one user): only the encode is launched; the level launch is left to
        decode_mean(..., fused_levels=True), which runs it together with the decode (gq_hsq_levels_decode_batched).
        dense: the identity-compressed tensors (the quantizer's, in its order) that the level launch also copies into the wire.
        Returns False (nothing launched) when a tensor is not a contiguous, 16-byte aligned f32
        tensor on this device: the caller then takes the per-tensor path for this step.
        With `errs` (error feedback, ps_quantizer.py:34-39) the same launches also do
        t += ef_scale*err (in place, before encoding) and err = t - decoded (in place, after).
        graph_header, table_current: see _choose_header."""
        if self.reference_draws and draws is None:
            return False
        if self._batch.path == 0:       # e.g. more than 384 tensors of d = 8 / 32 and no exact kernel for the shape
            return False
        if not self._choose_header(tensors, slot, self.align, errs, dense, graph_header, table_current):
            return False
        ef = ef_scale if errs is not None else None
        counter_seed = self._counter_seed(slot) if rng_slot is None else self._counter_seed(rng_slot, reserved=True)
        try:
            self._launch_encode(wire_user, ef, salt, counter_seed, draws)
            mode, seed, r_flat = self._level_draws(salt, counter_seed, draws)
            if skip_levels:
                self._pending_levels = (wire_user, mode, seed, r_flat, errs is not None)
            else:
                self._batch.levels(wire_user, mode, seed, r_flat, write_error=errs is not None)
        except BaseException:
            if graph_header is not None:
                self.graph_tables_abort()
            raise
        if graph_header is not None and not skip_levels:
            self._graph_tables_done(defer_reset)
        elif graph_header is not None:
            # the level launch is still to come and reads the graph's own tables: the descriptor goes back to the shared header
            # behind it (levels_decode); the accumulators' reset is handed to the caller now -- it rides in that same launch
            if self._resets:
                assert defer_reset is not None, "skip_levels is for the whole-step capture, which folds the resets into its last launch"
                defer_reset.append((self._dev[self._table_words:self._dense_at], self._acc_init))
        return True

    def fusable_levels(self):
        """The level launch and the decode of the one payload can be ONE launch (native.HSQBatch.levels_decode)."""
        c0 = self.codecs[0]
        return (self._batch.path == native.BATCH_PREFILTER and self.n_bit != 32 and not c0.packed6
                and self.level_dtype in (torch.uint8, torch.int16) and not getattr(self, "fma", False))

    def levels_decode(self, plain, tail):
        """The launch encode(..., skip_levels=True) left out + the decode of that payload (+ tail) -> the output views."""
        wire_user, mode, seed, r_flat, write_error = self._pending_levels
        self._pending_levels = None
        out, views = self._out_buffer(wire_user.device)
        try:
            self._batch.levels_decode(wire_user, mode, seed, r_flat, write_error, out, plain=plain, tail=tail)
        except BaseException:
            self.graph_tables_abort()
            raise
        self._batch.set_table(self._dev[:self._table_words])      # (the reset itself rode in the launch: tail.reset)
        return views


class BatchedPVQ(BatchedHSQ):
    """BatchedHSQ for ProbabilisticVectorCompressor tensors: the same wire, tables, level launch, decode-mean (with its step
    tail), fused error-feedback residual and graph machinery; the encode launch is gq_pvq_encode_batched (libgq_pvq.so), which
    projects on c_dagger and SAMPLES the codeword, and the descriptor's codebook -- what the level launch's residual and the
    decode read -- is the compressor's codewords.  The sampler always draws: one uniform per subvector from the compressor's
    gq_rng ("reference": the quantizer's draw plan gives a tensor its codeword draws and then its level draws; "device": the
    group's { seed, step } words, the level launch on another stream of the same words; "keyed": keyed by the subvector's l1).
    Shapes: d in {8, 16, 32}, K = 32 ... 256 in whole blocks of 32, byte codes; every other tensor keeps PVQCodec."""

    _level_draw_run = 1

    @staticmethod
    def eligible(codec):
        c = getattr(codec, "c", None)
        if type(codec) is not PVQCodec or c.K == c.dim:   # K == d: a random codebook per tensor
            return False
        return native.pvq_batched_serves(c.dim, c.K, codec.code_dtype)

    @staticmethod
    def group_key(codec):
        return ("pvq",) + BatchedHSQ.group_key(codec)

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        BatchedHSQ.__init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense)
        rng = self.codecs[0].c._rng
        self.keyed = rng == "keyed"
        self.counter = rng == "device"       # (also without stochastic levels: the sampler's draws)

    def _new_batch(self, cd0):
        self.c_dagger = cd0.c._on(self.device)[1]
        return native.PVQBatch(self._dev[:self._table_words], self.tile_seg, self.nseg, self.ntiles, self.codebook, self.c_dagger,
                               self.code_dtype, cd0.wire_level_kind(), self.n_bit, self.u_flat,
                               self._dev[self._table_words:self._dense_at].view(torch.int32), self.ws)

    def graphable(self):
        return (self.keyed or (self.counter and self.rng_pairs is not None)) and not self.reference_draws and self._batch.path != 0

    def _launch_encode(self, wire_user, ef, salt, counter_seed, draws):
        if self.reference_draws:
            mode, seed, r_flat = native.RANDOM_GIVEN, 0, self._given_draws(draws, 0)
        elif self.keyed:
            mode, seed, r_flat = native.RANDOM_DEVICE_KEYED, (salt * 0x2545F4914F6CDD1D + 0x5851F42D4C957F2D) & (2 ** 63 - 1), None
        elif self.counter and counter_seed is not None:
            mode, seed, r_flat = native.RANDOM_DEVICE_COUNTER, counter_seed, None
        else:
            mode, seed, r_flat = native.RANDOM_DEVICE, _next_seed() ^ salt, None
        self._batch.encode(wire_user, ef, mode, seed, r_flat)


class BatchedResidual(BatchedHSQ):
    """Every ResidualCompressor tensor of a model in four launches per record and one per apply, on BatchedHSQ's tables, header,
    draws and graph machinery.  Two descriptors over one tile space (native.RQBatch): stage 1's, whose table carries the
    pointers, and stage 2's, whose table holds layout only and never changes.  Per record: gq_hsq_encode_batched (with error
    feedback: v = grad + scale * error over grad), gq_hsq_levels_batched (+ the dense tensors' copy), gq_rq_encode2_batched --
    the PVQ walk over v - decode(stage 1), stage 1 read from the wire --, gq_hsq_levels_batched over stage 2; with error feedback
    a fifth launch leaves error = v - ((0 + d1) + d2), the reference's rounding (stage 1's fused residual would be v - d1).  Per
    apply: gq_rq_decode_sum_batched.  The header carries both stages' (min, max) accumulators behind the table.
    Draws: "reference" -- the quantizer's one torch.rand per record gives a tensor up to three runs (ResidualCodec.draw_runs);
    "device" -- the three consumers draw from three streams of the group's { seed, step } words (stage 2's level launch reads
    the words stage 2's encode derives for it); "keyed" as BatchedPVQ."""

    takes_tail = False

    @staticmethod
    def eligible(codec):
        if type(codec) is not ResidualCodec:
            return False
        first = codec.c.compressors[0]
        return first.K != first.dim      # K == d: a random codebook per tensor

    @staticmethod
    def group_key(codec):
        first = codec.c.compressors[0]
        return ("rq", first.dim, first.K, _esize(codec.code_dtype), _esize(codec.level_dtype), int(first.n_bit))

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        self.idxs = list(idxs)
        self.codecs = [codecs[i] for i in self.idxs]
        cd0 = self.codecs[0]
        first, second = cd0.c.compressors
        self.n_bit = first.n_bit
        self.random = bool(first.compressed_norm and first.norm_compressor.random)
        self.keyed = second._rng == "keyed"
        self.counter = second._rng == "device"       # (also without stochastic levels: the sampler's draws)
        self.reference_draws = cd0.uses_reference_draws()
        self.level_reference = bool(self.random and second._rng == "reference")
        self.draw_runs = cd0.draw_runs()
        self._r_gather = {}
        self.codebook = first._codebook_on(device)
        self.codebook2, self.c_dagger = second._on(device)
        if self.codebook2.shape == self.codebook.shape and torch.equal(self.codebook2, self.codebook):
            self.codebook2 = self.codebook      # one file behind both classes: the decode stages ONE image
        nseg = len(self.idxs)
        table = torch.zeros((nseg, 8), dtype=torch.int64)
        table2 = torch.zeros((nseg, 8), dtype=torch.int64)
        tile_seg = []
        tile, out_off = 0, 0
        self.out_off = []
        for s, (i, cd) in enumerate(zip(self.idxs, self.codecs)):
            ntile = (cd.M + 63) // 64
            for tab, st, o in ((table, cd.s1, offsets[i]), (table2, cd.s2, offsets[i] + cd.stage2_off)):
                tab[s, 1], tab[s, 2] = cd.M, tile
                tab[s, 3], tab[s, 4], tab[s, 5] = o + st.codes_off, o + st.levels_off, o + st.lbub_off
                tab[s, 6] = out_off
            tile_seg += [s] * ntile
            tile += ntile
            self.out_off.append(out_off)
            out_off += cd.numel
        self.ntiles, self.out_floats = tile, out_off
        self.tile_seg = torch.tensor(tile_seg, dtype=torch.int32, device=device)
        self._item_seg, self._nitems = self.tile_seg, tile
        init = torch.empty((2 * nseg, 2), dtype=torch.int32)      # stage 1's accumulators, then stage 2's
        init[:, 0], init[:, 1] = -1, 0            # 0xFFFFFFFF / 0: identities of the mapped min / max
        self._setup(table, init.view(torch.int64), device, slots, user_bytes, dense)
        self._layout2 = table2.clone()
        self._table2 = table2.view(-1).to(device)
        self.u_flat = torch.empty(self.ntiles * 64, dtype=torch.float32, device=device)
        self.u_flat2 = torch.empty(self.ntiles * 64, dtype=torch.float32, device=device)
        self.level2_words = torch.zeros(2, dtype=torch.int64, device=device)
        self.code_dtype, self.level_dtype = cd0.code_dtype, cd0.level_dtype
        self.align = 16
        self.ws = native.new_workspace(device, self.ntiles * 64)
        acc = self._dev[self._table_words:self._dense_at].view(torch.int32)
        self._batch = native.RQBatch(self._dev[:self._table_words], self._table2, self.tile_seg, self.nseg, self.ntiles, self.codebook,
                                     self.codebook2, self.c_dagger, self.code_dtype, cd0.wire_level_kind(), self.n_bit,
                                     self.u_flat, acc[:2 * nseg], self.ws, self.u_flat2, acc[2 * nseg:], self.level2_words)
        self.profile_slot = -1

    LEVEL2_SALT = 0x9FB21C651E98DF25      # stage 2's level launch where the host picks the seed (keyed draws)

    def graphable(self):
        return (self.keyed or (self.counter and self.rng_pairs is not None)) and not self.reference_draws and self._batch.path != 0

    def fusable_levels(self):
        return False

    def _draws_for(self, consumer, salt, counter_seed, draws):
        """(random_mode, seed, r_flat) of consumer 0 (stage 1's levels), 1 (stage 2's codewords) or 2 (stage 2's levels)."""
        if consumer != 1 and (self.n_bit == 32 or not self.random):
            return native.RANDOM_OFF, 0, None
        if self.reference_draws:
            return native.RANDOM_GIVEN, 0, self._given_draws(draws, self.draw_runs[consumer])
        if self.keyed:
            seed = (salt * 0x2545F4914F6CDD1D + 0x5851F42D4C957F2D) & (2 ** 63 - 1)
            return native.RANDOM_DEVICE_KEYED, (seed ^ self.LEVEL2_SALT) if consumer == 2 else seed, None
        if self.counter and counter_seed is not None:
            # (the encode salts the words' seed itself and leaves stage 2's level launch a seed of its own in level2_words)
            return native.RANDOM_DEVICE_COUNTER, self._batch.level2_seed if consumer == 2 else counter_seed, None
        return native.RANDOM_DEVICE, _next_seed() ^ salt, None

    def encode(self, tensors, wire_user, slot, salt, errs=None, ef_scale=None, draws=None, graph_header=None, dense=None, defer_reset=None,
               rng_slot=None, skip_levels=False, table_current=False):
        """BatchedHSQ.encode's contract (header, capture, error feedback) over the residual compressor's launches."""
        assert not skip_levels, "the fused level + decode launch is BatchedHSQ's (fusable_levels)"
        if self.reference_draws and draws is None:
            return False
        if self._batch.path == 0:
            return False
        if not self._choose_header(tensors, slot, self.align, errs, dense, graph_header, table_current):
            return False
        ef = ef_scale if errs is not None else None
        counter_seed = self._counter_seed(slot) if rng_slot is None else self._counter_seed(rng_slot, reserved=True)
        self._launch(graph_header, defer_reset, self._launches, wire_user, ef, errs is not None, salt, counter_seed, draws)
        return True

    def _launches(self, wire_user, ef, write_error, salt, counter_seed, draws):
        b = self._batch
        b.b1.encode(wire_user, ef)
        mode, seed, r_flat = self._draws_for(0, salt, counter_seed, draws)
        b.b1.levels(wire_user, mode, seed, r_flat)
        mode, seed, r_flat = self._draws_for(1, salt, counter_seed, draws)
        b.encode2(wire_user, mode, seed, r_flat)
        mode, seed, r_flat = self._draws_for(2, salt, counter_seed, draws)
        b.b2.levels(wire_user, mode, seed, r_flat)
        if write_error:      # error = v - ((0 + d1) + d2)  (ps_quantizer.py:37-39)
            b.decode(wire_user.view(1, -1), 1, None, mode=native.RQ_ERROR)

    def _range(self, lo, hi):
        if lo >= hi:
            return None
        ent = self._parts.get((lo, hi))
        if ent is None:
            i_lo = int(self._layout[lo, 2])
            i_hi = int(self._layout[hi, 2]) if hi < self.nseg else self._nitems
            if lo == 0:
                ent = self._batch.part(self._dev[:self._table_words], self._table2, self._item_seg, hi, i_hi)
            else:
                tabs = []
                for lay in (self._layout, self._layout2):
                    tab = lay[lo:hi].clone()
                    tab[:, 2] -= i_lo
                    tabs.append(tab.view(-1).to(self.device))
                items = (self._item_seg[i_lo:i_hi] - lo).contiguous()
                ent = self._batch.part(tabs[0], tabs[1], items, hi - lo, i_hi - i_lo)
            self._parts[(lo, hi)] = ent
        return ent


class BatchedQSGD(_BatchedBase):
    """All packed-form QSGD tensors in ONE gq_qsgd_compress_batched / gq_qsgd_decode_sum_batched launch.
    Tensors with WIDE buckets (TernGrad's `--c-dim 0`: the tensor is one bucket; any bucket of WIDE_MIN elements
    or more; see place_lone_buckets) form their own group on the chunked kernels (gq_qsgd_wide_*: bucket norms, codes, decode)."""

    takes_tail = True      # gq_qsgd_decode_sum_batched_tail (the library runs gq_mean_rows behind a decode path without the in-kernel form)
    WIDE_MIN = 1024        # buckets from here on go to the chunked kernels (place_lone_buckets)
    LONE_MIN = 256         # ... and a tensor that is ONE bucket may from here on
    NARROW_MAX = 4096      # the largest bucket the bucketed kernel is asked to walk

    @staticmethod
    def eligible(codec):
        return type(codec) is QSGDCodec and codec.bits != 0

    @staticmethod
    def is_wide(codec):
        return bool(getattr(codec, "_wide", codec.d >= BatchedQSGD.WIDE_MIN))

    @staticmethod
    def group_key(codec):
        return (codec.bits, codec.c.bit, int(BatchedQSGD.is_wide(codec)))

    @staticmethod
    def place_lone_buckets(codecs):
        """Which tensors go to the chunked (wide) kernels -- a chunk of 1,024 elements per wave, the bucket's max in a pass of
        its own -- and which to the bucketed kernel, which gives a bucket to 16 lanes (in registers up to 256 elements; above
        that the 16 lanes walk the bucket twice, an element pair per lane and trip):
          * buckets of at least WIDE_MIN = 1,024 elements are wide (whole chunks; ResNet-50 at c_dim 2048: 0.092 against 0.112 ms
            per step with the bucketed kernel's walk);
          * a tensor that IS one bucket of more than 256 elements joins them when there are wide tensors of its code format
            already, or two such tensors: for the bucketed kernel it is a latency chain, not throughput (TernGrad's
            1,024 ... 4,096-element tensors, ~60 buckets of the ResNet-50 list, kept one launch busy for 100 us: half of the step);
          * but a single wide tensor next to bucketed ones stays with them (up to 4,096 elements): a group of one is not
            batched at all (c_dim 512: the one 1,728-element tensor cost 0.12 ms per step as a group of its own)."""
        lone, wide, narrow = {}, {}, {}
        for cd in codecs:
            if not BatchedQSGD.eligible(cd):
                continue
            cd._wide = cd.d >= BatchedQSGD.WIDE_MIN
            fmt = (cd.bits, cd.c.bit)
            if cd._wide:
                wide.setdefault(fmt, []).append(cd)
            elif cd.Mb == 1 and cd.d > BatchedQSGD.LONE_MIN:
                lone.setdefault(fmt, []).append(cd)
            else:
                narrow.setdefault(fmt, []).append(cd)
        for fmt, cds in lone.items():
            if fmt in wide or len(cds) >= 2:
                for cd in cds:
                    cd._wide = True
                wide.setdefault(fmt, []).extend(cds)
            else:
                narrow.setdefault(fmt, []).extend(cds)
        for fmt, cds in wide.items():
            if len(cds) == 1 and narrow.get(fmt) and cds[0].d <= BatchedQSGD.NARROW_MAX:
                cds[0]._wide = False

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        self.idxs = list(idxs)
        self.codecs = [codecs[i] for i in self.idxs]
        c0 = self.codecs[0]
        self.n_bit, self.bits, self.random = c0.c.bit, c0.bits, bool(c0.c.random)
        self.keyed = bool(self.random and c0.c._rng == "keyed")
        self.counter = bool(self.random and c0.c._rng == "device")
        self.wide = self.is_wide(c0)
        assert all(cd.bits == self.bits and cd.c.bit == self.n_bit and self.is_wide(cd) == self.wide for cd in self.codecs)
        self.align = 8
        nseg = len(self.idxs)
        table = torch.zeros((nseg, 8), dtype=torch.int64)
        item_seg = []
        item, out_off, word = 0, 0, 0
        self.out_off = []
        for s, (i, cd) in enumerate(zip(self.idxs, self.codecs)):
            # items: buckets, or (wide) chunks of native.QSGD_WIDE_CHUNK elements of a bucket
            items = cd.Mb * (-(-cd.d // native.QSGD_WIDE_CHUNK)) if self.wide else cd.Mb
            table[s, 1], table[s, 2] = cd.d, item
            table[s, 3] = offsets[i] + cd.norm_off
            table[s, 4] = offsets[i] + cd.codes_off
            table[s, 5] = out_off
            table[s, 6] = word if self.wide else cd.Mb     # wide: the tensor's first word in norm_bits
            item_seg += [s] * items
            item += items
            word += (cd.Mb + 31) & ~31 if self.wide else 0     # a tensor's norm words start on their own 128-byte line
            self.out_off.append(out_off)
            out_off += (cd.numel + 3) & ~3          # tensors start 16-byte aligned in `out` (dwordx4 stores)
        self.nbuckets, self.out_floats = item, out_off
        self.bucket_seg = torch.tensor(item_seg, dtype=torch.int32, device=device)
        self._item_seg, self._nitems = self.bucket_seg, item
        # wide: max |v| per bucket is folded into words that the per-step header resets to zero
        extra = torch.zeros((word + 1) // 2, dtype=torch.int64) if self.wide else None
        self._setup(table, extra, device, slots, user_bytes, dense)
        # the bucket width most elements have: the bucketed kernels give a bucket d / 8 lanes (4 ... 16)
        by_width = {}
        for cd in self.codecs:
            by_width[cd.d] = by_width.get(cd.d, 0) + cd.numel
        hint = 0 if self.wide else max(by_width, key=by_width.get)
        self._batch = native.QSGDBatch(self._dev[:self._table_words], self.bucket_seg, self.nseg, self.nbuckets, self.n_bit,
                                       self.bits, self.wide,
                                       self._dev[self._table_words:self._dense_at].view(torch.int32) if self.wide else None,
                                       bucket_hint=hint)

    def graphable(self):
        """The compress launch takes a fresh seed per record when it rounds stochastically: only the deterministic form
        can be a HIP graph node (see BatchedHSQ.graphable)."""
        return not self.random or self.keyed or (self.counter and self.rng_pairs is not None)

    def encode(self, tensors, wire_user, slot, salt, errs=None, ef_scale=None, draws=None, graph_header=None, dense=None, defer_reset=None,
               rng_slot=None, table_current=False):
        """With `errs`: error feedback in the same launch (t += ef_scale*err, err = t - decoded, both in place).
        graph_header, table_current: see _choose_header; dense, rng_slot: see BatchedHSQ.encode."""
        counter_seed = self._counter_seed(slot) if rng_slot is None else self._counter_seed(rng_slot, reserved=True)
        if not self._choose_header(tensors, slot, 8, errs, dense, graph_header, table_current):
            return False
        if self.keyed:      # gq_rng = "keyed": every bucket's draws keyed by its norm, the seed never changes
            mode, seed = native.RANDOM_DEVICE_KEYED, (salt * 0x2545F4914F6CDD1D + 0x5851F42D4C957F2D) & (2 ** 63 - 1)
        elif self.counter and counter_seed is not None:      # gq_rng = "device": keyed by the slot's device step word
            mode, seed = native.RANDOM_DEVICE_COUNTER, counter_seed
        else:
            mode = native.RANDOM_DEVICE if self.random else native.RANDOM_OFF
            seed = (_next_seed() ^ salt) if self.random else 0
        self._launch(graph_header, defer_reset, self._batch.compress, wire_user, mode, seed, ef_scale if errs is not None else None)
        return True


def _item_draws(random, given, seed, counter_seed, salt):
    """(mode, seed, r) of an item group's compress: none where the rounding is to nearest; the given uniforms (laid out as the group
    reads them); the caller's seed; the group's { seed, step } pair (its address); a fresh seed per call."""
    if not random:
        return native.RANDOM_OFF, 0, None
    if given is not None:
        return native.RANDOM_GIVEN, 0, given
    if seed is not None:
        return native.RANDOM_DEVICE, int(seed), None
    if counter_seed is not None:
        return native.RANDOM_DEVICE_COUNTER, counter_seed, None
    return native.RANDOM_DEVICE, _next_seed() ^ salt, None


class _ItemGroup(_BatchedBase):
    """What the item-table groups share: a segment table over an item table (native._ItemBatch), a decode-mean without a step tail
    and ONE encode, whose compress also writes the dense decoded tensors where a caller asks for them -- which is what roundtrip
    returns.  What a group may state about its encode: what it refuses (WIRE_ALIGN, reference_draws: _refuses), EF_DENSE,
    _compress_args and, where its launches read one user's state (BatchedDGC, BatchedPowerSGD), _user_state over the state-table cache."""

    takes_tail = False
    align = 4
    WIRE_ALIGN = 1          # the wire's address is a multiple of so many bytes, or encode refuses
    # Error feedback takes its residual from the dense decode, so a record with it needs `out` (the group's own buffer where nobody asked):
    #   True  -- the sparsifiers (top-k, STC, threshold, Maurey): the residual launch subtracts the decoded tensors it finds there;
    #   False -- sign, MX / MXR, DRIVE / EDEN, PowerSGD: the launch that rounds an element (a tile) has its decoded value at hand.
    EF_DENSE = False
    random = counter = reference_draws = False      # the draws (BatchedMaurey, BatchedMX): see _drawn
    _state_tables = None    # {key: (device table, the buffers it names)} of a group whose launches read one user's state

    def _item_setup(self, codecs, offsets, idxs, device, slots, user_bytes, dense, items_of, columns, out_pad):
        """The group's tables and header.  items_of(codec): the items of a tensor; columns: {column of the segment table: its
        value per tensor} beside elements (1), first item (2), wire offset (3) and out offset (5); out_pad: a tensor's views in
        the output buffer start on a multiple of so many floats.  Returns (tensors, items)."""
        self.idxs = list(idxs)
        self.codecs = [codecs[i] for i in self.idxs]
        nseg = len(self.idxs)
        table = torch.zeros((nseg, 8), dtype=torch.int64)
        item_seg = []
        item, out_off = 0, 0
        self.out_off = []
        for s, (i, cd) in enumerate(zip(self.idxs, self.codecs)):
            items = items_of(cd)
            table[s, 1], table[s, 2], table[s, 3], table[s, 5] = cd.numel, item, offsets[i], out_off
            for col, values in columns.items():
                table[s, col] = values[s]
            item_seg += [s] * items
            item += items
            self.out_off.append(out_off)
            out_off += -(-cd.numel // out_pad) * out_pad
        self.out_floats = out_off
        self.item_seg = torch.tensor(item_seg, dtype=torch.int32, device=device)
        self._item_seg, self._nitems = self.item_seg, item
        self._setup(table, None, device, slots, user_bytes, dense)
        self._ef_out = None
        return nseg, item

    def graphable(self):
        return True

    def _ef_buffer(self, device):
        """The decoded tensors an error-feedback record needs and nobody asked for."""
        if self._ef_out is None or self._ef_out.device != device:
            self._ef_out = torch.empty(self.out_floats, dtype=torch.float32, device=device)
        return self._ef_out

    def encode(self, tensors, wire_user, slot, salt, errs=None, ef_scale=None, draws=None, graph_header=None, dense=None, defer_reset=None,
               rng_slot=None, table_current=False, out=None, seed=None):
        """One user's record: `tensors` compressed into the wire; out (the group's dtype [out_floats]): also their dense decode.  With
        `errs` (float32): error feedback in the same launches (t += ef_scale*err in front, err = t - decoded behind, both in place);
        a group with state gives `errs` its own meaning (_user_state).  draws (given uniforms, see _given_draws): required for gq_rng
        "reference", taken in any stochastic mode when handed in; seed: the device generator's seed for this call.  False --
        nothing launched -- where the group refuses or a tensor cannot be addressed.  graph_header, table_current: see
        _choose_header; dense, rng_slot: see BatchedHSQ.encode."""
        if self._refuses(wire_user, draws):
            return False
        ebufs, table, ef_on = self._user_state(errs)
        if table is False or not self._choose_header(tensors, slot, self.align, ebufs, dense, graph_header, table_current):
            return False
        if table is not None:
            self._batch.set_state(table)
        ef = ef_scale if ef_on else None
        if ef is not None and out is None and self.EF_DENSE:
            out = self._ef_buffer(wire_user.device)
        launches, args = self._compress_args(out, ef, table, slot, salt, rng_slot, draws, seed)
        self._launch(graph_header, defer_reset, launches, wire_user, *args)
        return True

    def _refuses(self, wire_user, draws):
        """What an encode refuses in front of the header: reference draws that are not there for every tensor, a misaligned wire."""
        return (self.reference_draws and not self._has_draws(draws)) or wire_user.data_ptr() % self.WIRE_ALIGN != 0

    def _user_state(self, errs):
        """errs -> (the error buffers for the header, the user's state table -- None: the group has none, False: refuse --, whether
        this is a record with error feedback)."""
        return errs, None, errs is not None

    def _compress_args(self, out, ef, table, slot, salt, rng_slot, draws, seed):
        """-> (the launches, their arguments behind `wire`)."""
        return self._batch.compress, (out, ef)

    def _has_draws(self, draws):
        return self.random and draws is not None and all(i in draws[1] for i in self.idxs)

    def _drawn(self, slot, salt, rng_slot, draws, seed):
        """(mode, seed, r) of this call (_item_draws): the given draws in the group's layout, `seed`, the { seed, step } pair of the
        slot (rng_slot: the reserved pair by name) where the quantizer gave the group pairs (`counter`), a fresh seed."""
        counter_seed = self._counter_seed(slot) if rng_slot is None else self._counter_seed(rng_slot, reserved=True)
        return _item_draws(self.random, self._given_draws(draws) if self._has_draws(draws) else None, seed,
                           counter_seed if self.counter else None, salt)

    # ---- one user's state behind the launches: a device table per set of state buffers, built once, never freed or moved (captured
    # graphs hold its address), which keeps its buffers alive.  The group states _state_key(errs) -> (key, the header's error
    # buffers), _state_valid(errs, key) and _state_rows(errs, key) -> (host table, the buffers it names).
    def _state_table(self, errs):
        """The device table of the state in `errs`, or False when its buffers cannot be addressed."""
        key = self._state_key(errs)[0]
        ent = self._state_tables.get(key)
        if ent is None:
            if not self._state_valid(errs, key):
                return False
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("%s: a state table is built by an eager record, not under stream capture" % type(self).__name__)
            host, buffers = self._state_rows(errs, key)
            ent = self._state_tables[key] = (host.view(-1).to(self.device), buffers)
        return ent[0]

    def _addressable(self, ts, numels):
        """Every tensor of one kind of state: one per tensor of the group, contiguous float32 of that size on the group's device."""
        dev_index = self.device.index if self.device.index is not None else torch._C._cuda_getDevice()
        return (len(ts) == self.nseg and all(map(_IS_CONTIGUOUS, ts)) and set(map(_DTYPE_OF, ts)) == _F32_ONLY
                and set(map(_GET_DEVICE, ts)) == {dev_index} and all(t.numel() == n for t, n in zip(ts, numels)))

    def upload(self, tensors, slot, errs=None, dense=None):
        """(a group with state, in front of an address-free graph's replay: the graph's launches read the state table of the buffers
        it was captured with -- the caller keys its graphs by those buffers' addresses, and a table, once built, stays where it is.
        A table that was never built: False)"""
        if self._state_tables is not None:
            key, errs = self._state_key(errs)
            if key is not None and key not in self._state_tables:
                return False
        return _BatchedBase.upload(self, tensors, slot, errs, dense)

    def decode_into(self, gathered, R, out, plain=False):
        """The decode-mean launch into a caller's buffer (_SparseCodec: a one-tensor group, its section at offset 0 of the rows)."""
        if not self.ready:
            self.upload_layout()
        self._batch.decode(gathered, R, out, plain=plain, **self._rotation_kw())

    def roundtrip(self, tensors, slot, salt, errs=None, ef_scale=None, draws=None, rng_slot=None, graph_header=None, defer_reset=None):
        """decompress(compress(t)) for every tensor of the group: the compress launches' own dense decode (the reference's signed
        zeros and NaNs, which the wire does not carry), no decode launch.  See _BatchedBase.roundtrip."""
        if self._tmp_wire is None:
            self._tmp_wire = torch.zeros((1, max(16, self.user_bytes)), dtype=torch.uint8, device=self.device)
        out, views = self._out_buffer(self.device)
        kw = {"graph_header": graph_header, "defer_reset": defer_reset} if graph_header is not None else {}
        if not self.encode(tensors, self._tmp_wire[0], slot, salt, errs, ef_scale, draws=draws, rng_slot=rng_slot, out=out, **kw):
            self._out_turn ^= 1      # (the buffer was not used)
            return None
        return views


class BatchedTopK(_ItemGroup):
    """All TopKSparsificationCompressor tensors in ONE gq_topk_compress_batched sequence (eight launches: three radix passes with
    a per-tensor pick behind each, counts, scan, write -- include/gq_topk.h) and ONE gq_topk_decode_sum_batched launch.  No
    draws: every launch replays from a HIP graph.  The compress also writes the dense decoded tensors (v * mask) where a caller
    asks for them: error feedback takes its residual from them, and the two-phase re-compress returns them, bit for bit the
    reference's decompress(compress(g))."""

    @staticmethod
    def eligible(codec):
        return type(codec) is TopKCodec

    @staticmethod
    def group_key(codec):
        return ()

    OUT_PAD = 1                 # a tensor's views in the output buffer are packed back to back
    BATCH = native.TopKBatch
    EF_DENSE = True

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        # an item is a chunk of elements
        nseg, item = self._item_setup(codecs, offsets, idxs, device, slots, user_bytes, dense,
                                      lambda cd: max(1, -(-cd.numel // native.TOPK_CHUNK)), {4: [codecs[i].k for i in idxs]}, self.OUT_PAD)
        self.random = False
        # the select's scratch (include/gq_topk.h): the histograms start zero and every compress leaves them zero
        scratch = self._scratch(nseg, item, device)
        self._hist, self._state, self._counts = scratch[:3]
        self._batch = self.BATCH(self._dev[:self._table_words], self.item_seg, nseg, item, *scratch)

    def _scratch(self, nseg, items, device):
        """hist, state, counts (and what a subclass's launches take behind them)."""
        return (torch.zeros(nseg * native.TOPK_HIST_BINS, dtype=torch.int32, device=device),
                torch.zeros(nseg * 4, dtype=torch.int32, device=device), torch.zeros(items * 2, dtype=torch.int32, device=device))

TopKCodec.GROUP = BatchedTopK


class BatchedDGC(BatchedTopK):
    """BatchedTopK with momentum correction and momentum factor masking (Deep Gradient Compression; include/gq_dgc.h): a record is
    gq_dgc_accumulate_batched (u <- m * u + g, also into the group's scratch), the top-k sequence in its error-feedback form at
    scale 1 over that scratch and v, and gq_dgc_mask_batched (u <- +0 at the indices just sent).  The gradients are read only.
    The group's own table carries the gradients' addresses, as BatchedTopK's does; the select reads ONE user's state table --
    scratch, u, v and the layout, built once per set of state buffers and never freed or moved (captured graphs hold its
    address) -- so nothing but the accumulate launch follows the
    gradients.  Wire, decode-mean, graph machinery and the plain compress (no state handed in: the two-phase re-compress of the
    mean, which has no momentum) are BatchedTopK's.
    encode's `errs` is the state, ([u per tensor], [v per tensor]) of one user, and `ef_scale` the momentum."""

    OUT_PAD = 4                 # 16-byte aligned tensors in the scratch: the accumulate launch stores float4 there
    BATCH = native.DGCBatch

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        BatchedTopK.__init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense)
        self._scratch = torch.empty(max(4, self.out_floats), dtype=torch.float32, device=device)
        self._state_tables = {}

    def _state_key(self, errs):
        return (None, None) if errs is None else ((tuple(map(_DATA_PTR, errs[0])), tuple(map(_DATA_PTR, errs[1]))), None)

    def _state_valid(self, errs, key):
        numels = [cd.numel for cd in self.codecs]
        return self._addressable(errs[0], numels) and self._addressable(errs[1], numels)

    def _state_rows(self, errs, key):
        """include/gq_dgc.h, state_table: the layout with the scratch for the gradients, u and v."""
        host = self._layout.clone()
        base = self._scratch.data_ptr()
        for s in range(self.nseg):
            host[s, 0], host[s, 6], host[s, 7] = base + 4 * self.out_off[s], key[0][s], key[1][s]
        return host, (list(errs[0]), list(errs[1]))

    def _user_state(self, errs):
        """errs = ([u], [v]) of one user, ef_scale = m: one record with momentum correction (the header carries no error buffers: the
        select's are the table's).  errs None: plain top-k, no error feedback."""
        return (None, None, False) if errs is None else (None, self._state_table(errs), True)

    def _compress_args(self, out, ef, table, *how):
        return (self._batch.compress, (out, ef)) if table is None else (self._batch.record, (out, float(ef)))


class BatchedSign(_ItemGroup):
    """All SignSGDCompressor tensors in ONE gq_sign_compress_batched launch and ONE gq_sign_decode_sum_batched launch
    (include/gq_sign.h).  No draws and no scratch: both replay from a HIP graph.  The compress also writes the dense sign(w)
    where a caller asks for it (the two-phase re-compress returns it); with error feedback it updates the gradient and the
    residual in the same launch.  The decode-mean sums the codes as integers and divides by R: gq_mean_rows' result over the
    dense signs, bit for bit."""

    @staticmethod
    def eligible(codec):
        return type(codec) is SignCodec

    @staticmethod
    def group_key(codec):
        return ()

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        # an item is a run of wire bytes; 16-byte aligned views in the output buffer: the launches store float4 there
        nseg, item = self._item_setup(codecs, offsets, idxs, device, slots, user_bytes, dense,
                                      lambda cd: max(1, -(-cd.nbytes // native.SIGN_ITEM_BYTES)), {}, 4)
        self.random = False
        self._batch = native.SignBatch(self._dev[:self._table_words], self.item_seg, nseg, item)

SignCodec.GROUP = BatchedSign


class BatchedMaurey(_ItemGroup):
    """All MaureySparsification tensors in ONE gq_maurey_compress_batched sequence (six launches: item sums, their scan, the
    draws counted, the counts' scan, the draws bucketed, the per-item placement -- include/gq_maurey.h) and ONE
    gq_maurey_decode_sum_batched launch.  Tensor s owns the draws [first draw, first draw + k) of the group's stream.  The compress
    also writes the dense decoded tensors where a caller asks for them: error feedback takes its residual from them and the
    two-phase re-compress returns them.  gq_rng "device" with the quantizer's { seed, step } pairs: nothing in the launches changes
    from record to record, they replay from a HIP graph and draw afresh every step; "reference": the quantizer's draw plan
    (torch.rand(k) per tensor, in parameter order) as given draws; "keyed" / a group without pairs: a fresh seed per call."""

    @staticmethod
    def eligible(codec):
        return type(codec) is MaureyCodec

    @staticmethod
    def group_key(codec):
        return (codec._rng,)

    EF_DENSE = True

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        ks = [codecs[i].k for i in idxs]
        first_draw = list(itertools.accumulate([0] + ks[:-1]))      # tensor s owns the draws [first, first + k) of the group's stream
        # an item is a chunk of elements (numel >= 1: never none); 16-byte aligned views in the output buffer
        nseg, item = self._item_setup(codecs, offsets, idxs, device, slots, user_bytes, dense,
                                      lambda cd: -(-cd.numel // native.MAUREY_CHUNK),
                                      {4: ks, 6: first_draw}, 4)
        self.ndraws = draw = sum(ks)
        rng = self.codecs[0]._rng
        self.random = True
        self.counter = rng == "device"          # the quantizer gives such a group its { seed, step } pairs (PSQuantizer._make_group)
        self.reference_draws = rng == "reference"
        # the sampler's scratch (include/gq_maurey.h): nothing in it has to be zero, every launch sequence rewrites what it reads
        self._sums = torch.empty(item * 4, dtype=torch.float64, device=device)
        self._totals = torch.empty(nseg, dtype=torch.float64, device=device)
        self._counts = torch.empty(item * 3, dtype=torch.int32, device=device)
        self._draw_item = torch.empty(draw, dtype=torch.int32, device=device)
        self._bucket = torch.empty(draw, dtype=torch.float32, device=device)
        self._r_gather = None
        self._batch = native.MaureyBatch(self._dev[:self._table_words], self.item_seg, nseg, item, draw, self._sums, self._totals,
                                         self._counts, self._draw_item, self._bucket)

    def graphable(self):
        """As BatchedPVQ.graphable: only the draws keyed by the device step words leave every launch argument unchanged."""
        return self.counter and self.rng_pairs is not None and not self.reference_draws

    def _given_draws(self, draws):
        """draws = (r_all on the device, {parameter index: offset of its k draws}) -> float32 [ndraws] in the group's layout (every
        tensor's draws at its first draw), one gather through an index built once (as BatchedHSQ._given_draws)."""
        r_all, offsets = draws
        if self._r_gather is None:
            idx = torch.cat([torch.arange(offsets[i], offsets[i] + cd.k) for i, cd in zip(self.idxs, self.codecs)])
            self._r_gather = (idx.to(self.device), torch.empty(self.ndraws, dtype=torch.float32, device=self.device))
        torch.index_select(r_all, 0, self._r_gather[0], out=self._r_gather[1])
        return self._r_gather[1]

    def _compress_args(self, out, ef, table, *how):
        return self._batch.compress, self._drawn(*how) + (out, ef)


MaureyCodec.GROUP = BatchedMaurey


class BatchedMX(_ItemGroup):
    """All MXCompressor tensors of one format in ONE gq_mx_compress_batched launch and ONE gq_mx_decode_sum_batched launch
    (include/gq_mx.h).  No scratch.  Element i of tensor s owns draw first draw + i of the group's stream (first draw = the
    elements of the tensors before it).  The compress also writes the dense decode where a caller asks for it (the two-phase
    re-compress returns it); with error feedback it updates the gradient and the residual in the same launch.  Deterministic
    rounding, or gq_rng "device" with the quantizer's { seed, step } pairs: nothing in the launches changes from record to
    record, they replay from a HIP graph (and draw afresh every step); "reference": the quantizer's draw plan (torch.rand(numel)
    per tensor, in parameter order) as given draws; "keyed" / a group without pairs: a fresh seed per call."""

    align = 4       # the class's default; every instance sets its own from its codecs' dtype (_set_dtype: 2 for bfloat16)
    WIRE_ALIGN = 16

    @staticmethod
    def eligible(codec):
        return type(codec) is MXCodec

    @staticmethod
    def group_key(codec):
        # (the dtype by name: the keys are sorted.  A model with float32 norms and bfloat16 weights gets two groups.)
        return (codec.format, int(codec.random), codec._rng, str(codec.dtype))

    def _set_dtype(self, dtype):
        """The group's tensor-side type (include/gq_mx.h) from its codecs, in front of the layout: 2-byte aligned sources and
        dense-copy sources and views on multiples of 8 elements in the output buffer for bfloat16, 4 and 4 for float32 -- either
        way a view starts 16-byte aligned, where a lane's 8 elements are one (two) 16-byte stores."""
        self.dtype, self._dtypes = dtype, {dtype}
        self.align = self._dense_align = 2 if dtype == torch.bfloat16 else 4
        self._out_pad = 16 // self.align

    def _layout(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        """The group's tables (host work only; the launch descriptor is __init__'s) -> (tensors, items)."""
        ns = [codecs[i].numel for i in idxs]
        first_draw = list(itertools.accumulate([0] + ns[:-1]))
        self._first_draw, self.ndraws = first_draw, sum(ns)
        # an item is a run of elements (numel >= 1: never none); 16-byte aligned views in the output buffer: 16-byte stores
        self._set_dtype(codecs[idxs[0]].dtype)
        return self._item_setup(codecs, offsets, idxs, device, slots, user_bytes, dense,
                                lambda cd: -(-cd.numel // native.MX_ITEM_ELEMS), {6: first_draw}, self._out_pad)

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        nseg, item = self._layout(codecs, offsets, idxs, device, slots, user_bytes, dense)
        c0 = self.codecs[0]
        self.format, self.random = c0.format, c0.random
        self.counter = self.random and c0._rng == "device"      # the quantizer gives such a group its { seed, step } pairs
        self.reference_draws = self.random and c0._rng == "reference"
        self._r = None
        self._batch = self._descriptor(nseg, item)

    def _descriptor(self, nseg, item):
        return native.MXBatch(self._dev[:self._table_words], self.item_seg, nseg, item, self.format, self.dtype)

    def graphable(self):
        return not self.random or (self.counter and self.rng_pairs is not None)

    def _given_draws(self, draws):
        """draws = (r_all on the device, {parameter index: offset of its numel draws}) -> float32 [ndraws] in the group's layout."""
        r_all, offsets = draws
        if self._r is None:
            self._r = torch.empty(self.ndraws, dtype=torch.float32, device=self.device)
        if len(self.idxs) == 1 and r_all.numel() >= offsets[self.idxs[0]] + self.ndraws and r_all.dtype == torch.float32:
            return r_all[offsets[self.idxs[0]]:offsets[self.idxs[0]] + self.ndraws]
        for i, cd, fd in zip(self.idxs, self.codecs, self._first_draw):
            self._r[fd:fd + cd.numel].copy_(r_all[offsets[i]:offsets[i] + cd.numel])
        return self._r

    _compress_args = BatchedMaurey._compress_args


MXCodec.GROUP = BatchedMX


class BatchedMXR(BatchedMX):
    """BatchedMX over libgq_mxr.so: all MXCompressor tensors of one format, rounding and set of sign words in ONE
    gq_mxr_compress_batched launch and ONE gq_mxr_decode_sum_batched launch (include/gq_mxr.h).  The layout, the draws and the
    graph rules are BatchedMX's; `out` and the residual of error feedback are inverse-rotated, and the decode-mean rotates the
    mean back once."""

    @staticmethod
    def eligible(codec):
        return type(codec) is MXRCodec

    @staticmethod
    def group_key(codec):
        return BatchedMX.group_key(codec) + tuple(codec.signs)

    def _descriptor(self, nseg, item):
        self.signs = self.codecs[0].signs
        return native.MXRBatch(self._dev[:self._table_words], self.item_seg, nseg, item, self.format, self.signs, self.dtype)


MXRCodec.GROUP = BatchedMXR


class BatchedDrive(_ItemGroup):
    """All DriveCompressor tensors of one scale mode and set of sign words in ONE gq_drive_compress_batched launch and ONE
    gq_drive_decode_sum_batched launch (include/gq_drive.h).  No draws and no scratch: both replay from a HIP graph with nothing
    to step.  The compress also writes the dense decode where a caller asks for it (the two-phase re-compress returns it); with
    error feedback it updates the gradient and the residual in the same launch.  The decode-mean adds the payloads in the rotated
    domain and rotates the mean back once -- which is why one group, and every user of it, has one set of sign words.
    Step mode (the codecs' `stepped`): the quantizer sets `rotation`, its { seed, step } pair, and both launches are the *_stepped
    ones, which read the words of the current step through that address -- still nothing in a launch changes, so the group stays
    graphable; the quantizer's aggregate moves the step word.  Without a pair the launches are the fixed ones: step 0.
    own (the codecs' `own`; SIGNS, PER STREAM): both launches are the *_streams ones.  A record into wire slot s compresses under
    stream `stream_base` + s -- the quantizer sets stream_base = rank * users per rank, so that the stream is the payload's row of
    the gather -- and the decode-mean rotates row r back under stream r.  The two-phase re-compress (rng_slot given) is one payload:
    stream 0.  The stream is a launch argument by value and a function of the slot, as a record graph's key is.  The launches read
    the quantizer's pair in either rotation mode (under 'fixed' nothing ever steps it); a group on its own makes one at step 0."""

    stream_base = 0
    WIRE_ALIGN = 16

    @staticmethod
    def eligible(codec):
        return type(codec) is DriveCodec

    @staticmethod
    def group_key(codec):
        return (codec.scale_mode, int(codec.stepped) + 2 * int(getattr(codec, "own", False))) + tuple(codec.signs)

    def _pair(self):
        """own: the pair the *_streams launches read -- the quantizer's, or (a group on its own) one made here at (seed, step 0)."""
        if self.rotation is None:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the rotation pair is made by the first eager launch, not under stream capture")
            seed = self.codecs[0].seed
            if seed is None:
                raise ValueError("user_rotation = 'own' needs the compressor's seed")
            seed = int(seed) & (2 ** 64 - 1)
            self.rotation = torch.tensor([[seed - (2 ** 64 if seed & 2 ** 63 else 0), 0]], dtype=torch.int64).to(self.device)
        return self.rotation

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        # an item is a run of elements (numel >= 1: never none); 16-byte aligned views in the output buffer: the launches store float4 there
        nseg, item = self._item_setup(codecs, offsets, idxs, device, slots, user_bytes, dense,
                                      lambda cd: -(-cd.numel // native.MX_ITEM_ELEMS), {}, 4)
        c0 = self.codecs[0]
        self.random = False
        self.scale_mode, self.signs, self.stepped = c0.scale_mode, c0.signs, c0.stepped
        self.own = bool(getattr(c0, "own", False))
        self._batch = self._make_batch(nseg, item)

    def _make_batch(self, nseg, item):
        return native.DriveBatch(self._dev[:self._table_words], self.item_seg, nseg, item, self.scale_mode, self.signs)

    def _compress_args(self, out, ef, table, slot, salt, rng_slot, *draws):
        if self.own:      # (rng_slot: the two-phase re-compress, ONE payload)
            return self._batch.compress, (out, ef, self._pair(), 0 if rng_slot is not None else self.stream_base + slot)
        return self._batch.compress, (out, ef, self.rotation)


DriveCodec.GROUP = BatchedDrive


class BatchedEden(BatchedDrive):
    """All EdenCompressor tensors of one (bits, scale mode, sign words) in ONE gq_eden_compress_batched launch and ONE
    gq_eden_decode_sum_batched launch (include/gq_eden.h).  BatchedDrive's host path on libgq_eden.so's descriptor."""

    @staticmethod
    def eligible(codec):
        return type(codec) is EdenCodec

    @staticmethod
    def group_key(codec):
        return (codec.bits, codec.scale_mode, int(codec.stepped) + 2 * int(getattr(codec, "own", False))) + tuple(codec.signs)

    def _make_batch(self, nseg, item):
        self.bits = self.codecs[0].bits
        return native.EdenBatch(self._dev[:self._table_words], self.item_seg, nseg, item, self.bits, self.scale_mode, self.signs)


EdenCodec.GROUP = BatchedEden


class BatchedThr(_ItemGroup):
    """All ThresholdSparsificationCompressor tensors of one (stages, fixed threshold) in ONE gq_thr_compress_batched sequence
    (`stages` reduce / pick pairs, then count, scan, write -- include/gq_thr.h) and ONE gq_thr_decode_sum_batched launch.  No draws:
    every launch replays from a HIP graph.  The compress also writes the dense decoded tensors (w * mask) where a caller asks for
    them: error feedback takes its residual from them, and the two-phase re-compress returns them."""

    @staticmethod
    def eligible(codec):
        return type(codec) is ThrCodec

    @staticmethod
    def group_key(codec):
        return (codec.stages, codec.eta)

    EF_DENSE = True

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        mine = [codecs[i] for i in idxs]
        nseg, item = self._item_setup(codecs, offsets, idxs, device, slots, user_bytes, dense,
                                      lambda cd: -(-cd.numel // native.THR_CHUNK),
                                      {4: [cd.k for cd in mine], 6: [cd.cap + (cd.stride << 32) for cd in mine]}, 1)
        self.random = False
        self.stages, self.eta = mine[0].stages, mine[0].eta
        assert all((cd.stages, cd.eta) == (self.stages, self.eta) for cd in mine)
        # the fit's and the compaction's scratch (include/gq_thr.h): written before it is read, nothing in it has to be zero
        self._sums = torch.empty(item, dtype=torch.float64, device=device)
        self._state = torch.empty(nseg * 4, dtype=torch.int32, device=device)
        self._counts = torch.empty(item * 2, dtype=torch.int32, device=device)
        self._batch = native.ThrBatch(self._dev[:self._table_words], self.item_seg, nseg, item, self._sums, self._state, self._counts,
                                      self.stages, min(cd.k for cd in mine), min(cd.cap for cd in mine), min(cd.stride for cd in mine))

    def _compress_args(self, out, ef, table, *how):
        return self._batch.compress, (out, ef, self.eta)

    def kept_counts(self, wire_user):
        """[(kept, found, eta), ...] of the group's tensors, read from the headers of one user's wire."""
        return [cd.header(wire_user, int(self._layout[s, 3])) for s, cd in enumerate(self.codecs)]


ThrCodec.GROUP = BatchedThr


class BatchedSTC(BatchedTopK):
    """All SparseTernaryCompressor tensors in ONE gq_stc_compress_batched sequence (top-k's eight launches: the count launch also sums
    the kept magnitudes per item, the scan launch folds them into mu, the write launch compacts 16-bit words -- include/gq_stc.h)
    and ONE gq_stc_decode_sum_batched launch.  Tables, scratch, encode and the graph machinery are BatchedTopK's; `sums` is the one
    buffer more."""

    @staticmethod
    def eligible(codec):
        return type(codec) is STCCodec

    BATCH = native.STCBatch

    def _scratch(self, nseg, items, device):
        self._sums = torch.empty(items, dtype=torch.float64, device=device)
        return BatchedTopK._scratch(self, nseg, items, device) + (self._sums,)


STCCodec.GROUP = BatchedSTC


class BatchedPowerSGD(_ItemGroup):
    """All PowerSGDCompressor tensors of one rank in ONE gq_psgd_compress_batched sequence (project, orthogonalise, back-project,
    fold, + the residual launch under error feedback or where the dense decode is asked for -- include/gq_psgd.h) and ONE
    gq_psgd_decode_sum_batched launch.  No draws: every launch replays from a HIP graph.  The group's item table is the TILE
    table (64 rows x 256 columns: back-project, fold, residual and decode run a workgroup per tile); the project launch has an
    item table of its own.  The warm starts are the caller's, as BatchedDGC's state is: encode's `errs` is
    (error buffers or None, [Q per tensor], user) of ONE user, and the launches read a device table of those addresses, built once
    per set of buffers and never moved (captured graphs hold its address)."""

    @staticmethod
    def eligible(codec):
        return type(codec) is PowerSGDCodec

    @staticmethod
    def group_key(codec):
        return (codec.rank, codec.seed)

    def __init__(self, codecs, offsets, idxs, device, slots, user_bytes, dense=None):
        mine = [codecs[i] for i in idxs]
        self.rank, self.seed = mine[0].rank, mine[0].seed
        R, P, RB, TC = self.rank, native.PSGD_PIECE, native.PSGD_ROW_BLOCK, native.PSGD_TILE_COLS
        # 16-byte aligned views in the output buffer: the decode stores float4 there
        nseg, tiles = self._item_setup(codecs, offsets, idxs, device, slots, user_bytes, dense,
                                       lambda cd: -(-cd.n // RB) * -(-cd.m // TC), {4: [cd.n for cd in mine]}, 4)
        self.random = False
        lay = torch.zeros((nseg, 4), dtype=torch.int64)
        aitem_seg, aitem, pw, cp = [], 0, 0, 0
        for s, cd in enumerate(mine):
            pieces = 1 if cd.m <= P else -(-cd.m // P)
            items = -(-cd.n // max(1, P // cd.m)) if cd.m <= P else cd.n * pieces
            lay[s, 0], lay[s, 1], lay[s, 2], lay[s, 3] = aitem, pw, cp, cd.param_index << 12
            aitem_seg += [s] * items
            aitem += items
            pw += cd.n * pieces * R
            cp += -(-cd.n // RB) * cd.m * R
        self._lay = lay.view(-1).to(device)
        self._aitem_seg = torch.tensor(aitem_seg, dtype=torch.int32, device=device)
        # scratch (include/gq_psgd.h): written before it is read in every compress
        self._pwork = torch.empty(pw, dtype=torch.float32, device=device)
        self._cpart = torch.empty(cp, dtype=torch.float32, device=device)
        self._flags = torch.empty(nseg * 4, dtype=torch.int32, device=device)
        self._batch = native.PSGDBatch(self._dev[:self._table_words], self.item_seg, nseg, tiles, rank=R, seed=self.seed, lay=self._lay,
                                       aitem_seg=self._aitem_seg, naitems=aitem, pwork=self._pwork, cpart=self._cpart, flags=self._flags)
        self._state_tables = {}

    def _state_key(self, errs):
        # (no warm starts: a key no table has)
        return ((), None) if errs is None else ((tuple(map(_DATA_PTR, errs[1])), int(errs[2])), errs[0])

    def _state_valid(self, errs, key):
        return (0 <= key[1] < native.PSGD_MAX_USERS and not any(p % 4 for p in key[0])
                and self._addressable(errs[1], [cd.m * self.rank for cd in self.codecs]))

    def _state_rows(self, errs, key):
        """include/gq_psgd.h, state: { Q, user } per tensor."""
        return torch.tensor([[p, key[1]] for p in key[0]], dtype=torch.int64), list(errs[1])

    def _user_state(self, errs):
        """errs = (error buffers or None, [Q], user): one record of that user.  With error buffers: e <- M + ef_scale * e before the
        projection and e <- that - decoded after it, in place; the gradients are read only."""
        if errs is None:
            raise ValueError("BatchedPowerSGD.encode: a record needs its user's warm starts, errs = (error buffers or None, [Q], user)")
        return errs[0], self._state_table(errs), errs[0] is not None


PowerSGDCodec.GROUP = BatchedPowerSGD


def default_codec_factory(compressor, numel, shape, packed6=False):
    if isinstance(compressor, ProbabilisticVectorCompressor):
        return PVQCodec(compressor, numel, shape, packed6)
    if isinstance(compressor, IdenticalCompressor):
        return DenseCodec(compressor, numel, shape)
    if isinstance(compressor, NearestNeighborCompressor):
        return HSQCodec(compressor, numel, shape, packed6)
    if isinstance(compressor, QSGDCompressor):
        return QSGDCodec(compressor, numel, shape)
    if isinstance(compressor, TopKSparsificationCompressor):
        return TopKCodec(compressor, numel, shape)
    if isinstance(compressor, SignSGDCompressor):
        return SignCodec(compressor, numel, shape)
    if isinstance(compressor, MaureySparsification):
        return MaureyCodec(compressor, numel, shape)
    if isinstance(compressor, MXCompressor):
        return (MXRCodec if getattr(compressor, "rotate", None) else MXCodec)(compressor, numel, shape)
    if isinstance(compressor, DriveCompressor):
        return DriveCodec(compressor, numel, shape)
    if isinstance(compressor, EdenCompressor):
        return EdenCodec(compressor, numel, shape)
    if isinstance(compressor, ThresholdSparsificationCompressor):
        return ThrCodec(compressor, numel, shape)
    if isinstance(compressor, SparseTernaryCompressor):
        return STCCodec(compressor, numel, shape)
    if isinstance(compressor, PowerSGDCompressor):
        # (a vector, a matrix thinner than the rank, factors no smaller than the tensor: uncompressed, whatever its size)
        return PowerSGDCodec(compressor, numel, shape) if compressor.compresses else DenseCodec(compressor, numel, shape)
    return GenericCodec(compressor, numel, shape)


def quantizer_codec_factory(compressor, numel, shape, packed6=False):
    """What PSQuantizer / RingQuantizer use when the caller names no factory: default_codec_factory, and the two-section wire
    for a ResidualCompressor of a shape libgq_rq.so serves.  (default_codec_factory itself still answers GenericCodec for that
    class -- tests/test_pvq_host.py pins it --, so the choice is made here, where the quantizers ask.)"""
    if isinstance(compressor, ResidualCompressor) and ResidualCodec.serves(compressor):
        return ResidualCodec(compressor, numel, shape, packed6)
    return default_codec_factory(compressor, numel, shape, packed6)
