"""The rotated microscaling compressor, host side (no GPU): the driver flags, the refusal in ring mode, the codec and group classes
chosen with and without rotation, groups split by sign words, the wire's size, the library's ABI."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mxr_contract as mxr  # noqa: E402
from test_mx_host import make_args  # noqa: E402


def test_driver_flags_and_their_refusals():
    from gq_amd import driver
    from gq_amd.compressors import MXCompressor
    p = driver.build_parser()
    a = p.parse_args(["--quantizer", "mx"])
    assert a.mx_rotate == "none" and a.mx_rotate_seed == 1
    a = p.parse_args(["--quantizer", "mx", "--mx-rotate", "hadamard", "--mx-rotate-seed", "7"])
    assert a.mx_rotate == "hadamard" and a.mx_rotate_seed == 7
    with pytest.raises(SystemExit):
        p.parse_args(["--quantizer", "mx", "--mx-rotate", "givens"])
    for none in (make_args(), make_args(mx_rotate=None), make_args(mx_rotate="none", mx_rotate_seed=3)):
        c = MXCompressor(2000, (2000,), none)
        assert c.rotate is None and c.rotate_signs is None
    c = MXCompressor(2000, (2000,), make_args(mx_rotate="hadamard"))
    assert c.rotate == "hadamard" and c.rotate_seed == 1 and c.rotate_signs == mxr.sign_words(1)
    c = MXCompressor(2000, (2000,), make_args(mx_rotate="hadamard", mx_rotate_seed=7))
    assert c.rotate_signs == mxr.sign_words(7) != mxr.sign_words(1) and all(0 <= w < 1 << 64 for w in c.rotate_signs)
    for bad in ("Hadamard", "fwht", 1, True):
        with pytest.raises(ValueError, match="mx_rotate"):
            MXCompressor(2000, (2000,), make_args(mx_rotate=bad))


def test_ring_mode_with_rotation_is_refused():
    from gq_amd.compressors import MXCompressor
    from gq_amd.quantizers import PSQuantizer, Quantizer, RingQuantizer
    params = [torch.nn.Parameter(torch.zeros(2000))]
    with pytest.raises(ValueError, match="ring mode"):
        RingQuantizer(MXCompressor, params, make_args(mode="ring", mx_rotate="hadamard"))
    with pytest.raises(ValueError, match="ring mode"):
        Quantizer(MXCompressor, params, make_args(mode="ring", mx_rotate="hadamard"))
    RingQuantizer(MXCompressor, params, make_args(mode="ring", mx_rotate="none"))       # without rotation: as before
    RingQuantizer(MXCompressor, params, make_args(mode="ring"))
    PSQuantizer(MXCompressor, params, make_args(mx_rotate="hadamard"))


def test_codec_and_group_classes_with_and_without_rotation():
    from gq_amd.codecs import (BatchedMX, BatchedMXR, DenseCodec, MXCodec, MXRCodec, default_codec_factory, mx_section_bytes,
                               quantizer_codec_factory)
    from gq_amd.compressors import MXCompressor
    from gq_amd.quantizers import PSQuantizer
    rot = MXCompressor(5000, torch.Size([5000]), make_args(mx_rotate="hadamard"))
    plain = MXCompressor(5000, torch.Size([5000]), make_args())
    for factory in (default_codec_factory, quantizer_codec_factory):
        cd = factory(rot, 5000, torch.Size([5000]))
        assert type(cd) is MXRCodec and BatchedMXR.eligible(cd) and not BatchedMX.eligible(cd) and cd.GROUP is BatchedMXR
        assert cd.signs == mxr.sign_words(1)
        pc = factory(plain, 5000, torch.Size([5000]))
        assert type(pc) is MXCodec and BatchedMX.eligible(pc) and not BatchedMXR.eligible(pc) and pc.GROUP is BatchedMX
    for n in (1, 255, 256, 257, 4097, 200704):
        for fmt in ("fp4", "fp8"):
            a = MXRCodec(MXCompressor(n, (n,), make_args(mx_format=fmt, mx_rotate="hadamard", random=1)), n, (n,))
            b = MXCodec(MXCompressor(n, (n,), make_args(mx_format=fmt, random=1)), n, (n,))
            assert a.nbytes == b.nbytes == mx_section_bytes(n, fmt) and a.draw_count() == b.draw_count() == n
            assert a.uses_reference_draws() == b.uses_reference_draws()
    shapes = [(256, 784), (256,), (10, 256), (10,), (300, 300)]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    q = PSQuantizer(MXCompressor, params, make_args(mx_rotate="hadamard", random=1, gq_rng="reference"))
    assert [type(c) for c in q.codecs] == [MXRCodec, DenseCodec, MXRCodec, DenseCodec, MXRCodec]
    assert [g[0] for g in q._groups] == [BatchedMXR] and q._groups[0][1] == [0, 2, 4]
    assert q._draw_total == sum(q.codecs[i].numel for i in (0, 2, 4))
    q0 = PSQuantizer(MXCompressor, params, make_args(random=1, gq_rng="reference"))
    assert [g[0] for g in q0._groups] == [BatchedMX] and q0.wire_bytes_per_user() == q.wire_bytes_per_user()
    assert q0.offsets == q.offsets


def test_groups_split_by_sign_words():
    from gq_amd.codecs import BatchedMX, BatchedMXR, MXCodec, MXRCodec
    from gq_amd.compressors import MXCompressor

    def key(**kw):
        return BatchedMXR.group_key(MXRCodec(MXCompressor(5000, (5000,), make_args(mx_rotate="hadamard", **kw)), 5000, (5000,)))

    assert key() == key(mx_rotate_seed=1) and key() != key(mx_rotate_seed=2)
    assert len({key(mx_rotate_seed=s, mx_format=f, random=r) for s in (1, 2) for f in ("fp4", "fp8") for r in (0, 1)}) == 8
    plain = BatchedMX.group_key(MXCodec(MXCompressor(5000, (5000,), make_args()), 5000, (5000,)))
    assert key()[:len(plain)] == plain and key()[len(plain):] == mxr.sign_words(1)
    assert sorted([key(mx_rotate_seed=2), key()]) is not None       # (the quantizer sorts its groups by key)


def test_mxr_library_is_built_and_exports_its_abi():
    from gq_amd import native
    if not os.path.exists(native.MXR_LIB_PATH):
        pytest.fail("libgq_mxr.so is not built (build() makes it)")
    L = native.mxr_lib()
    assert L.gq_mxr_abi_version() == native.MXR_ABI_VERSION
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "gq_mxr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)      # declarations only: the comments name the entry points too
    declared = sorted(set(re.findall(r"\b(gq_mxr_\w+)\s*\(", code)))
    assert declared == sorted(native.MXR_EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", native.MXR_LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("gq"))
    assert exported == declared
    assert "#define GQ_MXR_ABI_VERSION %d" % native.MXR_ABI_VERSION in hdr
    assert "#define GQ_MXR_BLOCK %d" % native.MXR_BLOCK in hdr and native.MXR_BLOCK == mxr.RBLOCK == 8 * native.MX_BLOCK
    assert native.MX_ITEM_ELEMS % native.MXR_BLOCK == 0
    assert ctypes.sizeof(native._MXRBatchStruct) == 80      # (mxr.hip static_asserts the same size)
    assert native._MXRBatchStruct._fields_[:-1] == native._MXBatchStruct._fields_ and native._MXRBatchStruct.signs.offset == 48
    # mx.hip and mxr.hip share their device functions through one header, their kernels and host path through another
    csrc = os.path.join(os.path.dirname(HERE), "gradient-quantization_amd", "csrc")
    for f in ("mx.hip", "mxr.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "mx_common.hpp"' in text and '#include "mx_kernels.hpp"' in text and "__global__" not in text


def test_descriptor_needs_a_device_table():
    from gq_amd import native
    with pytest.raises(native.GQNativeError):
        native.MXRBatch(torch.zeros(8, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 1, 1, signs=mxr.SEEDED)
