"""The rotated 2- / 3- / 4-bit compressor, host side (no GPU): EdenCompressor's arguments and refusals, the wire's size, the driver
flags, the codec and group classes, the refusals in ring mode, with bfloat16 parameters and with momentum correction, the ResNet-50
wire bytes the README quotes, the library's ABI."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import eden_contract as ec  # noqa: E402
import mxr_contract as mxr  # noqa: E402
from test_mx_host import make_args  # noqa: E402

ROOT = os.path.dirname(HERE)
RESNET50_BYTES = {2: 6331440, 3: 9268752, 4: 12206064}      # 3,394,128 (one bit: drive) + 2,937,312 per further bit


def test_compressor_arguments_and_refusals():
    import compressors as shim
    from gq_amd import compressors
    from gq_amd.compressors import EdenCompressor, MXCompressor
    assert "EdenCompressor" in compressors.__all__ and shim.EdenCompressor is EdenCompressor and "EdenCompressor" in shim.__all__
    c = EdenCompressor(2000, (2000,), make_args())
    assert c.bits == 4 and c.scale == "unbiased" and c.seed == 1 and c.signs == mxr.sign_words(1) == MXCompressor.sign_words(1)
    c = EdenCompressor(2000, (2000,), make_args(eden_bits=None, eden_scale=None, eden_seed=None))
    assert c.bits == 4 and c.scale == "unbiased" and c.seed == 1
    c = EdenCompressor(2000, (2000,), make_args(eden_bits=2, eden_scale="mse", eden_seed=7))
    assert c.bits == 2 and c.scale == "mse" and c.signs == mxr.sign_words(7) != mxr.sign_words(1) and all(0 <= w < 1 << 64 for w in c.signs)
    assert EdenCompressor(2000, (2000,), make_args(eden_bits=3)).bits == 3
    for bad in (0, 1, 5, 8, "4", 2.5, True):
        with pytest.raises(ValueError, match="eden_bits"):
            EdenCompressor(2000, (2000,), make_args(eden_bits=bad))
    for bad in ("MSE", "drive", 1, True):
        with pytest.raises(ValueError, match="eden_scale"):
            EdenCompressor(2000, (2000,), make_args(eden_scale=bad))
    c = EdenCompressor(2000, (2000,), make_args())
    for t in (torch.zeros(2000), torch.zeros(2000, dtype=torch.bfloat16), torch.zeros(2000, dtype=torch.float64)):
        with pytest.raises(TypeError, match="float32 tensors on the HIP device"):
            c.compress(t)
    sig = torch.ones(3)
    assert c.decompress(sig) is sig


@pytest.mark.parametrize("bits", ec.BITS)
def test_section_bytes(bits):
    from gq_amd.codecs import EdenCodec, eden_section_bytes
    from gq_amd.compressors import EdenCompressor
    assert [eden_section_bytes(n, bits) for n in (1, 256, 257, 1024, 1025)] == [32 * bits + 16, 32 * bits + 16, 64 * bits + 16, 128 * bits + 16,
                                                                                160 * bits + 32]
    for n in (1, 255, 256, 257, 4095, 4097, 2359296):
        assert eden_section_bytes(n, bits) == ec.section_bytes(n, bits) and eden_section_bytes(n, bits) % 16 == 0
        assert EdenCodec(EdenCompressor(n, (n,), make_args(eden_bits=bits)), n, (n,)).nbytes == ec.section_bytes(n, bits)
    assert eden_section_bytes(1 << 20, bits) * 8 / (1 << 20) == bits + 0.125
    with pytest.raises(ValueError):
        EdenCodec(EdenCompressor(0, (0,), make_args(eden_bits=bits)), 0, (0,))
    for bad in (1, 5, 0):
        with pytest.raises(ValueError, match="eden_bits"):
            eden_section_bytes(100, bad)


def test_driver_flags():
    from gq_amd import driver
    from gq_amd.compressors import EdenCompressor
    assert driver.quantizer_choices["eden"] is EdenCompressor
    p = driver.build_parser()
    a = p.parse_args(["--quantizer", "eden"])
    assert a.eden_bits == 4 and a.eden_scale == "unbiased" and a.eden_seed == 1
    a = p.parse_args(["--quantizer", "eden", "--eden-bits", "3", "--eden-scale", "mse", "--eden-seed", "9"])
    assert a.eden_bits == 3 and a.eden_scale == "mse" and a.eden_seed == 9
    for bad in (["--eden-bits", "1"], ["--eden-bits", "5"], ["--eden-scale", "l2"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--quantizer", "eden"] + bad)
    a = p.parse_args(["--quantizer", "eden", "--param-dtype", "bfloat16"])
    with pytest.raises(ValueError, match="bfloat16 needs --quantizer mx"):
        driver.check_param_dtype(a)


def test_codec_and_group_classes():
    from gq_amd.codecs import BatchedDrive, BatchedEden, DenseCodec, DriveCodec, EdenCodec, default_codec_factory, quantizer_codec_factory
    from gq_amd.compressors import DriveCompressor, EdenCompressor
    from gq_amd.quantizers import PSQuantizer
    comp = EdenCompressor(5000, torch.Size([5000]), make_args(eden_scale="mse", eden_bits=3))
    for factory in (default_codec_factory, quantizer_codec_factory):
        cd = factory(comp, 5000, torch.Size([5000]))
        assert type(cd) is EdenCodec and BatchedEden.eligible(cd) and not BatchedDrive.eligible(cd) and cd.GROUP is BatchedEden
        assert cd.signs == mxr.sign_words(1) and cd.scale_mode == 1 and cd.bits == 3 and cd.dtype == torch.float32
        dcd = factory(DriveCompressor(5000, (5000,), make_args()), 5000, torch.Size([5000]))
        assert type(dcd) is DriveCodec and not BatchedEden.eligible(dcd) and dcd.GROUP is BatchedDrive

    def key(**kw):
        return BatchedEden.group_key(EdenCodec(EdenCompressor(5000, (5000,), make_args(**kw)), 5000, (5000,)))

    assert key() == key(eden_seed=1, eden_scale="unbiased", eden_bits=4) and key() != key(eden_seed=2) and key() != key(eden_scale="mse")
    assert len({key(eden_seed=s, eden_scale=m, eden_bits=b) for s in (1, 2) for m in ("unbiased", "mse") for b in ec.BITS}) == 12
    assert sorted([key(eden_seed=2), key(), key(eden_bits=2)]) is not None       # (the quantizer sorts its groups by key)
    shapes = [(256, 784), (256,), (10, 256), (10,), (300, 300)]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    for bits in ec.BITS:
        for kw in ({}, {"ef": True}, {"two_phase": True, "ef": True}, {"num_users": 3}):
            q = PSQuantizer(EdenCompressor, params, make_args(eden_bits=bits, **kw))
            assert [type(c) for c in q.codecs] == [EdenCodec, DenseCodec, EdenCodec, DenseCodec, EdenCodec]
            assert [g[0] for g in q._groups] == [BatchedEden] and q._groups[0][1] == [0, 2, 4] and q._draw_total == 0
            assert q.wire_bytes_per_user() == (sum(ec.section_bytes(p.numel(), bits) for p in params if p.numel() > 1000) + 4 * 266 + 15) // 16 * 16


def test_refused_in_ring_mode_with_momentum_correction_and_with_bfloat16_parameters():
    from gq_amd.compressors import EdenCompressor
    from gq_amd.quantizers import PSQuantizer, Quantizer, RingQuantizer
    params = [torch.nn.Parameter(torch.zeros(2000))]
    with pytest.raises(ValueError, match="eden compressor is not available in ring mode"):
        RingQuantizer(EdenCompressor, params, make_args(mode="ring"))
    with pytest.raises(ValueError, match="eden compressor is not available in ring mode"):
        Quantizer(EdenCompressor, params, make_args(mode="ring", eden_scale="mse", eden_bits=2))
    with pytest.raises(ValueError, match="momentum_correction needs TopKSparsificationCompressor"):
        PSQuantizer(EdenCompressor, params, make_args(momentum_correction=0.9))
    assert type(Quantizer(EdenCompressor, params, make_args())) is PSQuantizer


@pytest.mark.parametrize("bits", ec.BITS)
def test_resnet50_wire_bytes(bits):
    """Host arithmetic: the ResNet-50 list's wire per user, the figures the README quotes, against the dense 94,083,376 bytes."""
    from gq_amd.compressors import EdenCompressor
    from gq_amd.quantizers import PSQuantizer
    with open(os.path.join(HERE, "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    q = PSQuantizer(EdenCompressor, params, make_args(eden_bits=bits))
    dense = sum(4 * p.numel() for p in params if p.numel() <= 1000)
    want = sum(ec.section_bytes(p.numel(), bits) for p in params if p.numel() > 1000) + dense
    assert q.wire_bytes_per_user() == (want + 15) // 16 * 16 == RESNET50_BYTES[bits]
    assert (bits + 0.125) / 32 < q.wire_bytes_per_user() / 94083376 < (bits + 0.17) / 32
    assert "{:,}".format(RESNET50_BYTES[bits]) in open(os.path.join(ROOT, "README.md")).read()
    if bits == 4:
        assert RESNET50_BYTES[4] < 12573200      # (the fp4 microscaling wire)


def test_eden_library_is_built_and_exports_its_abi():
    from gq_amd import native
    if not os.path.exists(native.EDEN_LIB_PATH):
        pytest.fail("libgq_eden.so is not built (build() makes it)")
    L = native.eden_lib()
    assert L.gq_eden_abi_version() == native.EDEN_ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "gq_eden.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)      # declarations only: the comments name the entry points too
    declared = sorted(set(re.findall(r"\b(gq_eden_\w+)\s*\(", code)))
    assert declared == sorted(native.EDEN_EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", native.EDEN_LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("gq"))
    assert exported == declared
    assert "#define GQ_EDEN_ABI_VERSION %d" % native.EDEN_ABI_VERSION in hdr
    assert "#define GQ_EDEN_BLOCK %d" % native.EDEN_BLOCK in hdr and native.EDEN_BLOCK == ec.BLOCK == native.MXR_BLOCK
    assert "#define GQ_EDEN_UNBIASED %d" % native.EDEN_UNBIASED in hdr and "#define GQ_EDEN_MSE %d" % native.EDEN_MSE in hdr
    assert "#define GQ_EDEN_MIN_BITS %d" % min(native.EDEN_BITS) in hdr and "#define GQ_EDEN_MAX_BITS %d" % max(native.EDEN_BITS) in hdr
    assert native.EDEN_SCALES == ec.MODES and native.EDEN_BITS == ec.BITS and native.MX_ITEM_ELEMS % native.EDEN_BLOCK == 0
    assert ctypes.sizeof(native._EdenBatchStruct) == 88 and native._EdenBatchStruct.signs.offset == 56      # (eden.hip static_asserts the size)
    names = [f[0] for f in native._EdenBatchStruct._fields_]
    assert names == [f[0] for f in native._DriveBatchStruct._fields_][:-1] + ["bits", "reserved", "signs"]
    # the rotation is one header, included and not copied; the file starts from the small libraries' prelude
    text = open(os.path.join(ROOT, "gradient-quantization_amd", "csrc", "eden.hip")).read()
    assert '#include "hadamard.hpp"' in text and '#include "gq_lib_prelude.hpp"' in text and '#include "rotq_kernels.hpp"' in text
    assert "__global__" not in text
    body = text.split("#include", 1)[1]
    assert "ds_swizzle" not in body and "update_dpp" not in body and "__shared__" not in body and "__syncthreads" not in body


def test_descriptor_needs_a_device_table():
    from gq_amd import native
    with pytest.raises(native.GQNativeError):
        native.EdenBatch(torch.zeros(8, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 1, 1, bits=3, signs=ec.SEEDED)
