"""The rotated 1-bit compressor, host side (no GPU): DriveCompressor's arguments and refusals, the wire's size, the driver flags, the
codec and group classes, the refusals in ring mode, with bfloat16 parameters and with momentum correction, the ResNet-50 wire
bytes the README quotes, the library's ABI."""
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
import drive_contract as dc  # noqa: E402
import mxr_contract as mxr  # noqa: E402
from test_mx_host import make_args  # noqa: E402

ROOT = os.path.dirname(HERE)


def test_compressor_arguments_and_refusals():
    from gq_amd import compressors
    from gq_amd.compressors import DriveCompressor, MXCompressor
    assert "DriveCompressor" in compressors.__all__
    c = DriveCompressor(2000, (2000,), make_args())
    assert c.scale == "unbiased" and c.seed == 1 and c.signs == mxr.sign_words(1) == MXCompressor.sign_words(1)
    c = DriveCompressor(2000, (2000,), make_args(drive_scale=None, drive_seed=None))
    assert c.scale == "unbiased" and c.seed == 1
    c = DriveCompressor(2000, (2000,), make_args(drive_scale="mse", drive_seed=7))
    assert c.scale == "mse" and c.signs == mxr.sign_words(7) != mxr.sign_words(1) and all(0 <= w < 1 << 64 for w in c.signs)
    for bad in ("MSE", "eden", 1, True):
        with pytest.raises(ValueError, match="drive_scale"):
            DriveCompressor(2000, (2000,), make_args(drive_scale=bad))
    c = DriveCompressor(2000, (2000,), make_args())
    for t in (torch.zeros(2000), torch.zeros(2000, dtype=torch.bfloat16), torch.zeros(2000, dtype=torch.float64)):
        with pytest.raises(TypeError, match="float32 tensors on the HIP device"):
            c.compress(t)
    sig = torch.ones(3)
    assert c.decompress(sig) is sig


def test_section_bytes():
    from gq_amd.codecs import DriveCodec, drive_section_bytes
    from gq_amd.compressors import DriveCompressor
    assert [drive_section_bytes(n) for n in (1, 256, 257, 1024, 1025, 4096)] == [48, 48, 80, 144, 192, 576]
    for n in (1, 7, 255, 256, 257, 4095, 4097, 200704, 2359296):
        assert drive_section_bytes(n) == dc.section_bytes(n) and drive_section_bytes(n) % 16 == 0
        assert DriveCodec(DriveCompressor(n, (n,), make_args()), n, (n,)).nbytes == dc.section_bytes(n)
    assert drive_section_bytes(1 << 20) * 8 / (1 << 20) == 1.125
    with pytest.raises(ValueError):
        DriveCodec(DriveCompressor(0, (0,), make_args()), 0, (0,))


def test_driver_flags():
    from gq_amd import driver
    from gq_amd.compressors import DriveCompressor
    assert driver.quantizer_choices["drive"] is DriveCompressor
    p = driver.build_parser()
    a = p.parse_args(["--quantizer", "drive"])
    assert a.drive_scale == "unbiased" and a.drive_seed == 1
    a = p.parse_args(["--quantizer", "drive", "--drive-scale", "mse", "--drive-seed", "9"])
    assert a.drive_scale == "mse" and a.drive_seed == 9
    with pytest.raises(SystemExit):
        p.parse_args(["--quantizer", "drive", "--drive-scale", "l2"])
    a = p.parse_args(["--quantizer", "drive", "--param-dtype", "bfloat16"])
    with pytest.raises(ValueError, match="bfloat16 needs --quantizer mx"):
        driver.check_param_dtype(a)


def test_codec_and_group_classes():
    from gq_amd.codecs import BatchedDrive, BatchedMXR, DenseCodec, DriveCodec, default_codec_factory, quantizer_codec_factory
    from gq_amd.compressors import DriveCompressor
    from gq_amd.quantizers import PSQuantizer
    comp = DriveCompressor(5000, torch.Size([5000]), make_args(drive_scale="mse"))
    for factory in (default_codec_factory, quantizer_codec_factory):
        cd = factory(comp, 5000, torch.Size([5000]))
        assert type(cd) is DriveCodec and BatchedDrive.eligible(cd) and not BatchedMXR.eligible(cd) and cd.GROUP is BatchedDrive
        assert cd.signs == mxr.sign_words(1) and cd.scale_mode == 1 and cd.dtype == torch.float32

    def key(**kw):
        return BatchedDrive.group_key(DriveCodec(DriveCompressor(5000, (5000,), make_args(**kw)), 5000, (5000,)))

    assert key() == key(drive_seed=1, drive_scale="unbiased") and key() != key(drive_seed=2) and key() != key(drive_scale="mse")
    assert len({key(drive_seed=s, drive_scale=m) for s in (1, 2) for m in ("unbiased", "mse")}) == 4
    assert sorted([key(drive_seed=2), key()]) is not None       # (the quantizer sorts its groups by key)
    shapes = [(256, 784), (256,), (10, 256), (10,), (300, 300)]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    for kw in ({}, {"ef": True}, {"two_phase": True, "ef": True}, {"num_users": 3}):
        q = PSQuantizer(DriveCompressor, params, make_args(**kw))
        assert [type(c) for c in q.codecs] == [DriveCodec, DenseCodec, DriveCodec, DenseCodec, DriveCodec]
        assert [g[0] for g in q._groups] == [BatchedDrive] and q._groups[0][1] == [0, 2, 4] and q._draw_total == 0
        assert q.wire_bytes_per_user() == (sum(dc.section_bytes(p.numel()) for p in params if p.numel() > 1000) + 4 * 266 + 15) // 16 * 16


def test_refused_in_ring_mode_with_momentum_correction_and_with_bfloat16_parameters():
    from gq_amd.compressors import DriveCompressor
    from gq_amd.quantizers import PSQuantizer, Quantizer, RingQuantizer
    params = [torch.nn.Parameter(torch.zeros(2000))]
    with pytest.raises(ValueError, match="ring mode"):
        RingQuantizer(DriveCompressor, params, make_args(mode="ring"))
    with pytest.raises(ValueError, match="ring mode"):
        Quantizer(DriveCompressor, params, make_args(mode="ring", drive_scale="mse"))
    with pytest.raises(ValueError, match="momentum_correction needs TopKSparsificationCompressor"):
        PSQuantizer(DriveCompressor, params, make_args(momentum_correction=0.9))
    assert type(Quantizer(DriveCompressor, params, make_args())) is PSQuantizer


def test_resnet50_wire_bytes():
    """Host arithmetic: the ResNet-50 list's wire per user, the figure the README quotes, against the dense 94,083,376 bytes."""
    from gq_amd.compressors import DriveCompressor
    from gq_amd.quantizers import PSQuantizer
    with open(os.path.join(HERE, "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    q = PSQuantizer(DriveCompressor, params, make_args())
    dense = sum(4 * p.numel() for p in params if p.numel() <= 1000)
    want = sum(dc.section_bytes(p.numel()) for p in params if p.numel() > 1000) + dense
    assert q.wire_bytes_per_user() == (want + 15) // 16 * 16 == 3394128
    assert 1.125 / 32 < q.wire_bytes_per_user() / 94083376 < 1.16 / 32
    assert "3,394,128" in open(os.path.join(ROOT, "README.md")).read()


def test_drive_library_is_built_and_exports_its_abi():
    from gq_amd import native
    if not os.path.exists(native.DRIVE_LIB_PATH):
        pytest.fail("libgq_drive.so is not built (build() makes it)")
    L = native.drive_lib()
    assert L.gq_drive_abi_version() == native.DRIVE_ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "gq_drive.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)      # declarations only: the comments name the entry points too
    declared = sorted(set(re.findall(r"\b(gq_drive_\w+)\s*\(", code)))
    assert declared == sorted(native.DRIVE_EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", native.DRIVE_LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("gq"))
    assert exported == declared
    assert "#define GQ_DRIVE_ABI_VERSION %d" % native.DRIVE_ABI_VERSION in hdr
    assert "#define GQ_DRIVE_BLOCK %d" % native.DRIVE_BLOCK in hdr and native.DRIVE_BLOCK == dc.BLOCK == native.MXR_BLOCK
    assert "#define GQ_DRIVE_UNBIASED %d" % native.DRIVE_UNBIASED in hdr and "#define GQ_DRIVE_MSE %d" % native.DRIVE_MSE in hdr
    assert native.DRIVE_SCALES == dc.MODES and native.MX_ITEM_ELEMS % native.DRIVE_BLOCK == 0
    assert ctypes.sizeof(native._DriveBatchStruct) == 80 and native._DriveBatchStruct.signs.offset == 48      # (drive.hip static_asserts the size)
    assert [f[0] for f in native._DriveBatchStruct._fields_] == [f[0] if f[0] != "format" else "scale_mode" for f in native._MXRBatchStruct._fields_]
    # the rotation is one header, included by both libraries and defined in neither
    csrc = os.path.join(ROOT, "gradient-quantization_amd", "csrc")
    for f in ("mxr.hip", "drive.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "hadamard.hpp"' in text and "ds_swizzle" not in text.split("#include", 1)[1]
    # drive.hip and eden.hip share their kernels and their host path through one header, which has no exchange of its own
    assert "ds_swizzle" not in open(os.path.join(csrc, "rotq_kernels.hpp")).read()
    for f in ("drive.hip", "eden.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "rotq_kernels.hpp"' in text and "__global__" not in text
    assert "__builtin_amdgcn_ds_swizzle" in open(os.path.join(csrc, "hadamard.hpp")).read()


def test_descriptor_needs_a_device_table():
    from gq_amd import native
    with pytest.raises(native.GQNativeError):
        native.DriveBatch(torch.zeros(8, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 1, 1, signs=dc.SEEDED)
