"""Rotation stepping of the DRIVE and EDEN compressors, host side (no GPU): the driver flags, drive_rotation / eden_rotation and their
refusals, the rotation mode in the groups' keys, the quantizer's rotation_step / set_rotation_step, the refusals in ring mode, the
stepped entry points in the bindings and the headers."""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import rot_step_contract as rs  # noqa: E402
from test_mx_host import make_args  # noqa: E402

ROOT = os.path.dirname(HERE)


def test_driver_flags():
    from gq_amd import driver
    p = driver.build_parser()
    a = p.parse_args(["--quantizer", "drive"])
    assert a.drive_rotation == "fixed" and a.eden_rotation == "fixed"
    a = p.parse_args(["--quantizer", "drive", "--drive-rotation", "step", "--ef"])
    assert a.drive_rotation == "step" and a.eden_rotation == "fixed" and a.ef
    a = p.parse_args(["--quantizer", "eden", "--eden-rotation", "step", "--eden-bits", "2"])
    assert a.eden_rotation == "step" and a.drive_rotation == "fixed"
    for flag in ("--drive-rotation", "--eden-rotation"):
        with pytest.raises(SystemExit):
            p.parse_args(["--quantizer", "drive", flag, "round"])
    helps = {a.dest: a.help for a in p._actions}
    for name in ("drive", "eden"):
        text = helps[name + "_rotation"]
        assert "'step' is what the 'unbiased' scale wants" in text and "'mse' with --ef does not need it" in text


def test_compressor_argument_and_refusals():
    from gq_amd.compressors import DriveCompressor, EdenCompressor
    for cls, name in ((DriveCompressor, "drive_rotation"), (EdenCompressor, "eden_rotation")):
        assert cls(2000, (2000,), make_args()).rotation == "fixed"                    # absent
        assert cls(2000, (2000,), make_args(**{name: None})).rotation == "fixed"
        assert cls(2000, (2000,), make_args(**{name: "fixed"})).rotation == "fixed"
        c = cls(2000, (2000,), make_args(**{name: "step", name.split("_")[0] + "_seed": 9}))
        assert c.rotation == "step" and c.seed == 9 and c.signs == rs.step_words(9, 0)      # (step 0: the fixed words)
        for bad in ("Step", "round", 1, True, ""):
            with pytest.raises(ValueError, match=name):
                cls(2000, (2000,), make_args(**{name: bad}))
        assert cls.rotation_words(9, 3) == rs.step_words(9, 3)
    # the other compressor's flag is not read
    assert DriveCompressor(2000, (2000,), make_args(eden_rotation="step")).rotation == "fixed"
    assert EdenCompressor(2000, (2000,), make_args(drive_rotation="step")).rotation == "fixed"


def test_group_key_holds_the_rotation_mode():
    from gq_amd.codecs import BatchedDrive, BatchedEden, DriveCodec, EdenCodec
    from gq_amd.compressors import DriveCompressor, EdenCompressor

    def dkey(**kw):
        return BatchedDrive.group_key(DriveCodec(DriveCompressor(5000, (5000,), make_args(**kw)), 5000, (5000,)))

    def ekey(**kw):
        return BatchedEden.group_key(EdenCodec(EdenCompressor(5000, (5000,), make_args(**kw)), 5000, (5000,)))

    assert dkey() == dkey(drive_rotation="fixed") != dkey(drive_rotation="step")
    assert ekey() == ekey(eden_rotation="fixed") != ekey(eden_rotation="step")
    assert len({dkey(drive_rotation=r, drive_scale=m, drive_seed=s) for r in ("fixed", "step") for m in ("unbiased", "mse") for s in (1, 2)}) == 8
    assert len({ekey(eden_rotation=r, eden_bits=b) for r in ("fixed", "step") for b in (2, 3, 4)}) == 6
    assert sorted([dkey(drive_rotation="step"), dkey()]) and sorted([ekey(eden_rotation="step"), ekey()])      # (the quantizer sorts its groups by key)
    cd = DriveCodec(DriveCompressor(5000, (5000,), make_args(drive_rotation="step")), 5000, (5000,))
    assert cd.stepped and cd.rotation is None      # (no pair outside a quantizer: step 0)
    assert not DriveCodec(DriveCompressor(5000, (5000,), make_args()), 5000, (5000,)).stepped


@pytest.mark.parametrize("name", ["drive", "eden"])
def test_quantizer_groups_and_rotation_step(name):
    from gq_amd.codecs import BatchedDrive, BatchedEden
    from gq_amd.compressors import DriveCompressor, EdenCompressor
    from gq_amd.quantizers import PSQuantizer, Quantizer
    Comp, Group = (DriveCompressor, BatchedDrive) if name == "drive" else (EdenCompressor, BatchedEden)
    shapes = [(256, 784), (256,), (10, 256), (10,), (300, 300)]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    q = Quantizer(Comp, params, make_args())
    assert type(q) is PSQuantizer
    with pytest.raises(ValueError, match="rotation is fixed"):
        q.rotation_step()
    with pytest.raises(ValueError, match="rotation is fixed"):
        q.set_rotation_step(3)
    q = Quantizer(Comp, params, make_args(**{name + "_rotation": "fixed"}))
    with pytest.raises(ValueError, match="rotation is fixed"):
        q.rotation_step()
    for kw in ({}, {"ef": True}, {"two_phase": True, "ef": True}, {"num_users": 3}):
        q = Quantizer(Comp, params, make_args(**dict(kw, **{name + "_rotation": "step", name + "_seed": 7})))
        assert [g[0] for g in q._groups] == [Group] and q._groups[0][1] == [0, 2, 4] and q._draw_total == 0
        assert all(q.codecs[i].stepped for i in (0, 2, 4))
        assert q.rotation_step() == 0
        q.set_rotation_step(5)
        assert q.rotation_step() == 5
        q.set_rotation_step(2 ** 64 - 1)
        assert q.rotation_step() == 2 ** 64 - 1
        assert q._rotation_seed == 7


def test_ring_mode_goes_on_refusing_both():
    from gq_amd.compressors import DriveCompressor, EdenCompressor
    from gq_amd.quantizers import Quantizer, RingQuantizer
    params = [torch.nn.Parameter(torch.zeros(2000))]
    for Comp, name in ((DriveCompressor, "drive_rotation"), (EdenCompressor, "eden_rotation")):
        for rot in ("fixed", "step"):
            with pytest.raises(ValueError, match="ring mode"):
                RingQuantizer(Comp, params, make_args(mode="ring", **{name: rot}))
            with pytest.raises(ValueError, match="ring mode"):
                Quantizer(Comp, params, make_args(mode="ring", **{name: rot}))


def test_bindings_and_headers_declare_the_stepped_entry_points():
    from gq_amd import native
    for exports, prefix, header in ((native.DRIVE_EXPORTS, "gq_drive_", "gq_drive.h"), (native.EDEN_EXPORTS, "gq_eden_", "gq_eden.h")):
        for call in ("compress_batched", "decode_sum_batched"):
            assert prefix + call in exports and prefix + call + "_stepped" in exports
        hdr = open(os.path.join(ROOT, "include", header)).read()
        assert "SIGNS, STEPPED" in hdr
        code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        for call in ("compress_batched_stepped", "decode_sum_batched_stepped"):
            m = re.search(r"int %s%s\(const %sbatch \*b, const uint64_t \*rotation," % (prefix, call, prefix), code)
            assert m, (header, call)      # the existing signature with the pair after the descriptor
    # the descriptors did not grow
    import ctypes
    assert ctypes.sizeof(native._DriveBatchStruct) == 80 and ctypes.sizeof(native._EdenBatchStruct) == 88
    assert native.DRIVE_ABI_VERSION == 1 and native.EDEN_ABI_VERSION == 1


def test_rotation_argument_of_the_bindings_is_checked():
    from gq_amd import native
    for bad in (torch.zeros((1, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int64), (1, 0)):
        with pytest.raises(TypeError, match="rotation"):
            native._rotation_ptr(bad)
    with pytest.raises(native.GQNativeError):      # a pair in host memory
        native._rotation_ptr(torch.zeros((1, 2), dtype=torch.int64))
