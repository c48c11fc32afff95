"""Per-user rotations of the DRIVE and EDEN compressors, host side (no GPU): the driver flags, drive_user_rotation /
eden_user_rotation and their refusals, the mode in the groups' keys, the *_streams entry points in the bindings and the headers,
ring mode's refusal -- and the stream assignment: on fake ranks (torch.distributed emulated in this process, in the style of
tests/test_exchange_fake_dist.py) with the native descriptors replaced by recorders, the stream handed to the native layer for
(rank, slot) is that payload's row of the gathered buffer, and the aggregate decodes from stream 0."""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import rot_step_contract as rs  # noqa: E402
import rot_user_contract as ru  # noqa: E402
from test_mx_host import make_args  # noqa: E402
from test_exchange_fake_dist import fake_dist  # noqa: E402,F401  (the fixture)

ROOT = os.path.dirname(HERE)


def test_driver_flags():
    from gq_amd import driver
    p = driver.build_parser()
    a = p.parse_args(["--quantizer", "drive"])
    assert a.drive_user_rotation == "shared" and a.eden_user_rotation == "shared"
    a = p.parse_args(["--quantizer", "drive", "--drive-user-rotation", "own", "--drive-rotation", "step"])
    assert a.drive_user_rotation == "own" and a.eden_user_rotation == "shared" and a.drive_rotation == "step"
    a = p.parse_args(["--quantizer", "eden", "--eden-user-rotation", "own"])
    assert a.eden_user_rotation == "own" and a.drive_user_rotation == "shared" and a.eden_rotation == "fixed"
    for flag in ("--drive-user-rotation", "--eden-user-rotation"):
        with pytest.raises(SystemExit):
            p.parse_args(["--quantizer", "drive", flag, "each"])


def test_compressor_argument_and_refusals():
    from gq_amd.compressors import DriveCompressor, EdenCompressor
    for cls, name in ((DriveCompressor, "drive_user_rotation"), (EdenCompressor, "eden_user_rotation")):
        assert cls(2000, (2000,), make_args()).user_rotation == "shared"                    # absent
        assert cls(2000, (2000,), make_args(**{name: None})).user_rotation == "shared"
        assert cls(2000, (2000,), make_args(**{name: "shared"})).user_rotation == "shared"
        c = cls(2000, (2000,), make_args(**{name: "own"}))
        assert c.user_rotation == "own" and c.rotation == "fixed" and c.signs == rs.step_words(1, 0)
        for bad in ("Own", "user", 1, True, ""):
            with pytest.raises(ValueError, match=name):
                cls(2000, (2000,), make_args(**{name: bad}))
        for seed, k in ((1, 0), (1, 1), (9, 7), (2 ** 64 - 1, 2 ** 31 - 1)):
            assert cls.stream_seed(seed, k) == ru.seed_of(seed, k)
            assert cls.rotation_words(cls.stream_seed(seed, k), 3) == ru.words_of(seed, 3, k)
        with pytest.raises(ValueError, match="non-negative"):
            cls.stream_seed(1, -1)
    # the other compressor's flag is not read
    assert DriveCompressor(2000, (2000,), make_args(eden_user_rotation="own")).user_rotation == "shared"
    assert EdenCompressor(2000, (2000,), make_args(drive_user_rotation="own")).user_rotation == "shared"


def test_group_key_holds_the_user_rotation():
    from gq_amd.codecs import BatchedDrive, BatchedEden, DriveCodec, EdenCodec
    from gq_amd.compressors import DriveCompressor, EdenCompressor

    def dkey(**kw):
        return BatchedDrive.group_key(DriveCodec(DriveCompressor(5000, (5000,), make_args(**kw)), 5000, (5000,)))

    def ekey(**kw):
        return BatchedEden.group_key(EdenCodec(EdenCompressor(5000, (5000,), make_args(**kw)), 5000, (5000,)))

    assert dkey() == dkey(drive_user_rotation="shared") != dkey(drive_user_rotation="own")
    assert ekey() == ekey(eden_user_rotation="shared") != ekey(eden_user_rotation="own")
    assert len({dkey(drive_rotation=r, drive_user_rotation=u) for r in ("fixed", "step") for u in ("shared", "own")}) == 4
    assert len({ekey(eden_rotation=r, eden_user_rotation=u) for r in ("fixed", "step") for u in ("shared", "own")}) == 4
    cd = DriveCodec(DriveCompressor(5000, (5000,), make_args(drive_user_rotation="own")), 5000, (5000,))
    assert cd.own and not cd.stepped and cd.rotation is None and cd.stream == 0 and cd.seed == 1
    assert not DriveCodec(DriveCompressor(5000, (5000,), make_args()), 5000, (5000,)).own


def test_bindings_and_headers_declare_the_streams_entry_points():
    from gq_amd import native
    for exports, prefix, header in ((native.DRIVE_EXPORTS, "gq_drive_", "gq_drive.h"), (native.EDEN_EXPORTS, "gq_eden_", "gq_eden.h")):
        hdr = open(os.path.join(ROOT, "include", header)).read()
        assert "SIGNS, PER STREAM" in hdr and "DECODE-MEAN, PER STREAM" in hdr and "0xD6E8FEB86659FD93" in hdr
        code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        assert prefix + "compress_batched_streams" in exports and prefix + "decode_sum_batched_streams" in exports
        assert re.search(r"int %scompress_batched_streams\(const %sbatch \*b, const uint64_t \*rotation, int32_t stream," % (prefix, prefix), code)
        assert re.search(r"int %sdecode_sum_batched_streams\(const %sbatch \*b, const uint64_t \*rotation, int32_t first_stream," % (prefix, prefix),
                         code)
    assert ctypes.sizeof(native._DriveBatchStruct) == 80 and ctypes.sizeof(native._EdenBatchStruct) == 88      # the descriptors did not grow
    assert native.DRIVE_ABI_VERSION == 1 and native.EDEN_ABI_VERSION == 1
    for bad in (1.0, "1", None, True):
        with pytest.raises(TypeError, match="stream"):
            native._stream_arg(bad)
    with pytest.raises(ValueError, match="int32"):
        native._stream_arg(2 ** 31)
    assert native._stream_arg(2 ** 31 - 1).value == 2 ** 31 - 1 and native._stream_arg(-1).value == -1      # (the library refuses it)


def test_ring_mode_goes_on_refusing_both():
    from gq_amd.compressors import DriveCompressor, EdenCompressor
    from gq_amd.quantizers import Quantizer, RingQuantizer
    params = [torch.nn.Parameter(torch.zeros(2000))]
    for Comp, name in ((DriveCompressor, "drive_user_rotation"), (EdenCompressor, "eden_user_rotation")):
        for mode in ("shared", "own"):
            with pytest.raises(ValueError, match="ring mode"):
                RingQuantizer(Comp, params, make_args(mode="ring", **{name: mode}))
            with pytest.raises(ValueError, match="ring mode"):
                Quantizer(Comp, params, make_args(mode="ring", **{name: mode}))


# ---- the stream assignment ------------------------------------------------------------------------------------------------------------
class _Recorder(object):
    """In the place of native.DriveBatch / native.EdenBatch: notes what each launch would have been handed."""

    calls = []

    def __init__(self, *a, **k):
        pass

    def part(self, *a):
        return self

    def set_table(self, *a):
        pass

    def set_dense(self, *a):
        pass

    def compress(self, wire, out=None, ef_scale=None, rotation=None, stream=None):
        _Recorder.calls.append(("compress", wire.data_ptr(), stream, rotation))

    def decode(self, gathered, R, out, plain=False, rotation=None, first_stream=None):
        _Recorder.calls.append(("decode", R, first_stream, rotation))


@pytest.fixture
def host_only(monkeypatch):
    """The quantizer's per-tensor route on CPU tensors down to the native descriptor, which is a recorder: no device is touched."""
    from gq_amd import codecs, native
    monkeypatch.setattr(native, "DriveBatch", _Recorder)
    monkeypatch.setattr(native, "EdenBatch", _Recorder)
    monkeypatch.setattr(codecs, "_require_device", lambda *a, **k: None)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: self)
    monkeypatch.setattr(codecs.BatchedDrive, "_choose_header", lambda self, *a, **k: True)
    monkeypatch.setattr(codecs.BatchedDrive, "upload_layout", lambda self: None)
    _Recorder.calls = []
    return _Recorder


SHAPES = [(5000,), (10,), (60, 50)]
USERS = 2


def _quantizer(name, **kw):
    from gq_amd import quantizers
    from gq_amd.compressors import DriveCompressor, EdenCompressor
    params = [torch.nn.Parameter(torch.zeros(*s)) for s in SHAPES]
    args = make_args(num_users=USERS, no_cuda=True, **dict({name + "_user_rotation": "own", name + "_seed": 5}, **kw))
    return quantizers.Quantizer(DriveCompressor if name == "drive" else EdenCompressor, params, args), params


@pytest.mark.parametrize("name", ["drive", "eden"])
@pytest.mark.parametrize("world", [1, 2, 4])
def test_the_stream_of_rank_and_slot_is_the_payloads_row_of_the_gather(fake_dist, host_only, monkeypatch, name, world):  # noqa: F811
    import torch.distributed as dist
    if world > 1:
        w = fake_dist(world)
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "is_available", lambda: True)
        monkeypatch.setattr(dist, "get_world_size", lambda group=None: world)
        monkeypatch.setattr(dist, "get_rank", lambda group=None: w.current)
    ranks = []
    for r in range(world):
        if world > 1:
            w.current = r
        q, params = _quantizer(name)
        for slot in range(USERS):
            for p in params:
                p.grad = torch.randn(p.shape)
            before = len(host_only.calls)
            q.record(slot, epoch=1)
            mine = host_only.calls[before:]
            # the two compressed tensors of this record, both under ONE stream, written into row `slot` of this rank's block
            assert [c[0] for c in mine] == ["compress", "compress"]
            row = q._wire[slot]
            assert all(row.data_ptr() <= c[1] < row.data_ptr() + q.user_bytes for c in mine)
            streams = set(c[2] for c in mine)
            assert len(streams) == 1
            stream = streams.pop()
            # ... and that row's place in the gathered buffer IS the stream (gq_amd.exchange: row = rank * users + user)
            if world > 1:
                gathered = q._ex.gathered
                assert gathered.shape[0] == world * USERS
                index = (row.data_ptr() - gathered.data_ptr()) // gathered.stride(0)
            else:
                index = (row.data_ptr() - q._wire.data_ptr()) // q._wire.stride(0)
            assert stream == index == r * USERS + slot, (world, r, slot, stream, index)
            assert all(c[3] is not None and c[3].tolist() == [[5, 0]] for c in mine)      # the pair of the seed, step 0
            assert all(cd.stream == 0 for cd in q.codecs if getattr(cd, "own", False))    # (left at 0 for every other compress)
        ranks.append(q)
    # the aggregate: every row of the gather, from stream 0
    q = ranks[0]
    if world > 1:
        w.current = 0
        monkeypatch.setattr(q._ex, "start", lambda *a, **k: (q._ex.gathered, ()))      # (the transfers are not this test's subject)
    before = len(host_only.calls)
    q.apply()
    dec = [c for c in host_only.calls[before:] if c[0] == "decode"]
    assert len(dec) == 2 and all(c[1] == world * USERS and c[2] == 0 for c in dec), dec


def test_shared_hands_no_stream_to_the_native_layer(host_only):
    q, params = _quantizer("drive", drive_user_rotation="shared")
    for slot in range(USERS):
        for p in params:
            p.grad = torch.randn(p.shape)
        q.record(slot, epoch=1)
    q.apply()
    assert host_only.calls and all(c[2] is None and c[3] is None for c in host_only.calls), host_only.calls


def test_two_phase_recompresses_under_stream_zero(host_only):
    q, params = _quantizer("drive", two_phase=True)
    for slot in range(USERS):
        for p in params:
            p.grad = torch.randn(p.shape)
        q.record(slot, epoch=1)
    before = len(host_only.calls)
    q.apply()
    second = [c for c in host_only.calls[before:] if c[0] == "compress"]
    assert len(second) == 2 and all(c[2] == 0 for c in second), second


def test_several_ranks_need_every_slot_recorded(fake_dist, host_only, monkeypatch):  # noqa: F811
    """Fewer records than slots are gathered at rank * recorded + slot: not the rows the streams were numbered with."""
    import torch.distributed as dist
    w = fake_dist(2)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: w.current)
    q, params = _quantizer("drive")
    for p in params:
        p.grad = torch.randn(p.shape)
    q.record(0, epoch=1)
    with pytest.raises(RuntimeError, match="every slot recorded"):
        q.apply()
