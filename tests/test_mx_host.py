"""The microscaling compressor, host side (no GPU): driver choice and flag, the wire's size, the group layout, the library's ABI and
its loader, the refusals that need no device."""
import ctypes
import os
import re
import subprocess
import sys
from argparse import Namespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp",
                num_users=1, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


def test_driver_offers_mx_and_its_flag():
    from gq_amd import driver
    from gq_amd.compressors import MXCompressor
    assert driver.quantizer_choices["mx"] is MXCompressor
    p = driver.build_parser()
    assert p.parse_args(["--quantizer", "mx"]).mx_format == "fp4"
    assert p.parse_args(["--quantizer", "mx", "--mx-format", "fp8"]).mx_format == "fp8"
    with pytest.raises(SystemExit):
        p.parse_args(["--quantizer", "mx", "--mx-format", "fp6"])
    assert MXCompressor(2000, (2000,), make_args()).format == "fp4"      # args without the attribute: the default
    assert MXCompressor(2000, (2000,), make_args(mx_format="fp8", random=1)).random is True
    with pytest.raises(ValueError):
        MXCompressor(2000, (2000,), make_args(mx_format="fp6"))
    import gq_amd.compressors as C
    assert "MXCompressor" in C.__all__


@pytest.mark.parametrize("n", [1, 31, 32, 33, 511, 512, 513, 4096, 4097, 200704, 25000000])
def test_section_bytes_follow_the_header(n):
    from gq_amd import native
    from gq_amd.codecs import MXCodec, mx_section_bytes
    from gq_amd.compressors import MXCompressor
    nb = (n + 31) // 32
    for name, fmt, per_block in (("fp4", native.MX_FP4, 16), ("fp8", native.MX_FP8, 32)):
        want = (nb + 15) // 16 * 16 + per_block * nb
        assert mx_section_bytes(n, name) == mx_section_bytes(n, fmt) == want == mx.section_bytes(n, fmt)
        cd = MXCodec(MXCompressor(n, (n,), make_args(mx_format=name)), n, (n,))
        assert cd.nbytes == want and cd.format == fmt
    with pytest.raises(ValueError):
        MXCodec(MXCompressor(0, (0,), make_args()), 0, (0,))


def test_resnet50_wire_bytes():
    """Host arithmetic: the ResNet-50 list's wire per user against the dense 94,083,376 bytes."""
    import json
    from gq_amd.compressors import MXCompressor
    from gq_amd.quantizers import PSQuantizer
    with open(os.path.join(HERE, "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    assert (4 * sum(p.numel() for p in params) + 15) // 16 * 16 == 94083376      # the dense wire, 16-byte aligned
    got = {}
    for fmt in ("fp4", "fp8"):
        q = PSQuantizer(MXCompressor, params, make_args(mx_format=fmt))
        dense = sum(4 * p.numel() for p in params if p.numel() <= 1000)
        want = sum(mx.section_bytes(p.numel(), mx.FP4 if fmt == "fp4" else mx.FP8) for p in params if p.numel() > 1000) + dense
        assert q.wire_bytes_per_user() == (want + 15) // 16 * 16
        got[fmt] = q.wire_bytes_per_user() / 94083376
    assert 4.25 / 32 < got["fp4"] < 4.3 / 32 and 8.25 / 32 < got["fp8"] < 8.3 / 32


def test_both_factories_route_to_the_codec_and_the_quantizers_group_it():
    from gq_amd.codecs import BatchedMX, DenseCodec, MXCodec, default_codec_factory, quantizer_codec_factory
    from gq_amd.compressors import MXCompressor
    from gq_amd.quantizers import PSQuantizer, RingQuantizer
    c = MXCompressor(5000, torch.Size([5000]), make_args())
    for factory in (default_codec_factory, quantizer_codec_factory):
        cd = factory(c, 5000, torch.Size([5000]))
        assert type(cd) is MXCodec and BatchedMX.eligible(cd)
    shapes = [(256, 784), (256,), (10, 256), (10,), (300, 300)]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    for cls, mode in ((PSQuantizer, "ps"), (RingQuantizer, "ring")):
        q = cls(MXCompressor, params, make_args(mode=mode, random=1, gq_rng="reference"))
        assert [type(c) for c in q.codecs] == [MXCodec, DenseCodec, MXCodec, DenseCodec, MXCodec]
        assert [g[0] for g in q._groups] == [BatchedMX] and q._groups[0][1] == [0, 2, 4]
        ns = [q.codecs[i].numel for i in (0, 2, 4)]
        assert q._draw_total == sum(ns) and q._draw_off == {0: 0, 2: ns[0], 4: ns[0] + ns[1]}      # one uniform per element
        assert all(off % 16 == 0 for c, off in zip(q.codecs, q.offsets) if type(c) is MXCodec)
    assert PSQuantizer(MXCompressor, params, make_args(random=1))._draw_total == 0          # gq_rng = "device": no host draws
    assert PSQuantizer(MXCompressor, params, make_args(gq_rng="reference"))._draw_total == 0      # deterministic: no draws at all
    # groups by format, rounding and generator
    keys = {BatchedMX.group_key(MXCodec(MXCompressor(5000, (5000,), make_args(mx_format=f, random=r)), 5000, (5000,)))
            for f in ("fp4", "fp8") for r in (0, 1)}
    assert len(keys) == 4


def test_group_layout_offsets(monkeypatch):
    """BatchedMX's own layout code, run without a device: the segment table it hands to _setup -- elements, first item, wire
    offset, out offset (16-byte aligned views), first draw -- the item table and the output buffer's size, against expectations
    worked out here from the header's rules."""
    import numpy as np
    from gq_amd.codecs import BatchedMX, DenseCodec, MXCodec
    from gq_amd.compressors import IdenticalCompressor, MXCompressor
    sizes = [1, 4096, 4097, 33, 3 * 4096 + 1]
    comp = MXCompressor(1, (1,), make_args(random=1))
    # the quantizer's parameter list: an identity-compressed tensor between the group's (idxs skips it), wire offsets as it lays them out
    codecs = [MXCodec(comp, n, (n,)) for n in sizes]
    codecs.insert(2, DenseCodec(IdenticalCompressor(), 10, (10,)))
    idxs = [0, 1, 3, 4, 5]
    offsets, off = [0] * 6, 0
    for i in idxs:
        offsets[i] = off
        off += codecs[i].nbytes
    offsets[2] = off
    seen = {}

    def capture(self, table, extra, device, slots, user_bytes, dense=None):
        seen.update(table=table.clone(), extra=extra, slots=slots, user_bytes=user_bytes, dense=dense)

    monkeypatch.setattr(BatchedMX, "_setup", capture)
    g = object.__new__(BatchedMX)
    nseg, items = g._layout(codecs, offsets, idxs, torch.device("cpu"), 3, off + 48, dense=[(off, 10)])
    t = seen["table"].numpy()
    assert (nseg, items) == (5, 9) and t.shape == (5, 8) and seen["extra"] is None and seen["dense"] == [(off, 10)]
    assert t[:, 1].tolist() == sizes                                   # elements
    assert t[:, 2].tolist() == [0, 1, 2, 4, 5]                         # first item: ceil(n / 4096) items per tensor
    want_off = [0, 32, 32 + 16 * 128 + 128, 0, 0]                      # sections: _up(nb) + 16 nb bytes (fp4)
    want_off[3] = want_off[2] + 16 * 129 + 144
    want_off[4] = want_off[3] + 16 * 2 + 16
    assert t[:, 3].tolist() == want_off == [offsets[i] for i in idxs]  # wire offset
    assert all(o % 16 == 0 for o in want_off)
    assert t[:, 5].tolist() == [0, 4, 4100, 8200, 8236] == g.out_off   # out offset: every view starts on a multiple of 4 floats
    assert t[:, 6].tolist() == [0, 1, 4097, 8194, 8227] == g._first_draw      # first draw: the elements of the tensors before
    assert np.all(t[:, [0, 4, 7]] == 0)                                # pointers are the upload's, column 4 is unused
    assert g.item_seg.tolist() == [0, 1, 2, 2, 3, 4, 4, 4, 4] and g.item_seg.dtype == torch.int32
    assert g.out_floats == 8236 + 12292 and g.ndraws == sum(sizes) and g.idxs == idxs
    assert [mx.items_of(n) for n in sizes] == [1, 1, 2, 1, 4] and [mx.section_bytes(n, mx.FP4) for n in sizes] == [codecs[i].nbytes for i in idxs]


def test_mx_library_is_built_and_exports_its_abi():
    from gq_amd import native
    if not os.path.exists(native.MX_LIB_PATH):
        pytest.fail("libgq_mx.so is not built (build() makes it)")
    L = native.mx_lib()
    assert L.gq_mx_abi_version() == native.MX_ABI_VERSION
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "gq_mx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)      # declarations only: the comments name the entry points too
    declared = sorted(set(re.findall(r"\b(gq_mx_\w+)\s*\(", code)))
    assert declared == sorted(native.MX_EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", native.MX_LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("gq"))
    assert exported == declared
    assert "#define GQ_MX_ABI_VERSION %d" % native.MX_ABI_VERSION in hdr
    assert "#define GQ_MX_ITEM_ELEMS %d" % native.MX_ITEM_ELEMS in hdr
    assert "#define GQ_MX_BLOCK %d" % native.MX_BLOCK in hdr
    assert "#define GQ_MX_FP4 %d" % native.MX_FP4 in hdr and "#define GQ_MX_FP8 %d" % native.MX_FP8 in hdr
    assert ctypes.sizeof(native._MXBatchStruct) == 48      # (mx.hip static_asserts the same size)


def test_loader_finds_the_library_like_the_others(tmp_path):
    """tests/test_native_loader.py's check for this library: a missing file and a stale ABI fail at the accessor."""
    from gq_amd import native
    desc, accessor, name = native.MX_LIBRARY, native.mx_lib, "libgq_mx.so"
    assert desc.name == name and os.path.basename(desc.path) == name
    saved = (desc.path, desc.abi, desc.handle)
    try:
        desc.handle = None
        desc.path = str(tmp_path / name)
        with pytest.raises(native.GQNativeError) as e:
            accessor()
        assert name + " not found at " + desc.path in str(e.value) and "build.py" in str(e.value)
        assert desc.handle is None
        desc.path = saved[0]
        desc.abi = saved[1] + 1
        with pytest.raises(native.GQNativeError) as e:
            accessor()
        assert str(e.value) == "%s has ABI version %d, this binding is written for %d: rebuild it" % (saved[0], saved[1], saved[1] + 1)
        assert desc.handle is None
    finally:
        desc.path, desc.abi, desc.handle = saved
    assert accessor() is not None and desc.handle is accessor()


def test_momentum_correction_stays_refused():
    from gq_amd.compressors import MXCompressor
    from gq_amd.quantizers import PSQuantizer, RingQuantizer
    params = [torch.nn.Parameter(torch.zeros(2000))]
    with pytest.raises(ValueError, match="TopKSparsificationCompressor"):
        PSQuantizer(MXCompressor, params, make_args(momentum_correction=0.9))
    with pytest.raises(ValueError, match="ring mode"):
        RingQuantizer(MXCompressor, params, make_args(mode="ring", momentum_correction=0.9))


def test_calls_fail_loudly_without_a_gpu_tensor():
    from gq_amd import native
    from gq_amd.codecs import MXCodec
    from gq_amd.compressors import MXCompressor
    c = MXCompressor(2048, (2048,), make_args())
    cd = MXCodec(c, 2048, torch.Size([2048]))
    with pytest.raises(native.GQNativeError):
        cd.encode_into(torch.randn(2048), torch.zeros(cd.nbytes, dtype=torch.uint8), 0, 0)
    with pytest.raises(TypeError):
        c.compress(torch.randn(2048))
    with pytest.raises(native.GQNativeError):
        native.MXBatch(torch.zeros(8, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 1, 1)
