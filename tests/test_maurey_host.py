"""Maurey sparsification, host side (no GPU): codec routing, the sparse wire's size, the CPU torch path, the library's ABI."""
import os
import re
from argparse import Namespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp",
                num_users=1, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


class _K(object):
    def __init__(self, k):
        self.k = k


def test_maurey_library_is_built_and_exports_its_abi():
    import ctypes
    import subprocess
    from gq_amd import native
    if not os.path.exists(native.MAUREY_LIB_PATH):
        pytest.fail("libgq_maurey.so is not built (build() makes it)")
    L = native.maurey_lib()
    assert L.gq_maurey_abi_version() == native.MAUREY_ABI_VERSION
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "gq_maurey.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)      # declarations only: the comments name the entry points too
    declared = sorted(set(re.findall(r"\b(gq_maurey_\w+)\s*\(", code)))
    assert declared == sorted(native.MAUREY_EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", native.MAUREY_LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("gq"))
    assert exported == declared
    assert "#define GQ_MAUREY_ABI_VERSION %d" % native.MAUREY_ABI_VERSION in hdr
    assert "#define GQ_MAUREY_CHUNK %d" % native.MAUREY_CHUNK in hdr
    assert "#define GQ_MAUREY_HEADER_BYTES %d" % native.MAUREY_HEADER_BYTES in hdr
    assert ctypes.sizeof(native._MaureyBatchStruct) == 96      # (maurey.hip static_asserts the same size)


def test_codec_bytes():
    """16 bytes of header, k words, zero padding to 16."""
    from gq_amd.codecs import MaureyCodec
    for k, want in ((1, 32), (3, 32), (4, 32), (5, 48)):
        assert MaureyCodec(_K(k), 5000, torch.Size([5000])).nbytes == want, k
    with pytest.raises(ValueError):
        MaureyCodec(_K(0), 5000, torch.Size([5000]))


def test_maurey_routes_to_the_sparse_codec():
    from gq_amd.codecs import BatchedMaurey, MaureyCodec, default_codec_factory, quantizer_codec_factory
    from gq_amd.compressors import MaureySparsification
    for n in (5000, 70001):
        c = MaureySparsification(n, torch.Size([n]), make_args())
        bit_for_idx = 32 if n > 65536 else 16
        assert c.cr == 32 * 16 // 14 and c.k == 32 * n // ((bit_for_idx + 1) * c.cr)      # the reference's arithmetic
        for factory in (default_codec_factory, quantizer_codec_factory):
            cd = factory(c, n, torch.Size([n]))
            assert type(cd) is MaureyCodec and cd.k == c.k and cd.nbytes == 16 + (4 * c.k + 15) // 16 * 16
            assert BatchedMaurey.eligible(cd)
    assert MaureySparsification(10, torch.Size([10]), make_args(c_dim=512)).k == 1      # never zero draws


def test_driver_offers_maurey():
    from gq_amd import driver
    from gq_amd.compressors import MaureySparsification
    assert driver.quantizer_choices["maurey"] is MaureySparsification


def test_quantizer_groups_every_maurey_tensor():
    from gq_amd.codecs import BatchedMaurey, DenseCodec, MaureyCodec
    from gq_amd.compressors import MaureySparsification
    from gq_amd.quantizers import PSQuantizer, RingQuantizer
    shapes = [(256, 784), (256,), (10, 256), (10,), (300, 300)]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    for cls, mode in ((PSQuantizer, "ps"), (RingQuantizer, "ring")):
        q = cls(MaureySparsification, params, make_args(mode=mode, gq_rng="reference"))
        assert [type(c) for c in q.codecs] == [MaureyCodec, DenseCodec, MaureyCodec, DenseCodec, MaureyCodec]
        assert [g[0] for g in q._groups] == [BatchedMaurey] and q._groups[0][1] == [0, 2, 4]
        ks = [q.codecs[i].k for i in (0, 2, 4)]
        assert q._draw_total == sum(ks) and q._draw_off == {0: 0, 2: ks[0], 4: ks[0] + ks[1]}      # one uniform per draw
        for c, off in zip(q.codecs, q.offsets):
            if type(c) is MaureyCodec:
                assert off % 16 == 0
    assert PSQuantizer(MaureySparsification, params, make_args())._draw_total == 0      # gq_rng = "device": no host draws


def test_cpu_tensors_keep_the_torch_path():
    from gq_amd.compressors import MaureySparsification
    n = 5000
    c = MaureySparsification(n, torch.Size([n]), make_args())
    torch.manual_seed(7)
    v = torch.randn(n)
    torch.manual_seed(3)
    scale, codes, signs = c.compress(v)
    torch.manual_seed(3)
    mag = v.abs()
    want_codes = torch.multinomial(mag / mag.sum(), c.k, replacement=True)
    assert torch.equal(codes, want_codes) and torch.equal(signs, torch.sign(v[want_codes]))
    assert torch.equal(scale, mag.sum() / c.k)
    dec = c.decompress([scale, codes, signs])
    want = torch.zeros(n)
    want.index_add_(0, want_codes, torch.sign(v[want_codes]))
    assert dec.device.type == "cpu" and torch.equal(dec, scale * want)
    assert hasattr(c, "_device_compress") and not hasattr(c, "_codecs")      # (a kernel path exists; a CPU tensor does not take it)


def test_maurey_calls_fail_loudly_without_a_gpu_tensor():
    from gq_amd import native
    from gq_amd.codecs import MaureyCodec
    cd = MaureyCodec(_K(55), 2048, torch.Size([2048]))
    with pytest.raises(native.GQNativeError):
        cd.encode_into(torch.randn(2048), torch.zeros(cd.nbytes, dtype=torch.uint8), 0, 0)
    with pytest.raises(native.GQNativeError):
        cd.roundtrip(torch.randn(2048), 0)
    with pytest.raises(native.GQNativeError):
        native.MaureyBatch(torch.zeros(8, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 1, 1)
