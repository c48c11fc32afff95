"""signSGD, host side (no GPU): codec routing, the 2-bit wire's size, the CPU torch path, the library's ABI."""
import json
import os
from argparse import Namespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp",
                num_users=1, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


def _resnet50_params():
    with open(os.path.join(GOLDEN, "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    return [torch.nn.Parameter(torch.zeros(s)) for s in shapes]


def test_sign_routes_to_the_2bit_codec():
    from gq_amd.codecs import BatchedSign, DenseCodec, SignCodec, default_codec_factory
    from gq_amd.compressors import IdenticalCompressor, SignSGDCompressor
    for n, want in ((5000, 1264), (1001, 256), (4096, 1024), (4097, 1040), (16, 16), (17, 16)):
        cd = default_codec_factory(SignSGDCompressor(n, torch.Size([n]), make_args()), n, torch.Size([n]))
        assert type(cd) is SignCodec and cd.nbytes == want, (n, cd.nbytes)
        assert BatchedSign.eligible(cd)
    assert type(default_codec_factory(IdenticalCompressor(), 10, torch.Size([10]))) is DenseCodec


def test_quantizer_groups_every_sign_tensor():
    from gq_amd.codecs import BatchedSign, SignCodec
    from gq_amd.compressors import SignSGDCompressor
    from gq_amd.quantizers import PSQuantizer
    q = PSQuantizer(SignSGDCompressor, _resnet50_params(), make_args())
    sign = [i for i, c in enumerate(q.codecs) if type(c) is SignCodec]
    assert len(sign) == 76 and sum(q.codecs[i].numel for i in sign) == 23_498_432
    assert [g[0] for g in q._groups] == [BatchedSign] and sorted(q._groups[0][1]) == sign


def test_resnet50_wire_is_2bit():
    """5,874,608 B of 2-bit sections per user (the decoded dense f32 was 93,993,728 B) + the 89,640 B dense region, rounded
    up to 16 B."""
    from gq_amd.codecs import SignCodec
    from gq_amd.compressors import SignSGDCompressor
    from gq_amd.quantizers import PSQuantizer
    q = PSQuantizer(SignSGDCompressor, _resnet50_params(), make_args())
    packed = sum(c.nbytes for c in q.codecs if type(c) is SignCodec)
    assert packed == 5_874_608
    assert q.dense_bytes == 89_640
    assert q.wire_bytes_per_user() == 5_964_256
    for c, off in zip(q.codecs, q.offsets):
        if type(c) is SignCodec:
            assert off % 16 == 0 and c.nbytes == -(-(-(-c.numel // 16) * 4) // 16) * 16


def test_ring_uses_the_2bit_codec():
    """The wire holds sign(v) exactly (no -0, no NaN), so the ring's hops may travel on it too."""
    from gq_amd.codecs import SignCodec
    from gq_amd.compressors import SignSGDCompressor
    from gq_amd.quantizers import RingQuantizer
    q = RingQuantizer(SignSGDCompressor, _resnet50_params(), make_args(mode="ring"))
    assert all(type(c) is SignCodec for c in q.codecs if c.numel > 1000)


def test_cpu_tensors_keep_torch_sign():
    from gq_amd.compressors import SignSGDCompressor
    torch.manual_seed(0)
    n = 4096
    c = SignSGDCompressor(n, torch.Size([n]), make_args())
    v = torch.randn(n)
    v[:4] = torch.tensor([0.0, -0.0, float("nan"), -float("inf")])
    got = c.decompress(c.compress(v))
    assert got.device.type == "cpu"
    assert torch.equal(got.view(torch.int32), torch.sign(v).view(torch.int32))
    assert hasattr(c, "_device_roundtrip") and not hasattr(c, "_codecs")      # (a kernel path exists; a CPU tensor does not take it)


def test_sign_library_is_built_and_exports_its_abi():
    import ctypes
    import subprocess
    from gq_amd import native
    if not os.path.exists(native.SIGN_LIB_PATH):
        pytest.fail("libgq_sign.so is not built (build() makes it)")
    L = native.sign_lib()
    assert L.gq_sign_abi_version() == native.SIGN_ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", native.SIGN_LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("gq"))
    assert exported == sorted(native.SIGN_EXPORTS)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "gq_sign.h")).read()
    for name in native.SIGN_EXPORTS:
        assert name + "(" in hdr
    assert "#define GQ_SIGN_ABI_VERSION %d" % native.SIGN_ABI_VERSION in hdr
    assert "#define GQ_SIGN_ITEM_BYTES %d" % native.SIGN_ITEM_BYTES in hdr
    assert ctypes.sizeof(native._SignBatchStruct) == 48      # (sign.hip static_asserts the same size)


def test_sign_calls_fail_loudly_without_a_gpu_tensor():
    from gq_amd import native
    from gq_amd.codecs import SignCodec
    from gq_amd.compressors import SignSGDCompressor
    cd = SignCodec(SignSGDCompressor(2048, torch.Size([2048]), make_args()), 2048, torch.Size([2048]))
    with pytest.raises(native.GQNativeError):
        cd.encode_into(torch.randn(2048), torch.zeros(cd.nbytes, dtype=torch.uint8), 0, 0)
    with pytest.raises(native.GQNativeError):
        cd.roundtrip(torch.randn(2048), 0)
    with pytest.raises(native.GQNativeError):
        native.SignBatch(torch.zeros(8, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 1, 1)
