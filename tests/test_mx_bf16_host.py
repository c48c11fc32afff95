"""bf16 through the microscaling compressor's host layers, without a GPU: the four new entry points in the headers and in the
binding's export lists, an ABI that did not move, group keys that split by dtype, a bf16 group's layout, float32 error buffers,
and the driver's refusal of --param-dtype bfloat16 with any other quantizer."""
import ctypes
import os
import re
import subprocess
import sys
from argparse import Namespace
from types import SimpleNamespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "gradient-quantization_amd"))

from gq_amd import native  # noqa: E402
from gq_amd.codecs import BatchedMX, BatchedMXR, MXCodec, MXRCodec  # noqa: E402
from gq_amd.compressors import MXCompressor  # noqa: E402

NEW = {"gq_mx.h": ["gq_mx_compress_batched_bf16", "gq_mx_decode_sum_batched_bf16"],
       "gq_mxr.h": ["gq_mxr_compress_batched_bf16", "gq_mxr_decode_sum_batched_bf16"]}


def _declarations(header):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return code


@pytest.mark.parametrize("header,exports", [("gq_mx.h", "MX_EXPORTS"), ("gq_mxr.h", "MXR_EXPORTS")])
def test_headers_declare_the_bf16_entry_points(header, exports):
    code = _declarations(header)
    for name in NEW[header]:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert m, name
        assert "uint16_t *out" in m.group(1) and "float *out" not in m.group(1)
        assert name in getattr(native, exports)
        twin = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name[:-len("_bf16")], code).group(1)
        assert re.sub(r"\s+", " ", twin).replace("float *out", "uint16_t *out") == re.sub(r"\s+", " ", m.group(1))


def test_exported_symbols_of_the_built_libraries():
    for lib, names in ((native.MX_LIBRARY, NEW["gq_mx.h"]), (native.MXR_LIBRARY, NEW["gq_mxr.h"])):
        if not os.path.exists(lib.path):
            pytest.fail("%s is not built" % lib.path)
        L = ctypes.CDLL(lib.path)
        for name in names:
            assert hasattr(L, name), name


def test_abi_numbers_and_struct_sizes_did_not_move():
    for header, macro in (("gq_mx.h", "GQ_MX_ABI_VERSION"), ("gq_mxr.h", "GQ_MXR_ABI_VERSION")):
        assert re.search(r"#define\s+%s\s+2\b" % macro, _declarations(header))
    assert native.MX_ABI_VERSION == native.MXR_ABI_VERSION == 2
    assert ctypes.sizeof(native._MXBatchStruct) == 48 and ctypes.sizeof(native._MXRBatchStruct) == 80


def test_a_stale_library_fails_at_the_loader(tmp_path):
    """The version number stayed, so the accessor check is what catches a library from before the bf16 entry points."""
    lib = native.Library("libgq_hsq.so", "GQ_NO_SUCH_VARIABLE", "gq_", native.ABI_VERSION, ["gq_abi_version", "gq_mx_compress_batched_bf16"])
    if not os.path.exists(lib.path):
        pytest.fail("%s is not built" % lib.path)
    with pytest.raises(AttributeError):
        native._load(lib)


def _comp(fmt="fp4", random=True, rotate=None):
    return MXCompressor(5000, (5000,), Namespace(mx_format=fmt, random=random, mx_rotate=rotate, mx_rotate_seed=1))


def test_group_keys_split_by_dtype():
    c = _comp()
    a, b = MXCodec(c, 5000, (5000,)), MXCodec(c, 5000, (5000,), torch.bfloat16)
    assert a.dtype == torch.float32 and b.dtype == torch.bfloat16 and a.nbytes == b.nbytes
    assert BatchedMX.group_key(a) != BatchedMX.group_key(b)
    assert BatchedMX.group_key(a)[:3] == BatchedMX.group_key(b)[:3]
    assert sorted([BatchedMX.group_key(b), BatchedMX.group_key(a)])      # (the quantizer sorts the keys)
    r = _comp(rotate="hadamard")
    ra, rb = MXRCodec(r, 5000, (5000,)), MXRCodec(r, 5000, (5000,), torch.bfloat16)
    assert BatchedMXR.group_key(ra) != BatchedMXR.group_key(rb) and rb.signs == ra.signs
    with pytest.raises(TypeError):
        MXCodec(c, 5000, (5000,), torch.float16)
    with pytest.raises(TypeError):
        a.set_dtype(torch.float64)


def _layout_only(cls, codecs):
    """The group's host-side layout without a device: _item_setup with the device work stubbed out."""
    g = cls.__new__(cls)
    g._setup = lambda *a, **k: None
    real = torch.tensor

    def on_cpu(data, dtype=None, device=None):
        return real(data, dtype=dtype)
    torch.tensor = on_cpu
    try:
        offs, off = [], 0
        for cd in codecs:
            offs.append(off)
            off += cd.nbytes
        g._layout(codecs, offs, list(range(len(codecs))), torch.device("cpu"), 1, off)
    finally:
        torch.tensor = real
    return g


@pytest.mark.parametrize("rotate", [None, "hadamard"])
def test_a_bf16_group_places_its_views_on_multiples_of_eight(rotate):
    c = _comp(rotate=rotate)
    cls, codec = (BatchedMXR, MXRCodec) if rotate else (BatchedMX, MXCodec)
    sizes = [1, 7, 9, 33, 4097, 1001]
    g = _layout_only(cls, [codec(c, n, (n,), torch.bfloat16) for n in sizes])
    assert g.dtype == torch.bfloat16 and g.align == 2 and g._dense_align == 2 and g._dtypes == {torch.bfloat16}
    assert all(o % 8 == 0 for o in g.out_off) and g.out_floats % 8 == 0
    assert g.out_off == [0, 8, 16, 32, 72, 72 + 4104]
    f = _layout_only(cls, [codec(c, n, (n,)) for n in sizes])
    assert f.dtype == torch.float32 and f.align == 4 and all(o % 4 == 0 for o in f.out_off) and f.out_off[:3] == [0, 4, 12]


def test_error_buffers_are_float32_whatever_the_parameter():
    from gq_amd.quantizers import PSQuantizer
    ps = [torch.nn.Parameter(torch.zeros(64, 32, dtype=torch.bfloat16)), torch.nn.Parameter(torch.zeros(1200, dtype=torch.bfloat16)),
          torch.nn.Parameter(torch.zeros(40, 40, dtype=torch.float32)), torch.nn.Parameter(torch.zeros(10, dtype=torch.bfloat16))]
    args = Namespace(mode="ps", ef=True, two_phase=True, num_users=2, scale="1.0", mx_format="fp8", random=False, gq_graph=False)
    q = PSQuantizer(MXCompressor, ps, args)
    for p in ps[:3]:
        assert all(e.dtype == torch.float32 and e.shape == p.shape for e in p.error) and p.server_error.dtype == torch.float32
    assert [type(c).__name__ for c in q.codecs] == ["MXCodec", "MXCodec", "MXCodec", "DenseCodec"]
    assert [c.dtype for c in q.codecs[:3]] == [torch.bfloat16, torch.bfloat16, torch.float32]
    # two bf16 tensors make a group; the lone float32 one takes the per-tensor route
    assert [(cls.__name__, idx) for cls, idx, _ in q._groups] == [("BatchedMX", [0, 1])]
    assert q.offsets[3] == q.dense_off and q.codecs[3].nbytes == 40      # the identity-compressed tensor travels as float32


def test_train_py_refuses_bf16_with_another_quantizer():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--param-dtype", "bfloat16", "--quantizer", "hsq"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0
    assert "--param-dtype bfloat16 needs --quantizer mx" in r.stderr
    from gq_amd import driver
    assert driver.check_param_dtype(SimpleNamespace(param_dtype="bfloat16", quantizer="mx")) == torch.bfloat16
    assert driver.check_param_dtype(SimpleNamespace(param_dtype="float32", quantizer="hsq")) == torch.float32
    assert driver.build_parser().parse_args([]).param_dtype == "float32"
