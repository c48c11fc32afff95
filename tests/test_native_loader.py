"""gq_amd.native's one loader over its six library descriptions (no GPU): a missing file and a stale library fail at the
accessor, with a message that names that library's file."""
import os

import pytest

from gq_amd import native

LIBRARIES = [(native.HSQ_LIBRARY, native.lib, "libgq_hsq.so"), (native.TOPK_LIBRARY, native.topk_lib, "libgq_topk.so"),
             (native.SIGN_LIBRARY, native.sign_lib, "libgq_sign.so"), (native.PVQ_LIBRARY, native.pvq_lib, "libgq_pvq.so"),
             (native.RQ_LIBRARY, native.rq_lib, "libgq_rq.so"), (native.MAUREY_LIBRARY, native.maurey_lib, "libgq_maurey.so")]


@pytest.mark.parametrize("desc,accessor,name", LIBRARIES, ids=[name for _, _, name in LIBRARIES])
def test_missing_and_stale_library_fail_at_the_accessor(desc, accessor, name, tmp_path):
    assert desc.name == name and os.path.basename(desc.path) == name
    saved = (desc.path, desc.abi, desc.handle)
    try:
        desc.handle = None
        desc.path = str(tmp_path / name)      # a file that does not exist
        with pytest.raises(native.GQNativeError) as e:
            accessor()
        assert name + " not found at " + desc.path in str(e.value) and "build.py" in str(e.value)
        assert desc.handle is None
        desc.path = saved[0]
        desc.abi = saved[1] + 1               # the binding expects another ABI than the file has
        with pytest.raises(native.GQNativeError) as e:
            accessor()
        assert str(e.value) == "%s has ABI version %d, this binding is written for %d: rebuild it" % (saved[0], saved[1], saved[1] + 1)
        assert desc.handle is None
    finally:
        desc.path, desc.abi, desc.handle = saved
    assert accessor() is not None and desc.handle is accessor()
