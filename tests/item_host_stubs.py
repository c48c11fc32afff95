"""Stand-ins that let the item-table host path (gq_amd.native._ItemBatch, gq_amd.codecs._ItemGroup) run without a device:
a library that records every entry-point call, device-pointer and stream getters that take CPU tensors, and a `_setup` that
keeps a group's header in host memory.  Used by test_item_binding.py and test_item_group_host.py."""
import ctypes

import torch

from gq_amd import codecs, native

ITEM_LIBRARIES = ("TOPK", "DGC", "SIGN", "MAUREY", "MX", "MXR", "DRIVE", "EDEN", "THR", "STC", "PSGD")


class RecordingLibrary(object):
    """Every attribute is an entry point that notes (name, arguments) and answers 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 0
        entry.__name__ = name
        return entry


def _dev_ptr(t, dtype=None, name="tensor"):
    """native._dev_ptr without the device checks: type, dtype and contiguity still hold."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if dtype is not None and t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return ctypes.c_void_p(t.data_ptr())


def install(monkeypatch):
    """One RecordingLibrary in place of every item-table library's handle; returns it."""
    rec = RecordingLibrary()
    for name in ITEM_LIBRARIES:
        monkeypatch.setattr(getattr(native, name + "_LIBRARY"), "handle", rec)
    monkeypatch.setattr(native, "_dev_ptr", _dev_ptr)
    monkeypatch.setattr(native, "_stream", lambda: ctypes.c_void_p(0))
    return rec


def host_setup(self, table, extra, device, slots, user_bytes, dense=None):
    """_BatchedBase._setup with the header kept on the host: what the item groups' constructors, encode and the state tables read."""
    self.nseg, self.device, self.user_bytes = table.shape[0], device, user_bytes
    self._table_words = self._dense_at = self.nseg * 8
    self.ndense = 0
    self._dev = table.view(-1).clone()
    self._layout = table.clone()
    self._parts, self.rng_pairs, self.ready, self._tmp_wire = {}, None, True, None
    self._outs, self._out_views, self._out_turn, self._out_gen = [None, None], [None, None], 0, 0


def install_groups(monkeypatch):
    """install() plus a host `_setup`, a current device of -1 (where CPU tensors live) and no stream capture."""
    rec = install(monkeypatch)
    monkeypatch.setattr(codecs._BatchedBase, "_setup", host_setup)
    monkeypatch.setattr(torch._C, "_cuda_getDevice", lambda: -1)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return rec
