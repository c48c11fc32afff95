"""libgq_ctk.so held to include/gq_ctk.h at tolerance 0, through BatchedChunkTopK as the quantizer lays a group out: every comparison is
np.array_equal against tests/ctk_contract.py (checked itself, with every claim made here about an input, in tests/test_ctk_contract.py).
Where float arithmetic can make a NaN (an input with inf or NaN; w = v + s * err), every NaN is mapped to one pattern first.
The wire starts as 0xAB with canary bytes in front of, between and behind the sections, `out` as 7.0 with a tail, and sources and error
buffers are views inside guarded buffers, every second one a float off 16-byte alignment: whole buffers are compared, canaries included."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ctk_contract as cc  # noqa: E402
import topk_contract as tc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, FILL, OUT_FILL, TAIL = 3.0, 0xAB, 7.0, 8
DEV = "cuda:0"


def _one_nan(a):
    b = tc.bits(a).copy()
    b[np.isnan(tc.f32(a))] = 0x7fc00000
    return b


def make_group(sizes, cr, dense_sizes=(), lead=16, gap=32):
    from gq_amd.codecs import BatchedChunkTopK, ChunkTopKCodec
    codecs = [ChunkTopKCodec(None, n, torch.Size([n]), cr=cr) for n in sizes]
    assert all(cd.nbytes == cc.section_size(n, cr) for cd, n in zip(codecs, sizes))
    offs, off = [], lead
    for cd in codecs:
        offs.append(off)
        off += cd.nbytes + gap
    dense = []
    for n in dense_sizes:
        dense.append((off, n))
        off += 4 * n
    ub = cc.up16(off) + 16
    g = BatchedChunkTopK(codecs, offs, list(range(len(codecs))), torch.device(DEV), 1, ub, dense=dense or None)
    return SimpleNamespace(g=g, offs=offs, dense=dense, ub=ub, sizes=list(sizes), cr=cr)


def _place(arr, off):
    big = torch.full((arr.size + 8,), GUARD, dtype=torch.float32, device=DEV)
    big[off:off + arr.size].copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    return big[off:off + arr.size], big


def _canon(G, wire):
    """The wire with every NaN of the sections' value arrays as one pattern."""
    wire = wire.copy()
    for n, off in zip(G.sizes, G.offs):
        K = cc.kept_count(n, G.cr)
        val = wire[off + cc.up16(2 * K):off + cc.up16(2 * K) + 4 * K]
        val[:] = _one_nan(val.view(np.float32)).view(np.uint8)
    return wire


def compress_and_check(G, vs, errs=None, s=None, dense_src=()):
    """One compress over a wire of 0xAB and an `out` of 7.0; the wire, `out`, the sources and the error buffers whole against the restatement."""
    ef = errs is not None
    src = [_place(v, i % 2) for i, v in enumerate(vs)]
    er = [_place(e, 2 * (i % 2)) for i, e in enumerate(errs)] if ef else []
    wire = torch.full((G.ub,), FILL, dtype=torch.uint8, device=DEV)
    out = torch.full((G.g.out_floats + TAIL,), OUT_FILL, dtype=torch.float32, device=DEV)
    kw = dict(errs=[t for t, _ in er], ef_scale=float(s)) if ef else {}
    if dense_src:
        kw["dense"] = [torch.from_numpy(a).to(DEV) for a in dense_src]
    assert G.g.encode([t for t, _ in src], wire, 0, 0, out=out, **kw)
    torch.cuda.synchronize()
    want_wire, want_out = np.full(G.ub, FILL, np.uint8), np.full(G.g.out_floats + TAIL, OUT_FILL, np.float32)
    for i, (n, off, oo) in enumerate(zip(G.sizes, G.offs, G.g.out_off)):
        w, D, e2 = cc.error_feedback(vs[i], errs[i], s, G.cr) if ef else (tc.f32(vs[i]), cc.dense(vs[i], G.cr), None)
        want_wire[off:off + cc.section_size(n, G.cr)] = cc.section_bytes(w, G.cr)
        want_out[oo:oo + n] = D
        for (t, big), at, want in [(src[i], i % 2, w)] + ([(er[i], 2 * (i % 2), e2)] if ef else []):
            guarded = np.full(n + 8, GUARD, np.float32)
            guarded[at:at + n] = want
            assert np.array_equal(_one_nan(big.cpu().numpy()), _one_nan(guarded)), "tensor %d (n = %d): the source, the residual or a guard" % (i, n)
    for a, (off, n) in zip(dense_src, G.dense):
        want_wire[off:off + 4 * n] = a.view(np.uint8)
    assert np.array_equal(_canon(G, wire.cpu().numpy()), _canon(G, want_wire)), "the wire: a section, a pad, a dense copy or a canary"
    assert np.array_equal(_one_nan(out.cpu().numpy()), _one_nan(want_out)), "the dense decode or its tail"


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
@pytest.mark.parametrize("cr", cc.CRS)
@pytest.mark.parametrize("kind", cc.KINDS)
def test_every_small_size(kind, cr, ef):
    """n = 1, cr - 1, cr (k_t = 0 and 1), 4,095, 4,096, 4,097 and two items plus cr + 1 in one group.  ef: err of the same kind at s = 0.75."""
    sizes = cc.SIZES(cr)
    G = make_group(sizes, cr)
    vs = [cc.make(kind, n, 100 + i) for i, n in enumerate(sizes)]
    errs = [cc.make("special" if kind == "special" else "gauss", n, 200 + i) for i, n in enumerate(sizes)]
    compress_and_check(G, vs, errs if ef else None, 0.75 if ef else None)


@pytest.mark.parametrize("last", cc.TIE_LASTS)
def test_ties_straddle_need_at_a_seam(last):
    compress_and_check(make_group([4096], cc.TIE_CR), [cc.tie_input(last)])


def test_seventy_tensors_and_dense_tensors_in_one_group():
    cyc = [1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 9000]
    sizes = [cyc[i % len(cyc)] for i in range(70)]
    vs = [cc.make(cc.KINDS[i % 4], n, 300 + i) for i, n in enumerate(sizes)]
    small = [tc.ordinary(n, 400 + n) for n in (10, 257)]
    compress_and_check(make_group(sizes, 3, dense_sizes=[a.size for a in small]), vs, dense_src=small)


DEC_N, DEC_CR = [2 * 4096 + 1000, 4096, 5], 16


@pytest.mark.parametrize("shift", [0, 2, 1], ids=["aligned", "off2", "off1"])
@pytest.mark.parametrize("R,plain", [(1, True), (1, False), (3, False), (8, False), (16, False)])
def test_decode_of_hand_built_payloads(R, plain, shift):
    """Payloads `shift` bytes off 16-byte alignment, positions in no order, a position beyond the item's length in every item (skipped), 0xEE
    between the sections; `out` a view three floats into a buffer of 7.0."""
    G = make_group(DEC_N, DEC_CR)
    secs = [cc.hand_sections(n, DEC_CR, R, 500 + i) for i, n in enumerate(DEC_N)]
    buf = np.full(shift + R * G.ub, 0xEE, np.uint8)
    for r in range(R):
        for off, per in zip(G.offs, secs):
            buf[shift + r * G.ub + off:shift + r * G.ub + off + per[r].size] = per[r]
    G.g.upload_layout()
    dev_buf = torch.from_numpy(buf).to(DEV)
    obig = torch.full((3 + G.g.out_floats + TAIL,), OUT_FILL, dtype=torch.float32, device=DEV)
    G.g._batch.decode(torch.as_strided(dev_buf, (R, G.ub), (G.ub, 1), shift), R, obig[3:3 + G.g.out_floats], plain=plain)
    torch.cuda.synchronize()
    want = np.full(3 + G.g.out_floats + TAIL, OUT_FILL, np.float32)
    for i, (n, oo) in enumerate(zip(DEC_N, G.g.out_off)):
        want[3 + oo:3 + oo + n] = cc.decode_mean(secs[i], n, DEC_CR, plain=plain)
    assert np.array_equal(_one_nan(obig.cpu().numpy()), _one_nan(want))      # (the pad floats between the tensors' views included)


def test_refusals_launch_nothing():
    from gq_amd import native
    G = make_group([4097, 8193], 16)
    G.g.upload_layout()
    wire = torch.full((G.ub + 16,), FILL, dtype=torch.uint8, device=DEV)
    out = torch.full((G.g.out_floats + 1,), OUT_FILL, dtype=torch.float32, device=DEV)
    b, L = G.g._batch, native.ctk_lib()
    nan = ctypes.c_float(float("nan"))
    W, O = wire.data_ptr(), out.data_ptr()
    comp = lambda w=W, o=O: L.gq_ctk_compress_batched(b.ref, ctypes.c_void_p(w), nan, ctypes.c_void_p(o), None)      # noqa: E731
    dec = lambda R=1, g=W, stride=G.ub, o=O, plain=0: L.gq_ctk_decode_sum_batched(b.ref, ctypes.c_void_p(g), ctypes.c_int64(stride), R,  # noqa: E731
                                                                                  ctypes.c_void_p(o), plain, None)
    calls = [comp, dec]
    for name, value in (("struct_bytes", 40), ("cr", 1), ("cr", 4097), ("nseg", 0), ("nitems", 0), ("seg_table", None), ("item_seg", None)):
        old = getattr(b.s, name)
        setattr(b.s, name, value)
        try:
            assert all(c() != 0 and L.gq_ctk_last_error() for c in calls), name
        finally:
            setattr(b.s, name, old)
    for rc in (comp(w=W + 4), comp(w=0), comp(o=O + 2), dec(o=O + 2), dec(o=0), dec(g=0), dec(R=0), dec(R=2, stride=-16), dec(R=2, plain=1)):
        assert rc != 0 and L.gq_ctk_last_error()
    torch.cuda.synchronize()
    assert bool((wire == FILL).all()) and bool((out == OUT_FILL).all()), "a refused call wrote something"
