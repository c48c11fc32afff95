"""libgq_ctk.so's PACKED16 launches held to include/gq_ctk.h at tolerance 0, through BatchedChunkTopK as the quantizer lays a group out:
every comparison is np.array_equal against tests/ctk_packed_contract.py.  Buffers, canaries and guards are test_gpu_zz_ctk_contract.py's: a
wire of 0xAB with bytes in front of, between and behind the sections, `out` as 7.0 with a tail, sources and error buffers as views inside
guarded buffers, every second one a float (4 bytes) off 16-byte alignment; whole buffers are compared.  The wire holds integers only; in
`out`, the sources and the residuals every NaN is mapped to one pattern first."""
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
import ctk_packed_contract as pc  # noqa: E402
import topk_contract as tc  # noqa: E402
from test_gpu_zz_ctk_contract import DEV, FILL, GUARD, OUT_FILL, TAIL, _one_nan, _place  # noqa: E402

pytestmark = pytest.mark.gpu


def make_group(sizes, cr, lead=16, gap=32):
    from gq_amd.codecs import BatchedChunkTopK, ChunkTopKCodec
    codecs = [ChunkTopKCodec(None, n, torch.Size([n]), cr=cr, values="packed16") for n in sizes]
    assert all(cd.nbytes == pc.section_size(n, cr) for cd, n in zip(codecs, sizes))
    offs, off = [], lead
    for cd in codecs:
        offs.append(off)
        off += cd.nbytes + gap
    ub = cc.up16(off) + 16
    g = BatchedChunkTopK(codecs, offs, list(range(len(codecs))), torch.device(DEV), 1, ub)
    return SimpleNamespace(g=g, offs=offs, ub=ub, sizes=list(sizes), cr=cr)


def compress_and_check(G, vs, errs=None, s=None):
    """One compress over a wire of 0xAB and an `out` of 7.0; the wire, `out`, the sources and the error buffers whole against the restatement."""
    ef = errs is not None
    src = [_place(v, i % 2) for i, v in enumerate(vs)]
    er = [_place(e, 2 * (i % 2)) for i, e in enumerate(errs)] if ef else []
    wire = torch.full((G.ub,), FILL, dtype=torch.uint8, device=DEV)
    out = torch.full((G.g.out_floats + TAIL,), OUT_FILL, dtype=torch.float32, device=DEV)
    kw = dict(errs=[t for t, _ in er], ef_scale=float(s)) if ef else {}
    assert G.g.encode([t for t, _ in src], wire, 0, 0, out=out, **kw)
    torch.cuda.synchronize()
    want_wire, want_out = np.full(G.ub, FILL, np.uint8), np.full(G.g.out_floats + TAIL, OUT_FILL, np.float32)
    for i, (n, off, oo) in enumerate(zip(G.sizes, G.offs, G.g.out_off)):
        w, D, e2 = pc.error_feedback(vs[i], errs[i], s, G.cr) if ef else (tc.f32(vs[i]), pc.dense(vs[i], G.cr), None)
        want_wire[off:off + pc.section_size(n, G.cr)] = pc.section_bytes(w, G.cr)
        want_out[oo:oo + n] = D
        for (t, big), at, want in [(src[i], i % 2, w)] + ([(er[i], 2 * (i % 2), e2)] if ef else []):
            guarded = np.full(n + 8, GUARD, np.float32)
            guarded[at:at + n] = want
            assert np.array_equal(_one_nan(big.cpu().numpy()), _one_nan(guarded)), "tensor %d (n = %d): the source, the residual or a guard" % (i, n)
    assert np.array_equal(wire.cpu().numpy(), want_wire), "the wire: the bounds, a word, a pad or a canary"
    assert np.array_equal(_one_nan(out.cpu().numpy()), _one_nan(want_out)), "the dense decode or its tail"


def _errs(vs, seed):
    return [cc.make("gauss", v.size, seed + i) for i, v in enumerate(vs)]


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
@pytest.mark.parametrize("cr", cc.CRS)
def test_every_small_size(cr, ef):
    """One, one short of one, one, one and a bit, two and a last item that keeps nothing, three and 17 (an odd and an even number of bounds)
    in one group, the kinds of tests/ctk_contract.py in turn; ef: Gaussian residuals at s = 0.75."""
    sizes = [1, 4095, 4096, 4097, 2 * 4096 + cr - 1, 3 * 4096 + 17]
    vs = [cc.make(cc.KINDS[i % len(cc.KINDS)], n, 600 + i) for i, n in enumerate(sizes)]
    compress_and_check(make_group(sizes, cr), vs, _errs(vs, 650) if ef else None, 0.75 if ef else None)


def hand_made(cr):
    """cr = 16: ties on the threshold across a lane, a wave and a register-step seam; an item of equal magnitudes (D == 0) in front of an
    item that keeps nothing; +-0 and subnormals; one inf above a finite T.  cr = 3 (kf = 1,365 words, 2,730 bytes: no multiple of 16): two
    small tensors whose items' word runs share a 16-byte group."""
    if cr == 3:
        return [cc.make("gauss", 4096 + 100, 701), cc.make("student", 2 * 4096 + 5, 702)]
    with_inf = cc.make("gauss", 4096, 703)
    with_inf[1234] = -np.inf
    return [cc.tie_input(last) for last in cc.TIE_LASTS] + [cc.make("equal", 4096 + 15, 704), tc.subnormal_input(), with_inf]


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
@pytest.mark.parametrize("cr", [16, 3])
def test_hand_made_items(cr, ef):
    vs = hand_made(cr)
    compress_and_check(make_group([v.size for v in vs], cr), vs, _errs(vs, 750) if ef else None, 1.0 if ef else None)


DEC_N, DEC_CR = [2 * 4096 + 1000, 4096, 5], 16


@pytest.mark.parametrize("R,plain", [(1, True), (1, False), (3, False), (8, False)])
def test_decode_of_hand_built_payloads(R, plain):
    """Payloads one byte off 16-byte alignment at an odd stride, positions in no order, bounds of their own per item and payload, the short
    item's first word naming a position not below its length (skipped), 0xEE between the sections; `out` a view three floats into 7.0."""
    G = make_group(DEC_N, DEC_CR)
    secs = [pc.hand_sections(n, DEC_CR, R, 800 + i) for i, n in enumerate(DEC_N)]
    stride = G.ub + 1
    buf = np.full(1 + R * stride, 0xEE, np.uint8)
    for r in range(R):
        for off, per in zip(G.offs, secs):
            buf[1 + r * stride + off:1 + r * stride + off + per[r].size] = per[r]
    G.g.upload_layout()
    dev_buf = torch.from_numpy(buf).to(DEV)
    obig = torch.full((3 + G.g.out_floats + TAIL,), OUT_FILL, dtype=torch.float32, device=DEV)
    G.g._batch.decode(torch.as_strided(dev_buf, (R, G.ub), (stride, 1), 1), R, obig[3:3 + G.g.out_floats], plain=plain)
    torch.cuda.synchronize()
    want = np.full(3 + G.g.out_floats + TAIL, OUT_FILL, np.float32)
    for i, (n, oo) in enumerate(zip(DEC_N, G.g.out_off)):
        want[3 + oo:3 + oo + n] = pc.decode_mean(secs[i], n, DEC_CR, plain=plain)
    assert np.array_equal(_one_nan(obig.cpu().numpy()), _one_nan(want))      # (the pad floats between the tensors' views included)
