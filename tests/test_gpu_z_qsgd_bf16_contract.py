"""The bf16 QSGD launches (gq_qsgd_batch.tensor_type = GQ_QSGD_TENSOR_BF16; include/gq_hsq.h, TENSOR-SIDE TYPE) bit
for bit against tests/qsgd_contract.py: the bf16 input widened to float32, the restatement run with the same draws, its float32
outputs narrowed by round to nearest even in numpy.  Wire, `out`, the stored-back gradient and the residual are compared with
np.array_equal (any NaN as one pattern); the tolerance is 0.

Every compress case is one launch over three tensors: one bucket; two buckets in a view that is 2-byte but not 16-byte aligned;
one item (the buckets a wave takes) plus one bucket.  Their buckets hold +-0, a bf16 subnormal, 0x7F7F, a zero bucket, and inf and
NaN in one bucket.  The decode cases hold, in payload 0, a norm of 9 significant bits whose levels 1 and 2 decode exactly between
two bf16 values."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import qsgd_contract as qc  # noqa: E402

pytestmark = pytest.mark.gpu
f32, u16 = np.float32, np.uint16
GUARD, FILL = 0x4040, 7.0        # bf16 3.0 between the gradients; 7.0 (a bf16 value) where `out` and the residuals belong to nobody

# name -> (shapes(cus), n_bit, wide).  The small ones: one bucket; two buckets (the misaligned view); one item of the bf16 compress (the
# buckets a wave takes) plus one bucket.  wide_n1: chunks end inside a bucket and a tensor.  wide_runs: qc.wide_shapes -- every wave
# has a RUN of three chunks or more, and runs cross buckets and tensors (the running max's hand-over, the prefetch across a record
# change).  many257: qc.many_shapes with 257 tensors -- the segment table does not fit LDS, three items a wave, every bucket path.
PATHS = {"c128_n2": (lambda cus: [(128, 1), (128, 2), (128, 9)], 2, False), "c32_n8": (lambda cus: [(32, 1), (32, 2), (32, 33)], 8, False),
         "c192_n2": (lambda cus: [(192, 1), (192, 2), (192, 9)], 2, False), "wide_n1": (lambda cus: [(1500, 2), (1026, 1), (2050, 1)], 1, True),
         "wide_runs": (lambda cus: qc.wide_shapes(cus), 1, True), "many257": (lambda cus: qc.many_shapes(cus, 257), 2, False)}
SMALL, BIG = ("c128_n2", "c192_n2", "c32_n8", "wide_n1"), ("many257", "wide_runs")
COMPRESS = ([(p, m, e) for p in SMALL for m in (qc.DEVICE, qc.OFF) for e in (None, 1.0, 0.46211715726)]
            + [(p, qc.DEVICE, e) for p in BIG for e in (None, 0.46211715726)])
DECODE = [(p, R) for p in SMALL for R in (1, 2, 8)] + [(p, 2) for p in BIG]


def widen(h):
    return (np.asarray(h, u16).astype(np.uint32) << np.uint32(16)).view(f32)


def narrow(x):
    b = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    r = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(u16)
    return np.where((b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000), u16(0x7FC0), r)


def same16(a, b):
    a, b = np.asarray(a, u16).reshape(-1), np.asarray(b, u16).reshape(-1)
    nan = np.isnan(widen(a)) & np.isnan(widen(b))
    return a.shape == b.shape and np.array_equal(a[~nan], b[~nan])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _place(arrs, fill, dtype, shift):
    """arrays in ONE device buffer, 8 elements of `fill` round each, starts on 16 bytes (+ shift[i] elements)"""
    offs, off = [], 8
    for a, s in zip(arrs, shift):
        offs.append(off + s)
        off += (a.size + 7) // 8 * 8 + 8
    host = np.full(off, fill, dtype)
    for a, o in zip(arrs, offs):
        host[o:o + a.size] = a.reshape(-1)
    buf = _dev(host.view(np.int16) if dtype == u16 else host)
    assert buf.data_ptr() % 16 == 0
    return buf, [buf.data_ptr() + host.itemsize * o for o in offs], offs, host


def _inputs(path):
    from gq_amd import native
    fn, n_bit, wide = PATHS[path]
    rs = np.random.RandomState(11)
    shapes = fn(native.device_info(0)[0])
    G = [narrow(qc.randn(rs, nb, dd)).reshape(nb, dd) for dd, nb in shapes]
    k = min(8, shapes[0][0])
    G[0][0, :k] = [0x0000, 0x8000, 0x0001, 0x8001, 0x7F7F, 0xFF7F, 0x3F80, 0xBF80][:k]      # +-0, subnormals, the largest finite
    G[1][-1, :] = 0                                                                     # a zero bucket: 0 / 0
    G[2][0, 3], G[2][0, 5] = 0x7F80, 0x7FC1                                             # inf and NaN in one bucket
    E = [qc.randn(rs, nb, dd, 0.25) for dd, nb in shapes]
    return shapes, n_bit, wide, G, E


@pytest.mark.parametrize("path,mode,ef_scale", COMPRESS)
def test_compress_is_the_float32_contract_on_the_widened_gradients(path, mode, ef_scale):
    from gq_amd import native
    shapes, n_bit, wide, G, E = _inputs(path)
    L = qc.Layout(shapes, qc.code_bits(n_bit, mode), wide=wide)
    seed = 0x1234567 if mode == qc.DEVICE else 0
    ef = ef_scale is not None
    wire_x, V, EN, _ = qc.expect_compress(L, [widen(g) for g in G], E if ef else None, ef_scale, n_bit, mode, seed)
    gbuf, gptr, goff, g0 = _place(G, GUARD, u16, [0, 1] + [0] * (len(G) - 2))       # the middle view: 2-byte aligned, not 16
    assert gptr[1] % 16 == 2
    ebuf, eptr, eoff, e0 = _place(E, FILL, f32, [0] * len(E))
    wire0 = np.full(L.ub, qc.CANARY, np.uint8)
    wire = _dev(wire0)
    nbits = _dev(np.zeros(L.nwords, np.int32)) if wide else None
    b = native.QSGDBatch(_dev(L.table(gptr, eptr if ef else None).reshape(-1)), _dev(L.item_seg()), L.nseg, L.nitems, n_bit, L.bits,
                         wide=wide, norm_bits=nbits, bucket_hint=0 if wide else shapes[0][0], dtype=torch.bfloat16)
    b.compress(wire, mode, seed, ef_scale)
    torch.cuda.synchronize()
    got, m = wire.cpu().numpy(), L.mask()
    assert np.array_equal(got[~m], wire0[~m]), "a byte outside the norm words and code bytes changed"
    for i in range(L.nseg):       # (a NaN norm: any NaN; the codes as they are)
        (n1, c1), (n2, c2) = L.get(got, i), L.get(wire_x, i)
        assert qc.same_bits(n1, n2, True) and np.array_equal(c1, c2), "wire of tensor %d" % i
    gexp = g0.copy()
    for i, v in enumerate(V):       # (without error feedback V is the widened gradient: narrow gives it back, NaN payloads aside)
        gexp[goff[i]:goff[i] + v.size] = narrow(v).reshape(-1)
    assert same16(gbuf.cpu().numpy().view(u16), gexp), "the stored-back gradient"
    if not ef:
        assert np.array_equal(gbuf.cpu().numpy().view(u16), g0), "a compress without error feedback wrote a gradient"
    eexp = e0.copy()
    if ef:
        for i, en in enumerate(EN):
            eexp[eoff[i]:eoff[i] + en.size] = en.reshape(-1)
    assert qc.same_bits(ebuf.cpu().numpy(), eexp, True), "the residual (float32, from the unrounded sum)"


@pytest.mark.parametrize("path,R", DECODE)
def test_decode_mean_adds_in_float32_and_rounds_once(path, R):
    from gq_amd import native
    shapes, n_bit, wide, G, _ = _inputs(path)
    bits = qc.code_bits(n_bit, qc.DEVICE)
    L = qc.Layout(shapes, bits, wide=wide)
    rs, k = np.random.RandomState(5), min(4, shapes[0][0])
    wires = []
    for r in range(R):       # hand-built payloads: the reference's codes of other users' finite gradients
        w = np.full(L.ub, qc.CANARY, np.uint8)
        for i, (d, nb) in enumerate(shapes):
            norm, code, _, _ = qc.compress_tensor(qc.randn(rs, nb, d), None, None, n_bit, bits, qc.DEVICE, 77 + r, 0, 0, wide)
            if r == 0 and i == 0:       # a norm of 9 significant bits; levels 1 and 2 of it lie between two bf16 values
                norm[0], code[0, :k] = f32(257.0 / 256.0), [1, 2, 1 | 1 << (bits - 1), 2 | 1 << (bits - 1)][:k]
            L.put(w, i, norm, code)
        wires.append(w)
    plain = R == 1
    ref = qc.expect_decode(L, wires, n_bit, plain, f32(FILL))
    if R == 1:       # the tie exists in the reference, and is rounded to even
        t = ref[L.out_off[0]:L.out_off[0] + k].view(np.uint32)
        assert all(int(x) & 0xFFFF == 0x8000 for x in t)
        assert [int(x) & 1 for x in narrow(ref[L.out_off[0]:L.out_off[0] + k])] == [0] * k
    gathered = _dev(np.stack(wires))
    out = _dev(np.full(L.out_n, narrow(f32(FILL)), u16).view(np.int16)).view(torch.bfloat16)
    b = native.QSGDBatch(_dev(L.table([0] * L.nseg).reshape(-1)), _dev(L.item_seg()), L.nseg, L.nitems, n_bit, bits, wide=wide,
                         norm_bits=_dev(np.zeros(L.nwords, np.int32)) if wide else None, bucket_hint=0 if wide else shapes[0][0],
                         dtype=torch.bfloat16)
    b.decode(gathered, R, out, plain=plain)
    torch.cuda.synchronize()
    assert same16(out.view(torch.int16).cpu().numpy().view(u16), narrow(ref)), "out, fill between the tensors included"
