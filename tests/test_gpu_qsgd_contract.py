"""The QSGD launches of libgq_hsq.so (csrc/qsgd_batched.hip, qsgd_wide.hip, qsgd.hip) held to include/gq_hsq.h bit for bit, through
native.QSGDBatch over hand-built tables and hand-built payloads: every comparison is np.array_equal on bytes or uint32 views against
tests/qsgd_contract.py (whose own checks, and one assertion for every claim made here about an input, are
tests/test_qsgd_contract.py).  Two stated conditions: the elements of buckets whose norm is +-inf are left out of the decode
comparison (the packed wire has no code for the reference's INT_MIN level; their count is asserted), and where
an input holds inf or NaN, any NaN equals any NaN.

The wire starts as 0xA5 with garbage where the launch writes, `out` and the error buffers of tensors without error feedback as 7.0,
the gradients sit in one buffer with 3.0 between them: after every launch every byte and float that belongs to nobody still holds
its fill, and without error feedback the gradients are unchanged.  A wire ends with its last codes section (rounded up to 16 bytes):
the decode needs no readable byte behind a codes section (include/gq_hsq.h).

The many-item cases are sized from the device's CU count: no launch has more than CUs x 8 workgroups of 4 waves (2,048 threads a
CU / 256), which the tests assert from the sizes they build.

user_stride_bytes >= 2^31, the pipelined decode's bail-out, needs 2 GiB per payload and is out of scope here."""
import ctypes
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

OUT_FILL, V_GUARD, V_GAP = 7.0, 3.0, 8
f32 = np.float32


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _cus():
    from gq_amd import native
    return native.device_info(0)[0]


def _place(arrs, fill, shift=None):
    """Float arrays in ONE device buffer, V_GAP floats of `fill` round each, starts 16-byte aligned (+ shift[i] floats)
    -> (buffer, pointers, offsets, host copy)"""
    offs, off = [], V_GAP
    for i, a in enumerate(arrs):
        offs.append(off + (shift[i] if shift else 0))
        off += (a.size + 3) // 4 * 4 + V_GAP
    host = np.full(off, fill, f32)
    for a, o in zip(arrs, offs):
        host[o:o + a.size] = a.reshape(-1)
    buf = _t(host)
    assert buf.data_ptr() % 16 == 0
    return buf, [buf.data_ptr() + 4 * o for o in offs], offs, host


def _words(seed, step):
    return torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed, step], dtype=torch.int64, device=_dev())


def run_compress(L, G, E, ef_scale, n_bit, mode, seed=0, step=0, hint=0, absent=(), gshift=None, eshift=None, dense=None, decoy=None):
    """One gq_qsgd_compress_batched launch over hand-built tables -> wire, gradient buffer, error buffer after it (numpy), what
    they were before, and norm_bits (wide)"""
    from gq_amd import native
    from types import SimpleNamespace
    gbuf, gptr, goff, g0 = _place(G, V_GUARD, gshift)
    ebuf = eptr = e0 = eoff = None
    if E is not None:
        ebuf, eptr, eoff, e0 = _place(E, OUT_FILL, eshift)
        eptr = [0 if i in absent else p for i, p in enumerate(eptr)]
    wire0 = np.full(L.ub, qc.CANARY, np.uint8)
    m = L.mask()
    wire0[m] = np.random.RandomState(3).randint(0, 256, size=int(m.sum())).astype(np.uint8)
    wire = _t(wire0)
    nb0 = None
    if L.wide:
        nb0 = np.full(L.nwords, 0x5A5A5A5A, np.uint32)
        for i, (d, nb) in enumerate(L.shapes):
            nb0[L.word0[i]:L.word0[i] + nb] = 0                    # zero before the compress, as the header says
        nbits = _t(nb0.view(np.int32))
    b = native.QSGDBatch(_t(L.table(gptr, eptr).reshape(-1)), _t(L.item_seg()), L.nseg, L.nitems, n_bit, L.bits, wide=L.wide,
                         norm_bits=nbits if L.wide else None, bucket_hint=hint)
    if decoy is not None:       # the descriptor is built over another table (other gradients): set_table brings the real one
        dbuf, dptr, _, _ = _place(decoy, V_GUARD)
        real = b.keep[0]
        b = native.QSGDBatch(_t(L.table(dptr, eptr).reshape(-1)), b.keep[1], L.nseg, L.nitems, n_bit, L.bits, wide=L.wide,
                             norm_bits=nbits if L.wide else None, bucket_hint=hint)
        b.set_table(real)
    if dense is not None:
        nbuf, nptr, _, _ = _place(dense, V_GUARD)
        b.set_dense(_t(L.dense_table(nptr).reshape(-1)), len(dense))
    words = _words(seed, step)
    b.compress(wire, mode, words.data_ptr() if mode == qc.COUNTER else seed, ef_scale)
    torch.cuda.synchronize()
    return SimpleNamespace(wire=wire.cpu().numpy(), wire0=wire0, g=gbuf.cpu().numpy(), g0=g0, goff=goff,
                           e=ebuf.cpu().numpy() if E is not None else None, e0=e0, eoff=eoff,
                           nbits=nbits.cpu().numpy().view(np.uint32) if L.wide else None, nb0=nb0, words=words.cpu().numpy())


def check_compress(L, G, E, ef_scale, n_bit, mode, seed=0, step=0, hint=0, absent=(), nan_equal=False, **kw):
    """the launch against the restatement: owned bytes, canaries, gradients, error buffers, norm_bits"""
    Ee = [None if i in absent else e for i, e in enumerate(E)] if E is not None else None
    wire, V, EN, N = qc.expect_compress(L, G, Ee, ef_scale if E is not None else None, n_bit, mode, seed, step)
    r = run_compress(L, G, E, ef_scale if E is not None else None, n_bit, mode, seed, step, hint, absent, **kw)
    m = L.mask()
    assert np.array_equal(r.wire[~m], r.wire0[~m]), "a byte outside the norm words and code bytes changed"
    if nan_equal:       # norms may be NaN: compare them as floats with NaN == NaN, the codes as bytes
        for i in range(L.nseg):
            (n1, c1), (n2, c2) = L.get(r.wire, i), L.get(wire, i)
            assert qc.same_bits(n1, n2, True) and np.array_equal(c1, c2), "tensor %d" % i
    else:
        assert np.array_equal(r.wire[m], wire[m])
    gexp = r.g0.copy()
    for i, v in enumerate(V):
        gexp[r.goff[i]:r.goff[i] + v.size] = v.reshape(-1)       # (v is g where there is no error feedback)
    assert qc.same_bits(r.g, gexp, nan_equal)
    if E is not None:
        eexp = r.e0.copy()
        for i, en in enumerate(EN):
            if i not in absent:
                eexp[r.eoff[i]:r.eoff[i] + en.size] = en.reshape(-1)
        assert qc.same_bits(r.e, eexp, nan_equal)
    assert r.words.tolist() == _words(seed, step).cpu().tolist(), "the compress changed the { seed, step } words"
    if L.wide:
        nexp = r.nb0.copy()
        for i, n in enumerate(N):
            nexp[L.word0[i]:L.word0[i] + n.size] = n.view(np.uint32)
        if nan_equal:
            assert qc.same_bits(r.nbits.view(f32), nexp.view(f32), True)
        else:
            assert np.array_equal(r.nbits, nexp)
    return wire


def run_decode(L, wires, n_bit, plain, hint=0, wshift=0, oshift=0, tail=None):
    """One gq_qsgd_decode_sum_batched(_tail) launch over R wires of L.ub bytes -> the whole `out` buffer; wshift / oshift move
    `gathered` (bytes) / `out` (floats) off their alignment"""
    from gq_amd import native
    R = len(wires)
    flat = np.full(R * L.ub + wshift + 64, qc.CANARY, np.uint8)
    for r, w in enumerate(wires):
        flat[wshift + r * L.ub:wshift + (r + 1) * L.ub] = w
    gat = _t(flat)
    assert gat.data_ptr() % 16 == 0
    gathered = gat[wshift:wshift + R * L.ub].view(R, L.ub)
    obuf = torch.full((L.out_n + oshift + 4,), OUT_FILL, dtype=torch.float32, device=_dev())
    assert obuf.data_ptr() % 16 == 0
    ptrs = [0] * L.nseg
    b = native.QSGDBatch(_t(L.table(ptrs).reshape(-1)), _t(L.item_seg()), L.nseg, L.nitems, n_bit, L.bits, wide=L.wide,
                         norm_bits=torch.zeros(L.nwords, dtype=torch.int32, device=_dev()) if L.wide else None, bucket_hint=hint)
    try:
        b.decode(gathered, R, obuf[oshift:oshift + L.out_n], plain=plain, tail=tail)
    except native.GQNativeError:
        torch.cuda.synchronize()
        assert np.all(obuf.cpu().numpy() == OUT_FILL), "a refused decode wrote to `out`"
        raise
    torch.cuda.synchronize()
    assert np.array_equal(gat.cpu().numpy(), flat), "the decode wrote to the wire"
    o = obuf.cpu().numpy()
    assert np.all(o[:oshift] == OUT_FILL) and np.all(o[oshift + L.out_n:] == OUT_FILL)
    return o[oshift:oshift + L.out_n]


def check_decode(L, wires, n_bit, plain, special=False, n_inf=0, **kw):
    exp = qc.expect_decode(L, wires, n_bit, plain, OUT_FILL)
    got = run_decode(L, wires, n_bit, plain, **kw)
    om = L.out_mask()
    assert np.array_equal(got[~om].view(np.uint32), exp[~om].view(np.uint32)), "`out` between the tensors changed"
    skip, n = qc.inf_norm_elements(L, wires)
    assert n == n_inf          # the buckets left out: exactly those the input was built with
    keep = om & ~skip
    assert qc.same_bits(got[keep], exp[keep], special)


# ---- the quotient window's edges (gap 1) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hint", [8, 32, 64, 128])
@pytest.mark.parametrize("n_bit,mode", [(1, qc.OFF), (2, qc.DEVICE), (6, qc.OFF), (6, qc.DEVICE), (8, qc.DEVICE), (15, qc.OFF)])
def test_window_edges(n_bit, mode, hint):
    """norms 2^-64, its predecessor, 2^20, its successor; a lane whose minimum is 2^-102 beside one with the predecessor; an exact
    zero beside ordinary elements -- in the register path (one and two units a lane) and the unit walk, between buckets that take
    the quick quotient and between buckets that do not"""
    G, _ = qc.edge_tensors(qc.lpb_of(hint))
    L = qc.Layout([(g.shape[1], g.shape[0]) for g in G], qc.code_bits(n_bit, mode))
    check_compress(L, G, None, None, n_bit, mode, seed=0x1234ABCD5678, hint=hint)


# ---- paths x lanes per bucket x code width x error feedback x nseg x draws (gaps 2, 3, 8) ------------------------------------------
@pytest.mark.parametrize("ci", range(len(qc.MATRIX)))
def test_path_matrix(ci):
    c = qc.MATRIX[ci]
    shapes, G, E, n_bit = qc.matrix_case(c)
    L = qc.Layout(shapes, c["bits"])
    absent = {i for i in range(L.nseg) if qc.err_absent(c, i)}
    wire = check_compress(L, G, E, 0.75 if c["ef"] else None, n_bit, c["mode"], seed=0xC0FFEE1234567, step=ci, hint=c["hint"], absent=absent)
    # the decode of that wire on the same tables: plain, and the mean of it and a second user's (other codes, other norms)
    check_decode(L, [wire], n_bit, True, hint=c["hint"])
    check_decode(L, [wire, qc.other_user(L, wire)], n_bit, False, hint=c["hint"])


@pytest.mark.parametrize("bits,mode", [(4, qc.OFF), (16, qc.DEVICE)])
def test_bucket_of_65536(bits, mode):
    n_bit = qc.N_BIT_OF[(bits, 0 if mode == qc.OFF else 1)]
    rs = np.random.RandomState(8)
    G = [qc.randn(rs, 2, 65536), qc.randn(rs, 3, 8)]
    L = qc.Layout([(65536, 2), (8, 3)], bits)
    wire = check_compress(L, G, None, None, n_bit, mode, seed=77, hint=0)
    check_decode(L, [wire], n_bit, True)


# ---- several items per wave, d, tensor and path changing between them (gap 4) -----------------------------------------------------
@pytest.mark.parametrize("bits,nseg,ef", [(4, 256, False), (8, 257, False), (16, 200, True), (4, 257, True)])
def test_many_items_per_wave(bits, nseg, ef):
    cus = _cus()
    shapes = qc.many_shapes(cus, nseg)
    L = qc.Layout(shapes, bits)
    assert L.nitems >= cus * 32 * 3 * 4          # at most cus * 8 workgroups of 4 waves, 4 buckets an item: 3 items a wave or more
    rs = np.random.RandomState(bits + nseg)
    G = [qc.randn(rs, nb, d) for d, nb in shapes]
    E = [qc.randn(rs, nb, d, 0.2) for d, nb in shapes] if ef else None
    n_bit = qc.N_BIT_OF[(bits, 1)]
    wire = check_compress(L, G, E, 1.0 if ef else None, n_bit, qc.DEVICE, seed=0xFEEDF00D, hint=128)
    check_decode(L, [wire, qc.other_user(L, wire), wire], n_bit, False, hint=128)


@pytest.mark.parametrize("hint", [8, 32, 64, 128])
@pytest.mark.parametrize("extra", [0, 1, 2])
def test_partial_last_item_and_short_waves(hint, extra):
    """cus * 32 * extra + 1 items: with the largest grid the launcher can choose (cus * 8 workgroups of 4 waves) the first wave runs
    extra + 1 items and every other wave `extra`, with a smaller grid more; the last item holds two buckets of the 4 ... 32 (one
    of each tensor), so the lanes behind them redo the last bucket and store nothing"""
    bpw = 64 // qc.lpb_of(hint)
    nb = bpw * _cus() * 32 * extra + 1
    shapes = [(8, nb), (10, 1)]
    rs = np.random.RandomState(extra)
    G = [qc.randn(rs, n, d) for d, n in shapes]
    L = qc.Layout(shapes, 4)
    assert (L.nitems + bpw - 1) // bpw == _cus() * 32 * extra + 1 and L.nitems % bpw == 2
    wire = check_compress(L, G, None, None, 3, qc.OFF, hint=hint)
    check_decode(L, [wire, wire, wire], 3, False, hint=hint)


# ---- the decode on hand-built payloads (gaps 5, 9) --------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [4, 8, 16])
@pytest.mark.parametrize("R,plain", [(1, True), (3, True), (9, True)] + [(R, False) for R in (1, 2, 3, 5, 6, 7, 8, 9, 16)])
def test_decode_payloads(bits, R, plain):
    """every code value, levels above 2^n_bit - 1 among them; norms subnormal, huge, +-inf, NaN, -0; plain: the decompress of ONE
    payload (a level 0 with the sign bit clear stays -0; with R > 1 the flag changes nothing: the sum is divided)"""
    L = qc.Layout(qc.dec_shapes(bits), bits)       # the wire ends with buckets of 6 codes: nothing behind them is read
    wires = qc.payload_wires(L, R)
    n_bit = {4: 2, 8: 5, 16: 8}[bits]
    check_decode(L, wires, n_bit, plain, special=True, n_inf=2, hint=(0, 8, 32, 64)[R % 4])


@pytest.mark.parametrize("bits", [4, 8, 16])
@pytest.mark.parametrize("wshift,oshift,pad", [(0, 0, 0), (4, 0, 0), (0, 0, 4), (0, 2, 0), (2, 0, 0), (0, 0, 2)])
def test_decode_misaligned(bits, wshift, oshift, pad):
    """`gathered`, `out` and the stride off the alignment that picks the pipelined kernel (4-bit codes: 4 bytes of the wire, 16 of
    `out`; 8- and 16-bit codes: 16 of the wire and the stride): the same results"""
    L = qc.Layout(qc.dec_shapes(4), bits, pad=pad)
    wires = qc.payload_wires(L, 3)
    check_decode(L, wires, {4: 2, 8: 5, 16: 8}[bits], False, special=True, n_inf=2, wshift=wshift, oshift=oshift)


@pytest.mark.parametrize("bits,wshift", [(4, 0), (8, 0), (8, 4), (16, 4)])
def test_decode_tail(bits, wshift):
    """the _tail entry with dense rows, two rng pairs and reset words, on a route that takes the tail in the launch (aligned) and on
    one that runs it behind the decode: the same results, `step` incremented exactly once, the reset words copied"""
    from gq_amd import native
    L = qc.Layout(qc.dec_shapes(4), bits)
    R = 3
    wires = qc.payload_wires(L, R)
    rs = np.random.RandomState(4)
    rows = rs.standard_normal((R, 37)).astype(f32)
    rows_t, mean_t = _t(rows), torch.full((37 + 4,), OUT_FILL, dtype=torch.float32, device=_dev())
    rng = torch.tensor([[11, 5], [12, 0x7FFFFFFFFFFFFFFE]], dtype=torch.int64, device=_dev())
    dst, src = torch.full((6,), -1, dtype=torch.int64, device=_dev()), torch.arange(6, dtype=torch.int64, device=_dev()) * 3 + 1
    tail = native.StepTail(rows=rows_t, out=mean_t[:37], rng_state=rng, reset=(dst[:5], src[:5]))
    check_decode(L, wires, {4: 2, 8: 5, 16: 8}[bits], False, special=True, n_inf=2, wshift=wshift, tail=tail)
    exp = qc.mean_of([rows[r] for r in range(R)], False)
    got = mean_t.cpu().numpy()
    assert qc.same_bits(got[:37], exp) and np.all(got[37:] == OUT_FILL)
    assert rng.cpu().tolist() == [[11, 6], [12, 0x7FFFFFFFFFFFFFFF]]
    assert dst.cpu().tolist() == [1, 4, 7, 10, 13, -1]


# ---- the draws, code for code (gap 6) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("mode,step", [(qc.DEVICE, 0), (qc.KEYED, 0), (qc.COUNTER, 0), (qc.COUNTER, 1)])
@pytest.mark.parametrize("n_bit", [2, 5, 8])
def test_draws(wide, mode, step, n_bit):
    """codes under the three device modes; every element of the tie tensors sits exactly on its own draw (`>`, not `>=`) and
    element 0 reaches the top level 2^n_bit; KEYED: the tie buckets are equal in norm at different bucket indices"""
    seed = 0x9E3779B97F4A7C15 if mode != qc.COUNTER else 0x1234567
    bits = qc.code_bits(n_bit, mode)
    rs = np.random.RandomState(n_bit)
    shapes = [(1026, 3), (34, 4), (2050, 2)] if wide else [(16, 9), (10, 5), (264, 3)]
    L = qc.Layout(shapes + shapes, bits, wide=wide)
    G = [qc.randn(rs, nb, d) for d, nb in shapes]
    for i, (d, nb) in enumerate(shapes):
        j = len(shapes) + i
        G.append(qc.tie_tensor(d, nb, n_bit, mode, seed, step, L.word0[j] if wide else L.first[j], wide))
    G[2][1] = G[2][0]                       # two buckets with equal data (equal norm bits) at different bucket indices
    wire = check_compress(L, G, None, None, n_bit, mode, seed=seed, step=step, hint=32)
    top = np.uint32((1 << (bits - 1)) | (1 << n_bit))
    for j in range(len(shapes), 2 * len(shapes)):
        code = L.get(wire, j)[1]
        assert np.all(code[:, 0] == top) and np.all((code[:, 1:] & np.uint32((1 << (bits - 1)) - 1)) == 0)


# ---- wide buckets (gap 7) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,ef", [(4, False), (4, True), (8, True), (16, False)])
def test_wide_runs_across_buckets_and_tensors(bits, ef):
    cus = _cus()
    shapes = qc.wide_shapes(cus)
    L = qc.Layout(shapes, bits, wide=True)
    assert L.nitems >= cus * 8 * 4 * 3           # cus * 8 workgroups of 4 waves: a run of 3 chunks or more each
    rs = np.random.RandomState(bits)
    G = [qc.randn(rs, nb, d) for d, nb in shapes]
    G[1][0, 3], G[2][1, 1000], G[4][2, 1025], G[8][0, 0] = np.nan, np.inf, np.nan, -np.inf       # NaN / inf win the integer max
    G[9][:] = 0
    E = [qc.randn(rs, nb, d, 0.2) for d, nb in shapes] if ef else None
    n = len(shapes)
    gshift, eshift = [0] * n, [0] * n
    gshift[5], eshift[6], gshift[20], eshift[21] = 2, 2, 2, 2     # 8- but not 16-byte aligned gradient / error pointers
    n_bit = qc.N_BIT_OF[(bits, 1)]
    wire = check_compress(L, G, E, 0.5 if ef else None, n_bit, qc.DEVICE, seed=99, absent={3} if ef else (), nan_equal=True,
                          gshift=gshift, eshift=eshift if ef else None)
    for R in (1, 3):
        check_decode(L, [wire] * R, n_bit, False, special=True, n_inf=2)


@pytest.mark.parametrize("bits", [4, 8, 16])
@pytest.mark.parametrize("R,plain", [(1, True), (3, True)] + [(R, False) for R in (1, 2, 3, 5, 6, 7, 8, 9, 16)])
def test_wide_decode_payloads(bits, R, plain):
    L = qc.Layout([(16, 12)] + [(d, 2) for d in qc.WIDE_D], bits, wide=True)
    wires = qc.payload_wires(L, R, seed=R)
    check_decode(L, wires, {4: 2, 8: 5, 16: 8}[bits], plain, special=True, n_inf=2)


# ---- the per-tensor form (csrc/qsgd.hip) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level_bytes", [1, 4])
@pytest.mark.parametrize("given", [False, True])
def test_per_tensor_compress_and_decode_sum(level_bytes, given, oracle):
    from gq_amd import native
    d, nb, n_bit = 24, 9, 3
    rs = np.random.RandomState(6)
    g = qc.randn(rs, nb, d)
    g[4] = 0                                        # a zero bucket: INT_MIN (int32) / 0 (uint8)
    r = rs.rand(nb, d).astype(f32)
    r[2] = np.floor(r[2] * 2.0 ** 20) * 2.0 ** -20
    g[2] = r[2] * f32(2.0 ** -n_bit)                # x == r exactly: x - l == r, no increment
    g[2, 0] = 1
    norm, sg, lv = (torch.empty(nb, dtype=torch.float32, device=_dev()), torch.full((nb * d + 8,), 9, dtype=torch.uint8, device=_dev()),
                    torch.full((nb * d + 8,), 9, dtype=torch.uint8 if level_bytes == 1 else torch.int32, device=_dev()))
    native.qsgd_compress(_t(g.reshape(-1)), d, n_bit, native.RANDOM_GIVEN if given else native.RANDOM_OFF, _t(r.reshape(-1)) if given else None,
                         0, norm, sg[:nb * d], lv[:nb * d])
    en, es, el = oracle.qsgd_compress(g, d, n_bit, 1 if given else 0, r)
    l2, s2 = qc.levels(g, qc.bucket_norm(g), n_bit, r if given else None)
    zero = np.repeat(np.arange(nb) == 4, d)
    assert np.array_equal(np.where(zero, 0, el), l2.reshape(-1)) and np.array_equal(np.where(zero, 1 - es, es), s2.reshape(-1))
    assert np.all(el[zero] == -2 ** 31)
    if level_bytes == 1:
        el = np.where(zero, 0, el)
    assert qc.same_bits(norm.cpu().numpy(), en)
    assert np.array_equal(sg.cpu().numpy(), np.concatenate([es, np.full(8, 9, np.uint8)]))
    assert np.array_equal(lv.cpu().numpy().astype(np.int64), np.concatenate([el, np.full(8, 9)]).astype(np.int64))
    if given:
        assert np.array_equal(el[2 * d + 1:3 * d], np.zeros(d - 1, el.dtype))
    for R in (1, 3, 8):
        N = np.stack([en * f32(1 + 0.37 * k) for k in range(R)])
        S = np.stack([np.roll(es, k) for k in range(R)])
        Lv = np.stack([np.roll(el, 3 * k) for k in range(R)])
        out = torch.full((nb * d + 4,), OUT_FILL, dtype=torch.float32, device=_dev())
        native.qsgd_decode_sum(_t(N.reshape(-1)), _t(S.reshape(-1)), _t(Lv.astype(np.uint8 if level_bytes == 1 else np.int32).reshape(-1)),
                               d, n_bit, out[:nb * d], R=R)
        dec = [oracle.qsgd_decompress(N[k], S[k], Lv[k], d, n_bit) for k in range(R)]
        exp = dec[0] if R == 1 else oracle.mean_users(np.stack(dec))
        got = out.cpu().numpy()
        assert qc.same_bits(got[:nb * d], exp) and np.all(got[nb * d:] == OUT_FILL)


# ---- error feedback and the per-tensor decode at tiny norms: the one de-quantiser (csrc/qsgd_common.hpp) on every path --------------------
TINY_PATHS = {       # path -> (d, tensors, bits, wide): lanes per bucket 16 (hint 128)
    "reg1": (128, 1, 4, False), "reg2": (256, 1, 4, False), "walk": (264, 1, 4, False), "pairs": (10, 1, 4, False),
    "generic": (10, 257, 8, False), "nolds4": (8, 257, 4, False), "wide": (1030, 1, 4, True),
}


@pytest.mark.parametrize("path", list(TINY_PATHS))
def test_error_feedback_with_subnormal_residuals(path):
    """three buckets a tensor: maxima 2^-120 ... 2^-140 (the decoded values and the new errors are subnormal), all +0, all -0"""
    d, nseg, bits, wide = TINY_PATHS[path]
    if not wide and nseg == 1:
        assert qc.compress_path(d, 16) == path
    # more tensors than QB_LDS_SEGS = 256 (csrc/qsgd_batched.hip): the launcher leaves the kernels that keep the table in LDS -- 8-bit
    # codes go to qsgd_compress_batched_kernel, 4-bit codes to qsgd_compress_batched4_kernel<EF, false>
    assert (nseg > 256) == (path in ("generic", "nolds4")) and (not wide or d % 1024 == 6)
    rs = np.random.RandomState(d)
    G, E = [], []
    for i in range(nseg):
        top = f32(2.0 ** -(120 + (5 * i) % 21))
        g, e = (rs.uniform(-0.5, 0.5, (3, d)) * top).astype(f32), (rs.uniform(-0.2, 0.2, (3, d)) * top).astype(f32)
        g[0, 0], e[0, 0] = top, 0
        g[1], e[1], g[2], e[2] = 0.0, 0.0, -0.0, -0.0
        G.append(g), E.append(e)
    with np.errstate(all="ignore"):
        v = G[-1] + f32(0.75) * E[-1]
    assert f32(2.0 ** -140) <= np.abs(v[0]).max() == v[0, 0] <= f32(2.0 ** -120) and np.signbit(v[2]).all() and not np.signbit(v[1]).any()
    L = qc.Layout([(d, 3)] * nseg, bits, wide=wide)
    check_compress(L, G, E, 0.75, qc.N_BIT_OF[(bits, 1)], qc.DEVICE, seed=0xABCDEF12345, hint=128)


@pytest.mark.parametrize("level_bytes", [1, 4])
@pytest.mark.parametrize("R", [1, 3])
def test_per_tensor_decode_sum_tiny_norms(level_bytes, R):
    """gq_qsgd_decode_sum against qsgd_compressor.py:69-70 spelled out: subnormal norms, level 0 with both signs, and for int32 levels
    the INT_MIN of a NaN quotient on a zero-norm bucket (why that instantiation keeps the product by 2 sign - 1)"""
    from gq_amd import native
    d, nb, n_bit = 8, 8, 3
    rs = np.random.RandomState(R + level_bytes)
    norm = np.stack([np.array([2.0 ** -130, 2.0 ** -149, 0.0, -0.0, 2.0 ** -126, 1.5 * 2.0 ** -127, 3.0, 2.0 ** -140], f32) * f32(1 + r) for r in range(R)])
    sg = rs.randint(0, 2, (R, nb, d)).astype(np.uint8)
    lv = rs.randint(0, 9, (R, nb, d)).astype(np.int64)
    lv[:, :, 0], sg[:, :, 0], lv[:, :, 1], sg[:, :, 1] = 0, 0, 0, 1
    if level_bytes == 4:
        lv[:, 2:4, 2:6] = -2 ** 31
    assert nb * d <= 64
    with np.errstate(all="ignore"):
        parts = [(lv[r].astype(f32) * (f32(2) * sg[r].astype(f32) - f32(1))) * norm[r][:, None] / f32(1 << n_bit) for r in range(R)]
    if level_bytes == 1:
        for r in range(R):
            assert qc.same_bits(parts[r], qc.decode_one(lv[r].astype(np.uint32) | (sg[r].astype(np.uint32) << np.uint32(8)), norm[r], n_bit, 9))
    exp = qc.mean_of(parts, R == 1).reshape(-1)
    assert not np.isnan(exp).any() and (np.abs(exp[exp != 0]) < f32(2.0 ** -126)).sum() >= 16
    out = torch.full((nb * d + 4,), OUT_FILL, dtype=torch.float32, device=_dev())
    native.qsgd_decode_sum(_t(norm.reshape(-1)), _t(sg.reshape(-1)), _t(lv.astype(np.uint8 if level_bytes == 1 else np.int32).reshape(-1)),
                           d, n_bit, out[:nb * d], R=R)
    got = out.cpu().numpy()
    assert qc.same_bits(got[:nb * d], exp) and np.all(got[nb * d:] == OUT_FILL)


# ---- part, set_table, set_dense ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,wide", [(4, False), (8, False), (4, True)])
def test_part_set_table_set_dense(bits, wide):
    """a compress whose descriptor was built over another table and got its own by set_table, with two uncompressed tensors riding
    in the launch (set_dense); then the decode of tensors 1 .. 2 alone through part(): the other tensors' `out` keeps its fill"""
    from gq_amd import native
    shapes = [(1026, 2), (34, 5), (2050, 2), (8, 6)] if wide else [(16, 9), (10, 5), (264, 3), (8, 6)]
    L = qc.Layout(shapes, bits, wide=wide, dense=(5, 1000))
    rs = np.random.RandomState(bits)
    G, decoy = [qc.randn(rs, nb, d) for d, nb in shapes], [qc.randn(rs, nb, d) for d, nb in shapes]
    D = [rs.standard_normal(n).astype(f32) for n in L.dense]
    n_bit = qc.N_BIT_OF[(bits, 1)]
    wire, _, _, _ = qc.expect_compress(L, G, None, None, n_bit, qc.DEVICE, 31)
    for o, a in zip(L.dense_off, D):
        wire[o:o + 4 * a.size] = a.view(np.uint8)
    r = run_compress(L, G, None, None, n_bit, qc.DEVICE, seed=31, dense=D, decoy=decoy)
    assert np.array_equal(r.wire, wire) and np.array_equal(r.g.view(np.uint32), r.g0.view(np.uint32))
    t, seg = L.part_table(1, 3)
    full = native.QSGDBatch(_t(L.table([0] * L.nseg).reshape(-1)), _t(L.item_seg()), L.nseg, L.nitems, n_bit, bits, wide=wide,
                            norm_bits=torch.zeros(L.nwords, dtype=torch.int32, device=_dev()) if wide else None)
    part = full.part(_t(t.reshape(-1)), _t(seg), 2, len(seg))
    wires = [wire, qc.other_user(L, wire)]
    out = torch.full((L.out_n,), OUT_FILL, dtype=torch.float32, device=_dev())
    part.decode(_t(np.stack(wires)), 2, out)
    torch.cuda.synchronize()
    exp = qc.expect_decode(L, wires, n_bit, False, OUT_FILL)
    for i in (0, 3):
        exp[L.out_off[i]:L.out_off[i] + shapes[i][0] * shapes[i][1]] = OUT_FILL
    assert qc.same_bits(out.cpu().numpy(), exp)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_untouched():
    from gq_amd import native
    lib = native.lib()
    L = qc.Layout([(16, 5), (10, 3)], 4)
    G = [qc.randn(np.random.RandomState(1), nb, d) for d, nb in L.shapes]
    gbuf, gptr, _, g0 = _place(G, V_GUARD)
    wire0 = np.full(L.ub, qc.CANARY, np.uint8)
    wire, out = _t(wire0), torch.full((L.out_n,), OUT_FILL, dtype=torch.float32, device=_dev())
    table, item = _t(L.table(gptr).reshape(-1)), _t(L.item_seg())
    words = _words(5, 0)

    def batch(**kw):
        b = native.QSGDBatch(table, item, L.nseg, L.nitems, kw.pop("n_bit", 2), kw.pop("bits", 4))
        for k, v in kw.items():
            setattr(b.s, k, v)
        return b

    def compress(b, mode=native.RANDOM_OFF, seed=0, w=wire):
        return lib.gq_qsgd_compress_batched(b.ref, ctypes.c_void_p(w.data_ptr() if w is not None else 0), ctypes.c_int(mode),
                                            ctypes.c_uint64(seed), ctypes.c_float(float("nan")), native._stream())

    def decode(b, R=1, w=wire, o=out):
        return lib.gq_qsgd_decode_sum_batched(b.ref, ctypes.c_void_p(w.data_ptr() if w is not None else 0), ctypes.c_int64(L.ub),
                                              ctypes.c_int(R), ctypes.c_void_p(o.data_ptr() if o is not None else 0), ctypes.c_int(0),
                                              native._stream())

    INV, UNS = -1, -2
    assert compress(batch(nseg=0)) == INV and compress(batch(nitems=0)) == INV and compress(batch(n_bit=0)) == INV
    assert decode(batch(nseg=0)) == INV and decode(batch(nitems=0)) == INV and decode(batch(n_bit=0)) == INV
    assert compress(batch(), w=None) == INV and decode(batch(), w=None) == INV and decode(batch(), o=None) == INV
    assert compress(batch(seg_table=None)) == INV and decode(batch(item_seg=None)) == INV
    assert compress(batch(bits=8, n_bit=5), mode=native.RANDOM_GIVEN) == UNS
    assert compress(batch(n_bit=15, bits=0), mode=native.RANDOM_DEVICE) == UNS       # top level 32768: no packed format
    assert compress(batch(bits=8)) == INV                                            # bits is not what n_bit packs to
    assert decode(batch(bits=5)) == INV and decode(batch(bits=0)) == INV
    assert decode(batch(), R=0) == INV
    assert compress(batch(), mode=native.RANDOM_DEVICE_COUNTER, seed=0) == INV
    assert compress(batch(), mode=native.RANDOM_DEVICE_COUNTER, seed=words.data_ptr() + 4) == INV
    assert compress(batch(struct_bytes=64)) == INV and decode(batch(struct_bytes=64)) == INV
    nbits = torch.zeros(L.nwords, dtype=torch.int32, device=_dev())
    wb = native.QSGDBatch(table, item, L.nseg, L.nitems, 2, 4, wide=True, norm_bits=nbits)
    assert decode(wb, w=wire[2:]) == INV and decode(wb, o=out[1:]) == INV           # wide: 4- / 16-byte alignment
    torch.cuda.synchronize()
    assert np.array_equal(wire.cpu().numpy(), wire0) and np.all(out.cpu().numpy() == OUT_FILL)
    assert np.array_equal(gbuf.cpu().numpy().view(np.uint32), g0.view(np.uint32)) and words.cpu().tolist() == [5, 0]
    assert int(nbits.abs().sum()) == 0
