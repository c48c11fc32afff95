"""libgq_drive.so held to include/gq_drive.h, bit for bit: every comparison is np.array_equal on bytes or uint32 views against
tests/drive_contract.py (whose own checks are tests/test_drive_contract.py) -- the whole wire section with canaries round the wire,
the dense `out`, the gradient and the residual after error feedback, guards round every buffer.
NaNs: the header leaves the sign and payload of a NaN that an ADDITION produces to the hardware.  So every NaN counts as one
pattern only in a block whose x' is not finite (an inf or a NaN in the input: there the code bits are not compared either, S
must be 0x7fc00000 and every decoded value a NaN) and in the decode of a block whose scale -- the decode's own input -- is not
finite or so large that the inverse transform overflows (S = +inf from a Q that overflowed; the hand-built payloads).  Which
blocks those are is computed from the restatement, never from what the kernels return; everywhere else all 32 bits count."""
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
import mx_contract as mx  # noqa: E402
import drive_contract as dc  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
ITEM, BLOCK = dc.ITEM, dc.BLOCK
GUARD = f32(-123.25)
CANARY_BYTES = 64
MODES = ["unbiased", "mse"]
BIG_S = f32(2.0 ** 100)      # from here on the inverse transform's sums may overflow


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _place(arr, off, dev):
    """arr as a view `off` floats into a guarded buffer of its own (4 * off bytes past a 16-byte boundary) -> (view, buffer)"""
    big = torch.full((arr.size + 8,), float(GUARD), dtype=torch.float32, device=dev)
    view = big[off:off + arr.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view, big


def _guards_intact(big, off, n):
    b = big.cpu().numpy()
    return np.all(b[:off] == GUARD) and np.all(b[off + n:] == GUARD)


def make_group(sizes, mode="unbiased", signs=dc.SEEDED, dense_sizes=()):
    from gq_amd.codecs import BatchedDrive, DriveCodec, drive_section_bytes
    dev = torch.device("cuda:0")
    comp = SimpleNamespace(scale=mode, signs=signs)
    codecs = [DriveCodec(comp, n, torch.Size([n])) for n in sizes]
    assert [cd.nbytes for cd in codecs] == [dc.section_bytes(n) for n in sizes] == [drive_section_bytes(n) for n in sizes]
    offs, dense, ub = dc.layout(sizes, dense_sizes)
    g = BatchedDrive(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=dense or None)
    return SimpleNamespace(g=g, codecs=codecs, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), mode=dc.MODES[mode], signs=signs)


def compress(G, vs, errs=None, s=None, dense_src=(), v_offs=None, e_offs=None, o_off=0, want_out=True):
    """One compress of the group into a wire full of 0xAB between canaries, `out` preset to 7.0 -> wire, out, the sources and error
    buffers afterwards (numpy)."""
    dev, g = G.dev, G.g
    nt = len(vs)
    v_offs = v_offs or [0] * nt
    e_offs = e_offs or [0] * nt
    src = [_place(v, o, dev) for v, o in zip(vs, v_offs)]
    er = [_place(e, o, dev) for e, o in zip(errs, e_offs)] if errs is not None else None
    ds = [torch.from_numpy(a).to(dev) for a in dense_src]
    whole = torch.full((G.ub + 2 * CANARY_BYTES,), mx.CANARY, dtype=torch.uint8, device=dev)
    wire = whole[CANARY_BYTES:CANARY_BYTES + G.ub]
    wire.fill_(0xAB)
    obig = torch.full((g.out_floats + 8,), 7.0, dtype=torch.float32, device=dev)
    out = obig[o_off:o_off + g.out_floats] if want_out else None
    kw = {}
    if er is not None:
        kw.update(errs=[e[0] for e in er], ef_scale=float(s))
    if ds:
        kw.update(dense=ds)
    assert g.encode([t for t, _ in src], wire, 0, 0, out=out, **kw)
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    assert np.all(w[:CANARY_BYTES] == mx.CANARY) and np.all(w[CANARY_BYTES + G.ub:] == mx.CANARY), "a write outside the wire"
    for (t, big), o, v in zip(src, v_offs, vs):
        assert _guards_intact(big, o, v.size), "a write outside the source"
    for e, o, a in zip(er or (), e_offs, errs or ()):
        assert _guards_intact(e[1], o, a.size), "a write outside the error buffer"
    ob = obig.cpu().numpy()
    assert np.all(ob[:o_off] == 7.0) and np.all(ob[o_off + g.out_floats:] == 7.0), "a write outside out"
    return SimpleNamespace(wire=w[CANARY_BYTES:CANARY_BYTES + G.ub], out=ob[o_off:o_off + g.out_floats],
                           src=[t.cpu().numpy() for t, _ in src], err=[e[0].cpu().numpy() for e in er] if er is not None else None)


def same_by_block(got, want, n, loose, what):
    """Element-wise: all 32 bits outside the `loose` blocks; inside them NaN where the contract has NaN, the bits elsewhere."""
    el = np.repeat(loose, BLOCK)[:n]
    assert mx.same(got[~el], want[~el]), what
    assert mx.same(got[el], want[el], nan_as_one=True), what + " (a block the contract leaves NaN)"


def check(G, res, vs, errs=None, s=None, nonfinite=False, out=True):
    """Every tensor's section, dense decode, gradient and residual against the restatement."""
    for i, v in enumerate(vs):
        n, off, oo = G.sizes[i], G.offs[i], G.g.out_off[i]
        nb = -(-n // BLOCK)
        e = errs[i] if errs is not None else None
        sec, D, w, ne, xp, S = dc.compress(v, G.mode, G.signs, e, s)
        bad_x, bad_s = dc.loose_blocks(xp, S)
        assert nonfinite or not bad_x.any(), "a finite test input whose rotated block is not finite"
        got = res.wire[off:off + sec.size]
        gc, wc = got[:nb * 32].reshape(nb, 32), sec[:nb * 32].reshape(nb, 32)
        assert np.array_equal(gc[~bad_x], wc[~bad_x]), "tensor %d (n = %d): code bytes" % (i, n)
        assert np.array_equal(got[nb * 32:nb * 36].view(np.uint32), sec[nb * 32:nb * 36].view(np.uint32)), "tensor %d (n = %d): scales" % (i, n)
        assert np.array_equal(got[nb * 36:], sec[nb * 36:]) and not got[nb * 36:].any(), "tensor %d (n = %d): the pad" % (i, n)
        loose = bad_x | bad_s | (np.abs(S) >= BIG_S)
        if out:
            same_by_block(res.out[oo:oo + n], D, n, loose, "tensor %d (n = %d): the compress's dense decode" % (i, n))
            assert np.isnan(res.out[oo:oo + n][np.repeat(bad_x, BLOCK)[:n]]).all() and not np.isfinite(res.out[oo:oo + n][np.repeat(bad_s, BLOCK)[:n]]).any()
            end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
            assert np.all(res.out[oo + n:end] == 7.0), "a write behind tensor %d's decode" % i
        if e is not None:
            assert mx.same(res.src[i], w, nonfinite), "tensor %d: g <- w" % i
            same_by_block(res.err[i], ne, n, loose, "tensor %d: err <- w - D" % i)
        else:
            assert mx.same(res.src[i], v), "tensor %d: the source changed without error feedback" % i
    last = G.offs[-1] + dc.section_bytes(G.sizes[-1])
    if not G.dense:
        assert np.all(res.wire[last:] == 0xAB)


@pytest.mark.parametrize("signs", ["seeded", "zero", "seed2"])
@pytest.mark.parametrize("mode", MODES)
def test_sizes(mode, signs):
    """n = 1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8193 in one group (lane, block, step and item seams, runs
    of 2 and 3 items); every tensor holds Gaussian, Student-t, +-0, subnormal and 2^63-sized blocks (the last overflow Q)."""
    vs = [dc.mixed(n, 100 + n) for n in dc.SIZES]
    G = make_group(dc.SIZES, mode, dc.SIGN_SETS[signs])
    check(G, compress(G, vs), vs)


@pytest.mark.parametrize("kind", sorted(dc.FINITE_KINDS))
@pytest.mark.parametrize("mode", MODES)
def test_input_kinds(mode, kind):
    """Whole tensors of one kind: Gaussian, Student-t, all-zero blocks with mixed +-0 (S = +0), subnormals, values that overflow Q."""
    sizes = [ITEM + 300, 257, 77]
    vs = [dc.FINITE_KINDS[kind](n, 500 + n) for n in sizes]
    G = make_group(sizes, mode)
    res = compress(G, vs)
    check(G, res, vs)
    S = dc.compress(vs[0], G.mode, G.signs)[5]
    if kind == "zeros":
        assert not mx.bits_of(S).any()
    if kind == "huge":
        assert np.isinf(S).all() if mode == "unbiased" else np.isfinite(S).all()


@pytest.mark.parametrize("mode", MODES)
def test_error_feedback(mode):
    """ef_scale 0, 1 and 0.5: w stored back, err = w - D; two consecutive records, the second from the first's residual and without
    `out`."""
    sizes = [ITEM + 7, 257, 100]
    G = make_group(sizes, mode)
    for s in (0.0, 1.0, 0.5):
        es = [dc.gaussian(n, 800 + n) for n in sizes]
        for step in (0, 1):
            vs = [dc.student(n, 700 + n + step) for n in sizes]
            res = compress(G, vs, errs=es, s=s, want_out=step == 0)
            check(G, res, vs, es, s, out=step == 0)
            es = [e.copy() for e in res.err]


def test_misaligned_views():
    """Source, error buffer and out each 4-byte but not 16-byte aligned, alone and together: the scalar paths."""
    sizes = [ITEM + 261, 300]
    vs = [dc.mixed(n, 200 + n) for n in sizes]
    es = [dc.gaussian(n, 300 + n) for n in sizes]
    G = make_group(sizes)
    for v_offs, e_offs, o_off in (([1, 0], [0, 0], 0), ([0, 0], [0, 3], 0), ([0, 0], [0, 0], 1), ([1, 2], [3, 1], 1)):
        res = compress(G, vs, errs=es, s=0.5, v_offs=v_offs, e_offs=e_offs, o_off=o_off)
        check(G, res, vs, es, 0.5)
    res = compress(G, vs, v_offs=[3, 1], o_off=2)
    check(G, res, vs)


@pytest.mark.parametrize("mode", MODES)
def test_nonfinite(mode):
    """One inf in a middle block, one NaN in the padded last block: S = 0x7fc00000 there, the block decodes to NaN, and the blocks
    between are finite to the bit."""
    w, bad = dc.nonfinite()
    G = make_group([w.size], mode)
    sec, D, _, _, xp, S = dc.compress(w, G.mode, G.signs)
    assert list(np.flatnonzero(~np.isfinite(xp).all(axis=1))) == bad and np.all(mx.bits_of(S[bad]) == mx.QNAN)
    res = compress(G, [w])
    check(G, res, [w], nonfinite=True)
    res = compress(G, [w], errs=[np.zeros_like(w)], s=1.0)
    check(G, res, [w], [np.zeros_like(w)], 1.0, nonfinite=True)
    ok = np.ones(w.size, bool)
    for b in bad:
        ok[b * BLOCK:(b + 1) * BLOCK] = False
    assert np.isfinite(res.out[:w.size][ok]).all() and np.isnan(res.out[:w.size][~ok]).all()


@pytest.mark.parametrize("mode", MODES)
def test_seventy_tensors_with_identity_tensors(mode):
    rs = np.random.RandomState(9)
    sizes = [int(x) for x in rs.randint(1, 3000, 70)]
    sizes[5], sizes[40] = ITEM + 3, 3 * ITEM
    dense_sizes = [10, 256, 1]
    vs = [dc.student(n, 400 + i) for i, n in enumerate(sizes)]
    dsrc = [mx.randn(n, 500 + n) for n in dense_sizes]
    G = make_group(sizes, mode, dense_sizes=dense_sizes)
    res = compress(G, vs, dense_src=dsrc)
    check(G, res, vs)
    for (off, n), a in zip(G.dense, dsrc):
        assert np.array_equal(res.wire[off:off + 4 * n].view(np.uint32), a.view(np.uint32)), "an identity tensor's copy"


def decode(G, secs_per_payload, R, plain=False, byte_shift=0, stride_pad=0, o_off=0):
    """The group's decode-mean of R payloads laid out at the group's offsets -> out (numpy).  byte_shift: the payloads start that
    many bytes past a 16-byte boundary; stride_pad: extra bytes between payloads."""
    dev, g = G.dev, G.g
    stride = G.ub + stride_pad
    buf = np.full(byte_shift + R * stride + 16, 0xAB, np.uint8)
    for r in range(R):
        for off, sec in zip(G.offs, secs_per_payload[r]):
            buf[byte_shift + r * stride + off:byte_shift + r * stride + off + sec.size] = sec
    t = torch.from_numpy(buf).to(dev)
    gathered = t[byte_shift:byte_shift + R * stride].view(R, stride)[:, :G.ub]
    obig = torch.full((g.out_floats + 8,), 7.0, dtype=torch.float32, device=dev)
    out = obig[o_off:o_off + g.out_floats]
    if not g.ready:
        g.upload_layout()
    g._batch.decode(gathered, R, out, plain=plain)
    torch.cuda.synchronize()
    ob = obig.cpu().numpy()
    assert np.all(ob[:o_off] == 7.0) and np.all(ob[o_off + g.out_floats:] == 7.0), "a write outside out"
    return ob[o_off:o_off + g.out_floats]


def check_decode(G, out, payloads, R, plain=False):
    for i, n in enumerate(G.sizes):
        secs = [payloads[r][i] for r in range(R)]
        want = dc.decode_mean(secs, n, G.signs, plain)
        Ss = np.stack([dc.unpack(s, n)[1] for s in secs])
        loose = ~(np.abs(Ss) < BIG_S).all(axis=0)      # (a NaN, an infinity or a huge scale among the block's R)
        oo = G.g.out_off[i]
        same_by_block(out[oo:oo + n], want, n, loose, "tensor %d (n = %d), R = %d" % (i, n, R))
        end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
        assert np.all(out[oo + n:end] == 7.0)


DEC_SIZES = [1, 255, 257, 600, ITEM + 255, 2 * ITEM + 1]


@pytest.mark.parametrize("signs", ["seeded", "zero"])
def test_decode_mean_of_hand_built_payloads(signs):
    """R = 1 ... 8 and 16, plain on and off at R = 1, on 4-byte aligned and misaligned `gathered`, a user stride larger than the
    section, `out` off a 16-byte boundary; scales 0, -0, subnormal, 3e38 and NaN, block 0 of payloads 0 and 1 cancelling to +0."""
    G = make_group(DEC_SIZES, signs=dc.SIGN_SETS[signs])
    sets = [dc.payloads(n, 16, seed=n) for n in DEC_SIZES]
    payloads = [[sets[i][r] for i in range(len(DEC_SIZES))] for r in range(16)]
    m = dc.mean_rotated([payloads[0][3], payloads[1][3]], DEC_SIZES[3])
    assert not mx.bits_of(m[0]).any(), "payloads 0 and 1 do not cancel to +0 in block 0"
    for R in (1, 2, 3, 4, 5, 6, 7, 8, 16):
        for shift, pad, o_off in ((0, 0, 0), (4, 48, 1), (3, 5, 0)):
            check_decode(G, decode(G, payloads, R, byte_shift=shift, stride_pad=pad, o_off=o_off), payloads, R)
    for shift in (0, 3):
        check_decode(G, decode(G, payloads, 1, plain=True, byte_shift=shift), payloads, 1, plain=True)


@pytest.mark.parametrize("mode", MODES)
def test_plain_decode_equals_the_compress_launchs_own_decode(mode):
    sizes = [ITEM + 300, 77]
    vs = [dc.student(n, 900 + n) for n in sizes]
    G = make_group(sizes, mode)
    res = compress(G, vs)
    payloads = [[res.wire[o:o + dc.section_bytes(n)].copy() for o, n in zip(G.offs, sizes)]]
    got = decode(G, payloads, 1, plain=True)
    assert np.array_equal(mx.bits_of(got), mx.bits_of(res.out))


@pytest.mark.parametrize("mode", MODES)
def test_launches_replay_from_a_graph(mode):
    """Compress (with error feedback and `out`) and decode-mean captured once and replayed: the replay's wire, out, w, err and mean
    equal the eager launches' and the contract's."""
    sizes = [ITEM + 257, 300]
    vs = [dc.student(n, 600 + n) for n in sizes]
    es = [dc.gaussian(n, 650 + n) for n in sizes]
    G = make_group(sizes, mode)
    eager = compress(G, vs, errs=es, s=0.5)
    check(G, eager, vs, es, 0.5)
    dev = G.dev
    src = [torch.from_numpy(v).to(dev) for v in vs]
    err = [torch.from_numpy(e).to(dev) for e in es]
    wire = torch.full((G.ub,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats,), 7.0, device=dev)
    mean = torch.full((G.g.out_floats,), 7.0, device=dev)
    assert G.g._choose_header(src, 0, G.g.align, err, None, None, False)
    b = G.g._batch

    def launches():
        b.compress(wire, out, 0.5)
        b.decode(wire.view(1, -1), 1, mean, plain=True)

    launches()      # (eagerly once: nothing is allocated under capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    for t, a in zip(src + err, vs + es):
        t.copy_(torch.from_numpy(a))
    wire.fill_(0xAB)
    out.fill_(7.0)
    mean.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(wire.cpu().numpy(), eager.wire) and np.array_equal(mx.bits_of(out.cpu().numpy()), mx.bits_of(eager.out))
    for t, a in zip(src + err, eager.src + eager.err):
        assert np.array_equal(mx.bits_of(t.cpu().numpy()), mx.bits_of(a))
    assert np.array_equal(mx.bits_of(mean.cpu().numpy()), mx.bits_of(eager.out))


def test_refusals():
    """Each refusal returns its code before any launch, leaves its text in gq_drive_last_error and writes nothing."""
    from gq_amd import native
    L = native.drive_lib()
    L.gq_drive_last_error.restype = ctypes.c_char_p
    dev = torch.device("cuda:0")
    G = make_group([300])
    v = torch.zeros(300, device=dev)
    wire = torch.full((2 * G.ub + 16,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats + 4,), 7.0, device=dev)
    assert G.g._choose_header([v], 0, 4, None, None, None, False)
    b = G.g._batch
    assert ctypes.sizeof(b.s) == 80 and tuple(b.s.signs) == dc.SEEDED
    one, two = wire[:G.ub].view(1, -1), wire[:2 * G.ub].view(2, -1)

    def refused(call, text):
        with pytest.raises(native.GQNativeError):
            call()
        assert text in L.gq_drive_last_error().decode(), L.gq_drive_last_error()

    refused(lambda: b.compress(wire[4:4 + G.ub]), "16-byte aligned")
    refused(lambda: b.decode(two, 2, out, plain=True), "plain")
    rc = L.gq_drive_decode_sum_batched(b.ref, ctypes.c_void_p(wire.data_ptr()), ctypes.c_int64(G.ub), ctypes.c_int(0), ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_int(0), None)
    assert rc < 0 and "R = 0" in L.gq_drive_last_error().decode()
    rc = L.gq_drive_decode_sum_batched(b.ref, ctypes.c_void_p(wire.data_ptr()), ctypes.c_int64(-16), ctypes.c_int(2), ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_int(0), None)
    assert rc < 0 and "stride" in L.gq_drive_last_error().decode()
    rc = L.gq_drive_decode_sum_batched(b.ref, None, ctypes.c_int64(G.ub), ctypes.c_int(1), ctypes.c_void_p(out.data_ptr()), ctypes.c_int(0), None)
    assert rc < 0 and "null pointer" in L.gq_drive_last_error().decode()
    rc = L.gq_drive_compress_batched(b.ref, ctypes.c_void_p(wire.data_ptr()), ctypes.c_float(float("nan")), ctypes.c_void_p(out.data_ptr() + 2), None)
    assert rc < 0 and "4-byte aligned" in L.gq_drive_last_error().decode()
    b.s.scale_mode = 2
    refused(lambda: b.compress(wire[:G.ub]), "scale_mode")
    refused(lambda: b.decode(one, 1, out), "scale_mode")
    b.s.scale_mode = -1
    refused(lambda: b.compress(wire[:G.ub]), "scale_mode")
    b.s.scale_mode = 0
    b.s.struct_bytes = 48      # gq_mx_batch's size: another library's descriptor
    refused(lambda: b.compress(wire[:G.ub]), "another size")
    refused(lambda: b.decode(one, 1, out), "another size")
    b.s.struct_bytes = 80
    table = b.s.seg_table
    b.s.seg_table = None
    refused(lambda: b.compress(wire[:G.ub]), "null table")
    refused(lambda: b.decode(one, 1, out), "null table")
    b.s.seg_table = table
    items = b.s.item_seg
    b.s.item_seg = None
    refused(lambda: b.compress(wire[:G.ub]), "null table")
    b.s.item_seg = items
    b.s.ndense = 1      # (the group has no dense table)
    refused(lambda: b.compress(wire[:G.ub]), "null dense table")
    b.s.ndense = 0
    b.s.nitems = 0
    refused(lambda: b.compress(wire[:G.ub]), "bad sizes")
    b.s.nitems = 1
    torch.cuda.synchronize()
    assert np.all(wire.cpu().numpy() == 0xAB) and np.all(out.cpu().numpy() == 7.0), "a refused call launched something"
    b.compress(wire[:G.ub])      # and the descriptor still works
    torch.cuda.synchronize()
    assert np.array_equal(wire[:G.ub].cpu().numpy()[:dc.section_bytes(300)], dc.compress(np.zeros(300, f32), dc.UNBIASED, dc.SEEDED)[0])
