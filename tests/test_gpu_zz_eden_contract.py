"""libgq_eden.so held to include/gq_eden.h, bit for bit: every comparison is np.array_equal on bytes or uint32 views against
tests/eden_contract.py (whose own checks are tests/test_eden_contract.py) -- the whole wire section with canaries round the wire,
the dense `out`, the gradient and the residual after error feedback, guards round every buffer.
NaNs: the header leaves the sign and payload of a NaN that an ADDITION produces to the hardware.  So every NaN counts as one
pattern only in a block whose x' is not finite (an inf or a NaN in the input: there the codes are not compared either, S must be
0x7fc00000 and every decoded value a NaN) and in the decode of a block whose scale -- the decode's own input -- is not finite
(S = +inf from a Q that overflowed; the hand-built payloads).  Which blocks those are is computed from the restatement, never
from what the kernels return; everywhere else all 32 bits count.
(zz: the file runs behind the other GPU tests, for the reason tests/test_gpu_z_mx6_api.py gives.)"""
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
import eden_contract as ec  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
ITEM, BLOCK = ec.ITEM, ec.BLOCK
GUARD = f32(-123.25)
CANARY_BYTES = 64
MODES = ["unbiased", "mse"]
# a finite scale from here on may overflow the decode-mean's sum or the inverse transform's: 2^110 * 2.74 (the top magnitude) * 17
# payloads * 256 terms < 2^128, so below it every bit is defined (the hand-built payloads' largest finite scale is 2^100)
BIG_S = f32(2.0 ** 110)


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


def make_group(sizes, bits, mode="unbiased", signs=ec.SEEDED, dense_sizes=()):
    from gq_amd.codecs import BatchedEden, EdenCodec, eden_section_bytes
    dev = torch.device("cuda:0")
    comp = SimpleNamespace(bits=bits, scale=mode, signs=signs)
    codecs = [EdenCodec(comp, n, torch.Size([n])) for n in sizes]
    assert [cd.nbytes for cd in codecs] == [ec.section_bytes(n, bits) for n in sizes] == [eden_section_bytes(n, bits) for n in sizes]
    offs, dense, ub = ec.layout(sizes, bits, dense_sizes)
    g = BatchedEden(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=dense or None)
    return SimpleNamespace(g=g, codecs=codecs, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), mode=ec.MODES[mode], signs=signs,
                           bits=bits)


def compress(G, vs, errs=None, s=None, dense_src=(), v_offs=None, e_offs=None, o_off=0, want_out=True):
    """One compress of the group into a wire full of 0xAB (garbage) between canaries, `out` preset to 7.0 -> wire, out, the sources
    and error buffers afterwards (numpy).  errs: a list with None for a tensor without an error buffer."""
    dev, g = G.dev, G.g
    nt = len(vs)
    v_offs = v_offs or [0] * nt
    e_offs = e_offs or [0] * nt
    src = [_place(v, o, dev) for v, o in zip(vs, v_offs)]
    er = [(_place(e, o, dev) if e is not None else None) for e, o in zip(errs, e_offs)] if errs is not None else None
    ds = [torch.from_numpy(a).to(dev) for a in dense_src]
    whole = torch.full((G.ub + 2 * CANARY_BYTES,), mx.CANARY, dtype=torch.uint8, device=dev)
    wire = whole[CANARY_BYTES:CANARY_BYTES + G.ub]
    wire.fill_(0xAB)
    obig = torch.full((g.out_floats + 8,), 7.0, dtype=torch.float32, device=dev)
    out = obig[o_off:o_off + g.out_floats] if want_out else None
    kw = {}
    if er is not None:
        kw.update(errs=[(e[0] if e is not None else src[i][0]) for i, e in enumerate(er)], ef_scale=float(s))
    if ds:
        kw.update(dense=ds)
    if er is not None and any(e is None for e in er):
        # the group's interface gives every tensor an error buffer or none: write the table's 0 by hand and launch on it
        assert not ds and g._choose_header([t for t, _ in src], 0, g.align, kw["errs"], None, None, False)
        table = g._dev[:g._table_words].view(-1, 8)
        assert table.dtype == torch.int64 and table.shape[0] == nt
        for i, e in enumerate(er):
            if e is None:
                table[i, 7] = 0
        g._batch.compress(wire, out, float(s))
        g.ready = False      # (the next call uploads its own table)
    else:
        assert g.encode([t for t, _ in src], wire, 0, 0, out=out, **kw)
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    assert np.all(w[:CANARY_BYTES] == mx.CANARY) and np.all(w[CANARY_BYTES + G.ub:] == mx.CANARY), "a write outside the wire"
    for (t, big), o, v in zip(src, v_offs, vs):
        assert _guards_intact(big, o, v.size), "a write outside the source"
    for e, o, a in zip(er or (), e_offs, errs or ()):
        assert e is None or _guards_intact(e[1], o, a.size), "a write outside the error buffer"
    ob = obig.cpu().numpy()
    assert np.all(ob[:o_off] == 7.0) and np.all(ob[o_off + g.out_floats:] == 7.0), "a write outside out"
    return SimpleNamespace(wire=w[CANARY_BYTES:CANARY_BYTES + G.ub], out=ob[o_off:o_off + g.out_floats],
                           src=[t.cpu().numpy() for t, _ in src],
                           err=[(e[0].cpu().numpy() if e is not None else None) for e in er] if er is not None else None)


def same_by_block(got, want, n, loose, what):
    """Element-wise: all 32 bits outside the `loose` blocks; inside them NaN where the contract has NaN, the bits elsewhere."""
    el = np.repeat(loose, BLOCK)[:n]
    assert mx.same(got[~el], want[~el]), what
    assert mx.same(got[el], want[el], nan_as_one=True), what + " (a block the contract leaves NaN)"


def check(G, res, vs, errs=None, s=None, nonfinite=False, out=True):
    """Every tensor's section, dense decode, gradient and residual against the restatement."""
    cb = 32 * G.bits
    for i, v in enumerate(vs):
        n, off, oo = G.sizes[i], G.offs[i], G.g.out_off[i]
        nb = -(-n // BLOCK)
        e = errs[i] if errs is not None else None
        sec, D, w, ne, xp, S, _ = ec.compress(v, G.bits, G.mode, G.signs, e, s)
        bad_x, bad_s = ec.loose_blocks(xp, S)
        assert nonfinite or not bad_x.any(), "a finite test input whose rotated block is not finite"
        got = res.wire[off:off + sec.size]
        gc, wc = got[:nb * cb].reshape(nb, cb), sec[:nb * cb].reshape(nb, cb)
        assert np.array_equal(gc[~bad_x], wc[~bad_x]), "tensor %d (n = %d): code bytes" % (i, n)
        assert np.array_equal(got[nb * cb:nb * (cb + 4)].view(np.uint32), sec[nb * cb:nb * (cb + 4)].view(np.uint32)), "tensor %d (n = %d): scales" % (i, n)
        assert np.array_equal(got[nb * (cb + 4):], sec[nb * (cb + 4):]) and not got[nb * (cb + 4):].any(), "tensor %d (n = %d): the pad" % (i, n)
        loose = bad_x | bad_s
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
    last = G.offs[-1] + ec.section_bytes(G.sizes[-1], G.bits)
    if not G.dense:
        assert np.all(res.wire[last:] == 0xAB)


@pytest.mark.parametrize("signs", ["seeded", "zero", "seed2"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", ec.BITS)
def test_sizes(bits, mode, signs):
    """n = 1, 255, 256, 257, 2047, 2048, 2049 (the step seam), 4095, 4096, 4097 (the item seam) and 2 * 4096 + 257 in one group;
    every tensor holds Gaussian, Student-t, +-0, subnormal, 2^-72-sized and 2^63-sized blocks (the last overflow Q); two seeds and
    all-zero sign words; the wire is full of garbage beforehand."""
    vs = ec.gpu_inputs(bits)["sizes"]
    assert [v.size for v in vs] == ec.SIZES and max(ec.SIZES) <= 2 * ITEM + 257
    G = make_group(ec.SIZES, bits, mode, ec.SIGN_SETS[signs])
    check(G, compress(G, vs), vs)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", ec.BITS)
def test_input_kinds_and_three_items(bits, mode):
    """Whole tensors of one kind -- Gaussian, Student-t, +-0 (S = +0), subnormals (Q = 0 with P > 0), 2^-72 (Q * 2^-8 subnormal),
    2^63 (Q = +inf with P finite) -- and a tensor of 3 * 4096 + 100 elements; with `out` and without."""
    inputs = ec.gpu_inputs(bits)
    for kind in sorted(ec.FINITE_KINDS):
        vs = inputs["kind_" + kind]
        G = make_group(ec.KIND_SIZES, bits, mode)
        check(G, compress(G, vs), vs)
    n = 3 * ITEM + 100
    v = dc.student(n, 17)
    G = make_group([n], bits, mode)
    check(G, compress(G, [v]), [v])
    check(G, compress(G, [v], want_out=False), [v], out=False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", ec.BITS)
def test_elements_on_a_threshold(bits, mode):
    """The blocks the CPU search found with an |x'_j| exactly on a theta_i: the compare is strict."""
    v = ec.on_threshold_tensor(bits)
    assert ec.on_threshold_blocks()[bits][1] >= 1
    G = make_group([v.size], bits, mode)
    res = compress(G, [v])
    check(G, res, [v])
    assert not np.array_equal(res.wire[:v.size * bits // 8], ec.compress(v, bits, G.mode, G.signs, ge=True)[0][:v.size * bits // 8])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", ec.BITS)
def test_error_feedback(bits, mode):
    """ef_scale 0.46211715726 and 1: w stored back (the product rounded, then the sum), err = w - D; two consecutive records, the
    second from the first's residual and without `out`; the middle tensor has no error buffer (0) and is compressed without."""
    sizes = [ITEM + 7, 300, 257, 100]
    G = make_group(sizes, bits, mode)
    for s in (0.46211715726, 1.0):
        es = [dc.gaussian(n, 800 + n) for n in sizes]
        es[1] = None
        for step in (0, 1):
            vs = [dc.student(n, 700 + n + step) for n in sizes]
            res = compress(G, vs, errs=es, s=s, want_out=step == 0)
            check(G, res, vs, es, s, out=step == 0)
            es = [(e.copy() if e is not None else None) for e in res.err]


@pytest.mark.parametrize("bits", ec.BITS)
def test_misaligned_views(bits):
    """Source, error buffer and out each 4-byte but not 16-byte aligned (offset by 1 - 3 floats), alone and together."""
    sizes = [ITEM + 261, 300]
    vs = [ec.mixed(n, 200 + n) for n in sizes]
    es = [dc.gaussian(n, 300 + n) for n in sizes]
    G = make_group(sizes, bits)
    for v_offs, e_offs, o_off in (([1, 0], [0, 0], 0), ([0, 0], [0, 3], 0), ([0, 0], [0, 0], 1), ([1, 2], [3, 1], 1)):
        res = compress(G, vs, errs=es, s=0.5, v_offs=v_offs, e_offs=e_offs, o_off=o_off)
        check(G, res, vs, es, 0.5)
    res = compress(G, vs, v_offs=[3, 1], o_off=2)
    check(G, res, vs)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", ec.BITS)
def test_nonfinite(bits, mode):
    """One inf in a middle block, one NaN in the padded last block: S = 0x7fc00000 there, the block decodes to NaN, and the blocks
    between are finite to the bit."""
    w, bad = ec.nonfinite()
    G = make_group([w.size], bits, mode)
    sec, D, _, _, xp, S, _ = ec.compress(w, bits, G.mode, G.signs)
    assert list(np.flatnonzero(~np.isfinite(xp).all(axis=1))) == bad and np.all(mx.bits_of(S[bad]) == mx.QNAN)
    res = compress(G, [w])
    check(G, res, [w], nonfinite=True)
    res = compress(G, [w], errs=[np.zeros_like(w)], s=1.0)
    check(G, res, [w], [np.zeros_like(w)], 1.0, nonfinite=True)
    ok = np.ones(w.size, bool)
    for b in bad:
        ok[b * BLOCK:(b + 1) * BLOCK] = False
    assert np.isfinite(res.out[:w.size][ok]).all() and np.isnan(res.out[:w.size][~ok]).all()


@pytest.mark.parametrize("bits", ec.BITS)
def test_seventy_tensors_with_identity_tensors(bits):
    rs = np.random.RandomState(9)
    sizes = [int(x) for x in rs.randint(1, 3000, 70)]
    sizes[5], sizes[40] = ITEM + 3, 2 * ITEM
    dense_sizes = [10, 256, 1]
    vs = [dc.student(n, 400 + i) for i, n in enumerate(sizes)]
    dsrc = [mx.randn(n, 500 + n) for n in dense_sizes]
    for mode in MODES:
        G = make_group(sizes, bits, mode, dense_sizes=dense_sizes)
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
        want = ec.decode_mean(secs, n, G.bits, G.signs, plain)
        Ss = np.stack([ec.unpack(s, n, G.bits)[1] for s in secs])
        loose = ~(np.abs(Ss) < BIG_S).all(axis=0)      # (a NaN or an infinity among the block's R scales)
        oo = G.g.out_off[i]
        same_by_block(out[oo:oo + n], want, n, loose, "tensor %d (n = %d), R = %d" % (i, n, R))
        end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
        assert np.all(out[oo + n:end] == 7.0)


DEC_SIZES = [1, 255, 257, 600, ITEM + 255, 2 * ITEM + 1]
MAX_R = 17


@pytest.mark.parametrize("signs", ["seeded", "zero"])
@pytest.mark.parametrize("bits", ec.BITS)
def test_decode_mean_of_hand_built_payloads(bits, signs):
    """R = 1 ... 17, plain on and off at R = 1, payloads at byte offsets 0 - 3 with even and odd strides, `out` off a 16-byte
    boundary; block 0 of every payload holds every code value at every position of a lane's b bytes; scales 0, -0, subnormal,
    2^100 (checked to the bit), inf and NaN; block 1 of payloads 0 and 1 cancels to +0."""
    G = make_group(DEC_SIZES, bits, signs=ec.SIGN_SETS[signs])
    sets = [ec.payloads(n, bits, MAX_R, seed=n) for n in DEC_SIZES]
    payloads = [[sets[i][r] for i in range(len(DEC_SIZES))] for r in range(MAX_R)]
    m = ec.mean_rotated([payloads[0][3], payloads[1][3]], DEC_SIZES[3], bits)
    assert not mx.bits_of(m[1]).any(), "payloads 0 and 1 do not cancel to +0 in block 1"
    shifts = ((0, 0, 0), (4, 48, 1), (3, 5, 0), (1, 0, 0), (2, 7, 3))
    for R in range(1, MAX_R + 1):
        for shift, pad, o_off in (shifts if R in (1, 2, 8, 17) else shifts[(R % 3):(R % 3) + 2]):
            check_decode(G, decode(G, payloads, R, byte_shift=shift, stride_pad=pad, o_off=o_off), payloads, R)
    for shift in (0, 1, 2, 3):
        check_decode(G, decode(G, payloads, 1, plain=True, byte_shift=shift), payloads, 1, plain=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", ec.BITS)
def test_plain_decode_against_the_mean_of_one(bits, mode):
    """plain returns the compress launch's own dense decode; the mean of R = 1 differs from it only by +0 + y and / 1, that is
    exactly where y is -0 (the mean gives +0)."""
    sizes = [ITEM + 300, 77, 600]
    vs = [dc.student(n, 900 + n) for n in sizes[:2]] + [dc.zeros_mixed(600, 4)]
    G = make_group(sizes, bits, mode)
    res = compress(G, vs)
    payloads = [[res.wire[o:o + ec.section_bytes(n, bits)].copy() for o, n in zip(G.offs, sizes)]]
    plain = decode(G, payloads, 1, plain=True)
    assert np.array_equal(mx.bits_of(plain), mx.bits_of(res.out))
    mean = decode(G, payloads, 1)
    check_decode(G, mean, payloads, 1)
    for i, n in enumerate(sizes):
        oo = G.g.out_off[i]
        y = ec.mean_rotated([payloads[0][i]], n, bits, plain=True)
        m = ec.mean_rotated([payloads[0][i]], n, bits)
        differ = mx.bits_of(y) != mx.bits_of(m)
        assert np.array_equal(differ, mx.bits_of(y) == np.uint32(0x80000000)), "rotated domain: plain and the mean of one differ at -0 only"
        if i < 2:
            assert not differ.any() and np.array_equal(mx.bits_of(plain[oo:oo + n]), mx.bits_of(mean[oo:oo + n]))
        else:
            assert differ.any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", ec.BITS)
def test_launches_replay_from_a_graph(bits, mode):
    """Compress (with error feedback and `out`) and decode-mean captured once and replayed twice: each replay's wire, out, w, err
    and mean equal the eager launches' and the contract's."""
    sizes = [ITEM + 257, 300]
    vs = [dc.student(n, 600 + n) for n in sizes]
    es = [dc.gaussian(n, 650 + n) for n in sizes]
    G = make_group(sizes, bits, mode)
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
    for _ in range(2):
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
    """Each refusal returns its code before any launch, leaves its text in gq_eden_last_error and writes nothing."""
    from gq_amd import native
    L = native.eden_lib()
    L.gq_eden_last_error.restype = ctypes.c_char_p
    dev = torch.device("cuda:0")
    G = make_group([300], 3)
    v = torch.zeros(300, device=dev)
    wire = torch.full((2 * G.ub + 16,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats + 4,), 7.0, device=dev)
    assert G.g._choose_header([v], 0, 4, None, None, None, False)
    b = G.g._batch
    assert ctypes.sizeof(b.s) == 88 and tuple(b.s.signs) == ec.SEEDED and b.s.bits == 3
    one, two = wire[:G.ub].view(1, -1), wire[:2 * G.ub].view(2, -1)

    def refused(call, text):
        with pytest.raises(native.GQNativeError):
            call()
        assert text in L.gq_eden_last_error().decode(), L.gq_eden_last_error()

    refused(lambda: b.compress(wire[4:4 + G.ub]), "16-byte aligned")
    refused(lambda: b.decode(two, 2, out, plain=True), "plain")
    rc = L.gq_eden_decode_sum_batched(b.ref, ctypes.c_void_p(wire.data_ptr()), ctypes.c_int64(G.ub), ctypes.c_int(0), ctypes.c_void_p(out.data_ptr()),
                                      ctypes.c_int(0), None)
    assert rc < 0 and "R = 0" in L.gq_eden_last_error().decode()
    rc = L.gq_eden_decode_sum_batched(b.ref, ctypes.c_void_p(wire.data_ptr()), ctypes.c_int64(-16), ctypes.c_int(2), ctypes.c_void_p(out.data_ptr()),
                                      ctypes.c_int(0), None)
    assert rc < 0 and "stride" in L.gq_eden_last_error().decode()
    rc = L.gq_eden_decode_sum_batched(b.ref, None, ctypes.c_int64(G.ub), ctypes.c_int(1), ctypes.c_void_p(out.data_ptr()), ctypes.c_int(0), None)
    assert rc < 0 and "null pointer" in L.gq_eden_last_error().decode()
    rc = L.gq_eden_decode_sum_batched(b.ref, ctypes.c_void_p(wire.data_ptr()), ctypes.c_int64(G.ub), ctypes.c_int(1), ctypes.c_void_p(out.data_ptr() + 2),
                                      ctypes.c_int(0), None)
    assert rc < 0 and "4-byte aligned" in L.gq_eden_last_error().decode()
    rc = L.gq_eden_compress_batched(b.ref, ctypes.c_void_p(wire.data_ptr()), ctypes.c_float(float("nan")), ctypes.c_void_p(out.data_ptr() + 2), None)
    assert rc < 0 and "4-byte aligned" in L.gq_eden_last_error().decode()
    rc = L.gq_eden_compress_batched(b.ref, None, ctypes.c_float(float("nan")), None, None)
    assert rc < 0 and "16-byte aligned" in L.gq_eden_last_error().decode()
    for bad in (1, 5, 0, -1, 8):
        b.s.bits = bad
        refused(lambda: b.compress(wire[:G.ub]), "bits %d" % bad)
        refused(lambda: b.decode(one, 1, out), "bits %d" % bad)
    b.s.bits = 3
    for bad in (2, -1):
        b.s.scale_mode = bad
        refused(lambda: b.compress(wire[:G.ub]), "scale_mode")
        refused(lambda: b.decode(one, 1, out), "scale_mode")
    b.s.scale_mode = 0
    b.s.struct_bytes = 80      # gq_drive_batch's size: another library's descriptor
    refused(lambda: b.compress(wire[:G.ub]), "another size")
    refused(lambda: b.decode(one, 1, out), "another size")
    b.s.struct_bytes = 88
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
    assert np.array_equal(wire[:G.ub].cpu().numpy()[:ec.section_bytes(300, 3)], ec.compress(np.zeros(300, f32), 3, ec.UNBIASED, ec.SEEDED)[0])
