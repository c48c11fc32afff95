"""libgq_mxr.so held to include/gq_mxr.h, bit for bit: every comparison is np.array_equal on bytes or uint32 views against
tests/mxr_contract.py (whose own checks are tests/test_mxr_contract.py) -- wire, dense out, the gradient and the residual after
error feedback; only where an input holds an infinity or a NaN does every NaN count as one pattern.  The harness (canaries round
the wire, guarded sources, `out` preset to 7.0) is tests/test_gpu_mx_contract.py's."""
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
import mxr_contract as mxr  # noqa: E402
import mx6_contract as m6  # noqa: E402
import mx_bf16_contract as bx  # noqa: E402
import test_gpu_mx_contract as base  # noqa: E402  (the harness: compress, decode, _split)
import test_gpu_z_mx_bf16_contract as zb  # noqa: E402  (the same harness over either tensor type and all four formats)

pytestmark = pytest.mark.gpu

f32 = np.float32
FMTS = [mx.FP4, mx.FP8]
NAMES = base.NAMES
ITEM = mx.ITEM
SEED = 0x1234567887654321


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def make_group(sizes, fmt, signs=mxr.SEEDED, random=True, rng="device", dense_sizes=(), rotated=True):
    from gq_amd.codecs import BatchedMX, BatchedMXR, MXCodec, MXRCodec
    dev = torch.device("cuda:0")
    comp = SimpleNamespace(format=NAMES[fmt], random=random, _rng=rng, rotate_signs=signs)
    codec, group = (MXRCodec, BatchedMXR) if rotated else (MXCodec, BatchedMX)
    codecs = [codec(comp, n, torch.Size([n])) for n in sizes]
    assert [cd.nbytes for cd in codecs] == [mx.section_bytes(n, fmt) for n in sizes]
    offs, dense, ub = mx.layout(sizes, fmt, dense_sizes)
    g = group(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=dense or None)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return SimpleNamespace(g=g, codecs=codecs, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), fmt=fmt, first=first, signs=signs)


def check(G, res, vs, rs=None, errs=None, s=None, nonfinite=False, out=True):
    """Every tensor's section, dense decode, gradient and residual against the restatement -> the contract's x' per tensor."""
    xps = []
    for i, v in enumerate(vs):
        n, off, oo = G.sizes[i], G.offs[i], G.g.out_off[i]
        e = errs[i] if errs is not None else None
        sec, D, w, ne, xp = mxr.compress(v, G.fmt, G.signs, rs[i] if rs is not None else None, e, s)
        xps.append(xp)
        got = res.wire[off:off + sec.size]
        nb = -(-n // 32)
        assert np.array_equal(got[:nb], sec[:nb]), "tensor %d (n = %d): scale bytes" % (i, n)
        assert np.array_equal(got[:mx._up(nb)], sec[:mx._up(nb)]), "tensor %d (n = %d): the scale bytes' pad" % (i, n)
        assert np.array_equal(got, sec), "tensor %d (n = %d): codes" % (i, n)
        if out:
            assert mx.same(res.out[oo:oo + n], D, nonfinite), "tensor %d (n = %d): the compress's dense decode" % (i, n)
            end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
            assert np.all(res.out[oo + n:end] == 7.0), "a write behind tensor %d's decode" % i
        if e is not None:
            assert mx.same(res.src[i], w, nonfinite), "tensor %d: g <- w" % i
            assert mx.same(res.err[i], ne, nonfinite), "tensor %d: err <- w - D" % i
        else:
            assert mx.same(res.src[i], v), "tensor %d: the source changed without error feedback" % i
    last = G.offs[-1] + mx.section_bytes(G.sizes[-1], G.fmt)
    if not G.dense:
        assert np.all(res.wire[last:] == 0xAB)
    return xps


def witness(G, res, xps, r=None, seed=None):
    """gq_mx_compress_batched, in this process, on the contract's x' with the same draws writes the identical wire."""
    P = make_group(G.sizes, G.fmt, random=G.g.random, rotated=False)
    if getattr(G.g, "rng_pairs", None) is not None:
        P.g.rng_pairs = G.g.rng_pairs
    plain = base.compress(P, xps, r=r, seed=seed)
    assert np.array_equal(plain.wire, res.wire), "the plain MX launch on x' writes another wire"


@pytest.mark.parametrize("mode", ["off", "given", "given_frac", "device", "counter"])
@pytest.mark.parametrize("fmt", FMTS)
def test_sizes(fmt, mode):
    """n = 1, 255, 256, 257, 287, 289, 511, 512, 4095, 4096, 4097, 4096 + 255, 3 * 4096 + 1 in one group under every random mode;
    given_frac: the draws r = frac(x'), under which the wire shows the last bit of the forward transform (test_mxr_contract.py)."""
    sizes = mxr.SIZES
    vs = [mxr.gradients(n, 100 + n) for n in sizes]
    G = make_group(sizes, fmt, random=mode != "off")
    r = seed = rs = None
    if mode == "given":
        r = np.random.RandomState(7).rand(sum(sizes)).astype(f32)
    elif mode == "given_frac":
        r = np.concatenate([mxr.frac_draws(mxr.forward(v, G.signs), fmt) for v in vs])
    elif mode == "device":
        seed = SEED
        rs = [mx.draws(mx.DEVICE, n, int(fd), seed) for n, fd in zip(sizes, G.first)]
    elif mode == "counter":
        G.g.rng_pairs = torch.tensor([[SEED, 41], [0, 0]], dtype=torch.int64, device=G.dev)
        rs = [mx.draws(mx.COUNTER, n, int(fd), SEED, 41) for n, fd in zip(sizes, G.first)]
    if r is not None:
        rs = base._split(r, sizes)
    res = base.compress(G, vs, r=r, seed=seed)
    xps = check(G, res, vs, rs)
    witness(G, res, xps, r=r, seed=seed)


@pytest.mark.parametrize("signs", ["zero", "ones", "seeded"])
@pytest.mark.parametrize("fmt", FMTS)
def test_sign_words(fmt, signs):
    """All-zero words (the pure Hadamard transform), all-ones, and the seeded ones; with error feedback."""
    sizes = [ITEM + 255, 600]
    vs = [mxr.gradients(n, 200 + n) for n in sizes]
    es = [mxr.gradients(n, 300 + n) for n in sizes]
    G = make_group(sizes, fmt, signs=mxr.SIGN_SETS[signs])
    r = np.random.RandomState(8).rand(sum(sizes)).astype(f32)
    res = base.compress(G, vs, r=r, errs=es, s=0.5)
    check(G, res, vs, base._split(r, sizes), es, 0.5)


@pytest.mark.parametrize("fmt", FMTS)
def test_misaligned_views(fmt):
    """Source, error buffer and out each off a 16-byte boundary, alone and together: the scalar paths."""
    sizes = [ITEM + 261, 300]
    vs = [mxr.gradients(n, 200 + n) for n in sizes]
    es = [mxr.gradients(n, 300 + n) for n in sizes]
    G = make_group(sizes, fmt)
    r = np.random.RandomState(8).rand(sum(sizes)).astype(f32)
    for v_offs, e_offs, o_off in (([1, 0], [0, 0], 0), ([0, 0], [0, 3], 0), ([0, 0], [0, 0], 1), ([1, 2], [3, 1], 1)):
        res = base.compress(G, vs, r=r, errs=es, s=0.5, v_offs=v_offs, e_offs=e_offs, o_off=o_off)
        check(G, res, vs, base._split(r, sizes), es, 0.5)


@pytest.mark.parametrize("fmt", FMTS)
def test_error_feedback_two_records(fmt):
    """Two consecutive records: the second starts from the first's residual; also without `out`."""
    sizes = [ITEM + 7, 257, 100]
    G = make_group(sizes, fmt)
    es = [mxr.gradients(n, 800 + n) for n in sizes]
    for step in (0, 1):
        vs = [mxr.gradients(n, 700 + n + step) for n in sizes]
        r = np.random.RandomState(11 + step).rand(sum(sizes)).astype(f32)
        res = base.compress(G, vs, r=r, errs=es, s=0.3, want_out=step == 0)
        check(G, res, vs, base._split(r, sizes), es, 0.3, out=step == 0)
        es = [e.copy() for e in res.err]
        assert all(np.all(np.isfinite(e)) for e in es)


@pytest.mark.parametrize("mode", ["off", "given"])
@pytest.mark.parametrize("fmt", FMTS)
def test_value_edges_finite(fmt, mode):
    """+-0 and subnormals, a block whose x' * 2^-4 is subnormal, sums that overflow to inf from a finite input (scale byte 0xFF in
    all 8 MX blocks).  The input is finite: no NaN is excused on the wire, in w or anywhere outside the overflow block's decode,
    whose values are NaN by the contract (scale byte 0xFF) -- there any NaN counts (an infinity arose inside the transform)."""
    w, at = mxr.edge_finite()
    for signs in ("zero", "seeded"):
        G = make_group([w.size], fmt, signs=mxr.SIGN_SETS[signs], random=mode != "off")
        r = np.random.RandomState(10).rand(w.size).astype(f32) if mode == "given" else None
        for errs in (None, [np.zeros_like(w)]):
            res = base.compress(G, [w], r=r, errs=errs, s=1.0 if errs else None)
            sec, D, ww, ne, xp = mxr.compress(w, fmt, G.signs, r, errs[0] if errs else None, 1.0 if errs else None)
            assert np.array_equal(res.wire[:sec.size], sec)
            o = slice(at["overflow"], at["overflow"] + 256)
            assert np.all(sec[at["overflow"] // 32:at["overflow"] // 32 + 8] == 255) and np.isnan(D[o]).all()
            keep = np.ones(w.size, bool)
            keep[o] = False
            assert mx.same(res.out[:w.size][keep], D[keep]), "the dense decode outside the overflow block: every bit"
            assert np.isnan(res.out[:w.size][o]).all()
            if errs:
                assert mx.same(res.src[0], ww) and mx.same(res.err[0][keep], ne[keep]) and np.isnan(res.err[0][o]).all()


@pytest.mark.parametrize("mode", ["off", "given"])
@pytest.mark.parametrize("fmt", FMTS)
def test_value_edges_nonfinite(fmt, mode):
    """One inf / one NaN in the first and the last position of a rotation block and in the tail: all 8 MX blocks of that rotation
    block get scale byte 0xFF, the blocks next to it stay finite to the bit, in the tail only the MX block that holds it."""
    w, at = mxr.edge_nonfinite()
    G = make_group([w.size], fmt, random=mode != "off")
    r = np.random.RandomState(10).rand(w.size).astype(f32) if mode == "given" else None
    res = base.compress(G, [w], r=r)
    check(G, res, [w], [r] if r is not None else None, nonfinite=True)
    res = base.compress(G, [w], r=r, errs=[np.zeros_like(w)], s=1.0)
    check(G, res, [w], [r] if r is not None else None, [np.zeros_like(w)], 1.0, nonfinite=True)
    for name in ("finite_a", "finite_b"):
        assert np.all(np.isfinite(res.out[at[name]:at[name] + 256]))


@pytest.mark.parametrize("fmt", FMTS)
def test_seventy_tensors_with_identity_tensors(fmt):
    rs = np.random.RandomState(9)
    sizes = [int(x) for x in rs.randint(1, 3000, 70)]
    sizes[5], sizes[40] = ITEM + 3, 3 * ITEM
    dense_sizes = [10, 256, 1]
    vs = [mxr.gradients(n, 400 + i) for i, n in enumerate(sizes)]
    dsrc = [mx.randn(n, 500 + n) for n in dense_sizes]
    G = make_group(sizes, fmt, dense_sizes=dense_sizes)
    r = rs.rand(sum(sizes)).astype(f32)
    res = base.compress(G, vs, r=r, dense_src=dsrc)
    check(G, res, vs, base._split(r, sizes))
    for (off, n), a in zip(G.dense, dsrc):
        assert np.array_equal(res.wire[off:off + 4 * n].view(np.uint32), a.view(np.uint32)), "an identity tensor's copy"


DEC_SIZES = [1, 255, 257, 600, ITEM + 255, 2 * ITEM]


def check_decode(G, out, payloads, R, plain=False):
    for i, n in enumerate(G.sizes):
        want = mxr.decode_mean([payloads[r][i] for r in range(R)], n, G.fmt, G.signs, plain)
        oo = G.g.out_off[i]
        assert mx.same(out[oo:oo + n], want, nan_as_one=True), "tensor %d (n = %d), R = %d" % (i, n, R)   # (payload 0 holds scale byte 0xFF)
        end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
        assert np.all(out[oo + n:end] == 7.0)


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_mean_of_hand_built_payloads(fmt):
    """R = 1 (plain and not), 2, 3, 8 and 16 on 8-byte aligned and misaligned `gathered`; every code value (FP8 code 127 among
    them), scale byte 0xFF in payload 0.  The mean first, then ONE inverse rotation (test_mxr_contract.py: the other order and a
    descending inverse would change bits of these very payloads)."""
    G = make_group(DEC_SIZES, fmt)
    sets = [mxr.payloads(n, fmt, 16, seed=n) for n in DEC_SIZES]
    payloads = [[sets[i][r] for i in range(len(DEC_SIZES))] for r in range(16)]
    for R in (1, 2, 3, 8, 16):
        for shift, pad, o_off in ((0, 0, 0), (4, 0, 1), (3, 5, 0)):
            check_decode(G, base.decode(G, payloads, R, byte_shift=shift, stride_pad=pad, o_off=o_off), payloads, R)
    for shift in (0, 3):
        check_decode(G, base.decode(G, payloads, 1, plain=True, byte_shift=shift), payloads, 1, plain=True)


@pytest.mark.parametrize("fmt", FMTS)
def test_plain_decode_equals_the_compress_launchs_own_decode(fmt):
    sizes = [ITEM + 300, 77]
    vs = [mxr.gradients(n, 900 + n) for n in sizes]
    G = make_group(sizes, fmt, random=False)
    res = base.compress(G, vs)
    payloads = [[res.wire[o:o + mx.section_bytes(n, fmt)].copy() for o, n in zip(G.offs, sizes)]]
    got = base.decode(G, payloads, 1, plain=True)
    assert np.array_equal(mx.bits_of(got), mx.bits_of(res.out))


@pytest.mark.parametrize("fmt", FMTS)
def test_launches_replay_from_a_graph_with_counter_draws(fmt):
    """Compress and decode-mean captured once and replayed twice with the step word moved in between: the draws differ between
    the replays and each replay matches the contract."""
    from gq_amd import native
    sizes = [ITEM + 257, 300]
    vs = [mxr.gradients(n, 600 + n) for n in sizes]
    G = make_group(sizes, fmt)
    dev = G.dev
    pairs = torch.tensor([[SEED, 5], [0, 0]], dtype=torch.int64, device=dev)
    src = [torch.from_numpy(v).to(dev) for v in vs]
    wire = torch.full((G.ub,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats,), 7.0, device=dev)
    mean = torch.full((G.g.out_floats,), 7.0, device=dev)
    assert G.g._choose_header(src, 0, G.g.align, None, None, None, False)
    b = G.g._batch

    def launches():
        b.compress(wire, native.RANDOM_DEVICE_COUNTER, pairs.data_ptr(), None, out)
        b.decode(wire.view(1, -1), 1, mean, plain=True)

    launches()      # (eagerly once: nothing is allocated under capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    seen = []
    for step in (5, 6):
        wire.fill_(0xAB)
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        res = SimpleNamespace(wire=wire.cpu().numpy(), out=out.cpu().numpy(), src=[t.cpu().numpy() for t in src], err=None)
        check(G, res, vs, [mx.draws(mx.COUNTER, n, int(fd), SEED, step) for n, fd in zip(sizes, G.first)])
        assert np.array_equal(mx.bits_of(mean.cpu().numpy()), mx.bits_of(res.out))
        seen.append(res.wire.copy())
        pairs[0, 1] += 1
    assert not np.array_equal(seen[0], seen[1]), "two replays drew the same numbers"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("fmt", bx.FMTS)
def test_what_is_not_rotated_is_the_plain_librarys_bytes(fmt, dtype):
    """The two libraries are two instantiations of one kernel body (csrc/mx_kernels.hpp), held against each other here with no
    restatement in between.  A tensor shorter than a rotation block (n = 1, 31, 255, one tensor each) is `the tail as it is`:
    libgq_mxr.so with the seeded sign words writes the wire, `out` and, under error feedback, w and err that libgq_mx.so writes,
    byte for byte.  n = 256 + 255 has one rotated block: the scale bytes from block 8 on, the code bytes, `out`, w and err from
    element 256 on agree likewise.  Nearest rounding and given draws, with and without error feedback; then the decode-mean of
    the same payloads at R = 1 (plain and not) and R = 3."""
    torch_dtype = torch.float32 if dtype == "f32" else torch.bfloat16
    bits = {m6.FP4: 4, m6.FP8: 8}.get(fmt, 6)

    def tail(res, n, nb_pad, k):
        """What of a launch's results belongs to the elements from k on: scale bytes, code bytes, out, source, residual."""
        sec = res.wire[:m6.section_bytes(n, fmt)]
        parts = [sec[k // 32:nb_pad], sec[nb_pad + k * bits // 8:], res.out[k:n], res.src[0][k:]]
        return parts + ([res.err[0][k:]] if res.err else [])

    for n, k in ((1, 0), (31, 0), (255, 0), (mxr.RBLOCK + 255, mxr.RBLOCK)):
        nb_pad = mx._up(-(-n // 32))
        v = mxr.gradients(n, 1100 + n) if dtype == "f32" else bx.randn16(n, 1100 + n)
        e = mxr.gradients(n, 1200 + n)
        r = np.random.RandomState(n).rand(n).astype(f32)
        payloads = []
        for mode in ("off", "given"):
            groups = {x: zb.make_group([n], fmt, dtype=torch_dtype, random=mode != "off", signs=mxr.SEEDED if x else None) for x in (False, True)}
            for errs in (None, [e]):
                plain, rot = (zb.compress(groups[x], [v], mode, r, errs=errs, s=0.5 if errs else None) for x in (False, True))
                if k == 0:
                    assert np.array_equal(plain.wire, rot.wire), "n = %d, %s, ef %s: the whole wire" % (n, mode, bool(errs))
                for name, a, b in zip(("scale bytes", "code bytes", "out", "g <- w", "err"), tail(plain, n, nb_pad, k), tail(rot, n, nb_pad, k)):
                    assert a.size == b.size and a.tobytes() == b.tobytes(), "n = %d, %s, ef %s: %s from element %d on" % (n, mode, bool(errs), name, k)
                if len(payloads) < 3:
                    payloads.append([plain.wire[:m6.section_bytes(n, fmt)].copy()])
        dec = base.decode if dtype == "f32" else zb.decode
        for R, is_plain in ((1, True), (1, False), (3, False)):
            a, b = (dec(groups[x], payloads, R, plain=is_plain)[k:n] for x in (False, True))
            assert a.size == n - k and a.tobytes() == b.tobytes(), "n = %d: the decode-mean, R = %d%s" % (n, R, ", plain" if is_plain else "")


def test_refusals():
    """Each refusal comes before any launch and leaves its text in gq_mxr_last_error."""
    from gq_amd import native
    L = native.mxr_lib()
    L.gq_mxr_last_error.restype = ctypes.c_char_p
    dev = torch.device("cuda:0")
    G = make_group([300], mx.FP4)
    v = torch.zeros(300, device=dev)
    wire = torch.full((G.ub + 16,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats,), 7.0, device=dev)
    assert G.g._choose_header([v], 0, 4, None, None, None, False)
    b = G.g._batch
    assert ctypes.sizeof(b.s) == 80 and tuple(b.s.signs) == mxr.SEEDED

    def refused(call, text):
        with pytest.raises(native.GQNativeError):
            call()
        assert text in L.gq_mxr_last_error().decode(), L.gq_mxr_last_error()

    refused(lambda: b.compress(wire[:G.ub], 3), "random_mode")
    refused(lambda: b.compress(wire[:G.ub], native.RANDOM_GIVEN), "without draws")
    refused(lambda: b.compress(wire[4:4 + G.ub], native.RANDOM_OFF), "16-byte aligned")
    refused(lambda: b.compress(wire[:G.ub], native.RANDOM_DEVICE_COUNTER, seed=0), "pair")
    refused(lambda: b.compress(wire[:G.ub], native.RANDOM_DEVICE_COUNTER, seed=12), "pair")
    fmt = b.s.format
    b.s.format = 2
    refused(lambda: b.compress(wire[:G.ub], native.RANDOM_OFF), "format")
    refused(lambda: b.decode(wire[:G.ub].view(1, -1), 1, out), "format")
    b.s.format = fmt
    b.s.struct_bytes = 48      # gq_mx_batch's size: the plain descriptor is not this library's
    refused(lambda: b.compress(wire[:G.ub], native.RANDOM_OFF), "another size")
    refused(lambda: b.decode(wire[:G.ub].view(1, -1), 1, out), "another size")
    b.s.struct_bytes = 80
    table = b.s.seg_table
    b.s.seg_table = None
    refused(lambda: b.compress(wire[:G.ub], native.RANDOM_OFF), "null table")
    refused(lambda: b.decode(wire[:G.ub].view(1, -1), 1, out), "null table")
    b.s.seg_table = table
    torch.cuda.synchronize()
    assert np.all(wire.cpu().numpy() == 0xAB) and np.all(out.cpu().numpy() == 7.0), "a refused call launched something"
    b.compress(wire[:G.ub], native.RANDOM_OFF)      # and the descriptor still works
    torch.cuda.synchronize()
    assert np.array_equal(wire[:G.ub].cpu().numpy()[:mx.section_bytes(300, mx.FP4)], mxr.compress(np.zeros(300, f32), mx.FP4, mxr.SEEDED)[0])
