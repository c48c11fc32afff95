"""The *_streams launches of libgq_drive.so and libgq_eden.so held to SIGNS, PER STREAM and DECODE-MEAN, PER STREAM of their headers,
bit for bit: the expected outputs are tests/rot_user_contract.py's; every comparison is np.array_equal on bytes or uint32 views,
through the helpers of the two existing GPU contract files (canaries round the wire, guards round every buffer).  The compress inputs
are finite Gaussians and Student-t values, so no block's NaNs are left to the hardware there; the hand-built payloads of the
decode-mean hold zero, subnormal, huge, infinite and NaN scales, handled as in those files (a block with such a scale among its R
counts as one NaN pattern; which blocks those are comes from the payloads, never from what the kernels return).
The descriptors carry garbage sign words: a *_streams launch must not read them.
Every launch is one workgroup per item of 4,096 elements, so "a workgroup that takes several items" has no counterpart here; the
long list below is sized from the CU count so that every CU takes workgroups of three tensors or more in turn."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402
import drive_contract as dc  # noqa: E402
import eden_contract as ec  # noqa: E402
import rot_step_contract as rs  # noqa: E402
import rot_user_contract as ru  # noqa: E402
import test_gpu_zz_drive_contract as tdc  # noqa: E402
import test_gpu_zz_eden_contract as tec  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
M64 = rs.M64
GARBAGE = (0xDEADBEEFDEADBEEF, 0x0123456789ABCDEF, M64, 0)
SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 8193]
DENSE = [300]
STREAMS = [0, 1, 7, 2 ** 31 - 1]
STEPS = [0, 3]
SEED = 5
KINDS = [("drive", "unbiased"), ("drive", "mse"), ("eden2", "unbiased"), ("eden2", "mse"), ("eden3", "unbiased"), ("eden3", "mse"),
         ("eden4", "unbiased"), ("eden4", "mse")]
IDS = ["%s-%s" % k for k in KINDS]
DEC_KINDS = ["drive", "eden2", "eden3", "eden4"]


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _signed(w):
    return (w & M64) - (1 << 64 if w & (1 << 63) else 0)


def make_pair(seed, step):
    return torch.tensor([[_signed(seed), _signed(step)]], dtype=torch.int64).cuda()


class _StreamsBatch(object):
    """The group's descriptor with the pair and `first_stream` on every decode (the existing helpers call _batch.decode without)."""

    def __init__(self, batch, pair, first):
        self._b, self._pair, self.first = batch, pair, first

    def decode(self, gathered, R, out, plain=False):
        return self._b.decode(gathered, R, out, plain=plain, rotation=self._pair, first_stream=self.first)

    def __getattr__(self, name):
        return getattr(self._b, name)


def make(kind, mode, sizes, seed, step, stream, dense_sizes=(), first=0):
    """-> (helper module, group of the existing contract file) whose compress runs under `stream` and whose decode-mean starts at
    stream `first`; G.signs: the words the restatement of ONE payload under `stream` rotates by."""
    if kind == "drive":
        T, G = tdc, tdc.make_group(sizes, mode, GARBAGE, dense_sizes)
    else:
        T, G = tec, tec.make_group(sizes, int(kind[-1]), mode, GARBAGE, dense_sizes)
    G.pair = make_pair(seed, step)
    G.g.own, G.g.rotation, G.g.stream_base = True, G.pair, stream      # BatchedDrive.encode: slot 0 -> stream_base
    G.g._batch = _StreamsBatch(G.g._batch, G.pair, first)
    G.signs = ru.words_of(seed, step, stream)
    G.kind, G.seed, G.step, G.T = kind, seed, step, T
    return T, G


def make_stepped(kind, mode, sizes, seed, step):
    """The same group on the existing *_stepped launches (tests/test_gpu_zz_rot_step_contract.py's way)."""
    import test_gpu_zz_rot_step_contract as trs
    return trs.make(kind, mode, sizes, seed, step)


# ---- compress -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("kind,mode", KINDS, ids=IDS)
def test_streams_compress(kind, mode, stream, step):
    """Wire, `out`, then err and the gradient stored back under error feedback (with and without `out`), one identity-compressed
    tensor riding along; canaries round the wire and guards round every buffer are tests/test_gpu_zz_drive_contract.compress's."""
    T, G = make(kind, mode, SIZES, SEED, step, stream, DENSE)
    vs = [dc.student(n, 100 + n) for n in SIZES]
    dsrc = [mx.randn(n, 500 + n) for n in DENSE]
    res = T.compress(G, vs, dense_src=dsrc)
    T.check(G, res, vs)
    for (off, n), a in zip(G.dense, dsrc):
        assert np.array_equal(res.wire[off:off + 4 * n].view(np.uint32), a.view(np.uint32)), "the identity tensor's copy"
    es = [dc.gaussian(n, 800 + n) for n in SIZES]
    res = T.compress(G, vs, errs=es, s=0.5, dense_src=dsrc)
    T.check(G, res, vs, es, 0.5)
    res = T.compress(G, vs, errs=es, s=0.5, dense_src=dsrc, want_out=False)
    T.check(G, res, vs, es, 0.5, out=False)
    torch.cuda.synchronize()
    assert G.pair.cpu().tolist() == [[SEED, step]], "a launch wrote the pair"


@pytest.mark.parametrize("kind,mode", [("drive", "unbiased"), ("eden3", "mse")], ids=["drive", "eden3"])
def test_misaligned_views(kind, mode):
    """Source, error buffer and out each 4-byte but not 16-byte aligned, alone and together: the scalar paths."""
    sizes = [dc.ITEM + 261, 300]
    vs = [dc.student(n, 200 + n) for n in sizes]
    es = [dc.gaussian(n, 300 + n) for n in sizes]
    T, G = make(kind, mode, sizes, SEED, 3, 7)
    for v_offs, e_offs, o_off in (([1, 0], [0, 0], 0), ([0, 0], [0, 3], 0), ([0, 0], [0, 0], 1), ([1, 2], [3, 1], 1)):
        T.check(G, T.compress(G, vs, errs=es, s=0.5, v_offs=v_offs, e_offs=e_offs, o_off=o_off), vs, es, 0.5)
    T.check(G, T.compress(G, vs, v_offs=[3, 1], o_off=2), vs)


@pytest.mark.parametrize("kind,mode", [("drive", "mse"), ("eden2", "unbiased"), ("eden4", "unbiased")], ids=["drive", "eden2", "eden4"])
def test_seventy_tensors_in_one_group(kind, mode):
    rng = np.random.RandomState(9)
    sizes = [int(x) for x in rng.randint(1, 3000, 70)]
    sizes[5], sizes[40] = dc.ITEM + 3, 3 * dc.ITEM
    vs = [dc.student(n, 400 + i) for i, n in enumerate(sizes)]
    T, G = make(kind, mode, sizes, SEED, 0, 7)
    T.check(G, T.compress(G, vs), vs)


_long = {}


def _long_list():
    """Tensors of one, two and three items (and a ragged end each), 3 x CU count items and more in all: every CU takes workgroups of
    several tensors in turn.  Built once, with its inputs."""
    if not _long:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        sizes, items, i = [], 0, 0
        while items < 3 * cus:
            k = 1 + i % 3
            sizes.append(k * dc.ITEM - (i * 37) % 300)
            items += k
            i += 1
        _long["sizes"], _long["items"], _long["cus"] = sizes, items, cus
        _long["vs"] = [dc.gaussian(n, 1000 + j) for j, n in enumerate(sizes)]
    return _long


@pytest.mark.parametrize("kind,mode", [("drive", "unbiased"), ("eden4", "unbiased")], ids=["drive", "eden4"])
def test_a_list_of_three_times_the_cu_count_items(kind, mode):
    L = _long_list()
    assert L["items"] >= 3 * L["cus"] and len(L["sizes"]) >= L["cus"]
    T, G = make(kind, mode, L["sizes"], SEED, 3, 1)
    res = T.compress(G, L["vs"])
    T.check(G, res, L["vs"])
    # and the decode-mean of that wire twice over, under streams 1 and 2 (the second payload decodes under another rotation)
    G.g._batch.first = 1
    payload = [res.wire[o:o + ru.section_bytes(kind, n)].copy() for o, n in zip(G.offs, L["sizes"])]
    out = T.decode(G, [payload, payload], 2)
    for i, n in enumerate(L["sizes"]):
        want = ru.decode_mean(kind, [payload[i], payload[i]], n, SEED, 3, first_stream=1)
        oo = G.g.out_off[i]
        assert np.array_equal(mx.bits_of(out[oo:oo + n]), mx.bits_of(want)), "tensor %d" % i


@pytest.mark.parametrize("kind,mode", KINDS, ids=IDS)
def test_stream_zero_is_the_stepped_compress_byte_for_byte(kind, mode):
    sizes = [257, dc.ITEM + 300, 77]
    vs = [dc.student(n, 300 + n) for n in sizes]
    es = [dc.gaussian(n, 400 + n) for n in sizes]
    for seed, step in ((1, 0), (M64, 3)):
        T, Gn = make(kind, mode, sizes, seed, step, 0)
        _, Gs = make_stepped(kind, mode, sizes, seed, step)
        a, b = T.compress(Gn, vs, errs=es, s=0.5), T.compress(Gs, vs, errs=es, s=0.5)
        assert np.array_equal(a.wire, b.wire) and np.array_equal(mx.bits_of(a.out), mx.bits_of(b.out))
        for x, y in zip(a.src + a.err, b.src + b.err):
            assert np.array_equal(mx.bits_of(x), mx.bits_of(y))


# ---- decode-mean --------------------------------------------------------------------------------------------------------------------
DEC_SIZES = [1, 255, 257, 600, dc.ITEM + 255]
MAX_R = 17
_payload_cache = {}


def hand_built(kind):
    """MAX_R payloads per tensor of DEC_SIZES (tests/drive_contract.payloads / tests/eden_contract.payloads: scales 0, -0, subnormal,
    3e38, NaN), and in block 0: payload 1 with every code all-zero, payload 2 with every code all-ones, payload 5 with S = +inf.
    -> payloads[r][i]; built once per kind and left unchanged."""
    if kind not in _payload_cache:
        bits = ru.bits_of_kind(kind)
        sets = []
        for n in DEC_SIZES:
            secs = dc.payloads(n, MAX_R, seed=n) if kind == "drive" else ec.payloads(n, bits, MAX_R, seed=n)
            for r, codes, S in ((1, 0, None), (2, (1 << bits) - 1, None), (5, None, np.inf)):
                c, s = dc.unpack(secs[r], n) if kind == "drive" else ec.unpack(secs[r], n, bits)
                if codes is not None:
                    c[0] = codes
                if S is not None:
                    s[0] = S
                secs[r] = dc.pack(c, s) if kind == "drive" else ec.pack(c, s, bits)
            sets.append(secs)
        _payload_cache[kind] = [[sets[i][r] for i in range(len(DEC_SIZES))] for r in range(MAX_R)]
    return _payload_cache[kind]


def check_decode(G, out, payloads, R, first, plain=False):
    for i, n in enumerate(G.sizes):
        secs = [payloads[r][i] for r in range(R)]
        want = ru.decode_mean(G.kind, secs, n, G.seed, G.step, first, plain)
        Ss = np.stack([ru.scales_of(G.kind, s, n) for s in secs])
        loose = ~(np.abs(Ss) < G.T.BIG_S).all(axis=0)      # (a NaN, an infinity or a huge scale among the block's R)
        oo = G.g.out_off[i]
        G.T.same_by_block(out[oo:oo + n], want, n, loose, "tensor %d (n = %d), R = %d, first stream %d" % (i, n, R, first))
        assert np.isnan(out[oo:oo + n][np.repeat(np.isnan(Ss).any(axis=0), dc.BLOCK)[:n]]).all()
        end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
        assert np.all(out[oo + n:end] == 7.0), "a write behind tensor %d's decode" % i


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("kind", DEC_KINDS)
def test_decode_mean_of_hand_built_payloads(kind, first):
    """R = 1 (plain and not), 2, 3, 8, 16, 17 on aligned payloads, on payloads at odd byte strides and on an `out` off a 16-byte
    boundary; `out` is preset and checked outside the tensors (tests/test_gpu_zz_drive_contract.decode)."""
    T, G = make(kind, "unbiased", DEC_SIZES, M64, 3, 0, first=first)
    payloads = hand_built(kind)
    for shift, pad, o_off in ((0, 0, 0), (3, 5, 1)):
        check_decode(G, T.decode(G, payloads, 1, plain=True, byte_shift=shift, stride_pad=pad, o_off=o_off), payloads, 1, first, plain=True)
        for R in (1, 2, 3, 8, 16, 17):
            check_decode(G, T.decode(G, payloads, R, byte_shift=shift, stride_pad=pad, o_off=o_off), payloads, R, first)
    check_decode(G, T.decode(G, payloads, 3, byte_shift=4, stride_pad=48), payloads, 3, first)      # (4-byte aligned, not 16)


@pytest.mark.parametrize("kind", DEC_KINDS)
def test_one_payload_from_stream_zero_is_the_stepped_decode_byte_for_byte(kind):
    """plain: every bit.  Not plain: every bit but the sign of a zero and the payload of a NaN (see below)."""
    payloads = hand_built(kind)
    for seed, step in ((1, 0), (M64, 3)):
        T, Gn = make(kind, "unbiased", DEC_SIZES, seed, step, 0)
        _, Gs = make_stepped(kind, "unbiased", DEC_SIZES, seed, step)
        for plain in (True, False):
            for shift in (0, 3):
                a, b = T.decode(Gn, payloads, 1, plain=plain, byte_shift=shift), T.decode(Gs, payloads, 1, plain=plain, byte_shift=shift)
                same = mx.bits_of(a) == mx.bits_of(b)
                if plain:
                    assert same.all(), (seed, step, plain, shift)
                else:
                    # m = (+0 + D) / 1 here, inverse((+0 + y) / 1) there: the same bits wherever the value is not a zero -- the
                    # per-stream order adds +0 AFTER the sign flip, which turns a -0 into +0, the stepped order before it -- and
                    # not a NaN, whose payload an addition chooses
                    assert (same | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))).all(), (seed, step, plain, shift)
                    assert same.sum() > a.size // 2


@pytest.mark.parametrize("kind", DEC_KINDS)
def test_two_identical_payloads_do_not_decode_as_under_the_shared_rotation(kind):
    """What the feature is: two users send the SAME bytes; under the shared rotation their mean is one user's decode, under their own
    rotations the second payload is rotated back by stream 1's words -- the restatement's output, and not the shared launch's."""
    sizes = [dc.ITEM + 300, 257]
    seed, step = 5, 3
    vs = [dc.gaussian(n, 70 + n) for n in sizes]
    T, Gn = make(kind, "unbiased", sizes, seed, step, 0)
    _, Gs = make_stepped(kind, "unbiased", sizes, seed, step)
    res = T.compress(Gn, vs)
    payload = [res.wire[o:o + ru.section_bytes(kind, n)].copy() for o, n in zip(Gn.offs, sizes)]
    own, shared = T.decode(Gn, [payload, payload], 2), T.decode(Gs, [payload, payload], 2)
    for i, n in enumerate(sizes):
        oo = Gn.g.out_off[i]
        want = ru.decode_mean(kind, [payload[i]] * 2, n, seed, step)
        assert np.array_equal(mx.bits_of(own[oo:oo + n]), mx.bits_of(want)), "tensor %d" % i
        assert np.array_equal(mx.bits_of(shared[oo:oo + n]), mx.bits_of(ru.decode_mean_rotated_sum(kind, [payload[i]] * 2, n, seed, step)))
        assert not np.array_equal(mx.bits_of(own[oo:oo + n]), mx.bits_of(shared[oo:oo + n])), "tensor %d: the shared launch's output" % i
    # two users under their own streams: the mean of their decodes.  Independent unbiased decodes put its error at 1 / sqrt(2) = 0.71
    # of one user's (tests/test_rot_user_contract.py: the law, within 10%); the shared rotation leaves it at 1.0.  0.85 lies between
    # the two; asserted on the tensor of 17 blocks, the law's size.
    T1, G1 = make(kind, "unbiased", sizes, seed, step, 1)
    res1 = T1.compress(G1, vs)
    p1 = [res1.wire[o:o + ru.section_bytes(kind, n)].copy() for o, n in zip(G1.offs, sizes)]
    both = T.decode(Gn, [payload, p1], 2)
    for i, n in enumerate(sizes):
        oo = Gn.g.out_off[i]
        assert np.array_equal(mx.bits_of(both[oo:oo + n]), mx.bits_of(ru.decode_mean(kind, [payload[i], p1[i]], n, seed, step)))
        if i == 0:
            assert dc.rel_l2(both[oo:oo + n], vs[i]) < 0.85 * dc.rel_l2(res.out[oo:oo + n], vs[i])


# ---- refusals, graphs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["drive", "eden4"])
def test_refusals(kind):
    """A negative stream, a first_stream + R that overflows int32, a null or misaligned pair, and what the stepped calls refuse:
    each returns its code before any launch and writes nothing."""
    from gq_amd import native
    T, G = make(kind, "unbiased", [300], 1, 0, 0)
    L = native.drive_lib() if kind == "drive" else native.eden_lib()
    prefix = "gq_drive_" if kind == "drive" else "gq_eden_"
    last = getattr(L, prefix + "last_error")
    last.restype = ctypes.c_char_p
    comp, dec = getattr(L, prefix + "compress_batched_streams"), getattr(L, prefix + "decode_sum_batched_streams")
    dev = G.dev
    v = torch.zeros(300, device=dev)
    wire = torch.full((2 * G.ub + 16,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats + 4,), 7.0, device=dev)
    assert G.g._choose_header([v], 0, 4, None, None, None, False)
    b, pair = G.g._batch._b, G.pair
    P, W, O = ctypes.c_void_p(pair.data_ptr()), ctypes.c_void_p(wire.data_ptr()), ctypes.c_void_p(out.data_ptr())
    nan, i32, i64, ci = ctypes.c_float(float("nan")), ctypes.c_int32, ctypes.c_int64, ctypes.c_int
    top = 2 ** 31 - 1

    def refused(rc, text):
        assert rc < 0 and text in last().decode(), (rc, last())

    refused(comp(b.ref, P, i32(-1), W, nan, O, None), "negative")
    refused(comp(b.ref, P, i32(-2 ** 31), W, nan, O, None), "negative")
    refused(dec(b.ref, P, i32(-1), W, i64(G.ub), ci(1), O, ci(0), None), "negative")
    refused(dec(b.ref, P, i32(top), W, i64(G.ub), ci(1), O, ci(0), None), "overflows int32")
    refused(dec(b.ref, P, i32(top - 1), W, i64(G.ub), ci(2), O, ci(0), None), "overflows int32")
    refused(comp(b.ref, None, i32(0), W, nan, O, None), "rotation")
    refused(comp(b.ref, ctypes.c_void_p(pair.data_ptr() + 4), i32(0), W, nan, O, None), "rotation")
    refused(dec(b.ref, None, i32(0), W, i64(G.ub), ci(1), O, ci(0), None), "rotation")
    refused(dec(b.ref, ctypes.c_void_p(pair.data_ptr() + 4), i32(0), W, i64(G.ub), ci(1), O, ci(0), None), "rotation")
    refused(comp(b.ref, P, i32(0), ctypes.c_void_p(wire.data_ptr() + 4), nan, O, None), "16-byte aligned")
    refused(comp(b.ref, P, i32(0), None, nan, O, None), "16-byte aligned")
    refused(comp(b.ref, P, i32(0), W, nan, ctypes.c_void_p(out.data_ptr() + 2), None), "4-byte aligned")
    refused(dec(b.ref, P, i32(0), W, i64(G.ub), ci(2), O, ci(1), None), "plain")
    refused(dec(b.ref, P, i32(0), W, i64(G.ub), ci(0), O, ci(0), None), "R = 0")
    refused(dec(b.ref, P, i32(0), W, i64(-16), ci(2), O, ci(0), None), "stride")
    refused(dec(b.ref, P, i32(0), None, i64(G.ub), ci(1), O, ci(0), None), "null pointer")
    size = b.s.struct_bytes
    b.s.struct_bytes = 48
    refused(comp(b.ref, P, i32(0), W, nan, O, None), "another size")
    refused(dec(b.ref, P, i32(0), W, i64(G.ub), ci(1), O, ci(0), None), "another size")
    b.s.struct_bytes = size
    b.s.scale_mode = 2
    refused(comp(b.ref, P, i32(0), W, nan, O, None), "scale_mode")
    b.s.scale_mode = 0
    table = b.s.seg_table
    b.s.seg_table = None
    refused(comp(b.ref, P, i32(0), W, nan, O, None), "null table")
    b.s.seg_table = table
    with pytest.raises(TypeError, match="stream"):      # the binding's own checks
        b.compress(wire[:G.ub], rotation=pair, stream=1.5)
    with pytest.raises(TypeError, match="rotation"):
        b.compress(wire[:G.ub], rotation=None, stream=1)
    torch.cuda.synchronize()
    assert np.all(wire.cpu().numpy() == 0xAB) and np.all(out.cpu().numpy() == 7.0), "a refused call launched something"
    b.compress(wire[:G.ub], rotation=pair, stream=top)      # and the descriptor still works, at the largest stream
    b.decode(wire[:G.ub].view(1, -1), 1, out[:G.g.out_floats], plain=True, rotation=pair, first_stream=top - 1)
    torch.cuda.synchronize()
    zero = np.zeros(300, f32)
    want = ru.compress(kind, zero, dc.UNBIASED, 1, 0, top)[0]
    assert np.array_equal(wire[:G.ub].cpu().numpy()[:want.size], want)


@pytest.mark.parametrize("kind,mode", [("drive", "unbiased"), ("eden3", "unbiased")], ids=["drive", "eden3"])
def test_one_graph_follows_the_step_word(kind, mode):
    """Compress under stream 3 and the decode-mean of two payloads from stream 3 captured as ONE graph and replayed with the step
    word moved in between: each replay's wire and outputs are the contract's at the step it finds."""
    sizes = [dc.ITEM + 257, 300]
    vs = [dc.student(n, 600 + n) for n in sizes]
    seed, stream = 5, 3
    T, G = make(kind, mode, sizes, seed, 0, stream, first=stream)
    dev, pair = G.dev, G.pair
    src = [torch.from_numpy(v).to(dev) for v in vs]
    wire = torch.full((2, G.ub), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats,), 7.0, device=dev)
    mean = torch.full((G.g.out_floats,), 7.0, device=dev)
    assert G.g._choose_header(src, 0, G.g.align, None, None, None, False)
    b = G.g._batch

    def launches():
        b.compress(wire[0], out, None, rotation=pair, stream=stream)
        b.decode(wire, 2, mean)      # (the proxy adds the pair and the first stream; row 1 is a copy of row 0, made below)

    launches()      # (eagerly once: nothing is allocated under capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    seen = []
    for step in (0, 4, 1):
        pair.copy_(torch.tensor([[seed, step]], dtype=torch.int64))
        # row 1: what ANOTHER user would have sent at this step under stream 4 -- the restatement's bytes
        other = np.full(G.ub, 0xAB, np.uint8)
        for i, (n, off) in enumerate(zip(sizes, G.offs)):
            sec = ru.compress(kind, vs[i], G.mode, seed, step, stream + 1)[0]
            other[off:off + sec.size] = sec
        wire[0].fill_(0xAB)
        wire[1].copy_(torch.from_numpy(other))
        out.fill_(7.0)
        mean.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        w, o, m = wire.cpu().numpy().copy(), out.cpu().numpy().copy(), mean.cpu().numpy().copy()
        seen.append(w[0])
        for i, (n, off) in enumerate(zip(sizes, G.offs)):
            got = ru.compress(kind, vs[i], G.mode, seed, step, stream)
            sec, D = got[0], got[1]
            oo = G.g.out_off[i]
            assert np.array_equal(w[0][off:off + sec.size], sec), "step %d, tensor %d: the wire" % (step, i)
            assert np.array_equal(mx.bits_of(o[oo:oo + n]), mx.bits_of(D)), "step %d, tensor %d: out" % (step, i)
            want = ru.decode_mean(kind, [sec, other[off:off + sec.size]], n, seed, step, first_stream=stream)
            assert np.array_equal(mx.bits_of(m[oo:oo + n]), mx.bits_of(want)), "step %d, tensor %d: the decode-mean" % (step, i)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])
    assert pair.cpu().tolist() == [[seed, 1]], "a launch wrote the pair"
    for t, v in zip(src, vs):
        assert np.array_equal(mx.bits_of(t.cpu().numpy()), mx.bits_of(v))
