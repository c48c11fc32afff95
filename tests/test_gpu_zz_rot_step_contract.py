"""The stepped launches of libgq_drive.so and libgq_eden.so held to SIGNS, STEPPED of their headers, bit for bit: the expected outputs
are tests/drive_contract.py's / tests/eden_contract.py's under the words tests/rot_step_contract.py gives for (seed, step); every
comparison is np.array_equal on bytes or uint32 views, through the helpers of the two existing GPU contract files (canaries round
the wire, guards round every buffer).  The inputs are finite Gaussians and Student-t values, so no block's NaNs are left to the
hardware on the compress side; the hand-built payloads of the decode-mean hold NaN, infinite and huge scales, handled as in those
files (such a block counts as one NaN pattern, which blocks those are comes from the restatement).
The descriptors carry garbage sign words: a stepped launch must not read them."""
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
import test_gpu_zz_drive_contract as tdc  # noqa: E402
import test_gpu_zz_eden_contract as tec  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
M64 = rs.M64
GARBAGE = (0xDEADBEEFDEADBEEF, 0x0123456789ABCDEF, M64, 0)
SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 8193]
DENSE = [300]
PAIRS = [(1, 0), (1, 1), (1, 2), (0, 5), (M64, 3), (1, 2 ** 62), (1, M64)]
KINDS = [("drive", "unbiased"), ("drive", "mse"), ("eden2", "unbiased"), ("eden2", "mse"), ("eden3", "unbiased"), ("eden3", "mse"),
         ("eden4", "unbiased"), ("eden4", "mse")]
IDS = ["%s-%s" % k for k in KINDS]


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _signed(w):
    return (w & M64) - (1 << 64 if w & (1 << 63) else 0)


def make_pair(seed, step):
    return torch.tensor([[_signed(seed), _signed(step)]], dtype=torch.int64).cuda()


class _SteppedBatch(object):
    """The group's descriptor with `rotation=` on every decode (the existing helpers call _batch.decode without it)."""

    def __init__(self, batch, pair):
        self._b, self._pair = batch, pair

    def decode(self, gathered, R, out, plain=False):
        return self._b.decode(gathered, R, out, plain=plain, rotation=self._pair)

    def __getattr__(self, name):
        return getattr(self._b, name)


def make(kind, mode, sizes, seed, step, dense_sizes=(), stepped=True, descriptor_signs=GARBAGE):
    """-> (helper module, group of the existing contract file).  stepped: the pair goes to both launches and the restatement runs
    under step_words(seed, step); otherwise the group is a fixed one under descriptor_signs."""
    if kind == "drive":
        T, G = tdc, tdc.make_group(sizes, mode, descriptor_signs, dense_sizes)
    else:
        T, G = tec, tec.make_group(sizes, int(kind[-1]), mode, descriptor_signs, dense_sizes)
    if stepped:
        G.pair = make_pair(seed, step)
        G.g.rotation = G.pair                      # BatchedDrive.encode hands it to the compress launch
        G.g._batch = _SteppedBatch(G.g._batch, G.pair)
        G.signs = rs.step_words(seed, step)        # what the restatement rotates by
    return T, G


def _section_bytes(kind, n):
    return dc.section_bytes(n) if kind == "drive" else ec.section_bytes(n, int(kind[-1]))


@pytest.mark.parametrize("seed,step", PAIRS)
@pytest.mark.parametrize("kind,mode", KINDS, ids=IDS)
def test_stepped_compress(kind, mode, seed, step):
    """Wire, `out`, then err and the gradient stored back under error feedback, with one identity-compressed tensor riding along."""
    T, G = make(kind, mode, SIZES, seed, step, DENSE)
    vs = [dc.student(n, 100 + n) for n in SIZES]
    dsrc = [mx.randn(n, 500 + n) for n in DENSE]
    res = T.compress(G, vs, dense_src=dsrc)
    T.check(G, res, vs)
    for (off, n), a in zip(G.dense, dsrc):
        assert np.array_equal(res.wire[off:off + 4 * n].view(np.uint32), a.view(np.uint32)), "the identity tensor's copy"
    es = [dc.gaussian(n, 800 + n) for n in SIZES]
    res = T.compress(G, vs, errs=es, s=0.5, dense_src=dsrc)
    T.check(G, res, vs, es, 0.5)
    res = T.compress(G, vs, errs=es, s=0.5, dense_src=dsrc, want_out=False)      # (the kernels without `out`)
    T.check(G, res, vs, es, 0.5, out=False)
    torch.cuda.synchronize()
    assert G.pair.cpu().tolist() == [[_signed(seed), _signed(step)]], "a launch wrote the pair"


@pytest.mark.parametrize("seed,step", [(1, 1), (M64, 3), (1, M64)])
@pytest.mark.parametrize("kind,mode", KINDS, ids=IDS)
def test_stepped_decode_mean(kind, mode, seed, step):
    """R = 1 plain, R = 1, R = 3 and R = 8 on aligned and misaligned payloads (hand-built: tests/drive_contract.payloads)."""
    sizes = [1, 255, 257, 600, dc.ITEM + 255]
    T, G = make(kind, mode, sizes, seed, step)
    if kind == "drive":
        sets = [dc.payloads(n, 8, seed=n) for n in sizes]
    else:
        sets = [ec.payloads(n, int(kind[-1]), 8, seed=n) for n in sizes]
    payloads = [[sets[i][r] for i in range(len(sizes))] for r in range(8)]
    for shift, pad, o_off in ((0, 0, 0), (3, 5, 1)):
        T.check_decode(G, T.decode(G, payloads, 1, plain=True, byte_shift=shift, stride_pad=pad, o_off=o_off), payloads, 1, plain=True)
        for R in (1, 3, 8):
            T.check_decode(G, T.decode(G, payloads, R, byte_shift=shift, stride_pad=pad, o_off=o_off), payloads, R)


@pytest.mark.parametrize("kind,mode", KINDS, ids=IDS)
def test_step_zero_is_the_fixed_launches_byte_for_byte(kind, mode):
    """The witness: in one process, the stepped launches at step 0 and the existing fixed launches under the seed's words."""
    sizes = [257, dc.ITEM + 300, 77]
    vs = [dc.student(n, 300 + n) for n in sizes]
    es = [dc.gaussian(n, 400 + n) for n in sizes]
    for seed in (1, 2, M64):
        T, Gs = make(kind, mode, sizes, seed, 0)
        _, Gf = make(kind, mode, sizes, seed, 0, stepped=False, descriptor_signs=rs.step_words(seed, 0))
        a, b = T.compress(Gs, vs, errs=es, s=0.5), T.compress(Gf, vs, errs=es, s=0.5)
        assert np.array_equal(a.wire, b.wire) and np.array_equal(mx.bits_of(a.out), mx.bits_of(b.out))
        for x, y in zip(a.src + a.err, b.src + b.err):
            assert np.array_equal(mx.bits_of(x), mx.bits_of(y))
        payloads = [[a.wire[o:o + _section_bytes(kind, n)].copy() for o, n in zip(Gs.offs, sizes)]] * 3
        for R, plain in ((1, True), (1, False), (3, False)):
            ds, df = T.decode(Gs, payloads, R, plain=plain), T.decode(Gf, payloads, R, plain=plain)
            assert np.array_equal(mx.bits_of(ds), mx.bits_of(df))


@pytest.mark.parametrize("kind,mode", KINDS, ids=IDS)
def test_one_graph_rotates_afresh_at_every_replay(kind, mode):
    """Compress, decode-mean and rng_step captured as ONE graph, replayed three times on one gradient: the wires and the outputs are
    the contract's at steps 0, 1 and 2, differ from one another, and the step word reads 3 afterwards."""
    from gq_amd import native
    sizes = [dc.ITEM + 257, 300]
    vs = [dc.student(n, 600 + n) for n in sizes]
    seed = 5
    T, G = make(kind, mode, sizes, seed, 0)
    dev, pair = G.dev, G.pair
    src = [torch.from_numpy(v).to(dev) for v in vs]
    wire = torch.full((G.ub,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats,), 7.0, device=dev)
    mean = torch.full((G.g.out_floats,), 7.0, device=dev)
    assert G.g._choose_header(src, 0, G.g.align, None, None, None, False)
    b = G.g._batch

    def launches():
        b.compress(wire, out, None, rotation=pair)
        b.decode(wire.view(1, -1), 1, mean, plain=True)      # (the proxy adds the pair)
        native.rng_step(pair)

    launches()      # (eagerly once: nothing is allocated under capture)
    torch.cuda.synchronize()
    assert pair.cpu().tolist() == [[seed, 1]]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    pair.copy_(torch.tensor([[seed, 0]], dtype=torch.int64))
    seen = []
    for step in range(3):
        wire.fill_(0xAB)
        out.fill_(7.0)
        mean.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        seen.append((wire.cpu().numpy().copy(), out.cpu().numpy().copy(), mean.cpu().numpy().copy()))
    assert pair.cpu().tolist() == [[seed, 3]]
    for step, (w, o, m) in enumerate(seen):
        signs = rs.step_words(seed, step)
        for i, (n, off) in enumerate(zip(sizes, G.offs)):
            got = dc.compress(vs[i], G.mode, signs) if kind == "drive" else ec.compress(vs[i], G.bits, G.mode, signs)
            sec, D = got[0], got[1]
            oo = G.g.out_off[i]
            assert np.array_equal(w[off:off + sec.size], sec), "replay %d, tensor %d: the wire" % (step, i)
            assert np.array_equal(mx.bits_of(o[oo:oo + n]), mx.bits_of(D)), "replay %d, tensor %d: out" % (step, i)
            assert np.array_equal(mx.bits_of(m[oo:oo + n]), mx.bits_of(D)), "replay %d, tensor %d: the decode" % (step, i)
    for a in range(3):
        for c in range(a + 1, 3):
            assert not np.array_equal(seen[a][0], seen[c][0]) and not np.array_equal(seen[a][1], seen[c][1])
    for t, v in zip(src, vs):
        assert np.array_equal(mx.bits_of(t.cpu().numpy()), mx.bits_of(v))


@pytest.mark.parametrize("kind", ["drive", "eden4"])
def test_refusals(kind):
    """A null or misaligned rotation is refused, and so is everything the fixed entry points refuse; nothing is launched."""
    from gq_amd import native
    T, G = make(kind, "unbiased", [300], 1, 0)
    L = native.drive_lib() if kind == "drive" else native.eden_lib()
    prefix = "gq_drive_" if kind == "drive" else "gq_eden_"
    last = getattr(L, prefix + "last_error")
    last.restype = ctypes.c_char_p
    comp, dec = getattr(L, prefix + "compress_batched_stepped"), getattr(L, prefix + "decode_sum_batched_stepped")
    dev = G.dev
    v = torch.zeros(300, device=dev)
    wire = torch.full((2 * G.ub + 16,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((G.g.out_floats + 4,), 7.0, device=dev)
    assert G.g._choose_header([v], 0, 4, None, None, None, False)
    b, pair = G.g._batch._b, G.pair
    P, W, O = ctypes.c_void_p(pair.data_ptr()), ctypes.c_void_p(wire.data_ptr()), ctypes.c_void_p(out.data_ptr())
    nan = ctypes.c_float(float("nan"))

    def refused(rc, text):
        assert rc < 0 and text in last().decode(), (rc, last())

    refused(comp(b.ref, None, W, nan, O, None), "rotation")
    refused(comp(b.ref, ctypes.c_void_p(pair.data_ptr() + 4), W, nan, O, None), "rotation")
    refused(dec(b.ref, None, W, ctypes.c_int64(G.ub), ctypes.c_int(1), O, ctypes.c_int(0), None), "rotation")
    refused(dec(b.ref, ctypes.c_void_p(pair.data_ptr() + 4), W, ctypes.c_int64(G.ub), ctypes.c_int(1), O, ctypes.c_int(0), None), "rotation")
    refused(comp(b.ref, P, ctypes.c_void_p(wire.data_ptr() + 4), nan, O, None), "16-byte aligned")
    refused(comp(b.ref, P, None, nan, O, None), "16-byte aligned")
    refused(comp(b.ref, P, W, nan, ctypes.c_void_p(out.data_ptr() + 2), None), "4-byte aligned")
    refused(dec(b.ref, P, W, ctypes.c_int64(G.ub), ctypes.c_int(2), O, ctypes.c_int(1), None), "plain")
    refused(dec(b.ref, P, W, ctypes.c_int64(G.ub), ctypes.c_int(0), O, ctypes.c_int(0), None), "R = 0")
    refused(dec(b.ref, P, W, ctypes.c_int64(-16), ctypes.c_int(2), O, ctypes.c_int(0), None), "stride")
    refused(dec(b.ref, P, None, ctypes.c_int64(G.ub), ctypes.c_int(1), O, ctypes.c_int(0), None), "null pointer")
    size = b.s.struct_bytes
    b.s.struct_bytes = 48
    refused(comp(b.ref, P, W, nan, O, None), "another size")
    refused(dec(b.ref, P, W, ctypes.c_int64(G.ub), ctypes.c_int(1), O, ctypes.c_int(0), None), "another size")
    b.s.struct_bytes = size
    b.s.scale_mode = 2
    refused(comp(b.ref, P, W, nan, O, None), "scale_mode")
    b.s.scale_mode = 0
    table = b.s.seg_table
    b.s.seg_table = None
    refused(comp(b.ref, P, W, nan, O, None), "null table")
    b.s.seg_table = table
    with pytest.raises(TypeError, match="rotation"):      # the binding's own check
        b.compress(wire[:G.ub], rotation=torch.zeros(2, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    assert np.all(wire.cpu().numpy() == 0xAB) and np.all(out.cpu().numpy() == 7.0), "a refused call launched something"
    b.compress(wire[:G.ub], rotation=pair)      # and the descriptor still works
    torch.cuda.synchronize()
    zero = np.zeros(300, f32)
    want = dc.compress(zero, dc.UNBIASED, G.signs)[0] if kind == "drive" else ec.compress(zero, 4, ec.UNBIASED, G.signs)[0]
    assert np.array_equal(wire[:G.ub].cpu().numpy()[:want.size], want)
