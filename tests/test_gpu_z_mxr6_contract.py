"""The two 6-bit formats through libgq_mxr.so, bit for bit: tests/mxr_contract.py's rotation composed with tests/mx6_contract.py
(compress_rotated / decode_mean_rotated), and -- in the same process -- the plain launch of libgq_mx.so on the contract's rotated
tensor as witness: it writes the identical wire.  The harness is tests/test_gpu_mx_contract.py's.
(The name sorts behind every other GPU test file: tests/test_gpu_z_mx6_api.py says why.)"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx6_contract as m6  # noqa: E402
import mxr_contract as mxr  # noqa: E402
import test_gpu_mx_contract as base  # noqa: E402  (the harness: compress, decode, _split)

pytestmark = pytest.mark.gpu

f32 = np.float32
FMTS = list(m6.FP6)
ITEM = m6.ITEM
SEED = 0x1234567887654321
# the sizes of tests/test_gpu_z_mx6_contract.py (one and two blocks, an odd number of blocks, the step seam, the item seam, two
# items + 1), then mxr_contract.SIZES' own (around the rotation block and three items)
SIZES = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, ITEM - 1, ITEM, ITEM + 1, 2 * ITEM + 1] + [n for n in mxr.SIZES if n not in (1, 4095, 4096, 4097)]


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def make_group(sizes, fmt, signs=mxr.SEEDED, random=True, rng="device", rotated=True):
    from gq_amd.codecs import BatchedMX, BatchedMXR, MXCodec, MXRCodec
    dev = torch.device("cuda:0")
    comp = SimpleNamespace(format=m6.NAMES[fmt], random=random, _rng=rng, rotate_signs=signs)
    codec, group = (MXRCodec, BatchedMXR) if rotated else (MXCodec, BatchedMX)
    codecs = [codec(comp, n, torch.Size([n])) for n in sizes]
    assert [cd.nbytes for cd in codecs] == [m6.section_bytes(n, fmt) for n in sizes]
    offs, dense, ub = m6.layout(sizes, fmt)
    g = group(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=None)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return SimpleNamespace(g=g, codecs=codecs, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), fmt=fmt, first=first, signs=signs)


def check(G, res, vs, rs=None, errs=None, s=None, nonfinite=False):
    """Every tensor's section (every byte), dense decode, gradient and residual against the restatement -> the contract's x'."""
    xps = []
    for i, v in enumerate(vs):
        n, off, oo = G.sizes[i], G.offs[i], G.g.out_off[i]
        e = errs[i] if errs is not None else None
        sec, D, w, ne, xp = m6.compress_rotated(v, G.fmt, G.signs, rs[i] if rs is not None else None, e, s)
        xps.append(xp)
        assert np.array_equal(res.wire[off:off + sec.size], sec), "tensor %d (n = %d): the section" % (i, n)
        assert m6.same(res.out[oo:oo + n], D, nonfinite), "tensor %d (n = %d): the compress's dense decode" % (i, n)
        end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
        assert np.all(res.out[oo + n:end] == 7.0), "a write behind tensor %d's decode" % i
        if e is not None:
            assert m6.same(res.src[i], w, nonfinite), "tensor %d: g <- w" % i
            assert m6.same(res.err[i], ne, nonfinite), "tensor %d: err <- w - D" % i
        else:
            assert m6.same(res.src[i], v), "tensor %d: the source changed without error feedback" % i
    assert np.all(res.wire[G.offs[-1] + m6.section_bytes(G.sizes[-1], G.fmt):] == 0xAB)
    return xps


def witness(G, res, xps, r=None, seed=None):
    """gq_mx_compress_batched, in this process, on the contract's x' with the same draws writes the identical wire."""
    P = make_group(G.sizes, G.fmt, random=G.g.random, rotated=False)
    if getattr(G.g, "rng_pairs", None) is not None:
        P.g.rng_pairs = G.g.rng_pairs
    plain = base.compress(P, xps, r=r, seed=seed)
    assert np.array_equal(plain.wire, res.wire), "the plain MX launch on x' writes another wire"


@pytest.mark.parametrize("mode", ["off", "given", "device", "counter"])
@pytest.mark.parametrize("fmt", FMTS)
def test_sizes(fmt, mode):
    sizes = SIZES
    vs = [mxr.gradients(n, 100 + n) for n in sizes]
    G = make_group(sizes, fmt, random=mode != "off")
    r = seed = rs = None
    if mode == "given":
        r = np.random.RandomState(7).rand(sum(sizes)).astype(f32)
        rs = base._split(r, sizes)
    elif mode == "device":
        seed = SEED
        rs = [m6.draws(m6.DEVICE, n, int(fd), seed) for n, fd in zip(sizes, G.first)]
    elif mode == "counter":
        G.g.rng_pairs = torch.tensor([[SEED, 41], [0, 0]], dtype=torch.int64, device=G.dev)
        rs = [m6.draws(m6.COUNTER, n, int(fd), SEED, 41) for n, fd in zip(sizes, G.first)]
    res = base.compress(G, vs, r=r, seed=seed)
    xps = check(G, res, vs, rs)
    witness(G, res, xps, r=r, seed=seed)


@pytest.mark.parametrize("fmt", FMTS)
def test_error_feedback_and_misaligned_views(fmt):
    sizes = [ITEM + 261, 300, 65]
    vs = [mxr.gradients(n, 200 + n) for n in sizes]
    es = [mxr.gradients(n, 300 + n) for n in sizes]
    G = make_group(sizes, fmt)
    r = np.random.RandomState(8).rand(sum(sizes)).astype(f32)
    for v_offs, e_offs, o_off in (([0, 0, 0], [0, 0, 0], 0), ([1, 2, 0], [3, 1, 1], 1)):
        res = base.compress(G, vs, r=r, errs=es, s=0.5, v_offs=v_offs, e_offs=e_offs, o_off=o_off)
        check(G, res, vs, base._split(r, sizes), es, 0.5)


@pytest.mark.parametrize("fmt", FMTS)
def test_nonfinite_values(fmt):
    w, at = mxr.edge_nonfinite()
    G = make_group([w.size], fmt, random=False)
    res = base.compress(G, [w])
    check(G, res, [w], nonfinite=True)
    for name in ("finite_a", "finite_b"):
        assert np.all(np.isfinite(res.out[at[name]:at[name] + 256]))


def payloads(n, fmt, R, seed):
    """mxr_contract.payloads over the 64 codes: scale bytes 110 ... 140, payload 0 with scale byte 0xFF in its last MX block and
    (two rotation blocks or more) in the last MX block of the second rotation block."""
    rs = np.random.RandomState(seed)
    nb = -(-n // 32)
    secs = []
    for r in range(R):
        code = rs.randint(0, 64, nb * 32)
        code[:64] = np.arange(64)[:nb * 32]
        sb = rs.randint(110, 141, nb).astype(np.uint8)
        if r == 0:
            sb[-1] = 255
            if n >= 2 * mxr.RBLOCK:
                sb[15] = 255
        secs.append(m6.pack(sb, code, fmt))
    return secs


DEC_SIZES = [1, 65, 255, 257, 600, ITEM + 255, 2 * ITEM]


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_mean_then_one_inverse_rotation(fmt):
    """R = 1 (plain and not) and 8 -- plus 2 and 3 -- on aligned and misaligned `gathered`: the mean first, then ONE inverse
    rotation."""
    G = make_group(DEC_SIZES, fmt)
    sets = [payloads(n, fmt, 8, seed=n) for n in DEC_SIZES]
    pl = [[sets[i][r] for i in range(len(DEC_SIZES))] for r in range(8)]

    def check_decode(out, R, plain=False):
        for i, n in enumerate(G.sizes):
            want = m6.decode_mean_rotated([pl[r][i] for r in range(R)], n, fmt, G.signs, plain)
            oo = G.g.out_off[i]
            assert m6.same(out[oo:oo + n], want, nan_as_one=True), "tensor %d (n = %d), R = %d" % (i, n, R)
            end = G.g.out_off[i + 1] if i + 1 < len(G.sizes) else G.g.out_floats
            assert np.all(out[oo + n:end] == 7.0)

    for R in (1, 2, 3, 8):
        for shift, pad, o_off in ((0, 0, 0), (4, 0, 1), (3, 5, 0)):
            check_decode(base.decode(G, pl, R, byte_shift=shift, stride_pad=pad, o_off=o_off), R)
    for shift in (0, 3):
        check_decode(base.decode(G, pl, 1, plain=True, byte_shift=shift), 1, plain=True)


@pytest.mark.parametrize("fmt", FMTS)
def test_plain_decode_equals_the_compress_launchs_own_decode(fmt):
    sizes = [ITEM + 300, 77]
    vs = [mxr.gradients(n, 900 + n) for n in sizes]
    G = make_group(sizes, fmt, random=False)
    res = base.compress(G, vs)
    pl = [[res.wire[o:o + m6.section_bytes(n, fmt)].copy() for o, n in zip(G.offs, sizes)]]
    assert np.array_equal(m6.bits_of(base.decode(G, pl, 1, plain=True)), m6.bits_of(res.out))


def test_refusals():
    import ctypes
    from gq_amd import native
    L = native.mxr_lib()
    L.gq_mxr_last_error.restype = ctypes.c_char_p
    G = make_group([300], m6.FP6_E3M2, random=False)
    v = torch.zeros(300, device=G.dev)
    wire = torch.full((G.ub,), 0xAB, dtype=torch.uint8, device=G.dev)
    out = torch.full((G.g.out_floats,), 7.0, device=G.dev)
    assert G.g._choose_header([v], 0, 4, None, None, None, False)
    b = G.g._batch
    fmt = b.s.format
    assert fmt == 0x32
    for bad in (2, 0x22, 6):
        b.s.format = bad
        for call in (lambda: b.compress(wire, native.RANDOM_OFF), lambda: b.decode(wire.view(1, -1), 1, out)):
            with pytest.raises(native.GQNativeError):
                call()
            assert "format" in L.gq_mxr_last_error().decode()
    b.s.format = fmt
    torch.cuda.synchronize()
    assert np.all(wire.cpu().numpy() == 0xAB) and np.all(out.cpu().numpy() == 7.0), "a refused call launched something"
