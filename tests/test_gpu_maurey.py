"""Maurey sparsification on the MI355X (libgq_maurey.so): the wire bytes against a CPU restatement of the contract
(include/gq_maurey.h; numpy, f64 / longdouble), the decode-mean's arithmetic, the multi-tensor table, error feedback, determinism,
graph replay through PSQuantizer, and one statistic of unbiasedness.  Every kernel test hands the draws in (GQ_RANDOM_GIVEN)."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = 16
SIGN = np.uint32(1 << 31)


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="1.0",
                num_users=1, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


class _K(object):
    def __init__(self, k):
        self.k = k


def _up(x, a=16):
    return (x + a - 1) // a * a


# ---- the contract restated on the CPU ----------------------------------------------------------------------------------
def ref_draws(w, u):
    """(index of every draw, C, T, t): the smallest i with t < C_i, C the running sum of |w| in longdouble."""
    C = np.cumsum(np.abs(w.astype(np.float32)).astype(np.longdouble))
    T = C[-1]
    t = u.astype(np.longdouble) * T
    return np.searchsorted(C, t, side="right"), C, T, t


def ref_words(w, idx):
    idx = np.sort(idx).astype(np.int64)
    return idx.astype(np.uint32) | np.where(w[idx] < 0, SIGN, np.uint32(0))


def ref_section(w, u, k):
    """The section's bytes: header (scale, 12 zero bytes), the sorted words, zero padding."""
    idx, C, T, t = ref_draws(w, u)
    sec = np.zeros((HEADER + _up(4 * k)) // 4, np.uint32)
    sec[0] = (np.float32(T) / np.float32(k)).view(np.uint32)
    sec[4:4 + k] = ref_words(w, idx)
    return sec.view(np.uint8)


def ref_dense(words, scale, n):
    """D = scale * (float)(+-m): one rounding per element, +0 where nothing was drawn."""
    idx = (words & ~SIGN).astype(np.int64)
    m = np.zeros(n, np.float32)
    np.add.at(m, idx, np.where(words & SIGN, np.float32(-1), np.float32(1)))
    d = np.float32(scale) * m
    d[m == 0] = np.float32(0)
    return d


def exact_case(n, k, seed):
    """Integers in [-8, 8], a tenth zero, the last element so that T = 2^p; u = (m + 0.5) / 2^p: every partial sum and every t is
    exact in f32 and f64 whatever the order of additions, and no t ties a boundary."""
    rs = np.random.RandomState(seed)
    v = rs.randint(-8, 9, size=n).astype(np.float32)
    v[rs.rand(n) < 0.1] = 0
    others = int(np.abs(v[:-1]).sum())
    p = 0
    while (1 << p) <= others:
        p += 1
    v[-1] = np.float32(((1 << p) - others) * (1 if rs.rand() < 0.5 else -1))
    u = ((rs.randint(0, 1 << p, size=k) + 0.5) / float(1 << p)).astype(np.float32)
    assert p <= 19 and float(np.abs(v.astype(np.float64)).sum()) == float(1 << p) and u.max() < 1
    assert np.array_equal(u.astype(np.float64) * (1 << p) - 0.5, np.floor(u.astype(np.float64) * (1 << p)))
    return v, u


def encode(v, u, k, out=False, seed=None):
    """One tensor through MaureyCodec -> (wire bytes, dense decode or None); the wire starts as 0xAB: every byte must be written."""
    from gq_amd.codecs import MaureyCodec
    dev = torch.device("cuda:0")
    n = v.size
    cd = MaureyCodec(_K(k), n, torch.Size([n]))
    wire = torch.full((cd.nbytes,), 0xAB, dtype=torch.uint8, device=dev)
    g = torch.from_numpy(v).to(dev)
    r = torch.from_numpy(u).to(dev) if u is not None else None
    dec = None
    if out:
        dec = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
        cd.encode_decode_into(g, wire, 0, 0, dec, r=r, seed=seed)
        dec = dec.cpu().numpy()
    else:
        cd.encode_into(g, wire, 0, 0, r=r, seed=seed)
    torch.cuda.synchronize()
    assert np.array_equal(g.cpu().numpy().view(np.uint32), v.view(np.uint32)), "the source changed without error feedback"
    return cd, wire, dec


def words_of(wire_np, k):
    return wire_np[HEADER:HEADER + 4 * k].view(np.uint32)


EXACT = [(1, 3), (17, 5), (4096, 124), (4097, 124), (20000, 600), (70001, 2000)]


@pytest.mark.parametrize("case", range(len(EXACT)), ids=["%dx%d" % nk for nk in EXACT])
def test_exact_inputs_byte_for_byte(case):
    n, k = EXACT[case]
    v, u = exact_case(n, k, case)
    idx, C, T, t = ref_draws(v, u)
    assert np.all(v[idx] != 0), "the restatement drew an element of weight zero"
    cd, wire, dec = encode(v, u, k, out=True)
    got = wire.cpu().numpy()
    want = ref_section(v, u, k)
    assert got.size == want.size == 16 + _up(4 * k)
    assert np.array_equal(got[:HEADER], want[:HEADER]), "header"
    assert np.array_equal(words_of(got, k), words_of(want, k)), "words"
    assert np.array_equal(got, want), "padding"
    d = ref_dense(words_of(want, k), want[:4].view(np.float32)[0], n)
    assert np.array_equal(dec.view(np.uint32), d.view(np.uint32)), "the compress's dense decode"


def test_one_dominant_element_takes_every_draw():
    n, k = 20000, 2000
    v = np.zeros(n, np.float32)
    v[5000] = -3
    u = np.random.RandomState(3).rand(k).astype(np.float32)
    cd, wire, dec = encode(v, u, k, out=True)
    got = wire.cpu().numpy()
    assert np.array_equal(words_of(got, k), np.full(k, 5000 | (1 << 31), np.uint32))
    assert np.array_equal(got, ref_section(v, u, k))
    want = np.zeros(n, np.float32)
    want[5000] = -3
    assert np.array_equal(dec.view(np.uint32), want.view(np.uint32))
    out = torch.empty(n, dtype=torch.float32, device=wire.device)
    cd.decode_wire(wire, 0, out)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_degenerate_tensors():
    """T == 0 or not finite: every draw is index 0 with a plus sign, scale as computed, +0 wherever nothing was drawn."""
    n, k = 5000, 124
    u = np.random.RandomState(4).rand(k).astype(np.float32)
    zeros = np.zeros(n, np.float32)
    zeros[1::3] = np.float32(-0.0)
    cd, wire, dec = encode(zeros, u, k, out=True)
    got = wire.cpu().numpy()
    assert np.array_equal(got, np.zeros(got.size, np.uint8))      # scale 0, words 0, padding
    assert np.array_equal(dec.view(np.uint32), np.zeros(n, np.uint32))
    out = torch.full((n,), 7.0, dtype=torch.float32, device=wire.device)
    cd.decode_wire(wire, 0, out)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.zeros(n, np.uint32))
    v = np.random.RandomState(5).standard_normal(n).astype(np.float32)
    v[7] = np.inf
    cd, wire, dec = encode(v, u, k, out=True)
    got = wire.cpu().numpy()
    assert np.array_equal(words_of(got, k), np.zeros(k, np.uint32))
    assert not np.isfinite(got[:4].view(np.float32)[0]) and not got[4:HEADER].any() and not got[HEADER + 4 * k:].any()
    for d in (dec, cd.decode_mean(wire.view(1, -1), 0, 1, plain=True).cpu().numpy()):
        assert not np.isfinite(d[0]) and np.array_equal(d[1:].view(np.uint32), np.zeros(n - 1, np.uint32))


GAUSS = [(4097, 124, 11), (20000, 600, 12), (70001, 2000, 13)]


@pytest.mark.parametrize("n,k,seed", GAUSS, ids=["%dx%d" % (n, k) for n, k, _ in GAUSS])
def test_gaussian_inputs_against_longdouble(n, k, seed):
    """Every word equals the longdouble searchsorted answer.  A draw within 1e-10 * T of a CDF boundary would be excused (50x the
    worst-case f64 summation error n * 2^-53 * T ~ 2e-12 * T); none is for these seeds (the nearest lies 4.1e-9 * T away), so
    nothing is hidden.  scale: within 2 ulp (f32) of the longdouble T / k -- one rounding of T, one of the division."""
    rs = np.random.RandomState(seed)
    v = (rs.standard_normal(n) * 1e-3).astype(np.float32)
    u = rs.rand(k).astype(np.float32)
    idx, C, T, t = ref_draws(v, u)
    below = np.where(idx > 0, C[np.maximum(idx - 1, 0)], np.longdouble(0))
    dist = np.minimum(C[idx] - t, t - below)
    excused = dist < np.longdouble(1e-10) * T
    print("n = %d: nearest draw %.3g * T from a boundary, %d excused" % (n, float(dist.min() / T), int(excused.sum())))
    assert int(excused.sum()) == 0
    cd, wire, dec = encode(v, u, k, out=True)
    got = wire.cpu().numpy()
    assert np.array_equal(words_of(got, k), ref_words(v, idx))
    assert not got[4:HEADER].any() and not got[HEADER + 4 * k:].any()
    scale = got[:4].view(np.float32)[0]
    exact = T / np.longdouble(k)
    ulp = np.spacing(np.float32(exact))
    print("scale %r, longdouble T / k %r, %.3g ulp apart" % (scale, float(exact), float(abs(np.longdouble(scale) - exact) / ulp)))
    assert abs(np.longdouble(scale) - exact) <= 2 * np.longdouble(ulp)
    assert np.array_equal(dec.view(np.uint32), ref_dense(words_of(got, k), scale, n).view(np.uint32))


def test_decode_plain_and_mean_of_three():
    """R = 1 plain against scale * bincount in f32; R = 3 with different draws against (+0 + D_0 + D_1 + D_2) / 3 in f32."""
    n, k = 20000, 600
    rs = np.random.RandomState(21)
    v = rs.randint(-8, 9, size=n).astype(np.float32) * np.float32(0.37)
    v[:40] *= 400      # heavy elements: many duplicates, both signs
    rows, dense = [], []
    for r in range(3):
        u = rs.rand(k).astype(np.float32)
        cd, wire, _ = encode(v, u, k)
        rows.append(wire)
        w = wire.cpu().numpy()
        words = words_of(w, k)
        assert np.array_equal(words, ref_words(v, ref_draws(v, u)[0]))
        assert len(np.unique(words)) < k - 20 and (words & SIGN).any() and not (words & SIGN).all()
        dense.append(ref_dense(words, w[:4].view(np.float32)[0], n))
    plain = cd.decode_mean(rows[0].view(1, -1), 0, 1, plain=True).cpu().numpy()
    assert np.array_equal(plain.view(np.uint32), dense[0].view(np.uint32))
    gathered = torch.stack(rows)
    got = cd.decode_mean(gathered, 0, 3).cpu().numpy()
    want = (((np.zeros(n, np.float32) + dense[0]) + dense[1]) + dense[2]) / np.float32(3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    one = cd.decode_mean(rows[1].view(1, -1), 0, 1).cpu().numpy()      # the aggregate of one payload: (+0 + D) / 1
    assert np.array_equal(one.view(np.uint32), (np.zeros(n, np.float32) + dense[1]).view(np.uint32))


def _group(sizes, ks, dense_sizes, dev):
    """A BatchedMaurey over tensors of `sizes`, its wire laid out as the quantizer lays it out (dense tensors behind)."""
    from gq_amd.codecs import BatchedMaurey, MaureyCodec
    codecs = [MaureyCodec(_K(k), n, torch.Size([n])) for n, k in zip(sizes, ks)]
    offs, off = [], 0
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes)
    dense = []
    for n in dense_sizes:
        dense.append((off, n))
        off += 4 * n
    user_bytes = _up(off)
    return BatchedMaurey(codecs, offs, list(range(len(codecs))), dev, 1, user_bytes, dense=dense or None), codecs, offs, dense, user_bytes


def test_multi_tensor_sections_equal_the_one_tensor_codec():
    dev = torch.device("cuda:0")
    sizes, ks = [1001, 17, 4097, 20000, 1], [27, 5, 124, 600, 3]
    rs = np.random.RandomState(31)
    vs = [(rs.standard_normal(n) * 1e-2).astype(np.float32) for n in sizes]
    us = [rs.rand(k).astype(np.float32) for k in ks]
    small = [rs.standard_normal(n).astype(np.float32) for n in (10, 257)]
    g, codecs, offs, dense, ub = _group(sizes, ks, [10, 257], dev)
    assert [int(x) for x in g._layout[:, 6]] == [0, 27, 32, 156, 756] and g.ndraws == 759
    r_all = torch.from_numpy(np.concatenate(us)).to(dev)
    starts = np.concatenate([[0], np.cumsum(ks)[:-1]])
    draws = (r_all, {i: int(s) for i, s in enumerate(starts)})
    wire = torch.full((ub,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((g.out_floats,), 7.0, dtype=torch.float32, device=dev)
    ts = [torch.from_numpy(v).to(dev) for v in vs]
    ds = [torch.from_numpy(a).to(dev) for a in small]
    assert g.encode(ts, wire, 0, 0, draws=draws, dense=ds, out=out)
    torch.cuda.synchronize()
    w = wire.cpu().numpy()
    for v, u, k, cd, off, oo in zip(vs, us, ks, codecs, offs, g.out_off):
        _, single, dec = encode(v, u, k, out=True)
        assert np.array_equal(w[off:off + cd.nbytes], single.cpu().numpy()), "section of the %d-element tensor" % v.size
        assert np.array_equal(out.cpu().numpy()[oo:oo + v.size].view(np.uint32), dec.view(np.uint32))
    for a, (off, n) in zip(small, dense):
        assert np.array_equal(w[off:off + 4 * n].view(np.uint32), a.view(np.uint32)), "an identity-compressed tensor"
    views = g.decode_mean(wire.view(1, -1), 1, plain=True)
    for vw, oo, v in zip(views, g.out_off, vs):
        assert np.array_equal(vw.cpu().numpy().view(np.uint32), out.cpu().numpy()[oo:oo + v.size].view(np.uint32))


def test_error_feedback_in_the_launches():
    """The source becomes w = v + s * err (the product rounded, then the sum), the residual w - D, out the decode of the wire."""
    dev = torch.device("cuda:0")
    sizes, ks, s = [4097, 20000], [124, 600], np.float32(0.75)
    rs = np.random.RandomState(41)
    vs = [(rs.standard_normal(n) * 1e-2).astype(np.float32) for n in sizes]
    es = [(rs.standard_normal(n) * 1e-2).astype(np.float32) for n in sizes]
    us = [rs.rand(k).astype(np.float32) for k in ks]
    g, codecs, offs, _, ub = _group(sizes, ks, [], dev)
    draws = (torch.from_numpy(np.concatenate(us)).to(dev), {0: 0, 1: ks[0]})
    ts = [torch.from_numpy(v).to(dev) for v in vs]
    errs = [torch.from_numpy(e).to(dev) for e in es]
    wire = torch.zeros(ub, dtype=torch.uint8, device=dev)
    out = torch.full((g.out_floats,), 7.0, dtype=torch.float32, device=dev)
    assert g.encode(ts, wire, 0, 0, errs=errs, ef_scale=float(s), draws=draws, out=out)
    torch.cuda.synchronize()
    views = g.decode_mean(wire.view(1, -1), 1, plain=True)
    for v, e, u, k, t, er, cd, off, oo, vw in zip(vs, es, us, ks, ts, errs, codecs, offs, g.out_off, views):
        w = v + s * e
        assert np.array_equal(t.cpu().numpy().view(np.uint32), w.view(np.uint32)), "the source is not v + s * err"
        words = words_of(wire.cpu().numpy()[off:off + cd.nbytes], k)
        assert np.array_equal(words, ref_words(w, ref_draws(w, u)[0]))
        d = out.cpu().numpy()[oo:oo + v.size]
        assert np.array_equal(d.view(np.uint32), vw.cpu().numpy().view(np.uint32)), "out is not the decode of the wire"
        assert np.array_equal(er.cpu().numpy().view(np.uint32), (w - d).view(np.uint32)), "the residual is not w - D"


def test_same_compress_same_bytes():
    n, k = 70001, 2000
    rs = np.random.RandomState(51)
    v = (rs.standard_normal(n) * 1e-3).astype(np.float32)
    u = rs.rand(k).astype(np.float32)
    a, b = encode(v, u, k)[1].cpu(), encode(v, u, k)[1].cpu()
    assert torch.equal(a, b)
    a, b, c = (encode(v, None, k, seed=s)[1].cpu() for s in (1234, 1234, 1235))      # the device generator, a fixed seed
    assert torch.equal(a, b) and not torch.equal(a, c)
    words = words_of(a.numpy(), k)
    assert np.array_equal(words & ~SIGN, np.sort(words & ~SIGN)) and (words & ~SIGN).max() < n


def _counting_seeds():
    n = [0]

    def source():
        n[0] += 1
        return (n[0] * 0x9E3779B97F4A7C15 + 12345) & (2 ** 63 - 1)
    return source


def _run_quantizer(graph, steps=7):
    from gq_amd import driver
    from gq_amd.compressors import shared_seeds
    from gq_amd.quantizers import PSQuantizer
    dev = torch.device("cuda:0")
    shapes = [(256, 784), (256,), (10, 256), (10,), (300, 300)]      # driver.FCN's tensors and one more
    rs = np.random.RandomState(61)
    grads = [[torch.from_numpy((rs.standard_normal(s) * 1e-2).astype(np.float32)).to(dev) for s in shapes] for _ in range(2)]
    params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
    wires, aggs = [], []
    with shared_seeds(_counting_seeds()):
        q = PSQuantizer(driver.quantizer_choices["maurey"], params, make_args(gq_rng="device", num_users=2, gq_graph=graph))
        for step in range(steps):
            for user in range(2):
                for p, gr in zip(params, grads[user]):
                    p.grad = gr.clone()      # (apply() rebinds p.grad.data to the aggregate)
                q.record(user, 0)
            torch.cuda.synchronize()
            wires.append(q._wire.cpu().clone())
            q.apply()
            torch.cuda.synchronize()
            aggs.append([p.grad.detach().cpu().clone() for p in params])
    return q, wires, aggs


def test_quantizer_replays_from_graphs_and_draws_afresh():
    from gq_amd.codecs import BatchedMaurey
    q, wires, aggs = _run_quantizer(True)
    assert [g[0] for g in q._groups] == [BatchedMaurey] and q._groups[0][2].graphable()
    p = q.record_paths
    assert p["eager"] >= 1 and sum(p.values()) - p["eager"] >= 6, p      # (the last three steps' six records at the least)
    q2, wires2, aggs2 = _run_quantizer(False)
    assert q2.record_paths["eager"] == sum(q2.record_paths.values())
    for step, (w, w2, a, a2) in enumerate(zip(wires, wires2, aggs, aggs2)):
        assert torch.equal(w, w2), "step %d: the replayed wire differs from the eager one" % step
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, a2)), "step %d" % step
    assert not torch.equal(wires[-1], wires[-2]) and not torch.equal(wires[-2], wires[-3])      # the counter advances: fresh draws per replay
    assert not torch.equal(wires[-1][0], wires[-1][1])      # and the two users draw from their own pairs
    # the aggregate is the mean of the two payloads' decodes
    k0 = q.codecs[0].k
    w = wires[-1].numpy()
    dense = [ref_dense(words_of(w[u], k0), w[u][:4].view(np.float32)[0], 256 * 784) for u in range(2)]
    want = ((np.zeros(256 * 784, np.float32) + dense[0]) + dense[1]) / np.float32(2)
    assert np.array_equal(aggs[-1][0].numpy().reshape(-1).view(np.uint32), want.view(np.uint32))


def test_mean_decode_is_unbiased():
    """n = 4097, k = 124, 512 device-mode compresses with seeds 0 ... 511: |mean decode - v| stays within 6 standard errors,
    T * sqrt(p (1 - p) / (124 * 512)) with p = |v| / T, at every coordinate.  The magnitudes lie in [0.5, 1.5] * 1e-3 (every
    coordinate is drawn ~8 to ~23 times over the run, so the normal bound means something) and a quarter of the coordinates are
    zero: those have p = 0 and must decode to exactly 0."""
    from gq_amd.codecs import MaureyCodec
    dev = torch.device("cuda:0")
    n, k, runs = 4097, 124, 512
    rs = np.random.RandomState(71)
    v = ((0.5 + rs.rand(n)) * 1e-3 * np.where(rs.rand(n) < 0.5, -1, 1)).astype(np.float32)
    v[rs.rand(n) < 0.25] = 0
    cd = MaureyCodec(_K(k), n, torch.Size([n]))
    g = torch.from_numpy(v).to(dev)
    wire = torch.empty(cd.nbytes, dtype=torch.uint8, device=dev)
    dec = torch.empty(n, dtype=torch.float32, device=dev)
    acc = torch.zeros(n, dtype=torch.float64, device=dev)
    for seed in range(runs):
        cd.encode_decode_into(g, wire, 0, 0, dec, seed=seed)
        acc += dec
    mu = (acc / runs).cpu().numpy()
    T = np.abs(v.astype(np.float64)).sum()
    p = np.abs(v.astype(np.float64)) / T
    se = T * np.sqrt(p * (1 - p) / (k * runs))
    z = np.abs(mu - v.astype(np.float64)) / np.where(se > 0, se, 1)
    print("worst coordinate: %.2f standard errors; zero-weight coordinates drawn: %d" % (z[se > 0].max(), int((mu[se == 0] != 0).sum())))
    assert np.all(mu[se == 0] == 0)
    assert np.all(np.abs(mu - v.astype(np.float64)) <= 6 * se)


def test_compressor_signature_on_a_device_tensor():
    """MaureySparsification.compress of a CUDA float32 tensor: [scale, codes int64[k] ascending, signs f32[k]] read back from the
    wire; decompress is the reference's scale * (sum of signs per index)."""
    from gq_amd.compressors import MaureySparsification
    n = 70001
    c = MaureySparsification(n, torch.Size([n]), make_args(gq_rng="device"))
    v = torch.from_numpy((np.random.RandomState(81).standard_normal(n) * 1e-3).astype(np.float32)).cuda()
    scale, codes, signs = c.compress(v)
    assert codes.dtype == torch.int64 and codes.shape == (c.k,) and signs.dtype == torch.float32 and signs.shape == (c.k,)
    assert scale.dim() == 0 and scale.dtype == torch.float32
    assert bool((codes[1:] >= codes[:-1]).all()) and int(codes.max()) < n
    assert torch.equal(signs, torch.sign(v[codes]))
    exact = float(v.double().abs().sum()) / c.k
    assert abs(float(scale) - exact) <= 2 * float(np.spacing(np.float32(exact)))
    dec = c.decompress([scale, codes, signs])
    want = torch.zeros(n, device="cuda").index_add_(0, codes, signs) * scale
    assert dec.shape == (n,) and torch.equal(dec, want)
