"""The probabilistic vector compressor's multi-tensor path on an MI355X.  Every comparison is at tolerance 0: against the
per-tensor kernel (gq_pvq_encode), against the per-tensor codecs (gq_no_batch), eager against replayed."""
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
FCN_SHAPES = [(256, 784), (256,), (10, 256), (10,)]
CANARY = 0xA5


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=1, ef=False, two_phase=False, scale="exp",
                num_users=1, mode="ps", cr=256, gq_rng="reference")
    base.update(kw)
    return Namespace(**base)


def _group(Ms, d, K, dev, n_bit=6, random=1, rng="reference"):
    """A BatchedPVQ over tensors of Ms subvectors with canary bytes between the wire sections -> (group, codecs, offsets, wire)."""
    from gq_amd.codecs import BatchedPVQ, PVQCodec
    from gq_amd.compressors import ProbabilisticVectorCompressor
    from gq_amd.codebook import load_codebook
    full = load_codebook(d, 256)
    codecs = []
    for M in Ms:
        n = M * d
        c = ProbabilisticVectorCompressor(n, torch.Size([n]), make_args(c_dim=d, k_bit=8, n_bit=n_bit, random=random, gq_rng=rng))
        if K != 256:      # a codebook of K rows: the first K codewords and their own pseudo-inverse
            cw = np.ascontiguousarray(full[:K])
            c.K, c.codewords = K, torch.from_numpy(cw)
            c.c_dagger = torch.from_numpy(np.ascontiguousarray(np.linalg.pinv(cw.T).astype(np.float32)))
        cd = PVQCodec(c, n, torch.Size([n]))
        assert BatchedPVQ.eligible(cd)
        codecs.append(cd)
    offsets, off = [], 64
    for cd in codecs:
        offsets.append(off)
        off += (cd.nbytes + 15) // 16 * 16 + 64      # 64 canary bytes behind every tensor's sections
    wire = torch.full((1, off), CANARY, dtype=torch.uint8, device=dev)
    grp = BatchedPVQ(codecs, offsets, list(range(len(Ms))), dev, 1, off)
    return grp, codecs, offsets, wire


def _canaries_intact(wire, codecs, offsets):
    w = wire[0].cpu().numpy()
    mask = np.ones(w.size, bool)
    for cd, off in zip(codecs, offsets):
        cb = 1
        mask[off + cd.codes_off:off + cd.codes_off + cd.M * cb] = False
        mask[off + cd.levels_off:off + cd.levels_off + cd._level_bytes] = False
        mask[off + cd.lbub_off:off + cd.lbub_off + 8] = False
    return bool((w[mask] == CANARY).all())


def _tensors(Ms, d, seed, dev, special=True):
    g = torch.Generator().manual_seed(seed)
    ts = []
    for k, M in enumerate(Ms):
        t = torch.randn(M * d, generator=g) * (10.0 ** ((k % 5) - 3))
        if special and M >= 8:
            t[:d] = 0.0                               # an all-zero subvector
            t[3 * d + 1] = float("nan")
            t[5 * d + 2] = float("inf")
            t[6 * d:7 * d] = 1e-30                    # quotients outside the fast walk's range
        ts.append(t.to(dev))
    return ts


RAGGED = [1, 63, 64, 65, 150_000, 7, 128, 1000]      # 150,000 subvectors of 16 floats = 2.4 M elements between small tensors


def _check_against_flat(Ms, d, K, seed, n_bit=6, ef_scale=None):
    """One multi-tensor encode + level launch over tensors of Ms subvectors against the flat kernel (gq_pvq_encode) and the
    flat level launch per tensor, given the same draws: codes, u, (lb, ub), levels and the canaries round the wire sections.
    ef_scale: through gq_pvq_encode_batched's error-feedback form, every third tensor without an error buffer; the flat
    kernel is fed g + e * s as two separately rounded torch operations, which is also what the launch must leave over the
    gradients that have an error buffer (the others stay as they are)."""
    from gq_amd import native
    dev = torch.device("cuda:0")
    grp, codecs, offsets, wire = _group(Ms, d, K, dev, n_bit=n_bit)
    ts = _tensors(Ms, d, seed, dev)
    total = sum(2 * M for M in Ms)
    torch.manual_seed(seed)
    r_all = torch.rand(total).to(dev)
    draw_off, n = {}, 0
    for i, M in enumerate(Ms):
        draw_off[i] = n
        n += 2 * M
    if ef_scale is None:
        assert grp.encode([t.clone() for t in ts], wire[0], 0, 0, draws=(r_all, draw_off))
    else:
        s_dev = torch.tensor(ef_scale, dtype=torch.float32, device=dev)
        nothing = torch.empty(0, dtype=torch.float32, device=dev)
        assert nothing.data_ptr() == 0
        errs = [nothing if i % 3 == 2 else e for i, e in enumerate(_tensors(Ms, d, seed + 1, dev, special=False))]
        before = [t.clone() for t in ts]
        grads = [t.clone() for t in ts]
        ts = [g if e is nothing else g + e * s_dev for g, e in zip(before, errs)]      # the product rounded, then the sum
        assert grp._upload(grads, 0, grp.align, errs)
        grp._batch.encode(wire[0], ef_scale, native.RANDOM_GIVEN, 0, grp._given_draws((r_all, draw_off), 0))
        grp._batch.levels(wire[0], native.RANDOM_GIVEN, 0, grp._given_draws((r_all, draw_off), 1))
        for i, (g, v, g0, e) in enumerate(zip(grads, ts, before, errs)):
            assert torch.equal(g.view(torch.int32), (g0 if e is nothing else v).view(torch.int32)), (i, Ms[i], "the gradient afterwards")
    torch.cuda.synchronize()
    assert _canaries_intact(wire, codecs, offsets)
    for i, (cd, t) in enumerate(zip(codecs, ts)):
        M = cd.M
        _, cdag = cd.c._on(dev)
        codes = torch.empty(M, dtype=torch.uint8, device=dev)
        u = torch.empty(M, dtype=torch.float32, device=dev)
        ws = native.new_workspace(dev, M)
        o = draw_off[i]
        native.pvq_encode(t, cdag, codes, u, ws, native.RANDOM_GIVEN, r_all[o:o + M].contiguous(), 0)
        lb_ub = torch.empty(2, dtype=torch.float32, device=dev)
        levels = torch.empty(M, dtype=torch.uint8, device=dev)
        native.hsq_levels(u, n_bit, native.RANDOM_GIVEN, r_all[o + M:o + 2 * M].contiguous(), 0, ws, lb_ub, levels)
        wc, wl, wb = cd._views(wire[0], offsets[i])
        first = int(grp._layout[i, 2]) * 64
        assert torch.equal(wc, codes), (i, M, "codes")
        assert int(codes.max()) < K
        assert torch.equal(grp.u_flat[first:first + M].view(torch.int32), u.view(torch.int32)), (i, M, "u")
        assert torch.equal(wb.view(torch.int32), lb_ub.view(torch.int32)), (i, M, "lb, ub")
        assert torch.equal(wl, levels), (i, M, "levels")


@pytest.mark.parametrize("d,K", [(16, 256), (8, 256), (32, 256), (16, 32), (16, 64), (8, 64), (32, 64)])
def test_multi_tensor_encode_equals_the_flat_kernel(d, K):
    Ms = RAGGED if d == 16 else [1, 63, 64, 65, 5000, 7, 128]
    _check_against_flat(Ms, d, K, 11 + d + K)


def _run_list(d, which):
    """tests/rq_contract.py's multi-tile list (five large tensors, 300 small ones of 1 ... 200 subvectors between them) sized
    from the device's CU count: more tiles than twice the waves the launch can have resident, so every wave's run holds two
    tiles or more and runs cross tensors; the second total is no multiple of the waves, so some waves run one tile more."""
    import rq_contract as rc
    from gq_amd import native
    cus = native.device_info(0)[0]
    total = rc.multi_tile_totals(d, cus)[which]
    Ms = rc.multi_tile_Ms(d, cus, total)
    assert sum((M + 63) // 64 for M in Ms) == total > rc.encode_wave_bound(d, cus)
    assert which == 0 or (total + 1) % (4 * cus) == 0
    return Ms


@pytest.mark.parametrize("which", [0, 1], ids=["above_the_bound", "one_short_of_twice_the_bound"])
@pytest.mark.parametrize("d,K", [(8, 64), (16, 256), (32, 64)])
def test_encode_runs_that_cross_tensors(d, K, which):
    """The run walker under gq_pvq_encode_batched: the wave's run of tiles, the prefetch across a tile's encode, the fold of
    (min, max) where the tensor changes inside a run, waves_with_one_more -- every tensor against the flat kernel."""
    _check_against_flat(_run_list(d, which), d, K, 200 + d + which)


@pytest.mark.parametrize("which", [0, 1], ids=["above_the_bound", "one_short_of_twice_the_bound"])
@pytest.mark.parametrize("d,K", [(8, 64), (16, 256), (32, 64)])
def test_encode_runs_with_error_feedback(d, K, which):
    """The same lists through the error-feedback form (d = 16: the instantiation built for two waves per SIMD), every third
    tensor without an error buffer: v = g + e * s is encoded and left over the gradient, the other gradients are untouched."""
    _check_against_flat(_run_list(d, which), d, K, 300 + d + which, ef_scale=0.3)


def test_misaligned_counter_address_is_refused():
    """GQ_RANDOM_DEVICE_COUNTER with an address that is not 8-byte aligned: GQ_ERR_INVALID_ARG, and nothing is launched --
    wire, u_flat and seg_minmax stay as they were."""
    from gq_amd import native
    dev = torch.device("cuda:0")
    Ms = [65, 700, 7]
    grp, codecs, offsets, wire = _group(Ms, 16, 256, dev, rng="device")
    assert grp._upload(_tensors(Ms, 16, 3, dev), 0, grp.align)
    grp.u_flat.fill_(7.0)
    words = torch.tensor([0x1234ABCD5678EF01, 5, 0], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    minmax = grp._dev[grp._table_words:grp._dense_at]
    was = (wire.clone(), grp.u_flat.clone(), minmax.clone())
    assert words.data_ptr() % 8 == 0
    with pytest.raises(native.GQNativeError):
        grp._batch.encode(wire[0], None, native.RANDOM_DEVICE_COUNTER, words.data_ptr() + 4)
    torch.cuda.synchronize()
    assert torch.equal(wire, was[0]) and torch.equal(grp.u_flat.view(torch.int32), was[1].view(torch.int32)) and torch.equal(minmax, was[2])
    grp._batch.encode(wire[0], None, native.RANDOM_DEVICE_COUNTER, words.data_ptr())      # the same rig is served when asked properly
    torch.cuda.synchronize()
    assert not torch.equal(wire, was[0]) and _canaries_intact(wire, codecs, offsets)


@pytest.mark.parametrize("eps", ["1e-3", "-1e-3"], ids=["wave_walk", "term_by_term"])
def test_walks_behind_the_fast_path(eps):
    """$GQ_PVQ_EPS widened: most lanes leave the lane-local walk (as tests/test_gpu_kernels.py does for the flat kernel).  The
    libraries read it once, so the comparison runs in a child process."""
    env = dict(os.environ, GQ_PVQ_EPS=eps)
    pkg = os.path.join(os.path.dirname(HERE), "gradient-quantization_amd")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_pvq as t; t._check_against_flat([1, 63, 64, 65, 3000, 7], 16, 256, 5); "
            "t._check_against_flat([65, 700], 8, 64, 6); t._check_against_flat([65, 700], 32, 256, 7); print('ok')" % (HERE, pkg))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(HERE))
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def _params(shapes, dev):
    return [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]


def _grads(seed, shapes, users, steps, scale=1e-2):
    g = torch.Generator().manual_seed(seed)
    return [[[torch.randn(s, generator=g) * scale for s in shapes] for _ in range(users)] for _ in range(steps)]


def _run(cls, shapes, grads, seed=77, factory=None, **kw):
    from gq_amd.compressors import ProbabilisticVectorCompressor
    dev = torch.device("cuda:0")
    params = _params(shapes, dev)
    users = len(grads[0])
    q = cls(ProbabilisticVectorCompressor, params, make_args(num_users=users, **kw), **({"codec_factory": factory} if factory else {}))
    torch.manual_seed(seed)
    from gq_amd import compressors
    compressors._seed_counter[0] = 0      # (the per-call seeds count calls process-wide: two runs compared draw for draw start alike)
    outs, wires = [], []
    for step in grads:
        for u, gs in enumerate(step):
            for p, g in zip(params, gs):
                p.grad = g.to(dev).clone()
            q.record(u, 1)
        torch.cuda.synchronize()
        wires.append(q._wire[:users].clone())
        q.apply()
        outs.append([p.grad.detach().clone() for p in params])
    res = [[e.clone() for e in p.error] for p in params] if kw.get("ef") else []
    return outs, res, wires, q


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


BIG = [(64, 64, 3, 3), (64,), (256, 64, 1, 1), (128, 128, 3, 3), (10, 512), (512, 256, 1, 1), (10,), (2048,)]


_CASES = [("plain", dict()), ("ef", dict(ef=True)), ("twophase", dict(two_phase=True)), ("ef_twophase", dict(ef=True, two_phase=True)),
          ("n32", dict(n_bit=32)), ("random0", dict(random=0)), ("packed6", dict(gq_wire_levels="packed6", n_bit=5))]
# (the ring has no second phase: ring_quantizer.py)
_MODE_CASES = [("ps", n, k) for n, k in _CASES] + [("ring", n, k) for n, k in _CASES if not k.get("two_phase")]


@pytest.mark.parametrize("mode,kw", [(m, k) for m, _, k in _MODE_CASES], ids=["%s-%s" % (m, n) for m, n, _ in _MODE_CASES])
def test_quantizers_batched_equal_per_tensor(mode, kw):
    """gq_rng = "reference": the multi-tensor launches (error feedback fused into them) against the per-tensor codecs with the
    unfused axpy / decode / subtract sequence -- aggregate, residuals and wires identical, graphs on and off."""
    from gq_amd.codecs import BatchedPVQ
    from gq_amd.quantizers import PSQuantizer, RingQuantizer
    cls = PSQuantizer if mode == "ps" else RingQuantizer
    grads = _grads(3, BIG, 3, 3)
    a, ra, wa, qa = _run(cls, BIG, grads, mode=mode, **kw)
    b, rb, wb, qb = _run(cls, BIG, grads, mode=mode, gq_no_batch=True, **kw)
    c, rc, wc, qc = _run(cls, BIG, grads, mode=mode, gq_graph=False, **kw)
    assert [g[0] for g in qa._groups] == [BatchedPVQ] and qb._groups == []
    for x, y in ((a, b), (a, c)):
        for s1, s2 in zip(x, y):
            assert _same(s1, s2)
    for r1, r2 in zip(ra, rb):
        assert _same(r1, r2)
    for w1, w2 in zip(wa, wb):
        assert torch.equal(w1, w2)


def test_resnet50_list_batched_equals_per_tensor():
    import json
    from gq_amd.quantizers import PSQuantizer
    with open(os.path.join(HERE, "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    grads = _grads(9, shapes, 2, 1)
    a, _, wa, qa = _run(PSQuantizer, shapes, grads)
    b, _, wb, _ = _run(PSQuantizer, shapes, grads, gq_no_batch=True)
    assert _same(a[0], b[0]) and torch.equal(wa[0], wb[0])
    assert len(qa._groups) == 1 and len(qa._groups[0][1]) == 76


def _oracle_l1_and_projection(orc, cd, grad, codes):
    """The oracle's sequential-f32 l1 of every subvector and its f32 projection on the chosen codeword (gq_oracle_pvq_encode's
    own sub-results: l1 and p do not depend on the draw)."""
    g = grad.detach().cpu().numpy().reshape(-1)
    _, _, l1, p, _ = orc.pvq_encode(g, cd.c.c_dagger.cpu().numpy(), np.zeros(cd.M, np.float32), sub_rows=cd.M)
    l1 = np.asarray(l1, np.float32).reshape(-1)
    p = np.asarray(p, np.float32).reshape(cd.M, -1)
    return l1, p[np.arange(cd.M), codes.astype(np.int64)]


def test_device_draws_replay_and_move_on(oracle):
    """gq_rng = "device": a step replays from the graph with the counter's draws -- the wire of the replayed step is the wire of
    the eager step at the same counter --, two consecutive steps on the same gradients give different codes, and for EVERY
    tensor of the group: every code below K, |u| EQUAL to the oracle's l1 of the subvector, sign(u) equal to the sign of the
    oracle's projection on the chosen codeword (u = sign(p) * l1 exactly: no tolerance, no subvector left out)."""
    from gq_amd.quantizers import PSQuantizer
    grads1 = _grads(4, BIG, 1, 1)
    steps = 6
    same = [grads1[0]] * steps
    a, _, wa, qa = _run(PSQuantizer, BIG, same, gq_rng="device")
    b, _, wb, qb = _run(PSQuantizer, BIG, same, gq_rng="device", gq_graph=False)
    assert qb.record_paths["eager"] == steps and sum(v for k, v in qa.record_paths.items() if k != "eager") >= 2, qa.record_paths
    for s in range(steps):
        assert torch.equal(wa[s], wb[s]), s      # same seeds (torch.manual_seed), same counters: replayed == eager
        assert _same(a[s], b[s])
    grp = qa._groups[0][2]
    for s_idx, i in enumerate(grp.idxs):
        cd, off = qa.codecs[i], qa.offsets[i]
        c0 = cd._views(wa[0][0], off)[0]
        c1 = cd._views(wa[1][0], off)[0]
        assert int((c0 != c1).sum()) > cd.M // 2, i
        codes = cd._views(wa[-1][0], off)[0].cpu().numpy()
        assert int(codes.max()) < 256
        first = int(grp._layout[s_idx, 2]) * 64
        u = grp.u_flat[first:first + cd.M].cpu().numpy()
        l1, sel = _oracle_l1_and_projection(oracle, cd, grads1[0][0][i], codes)
        want = (np.sign(sel) * l1).astype(np.float32)
        assert np.array_equal(u.view(np.uint32), want.view(np.uint32)), (i, int((u.view(np.uint32) != want.view(np.uint32)).sum()))


def _uniform01_host(seed, idx):
    """uniform01 of csrc/gq_common.hpp, recomputed on the host (uint32 arithmetic)."""
    M32 = 0xFFFFFFFF
    out = np.empty(len(idx), np.float32)
    for n, i in enumerate(idx):
        h = (i + (seed & M32) * 0x9E3779B1) & M32
        h ^= h >> 16
        h = (h * 0x7FEB352D) & M32
        h ^= h >> 15
        h = (h * 0x846CA68B) & M32
        h ^= h >> 16
        h = (h + (((seed >> 32) & M32) ^ (((i >> 32) * 0x85EBCA77) & M32))) & M32
        h = (h * 0xC2B2AE3D) & M32
        h ^= h >> 15
        out[n] = np.float32(h >> 8) * np.float32(2.0 ** -24)
    return out


PVQ_STREAM_SALT = 0xA0761D6478BD642F      # PW_SAMPLER_SALT of csrc/pvq_walk.hpp


def _resolved_counter_seed(seed, step):
    """resolve_seed of csrc/gq_common.hpp: the launch's seed from the { seed, step } words."""
    M64 = (1 << 64) - 1
    z = (step + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (seed ^ z ^ (z >> 31)) & M64


def _keyed_seed(seed, a_bits, b_bits):
    M64 = (1 << 64) - 1
    k = ((a_bits << 32) | b_bits) & M64
    return (seed ^ ((k * 0x9E3779B97F4A7C15) & M64) ^ (k >> 29)) & M64


@pytest.mark.parametrize("mode", ["device", "counter", "keyed"])
def test_sampler_and_levels_draw_from_different_streams(mode, oracle):
    """Both launches are given the SAME seed argument.  The sampler must have used uniform01(seed ^ salt, slot) -- keyed mode: of
    the seed keyed by the subvector's l1 -- and not the level launch's uniform01(seed, slot): with the sampler's uniforms
    recomputed on the host the oracle's encode reproduces the kernel's codes exactly, and with the level launch's uniforms it
    does not.  The levels, in turn, are the oracle's for the unsalted stream (device and counter mode; the keyed level stream
    is keyed by (lb, ub) and is checked to differ from the sampler's draws)."""
    from gq_amd import native
    dev = torch.device("cuda:0")
    M = 4096
    grp, codecs, offsets, wire = _group([M, 640], 16, 256, dev, rng="keyed" if mode == "keyed" else "device")
    ts = _tensors([M, 640], 16, 1, dev, special=False)
    assert grp._upload(ts, 0, grp.align)
    seed = 0x1234ABCD5678EF01
    if mode == "counter":
        words = torch.tensor([[seed, 5]], dtype=torch.int64, device=dev)
        arg_mode, arg_seed, eff = native.RANDOM_DEVICE_COUNTER, words.data_ptr(), _resolved_counter_seed(seed, 5)
    elif mode == "keyed":
        arg_mode, arg_seed, eff = native.RANDOM_DEVICE_KEYED, seed, seed
    else:
        arg_mode, arg_seed, eff = native.RANDOM_DEVICE, seed, seed
    grp._batch.encode(wire[0], None, arg_mode, arg_seed)
    grp._batch.levels(wire[0], arg_mode, arg_seed)
    torch.cuda.synchronize()
    for s_idx, (cd, t) in enumerate(zip(codecs, ts)):
        first = int(grp._layout[s_idx, 2]) * 64
        idx = list(range(first, first + cd.M))
        g = t.cpu().numpy()
        cdag = cd.c.c_dagger.cpu().numpy()
        codes, levels, lb_ub = [v.cpu().numpy() for v in cd._views(wire[0], offsets[s_idx])]
        if mode == "keyed":
            _, _, l1, _, _ = oracle.pvq_encode(g, cdag, np.zeros(cd.M, np.float32), sub_rows=cd.M)
            lb = np.asarray(l1, np.float32).reshape(-1).view(np.uint32)
            r_samp = np.concatenate([_uniform01_host(_keyed_seed(eff ^ PVQ_STREAM_SALT, int(b), int(b)), [i]) for b, i in zip(lb, idx)])
            bb = lb_ub.view(np.uint32)
            r_lvl = _uniform01_host(_keyed_seed(eff, int(bb[0]), int(bb[1])), idx)
        else:
            r_samp = _uniform01_host(eff ^ PVQ_STREAM_SALT, idx)
            r_lvl = _uniform01_host(eff, idx)
        assert not np.array_equal(r_samp, r_lvl)
        want_codes, want_u = oracle.pvq_encode(g, cdag, r_samp)
        assert np.array_equal(codes.astype(np.int32), want_codes.astype(np.int32)), (mode, s_idx, "the sampler's stream")
        wrong_codes, _ = oracle.pvq_encode(g, cdag, r_lvl)
        assert int((wrong_codes.astype(np.int32) != codes.astype(np.int32)).sum()) > cd.M // 2, "the sampler drew from the level launch's stream"
        lb, ub, want_levels = oracle.scalar_levels(want_u, 6, 1, r_lvl)
        assert np.array_equal(lb_ub.view(np.uint32), np.array([lb, ub], np.float32).view(np.uint32))
        assert np.array_equal(levels.astype(np.int32), want_levels), (mode, s_idx, "the level launch's stream")
    assert _canaries_intact(wire, codecs, offsets)


def test_training_iterations_replay_from_the_address_free_graph():
    """driver.FCN trained with `--quantizer pvq`'s class, gradients at new addresses every step: after the first eager steps the
    records replay from graphs, the address-free form among them; the loss stays finite."""
    from gq_amd import driver
    from gq_amd.quantizers import PSQuantizer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = driver.FCN().to(dev)
    args = make_args(gq_rng="device")
    q = PSQuantizer(driver.quantizer_choices["pvq"], model.parameters(), args)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    x = torch.randn(32, 784, device=dev)
    y = torch.randint(0, 10, (32,), device=dev)
    hold = []
    for it in range(12):
        opt.zero_grad(set_to_none=True)
        hold.append(torch.empty(1 + 4096 * it, device=dev))      # (kept alive: the next gradients land elsewhere)
        loss = torch.nn.functional.cross_entropy(model(x), y)
        loss.backward()
        q.record(0, 1)
        q.apply()
        opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    p = q.record_paths
    replayed = p["graph"] + p["whole_step"] + p["graph_any_address"] + p["whole_step_any_address"]
    assert p["eager"] <= 3 and replayed >= 9, p
    assert p["graph_any_address"] + p["whole_step_any_address"] >= 1, p


import pvq_fixture_util as fxu  # noqa: E402


@pytest.mark.parametrize("graph", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("no_batch", [False, True], ids=["batched", "per_tensor"])
@pytest.mark.parametrize("name", fxu.FCN_FIXTURES + [fxu.RESNET_FIXTURE])
def test_reference_fixtures_through_the_real_quantizers(name, no_batch, graph):
    """Every pvqpsq_* / pvqring_* / pvqpsqd_* fixture (the reference's own quantizers over its own class, CPU draws) through
    PSQuantizer / RingQuantizer on the kernels with gq_rng = "reference": codes, levels, (lb, ub) of every user, every aggregate,
    the residuals -- identical."""
    from gq_amd.codecs import BatchedPVQ
    diffs, q = fxu.run_fixture(name, torch.device("cuda:0"), gq_no_batch=no_batch, gq_graph=graph)
    assert not diffs, diffs[:8]
    assert [g[0] for g in q._groups] == ([] if no_batch else [BatchedPVQ])


def test_launch_counts_per_record_and_apply():
    """One encode + one level launch per record and one decode-mean per apply for the group (library calls counted by
    native.CALLS), in ps and ring mode, with and without error feedback; two-phase adds one encode + levels + decode."""
    from gq_amd import native
    from gq_amd.quantizers import PSQuantizer, RingQuantizer
    dev = torch.device("cuda:0")
    shapes = [(64, 64, 3, 3), (256, 64, 1, 1), (128, 128, 3, 3)]      # compressed tensors only: nothing but the group launches
    for cls, mode, kw, rec_calls, app_calls in ((PSQuantizer, "ps", {}, 2, 1), (PSQuantizer, "ps", dict(ef=True), 2, 1),
                                                (PSQuantizer, "ps", dict(two_phase=True), 2, 4),
                                                (PSQuantizer, "ps", dict(ef=True, two_phase=True), 2, 4),
                                                (RingQuantizer, "ring", {}, 3, 0), (RingQuantizer, "ring", dict(ef=True), 3, 0)):
        params = _params(shapes, dev)
        q = cls(fxu_compressor(), params, make_args(mode=mode, gq_graph=False, num_users=2, **kw))
        torch.manual_seed(1)
        for step in range(2):
            for u in range(2):
                for p in params:
                    p.grad = torch.randn(p.shape, device=dev) * 1e-2
                before = native.CALLS[0]
                q.record(u, 1)
                assert native.CALLS[0] - before == rec_calls, (mode, kw, "record", native.CALLS[0] - before)
            before = native.CALLS[0]
            q.apply()
            assert native.CALLS[0] - before == app_calls, (mode, kw, "apply", native.CALLS[0] - before)


def fxu_compressor():
    from gq_amd.compressors import ProbabilisticVectorCompressor
    return ProbabilisticVectorCompressor


def test_train_py_quantizer_pvq_trains():
    import json
    import math
    root = os.path.dirname(HERE)
    cmd = [sys.executable, os.path.join(root, "train.py"), "--quantizer", "pvq", "--network", "fcn", "--dataset", "mnist", "--c-dim", "16",
           "--k-bit", "8", "--n-bit", "6", "--num-users", "2", "--epochs", "1", "--train-size", "1024", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]


@pytest.mark.parametrize("mode,ef", [("ps", True), ("ring", False)])
def test_two_ranks_on_one_gpu_equal_single_process(tmp_path, mode, ef):
    """Two ranks (two local users each) exchange the wire over gloo on cuda:0; == four users in one process, bit for bit."""
    script = os.path.join(HERE, "_dist_worker_pvq.py")
    out = str(tmp_path / "res")
    port = 33300 + (os.getpid() % 1500) + (0 if mode == "ps" else 5) + (11 if ef else 0)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    procs = [subprocess.Popen([sys.executable, script, str(r), "2", out, mode, "1" if ef else "0"], env=env) for r in range(2)]
    try:
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    for k in r0.files:
        assert np.array_equal(r0[k].view(np.uint32), r1[k].view(np.uint32)), "ranks disagree on " + k
    import _dist_worker_pvq as w
    single = w.run_single_process(4, mode, ef)
    assert sorted(single) == sorted(r0.files)
    for k in single:
        assert np.array_equal(single[k].view(np.uint32), r0[k].view(np.uint32)), k
