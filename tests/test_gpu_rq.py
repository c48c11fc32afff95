"""The residual compressor's two-section wire and multi-tensor path on an MI355X.  Every comparison is at tolerance 0: against the
per-tensor kernel (gq_pvq_encode's stage1 form), against torch.stack([d1, d2]).sum(0) + gq_mean_rows, against the GenericCodec
path on the same draws, against the reference's fixtures, eager against replayed."""
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
CANARY = 0xA5


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=1, ef=False, two_phase=False, scale="exp",
                num_users=1, mode="ps", cr=256, gq_rng="reference")
    base.update(kw)
    return Namespace(**base)


def _group(Ms, d, dev, users=1, **kw):
    """A BatchedResidual over tensors of Ms subvectors, canary bytes between the tensors' wire sections."""
    from gq_amd.codecs import BatchedResidual, ResidualCodec
    from gq_amd.compressors import ResidualCompressor
    codecs = []
    for M in Ms:
        n = M * d
        cd = ResidualCodec(ResidualCompressor(n, torch.Size([n]), make_args(c_dim=d, **kw)), n, torch.Size([n]))
        assert BatchedResidual.eligible(cd)
        codecs.append(cd)
    offsets, off = [], 64
    for cd in codecs:
        offsets.append(off)
        off += (cd.nbytes + 15) // 16 * 16 + 64
    wire = torch.full((users, off), CANARY, dtype=torch.uint8, device=dev)
    return BatchedResidual(codecs, offsets, list(range(len(Ms))), dev, 1, off), codecs, offsets, wire


def _canaries_intact(wire, codecs, offsets):
    w = wire.cpu().numpy()
    mask = np.ones(w.shape[1], bool)
    for cd, off in zip(codecs, offsets):
        for st, o in ((cd.s1, off), (cd.s2, off + cd.stage2_off)):
            mask[o + st.codes_off:o + st.codes_off + cd.M] = False
            mask[o + st.levels_off:o + st.levels_off + st._level_bytes] = False
            mask[o + st.lbub_off:o + st.lbub_off + 8] = False
    return bool((w[:, mask] == CANARY).all())


def _tensors(Ms, d, seed, dev, special=True):
    g = torch.Generator().manual_seed(seed)
    ts = []
    for k, M in enumerate(Ms):
        t = torch.randn(M * d, generator=g) * (10.0 ** ((k % 5) - 3))
        if special and M >= 8:
            t[:d] = 0.0                               # an all-zero subvector
            t[6 * d:7 * d] = 1e-30
        ts.append(t.to(dev))
    return ts


RAGGED = [1, 63, 64, 65, 40_000, 7, 128, 1000]


@pytest.mark.parametrize("d,kw", [(16, {}), (8, {}), (32, {}), (16, dict(n_bit=32)), (16, dict(n_bit=8)), (16, dict(random=0))],
                         ids=["d16", "d8", "d32", "d16_n32", "d16_int16", "d16_det"])
def test_stage2_encode_equals_the_per_tensor_kernel(d, kw):
    """The group's four launches against ResidualCodec's per-tensor launches (gq_hsq_encode + levels, gq_pvq_encode's stage1
    form + levels) on given draws: both sections of every tensor, byte for byte; nothing written outside the sections."""
    dev = torch.device("cuda:0")
    Ms = RAGGED if d == 16 else [1, 63, 64, 65, 5000, 7, 128]
    grp, codecs, offsets, wire = _group(Ms, d, dev, **kw)
    ts = _tensors(Ms, d, 3 + d, dev)
    torch.manual_seed(5)
    draw_off, n = {}, 0
    for i, cd in enumerate(codecs):
        draw_off[i] = n
        n += cd.draw_count()
    r_all = torch.rand(n).to(dev)
    assert grp.encode([t.clone() for t in ts], wire[0], 0, 0, draws=(r_all, draw_off))
    torch.cuda.synchronize()
    assert _canaries_intact(wire, codecs, offsets)
    for i, (cd, t) in enumerate(zip(codecs, ts)):
        single = torch.full((cd.nbytes,), CANARY, dtype=torch.uint8, device=dev)
        cd.encode_into(t.clone(), single, 0, 0, r=r_all[draw_off[i]:draw_off[i] + cd.draw_count()])
        for st, o in ((cd.s1, 0), (cd.s2, cd.stage2_off)):
            for a, b, what in zip(st._views(wire[0], offsets[i] + o), st._views(single, o), ("codes", "levels", "lb, ub")):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (i, cd.M, o, what)


def _reference_mean(codecs, offsets, wire, R):
    """torch.stack([d1, d2]).sum(0) per user from the per-stage decodes, then gq_mean_rows."""
    from gq_amd import native
    outs = []
    for cd, off in zip(codecs, offsets):
        rows = []
        for r in range(R):
            ds = []
            for st, o in ((cd.s1, off), (cd.s2, off + cd.stage2_off)):
                d = torch.empty(cd.numel, dtype=torch.float32, device=wire.device)
                st._decode(wire[r:r + 1], o, 1, d)
                ds.append(d)
            rows.append(torch.stack(ds, dim=0).sum(dim=0))
        out = torch.empty(cd.numel, dtype=torch.float32, device=wire.device)
        native.mean_rows(torch.stack(rows, 0), out)
        outs.append(out)
    return outs


@pytest.mark.parametrize("R", [1, 2, 3, 8])
@pytest.mark.parametrize("d,kw", [(16, {}), (8, {}), (32, {}), (16, dict(n_bit=32))], ids=["d16", "d8", "d32", "d16_n32"])
def test_decode_mean_equals_the_stacked_sums(R, d, kw):
    """gq_rq_decode_sum_batched over R payloads against the per-stage decodes, torch.stack([d1, d2]).sum(0) per user and
    gq_mean_rows; the per-tensor codec's one-row call too.  -0 cases: payloads are overwritten so that both stages decode an
    element to -0 (the sum must be +0), and one user's two stages cancel exactly."""
    dev = torch.device("cuda:0")
    Ms = [1, 63, 64, 65, 3000, 7, 128]
    grp, codecs, offsets, wire = _group(Ms, d, dev, users=R, **kw)
    for r in range(R):
        ts = _tensors(Ms, d, 100 + r, dev)
        draw_off, n = {}, 0
        for i, cd in enumerate(codecs):
            draw_off[i] = n
            n += cd.draw_count()
        assert grp.encode(ts, wire[r], 0, 0, draws=(torch.rand(n).to(dev), draw_off))
    # -0: tensor 3 of every payload gets all-zero norms in both stages with codes whose codeword has negative entries
    cd, off = codecs[3], offsets[3]
    for r in range(R):
        for st, o in ((cd.s1, off), (cd.s2, off + cd.stage2_off)):
            codes, levels, lb_ub = st._views(wire[r], o)
            if kw.get("n_bit") == 32:
                levels.zero_()
            else:
                levels.zero_()
                lb_ub.zero_()
    # exact cancellation: tensor 2 of payload 0 carries stage 1's payload in stage 2 with the bounds negated
    cd2, off2 = codecs[2], offsets[2]
    if kw.get("n_bit") != 32:
        c1, l1, b1 = cd2.s1._views(wire[0], off2)
        c2, l2, b2 = cd2.s2._views(wire[0], off2 + cd2.stage2_off)
        c2.copy_(c1)
        l2.copy_(l1)
        b2.copy_(-b1)
    want = _reference_mean(codecs, offsets, wire, R)
    views = grp.decode_mean(wire, R)
    torch.cuda.synchronize()
    for i, (v, w) in enumerate(zip(views, want)):
        assert torch.equal(v.view(-1).view(torch.int32), w.view(torch.int32)), (R, i)
        single = codecs[i].decode_mean(wire, offsets[i], R)
        assert torch.equal(single.view(-1).view(torch.int32), w.view(torch.int32)), (R, i, "one-row table")
    z = views[3].view(-1)
    assert bool((z == 0).all()) and not bool(torch.signbit(z).any())      # -0 + -0 from +0 is +0
    cb = codecs[3].c.compressors[0]._codebook_on(dev)
    assert bool((cb < 0).any())
    if R == 1:
        plain = grp.decode_mean(wire, 1, plain=True)
        for v, w in zip(plain, want):
            assert torch.equal(v.view(-1).view(torch.int32), w.view(torch.int32))


def _params(shapes, dev):
    return [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]


def _grads(seed, shapes, users, steps, scale=1e-2):
    g = torch.Generator().manual_seed(seed)
    return [[[torch.randn(s, generator=g) * scale for s in shapes] for _ in range(users)] for _ in range(steps)]


def generic_factory(comp, numel, shape, packed6=False):
    from gq_amd.codecs import DenseCodec, GenericCodec
    from gq_amd.compressors import IdenticalCompressor
    return DenseCodec(comp, numel, shape) if isinstance(comp, IdenticalCompressor) else GenericCodec(comp, numel, shape)


def _run(cls, shapes, grads, seed=77, factory=None, **kw):
    from gq_amd import compressors
    from gq_amd.compressors import ResidualCompressor
    dev = torch.device("cuda:0")
    params = _params(shapes, dev)
    users = len(grads[0])
    q = cls(ResidualCompressor, params, make_args(num_users=users, **kw), **({"codec_factory": factory} if factory else {}))
    torch.manual_seed(seed)
    compressors._seed_counter[0] = 0
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
          ("n32", dict(n_bit=32)), ("random0", dict(random=0))]
_MODE_CASES = [("ps", n, k) for n, k in _CASES] + [("ring", n, k) for n, k in _CASES if not k.get("two_phase")]


@pytest.mark.parametrize("mode,kw", [(m, k) for m, _, k in _MODE_CASES], ids=["%s-%s" % (m, n) for m, n, _ in _MODE_CASES])
def test_quantizers_batched_per_tensor_and_generic_agree(mode, kw):
    """gq_rng = "reference", the same draws: the multi-tensor launches, the per-tensor codec (gq_no_batch), eager launches
    (gq_graph off) and the GenericCodec path -- ResidualCompressor.compress / decompress per tensor, dense f32 on the wire, the
    path before this codec -- give the same aggregates and residuals; batched and per tensor the same wire."""
    from gq_amd.codecs import BatchedResidual
    from gq_amd.quantizers import PSQuantizer, RingQuantizer
    cls = PSQuantizer if mode == "ps" else RingQuantizer
    grads = _grads(3, BIG, 3, 3)
    a, ra, wa, qa = _run(cls, BIG, grads, mode=mode, **kw)
    b, rb, wb, qb = _run(cls, BIG, grads, mode=mode, gq_no_batch=True, **kw)
    c, rc, wc, qc = _run(cls, BIG, grads, mode=mode, gq_graph=False, **kw)
    g, rg, wg, qg = _run(cls, BIG, grads, mode=mode, factory=generic_factory, **kw)
    assert [x[0] for x in qa._groups] == [BatchedResidual] and qb._groups == [] and qg._groups == []
    for x, y in ((a, b), (a, c), (a, g)):
        for s1, s2 in zip(x, y):
            assert _same(s1, s2)
    for r2 in (rb, rc, rg):
        for r1, rr in zip(ra, r2):
            assert _same(r1, rr)
    for w1, w2 in zip(wa, wb):
        assert torch.equal(w1, w2)
    assert qa.wire_bytes_per_user() < qg.wire_bytes_per_user() // 4


import rq_fixture_util as fxu  # noqa: E402


@pytest.mark.parametrize("graph", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("no_batch", [False, True], ids=["batched", "per_tensor"])
@pytest.mark.parametrize("name", fxu.FCN_FIXTURES)
def test_reference_fixtures_through_the_real_quantizers(name, no_batch, graph):
    from gq_amd.codecs import BatchedResidual
    diffs, q = fxu.run_fixture(name, torch.device("cuda:0"), gq_no_batch=no_batch, gq_graph=graph)
    assert not diffs, diffs[:8]
    assert [g[0] for g in q._groups] == ([] if no_batch else [BatchedResidual])


def test_device_draws_replay_and_move_on():
    """gq_rng = "device": steps replay from graphs with the counter's draws -- the wire of a replayed step is the wire of the
    eager step at the same counter --, consecutive steps on the same gradients give other codes and levels, and the three
    consumers draw from different streams: stage 2's levels are not stage 1's rounding pattern."""
    from gq_amd.quantizers import PSQuantizer
    grads1 = _grads(4, BIG, 1, 1)
    steps = 6
    same = [grads1[0]] * steps
    a, _, wa, qa = _run(PSQuantizer, BIG, same, gq_rng="device")
    b, _, wb, qb = _run(PSQuantizer, BIG, same, gq_rng="device", gq_graph=False)
    assert qb.record_paths["eager"] == steps and sum(v for k, v in qa.record_paths.items() if k != "eager") >= 2, qa.record_paths
    for s in range(steps):
        assert torch.equal(wa[s], wb[s]), s
        assert _same(a[s], b[s])
    grp = qa._groups[0][2]
    for i in grp.idxs:
        cd, off = qa.codecs[i], qa.offsets[i]
        c0, l0, _ = cd.s2._views(wa[0][0], off + cd.stage2_off)
        c1, l1, _ = cd.s2._views(wa[1][0], off + cd.stage2_off)
        assert int((c0 != c1).sum()) > cd.M // 2, i
        k0 = cd.s1._views(wa[0][0], off)
        k1 = cd.s1._views(wa[1][0], off)
        assert torch.equal(k0[0], k1[0]) and not torch.equal(k0[1], k1[1])      # stage 1: the same codes, other roundings


def test_launch_counts_per_record_and_apply():
    """Four launches per record and one per apply for the group (library calls counted by native.CALLS), eager and -- the same
    calls captured -- replayed as one graph launch; error feedback adds the residual's launch, two-phase one more record's
    worth + its decode."""
    from gq_amd import native
    from gq_amd.compressors import ResidualCompressor
    from gq_amd.quantizers import PSQuantizer, RingQuantizer
    dev = torch.device("cuda:0")
    shapes = [(64, 64, 3, 3), (256, 64, 1, 1), (128, 128, 3, 3)]      # compressed tensors only: nothing but the group launches
    for cls, mode, kw, rec_calls, app_calls in ((PSQuantizer, "ps", {}, 4, 1), (PSQuantizer, "ps", dict(ef=True), 5, 1),
                                                (PSQuantizer, "ps", dict(two_phase=True), 4, 6),
                                                (RingQuantizer, "ring", {}, 5, 0), (RingQuantizer, "ring", dict(ef=True), 6, 0)):
        params = _params(shapes, dev)
        q = cls(ResidualCompressor, params, make_args(mode=mode, gq_graph=False, num_users=2, **kw))
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
    # replayed: a step of one user, gq_rng = "device".  Its first, eager run makes these calls -- 4 for the record, the decode-mean
    # and the step of the draws' words for the apply (the group's decode takes no tail along) --, and the graph that replays
    # it holds those launches and nothing else
    params = _params(shapes, dev)
    q = PSQuantizer(ResidualCompressor, params, make_args(gq_rng="device"))
    grads = [torch.randn(p.shape, device=dev) * 1e-2 for p in params]
    for step in range(12):
        for p, g in zip(params, grads):
            p.grad = g.detach()
        before = native.CALLS[0]
        q.record(0, 1)
        mid = native.CALLS[0]
        q.apply()
        if step == 0:
            assert (mid - before, native.CALLS[0] - mid) == (4, 2), (mid - before, native.CALLS[0] - mid)
    torch.cuda.synchronize()
    paths = q.record_paths
    assert paths["eager"] <= 3 and paths["whole_step"] + paths["whole_step_any_address"] >= 3, paths      # (12 steps: 3 eager, 4 as record graphs, then whole steps)
    plans = [e[1] for e in q._step_graphs.values() if e[1] is not None]
    assert plans
    for plan in plans:
        if isinstance(plan, native.LaunchPlan):
            assert plan.nodes == 6, plan.nodes      # 4 per record + 1 per apply + the aggregate's step / reset launch


def test_driver_quantizer_rq_trains():
    import json
    import math
    root = os.path.dirname(HERE)
    cmd = [sys.executable, os.path.join(root, "train.py"), "--quantizer", "rq", "--network", "fcn", "--dataset", "mnist", "--c-dim", "16",
           "--k-bit", "8", "--n-bit", "6", "--num-users", "2", "--epochs", "1", "--train-size", "1024", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]


@pytest.mark.parametrize("mode,ef", [("ps", True), ("ring", False)])
def test_two_ranks_on_one_gpu_equal_single_process(tmp_path, mode, ef):
    """Two ranks (two local users each) exchange the wire over gloo on cuda:0; == four users in one process, bit for bit."""
    script = os.path.join(HERE, "_dist_worker_rq.py")
    out = str(tmp_path / "res")
    port = 35300 + (os.getpid() % 1500) + (0 if mode == "ps" else 5) + (11 if ef else 0)
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
    import _dist_worker_rq as w
    single = w.run_single_process(4, mode, ef)
    assert sorted(single) == sorted(r0.files)
    for k in single:
        assert np.array_equal(single[k].view(np.uint32), r0[k].view(np.uint32)), k
