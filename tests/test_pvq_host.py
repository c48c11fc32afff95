"""The probabilistic vector compressor on the HSQ wire, host side (no GPU): codec routing, wire size, grouping, the draw plan,
the library's ABI, the driver's switch, and the parameter-server host logic on the CPU oracle."""
import ctypes
import json
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)

FCN_SHAPES = [(256, 784), (256,), (10, 256), (10,)]


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=1, ef=False, two_phase=False, scale="exp",
                num_users=1, mode="ps", cr=256, gq_rng="reference")
    base.update(kw)
    return Namespace(**base)


def _params(shapes):
    return [torch.nn.Parameter(torch.zeros(s)) for s in shapes]


def _resnet50_shapes():
    with open(os.path.join(GOLDEN, "resnet50_cifar_shapes.json")) as f:
        return json.load(f)["parameter_shapes"]


def test_factory_gives_the_pvq_codec():
    from gq_amd.codecs import BatchedHSQ, BatchedPVQ, GenericCodec, HSQCodec, PVQCodec, default_codec_factory
    from gq_amd.compressors import NearestNeighborCompressor, ProbabilisticVectorCompressor, ResidualCompressor
    n = 4096
    cd = default_codec_factory(ProbabilisticVectorCompressor(n, torch.Size([n]), make_args()), n, torch.Size([n]))
    assert type(cd) is PVQCodec and BatchedPVQ.eligible(cd) and not BatchedHSQ.eligible(cd)
    hs = default_codec_factory(NearestNeighborCompressor(n, torch.Size([n]), make_args()), n, torch.Size([n]))
    assert type(hs) is HSQCodec and not BatchedPVQ.eligible(hs)
    assert cd.nbytes == hs.nbytes and (cd.codes_off, cd.levels_off, cd.lbub_off) == (hs.codes_off, hs.levels_off, hs.lbub_off)
    assert BatchedPVQ.group_key(cd) != BatchedHSQ.group_key(hs)
    # out of scope here: the two-stage compressor keeps its path
    rs = default_codec_factory(ResidualCompressor(n, torch.Size([n]), make_args()), n, torch.Size([n]))
    assert type(rs) is GenericCodec


def test_resnet50_wire_is_the_hsq_wire_and_one_group():
    from gq_amd.codecs import BatchedPVQ, PVQCodec
    from gq_amd.compressors import NearestNeighborCompressor, ProbabilisticVectorCompressor
    from gq_amd.quantizers import PSQuantizer
    shapes = _resnet50_shapes()
    for s in shapes + [list(s) for s in FCN_SHAPES]:
        n = int(np.prod(s))
        assert n <= 1000 or n % 16 == 0      # neither class alters the sub-dimension of these models
    qp = PSQuantizer(ProbabilisticVectorCompressor, _params(shapes), make_args())
    qh = PSQuantizer(NearestNeighborCompressor, _params(shapes), make_args())
    assert qp.wire_bytes_per_user() == qh.wire_bytes_per_user()
    assert qp.wire_bytes_per_user() < 94_083_376 // 10      # the decoded dense f32 of the generic path
    assert qp.offsets == qh.offsets
    pv = [i for i, c in enumerate(qp.codecs) if type(c) is PVQCodec]
    assert len(pv) == 76
    assert [g[0] for g in qp._groups] == [BatchedPVQ] and sorted(qp._groups[0][1]) == pv
    qn = PSQuantizer(ProbabilisticVectorCompressor, _params(shapes), make_args(gq_no_batch=True))
    assert qn._groups == []


def test_other_shapes_stay_out_of_the_group():
    from gq_amd.codecs import BatchedPVQ, PVQCodec, default_codec_factory
    from gq_amd.compressors import ProbabilisticVectorCompressor
    np.random.seed(0)
    for kw, want in ((dict(c_dim=16, k_bit=8), True), (dict(c_dim=8, k_bit=8), True), (dict(c_dim=32, k_bit=8), True),
                     (dict(c_dim=16, k_bit=4), False),      # K == d: a random orthogonal codebook per tensor
                     (dict(c_dim=12, k_bit=8), False), (dict(c_dim=24, k_bit=8), False)):
        n = 96 * 64
        cd = default_codec_factory(ProbabilisticVectorCompressor(n, torch.Size([n]), make_args(**kw)), n, torch.Size([n]))
        assert type(cd) is PVQCodec and BatchedPVQ.eligible(cd) is want, kw


def test_draw_plan_two_slices_in_the_reference_order():
    from gq_amd.compressors import ProbabilisticVectorCompressor
    from gq_amd.quantizers import PSQuantizer
    q = PSQuantizer(ProbabilisticVectorCompressor, _params(FCN_SHAPES), make_args())
    Ms = [256 * 784 // 16, 10 * 256 // 16]
    assert q._draw_off == {0: 0, 2: 2 * Ms[0]} and q._draw_total == 2 * sum(Ms)
    assert q.codecs[0].draw_count() == 2 * Ms[0]
    # without stochastic levels, and with f32 norms, only the sampler draws
    for kw in (dict(random=0), dict(n_bit=32)):
        q1 = PSQuantizer(ProbabilisticVectorCompressor, _params(FCN_SHAPES), make_args(**kw))
        assert q1._draw_off == {0: 0, 2: Ms[0]} and q1._draw_total == sum(Ms), kw
    # gq_rng = "device": no host draws at all
    assert PSQuantizer(ProbabilisticVectorCompressor, _params(FCN_SHAPES), make_args(gq_rng="device"))._draw_total == 0
    # ONE torch.rand(total) is the reference's separate calls, per tensor: codewords (:52), then levels (prob_scalar:23)
    for sizes in ([12544, 12544, 160, 160], [108, 108, 7, 7], [12544, 160]):
        torch.manual_seed(1234)
        parts = torch.cat([torch.rand(m) for m in sizes])
        torch.manual_seed(1234)
        assert torch.equal(torch.rand(sum(sizes)), parts), sizes


def test_pvq_library_abi_and_driver_switch():
    from gq_amd import driver, native
    from gq_amd.compressors import ProbabilisticVectorCompressor
    L = native.pvq_lib()
    assert L.gq_pvq_abi_version() == native.PVQ_ABI_VERSION == 1
    for d, K, cb, want in ((16, 256, 1, 1), (8, 32, 1, 1), (32, 64, 1, 1), (12, 256, 1, 0), (16, 16, 1, 0), (16, 512, 4, 0), (16, 48, 1, 0),
                           (64, 256, 1, 0)):
        assert L.gq_pvq_batched_serves(d, K, cb) == want
        assert native.pvq_batched_serves(d, K, torch.uint8 if cb == 1 else torch.int32) is bool(want)
    assert ctypes.sizeof(native._PVQBatchStruct) == 24
    assert native.lib().gq_abi_version() == 5      # libgq_hsq.so is as it was
    assert driver.quantizer_choices["pvq"] is ProbabilisticVectorCompressor
    assert driver.build_parser().parse_args(["--quantizer", "pvq"]).quantizer == "pvq"


def _fcn_grads(seed, users, steps):
    g = torch.Generator().manual_seed(seed)
    return [[[torch.randn(s, generator=g) * 1e-2 for s in FCN_SHAPES] for _ in range(users)] for _ in range(steps)]


def _run_cpu(cls, grads, users, one_call, **kw):
    """PSQuantizer on the oracle codec.  one_call: the quantizer's draw plan; else every codec draws for itself, per tensor and
    in parameter order, as the reference's compressors do."""
    from oracle_codec_pvq import oracle_pvq_codec_factory
    from gq_amd.compressors import ProbabilisticVectorCompressor
    params = _params(FCN_SHAPES)
    q = cls(ProbabilisticVectorCompressor, params, make_args(num_users=users, no_cuda=True, **kw), codec_factory=oracle_pvq_codec_factory)
    if not one_call:
        q._draws = lambda device: None
        q._draw_total = 0
    torch.manual_seed(77)
    outs = []
    for step in grads:
        for u, gs in enumerate(step):
            for p, g in zip(params, gs):
                p.grad = g.clone()
            q.record(u, 1)
        q.apply()
        outs.append([p.grad.detach().clone() for p in params])
    res = [[e.clone() for e in p.error] for p in params] if kw.get("ef") else []
    return outs, res, q


@pytest.mark.parametrize("kw", [dict(), dict(ef=True), dict(two_phase=True), dict(ef=True, two_phase=True), dict(n_bit=32), dict(random=0)],
                         ids=["plain", "ef", "twophase", "ef_twophase", "n32", "random0"])
def test_ps_host_logic_draw_plan_equals_per_tensor_draws(kw):
    """The one-call draw plan hands every tensor the numbers its own torch.rand calls would have drawn: the aggregate, the
    residuals and the wire are identical, bit for bit, over three users and two steps."""
    from gq_amd.quantizers import PSQuantizer
    grads = _fcn_grads(5, 3, 2)
    a, ra, qa = _run_cpu(PSQuantizer, grads, 3, True, **kw)
    b, rb, qb = _run_cpu(PSQuantizer, grads, 3, False, **kw)
    assert qa._draw_total > 0 and qb._draw_total == 0
    for x, y in zip([t for s in a for t in s] + [t for r in ra for t in r], [t for s in b for t in s] + [t for r in rb for t in r]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(qa._wire, qb._wire)
    # and it is not the identity: the aggregate differs from the plain mean of the gradients
    mean0 = torch.stack([g[0] for g in grads[-1]]).mean(0)
    assert not torch.equal(a[-1][0], mean0)


import pvq_fixture_util as fxu  # noqa: E402


@pytest.mark.parametrize("name", fxu.FCN_FIXTURES)
def test_ps_host_logic_reproduces_the_reference_fixtures(name):
    """The reference's own PSQuantizer / RingQuantizer over its ProbabilisticVectorCompressor (tests/golden/make_golden_pvqpsq.py)
    against this project's quantizers on the CPU oracle codec, gq_rng = "reference": every user's codes, levels and (lb, ub), every
    step's aggregate, the residuals and server residuals -- identical.  Pins the draw order (codewords, then levels, per tensor in
    parameter order, the second phase included) and the error-feedback / two-phase sequence to the reference, not to this code."""
    from oracle_codec_pvq import oracle_pvq_codec_factory
    diffs, q = fxu.run_fixture(name, torch.device("cpu"), oracle_pvq_codec_factory)
    assert not diffs, diffs[:8]
    assert q._draw_total > 0
