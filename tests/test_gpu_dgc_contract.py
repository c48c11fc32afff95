"""libgq_dgc.so and the top-k select between its two launches held to include/gq_dgc.h, through BatchedDGC as the quantizer lays a
group out: np.array_equal on the wire, u and v after EVERY one of three consecutive records against tests/dgc_contract.py (whose own
checks, and one assertion for every claim made here about an input, are tests/test_dgc_contract.py).  Values are compared as
canonical bits (dc.canon: which NaN an addition yields is not part of the contract), indices and every other byte as they are.

The wire starts as 0xAB, gradients and state are views inside guarded buffers; after every record the gradients are unchanged,
the guards intact, the histogram zero and every byte outside the sections still holds its fill."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import dgc_contract as dc  # noqa: E402
import topk_contract as tc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, FILL = 3.0, 0xAB


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


class _K(object):
    def __init__(self, k):
        self.k = k


def _up(x, a=16):
    return (x + a - 1) // a * a


def _place(arr, off, dev):
    big = torch.full((arr.size + 8,), GUARD, dtype=torch.float32, device=dev)
    view = big[off:off + arr.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    return view, big


def _guards_intact(big, off, n):
    b = big.cpu().numpy()
    return np.all(b[:off] == GUARD) and np.all(b[off + n:] == GUARD)


def make_group(sizes, ks, dense_sizes=()):
    from gq_amd.codecs import BatchedDGC, TopKCodec
    dev = torch.device("cuda:0")
    codecs = [TopKCodec(_K(k), n, torch.Size([n])) for n, k in zip(sizes, ks)]
    offs, off = [], 0
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes)
    dense = []
    for n in dense_sizes:
        dense.append((off, n))
        off += 4 * n
    ub = _up(off) + 16
    g = BatchedDGC(codecs, offs, list(range(len(codecs))), dev, 1, ub, dense=dense or None)
    return SimpleNamespace(g=g, offs=offs, dense=dense, ub=ub, dev=dev, sizes=list(sizes), ks=list(ks))


class User(object):
    """One user slot: its state on the device (guarded views) and the restatement's."""

    def __init__(self, G, m, u0=None, v0=None, off=0):
        self.G, self.m, self.off = G, m, off
        self.want = dc.State(G.sizes, G.ks, m, u0, v0)
        self.u = [_place(a, off, G.dev) for a in self.want.u]
        self.v = [_place(a, off, G.dev) for a in self.want.v]

    def record(self, gs, g_off=0, garbage=False, dense_src=()):
        G, g = self.G, self.G.g
        src = [_place(a, g_off, G.dev) for a in gs]
        ds = [torch.from_numpy(a).to(G.dev) for a in dense_src]
        wire = torch.full((G.ub,), FILL, dtype=torch.uint8, device=G.dev)
        if garbage:      # every scratch buffer except the histogram, which the contract wants zero and every compress leaves zero
            g._scratch.copy_(torch.from_numpy(tc.from_bits(np.random.RandomState(1).randint(0, 2 ** 32, g._scratch.numel(), dtype=np.uint64)
                                                           .astype(np.uint32))))
            g._ef_buffer(G.dev).fill_(float("nan"))
            g._state.random_(-2 ** 31, 2 ** 31 - 1)
            g._counts.random_(-2 ** 31, 2 ** 31 - 1)
        kw = {"dense": ds} if ds else {}
        assert g.encode([t for t, _ in src], wire, 0, 0, errs=([t for t, _ in self.u], [t for t, _ in self.v]), ef_scale=self.m, **kw)
        torch.cuda.synchronize()
        secs = self.want.record(gs)
        w = wire.cpu().numpy()
        covered = np.zeros(G.ub, bool)
        assert not g._hist.cpu().numpy().any(), "the record left the histogram non-zero"
        for i, (n, k, off) in enumerate(zip(G.sizes, G.ks, G.offs)):
            what = "tensor %d (n = %d, k = %d)" % (i, n, k)
            assert np.array_equal(dc.canon_section(w[off:off + 8 * k], k), dc.canon_section(secs[i], k)), what + ": wire"
            covered[off:off + 8 * k] = True
            assert np.array_equal(dc.canon(self.u[i][0].cpu().numpy()), dc.canon(self.want.u[i])), what + ": u"
            assert np.array_equal(dc.canon(self.v[i][0].cpu().numpy()), dc.canon(self.want.v[i])), what + ": v"
            assert np.array_equal(tc.bits(src[i][0].cpu().numpy()), tc.bits(gs[i])), what + ": the gradient was written"
            for big in (src[i][1], ):
                assert _guards_intact(big, g_off, n), what + ": a write outside the gradient"
            assert _guards_intact(self.u[i][1], self.off, n) and _guards_intact(self.v[i][1], self.off, n), what + ": a write outside the state"
        for (off, n), a in zip(G.dense, dense_src):
            assert np.array_equal(w[off:off + 4 * n], a.view(np.uint8)), "dense copy"
            covered[off:off + 4 * n] = True
        assert np.all(w[~covered] == FILL), "a byte outside the sections was written"


def run(case, m, **kw):
    sizes, ks, steps = case[:3]
    u0, v0 = (case[3], case[4]) if len(case) == 5 else (None, None)
    G = make_group(sizes, ks)
    user = User(G, m, u0, v0)
    for gs in steps:
        user.record(gs, **kw)


@pytest.mark.parametrize("m", dc.MOMENTA)
def test_item_seams(m):
    run(dc.seam_case(), m)


@pytest.mark.parametrize("m", dc.MOMENTA)
def test_k_zero_one_all_and_two_mask_workgroups(m):
    run(dc.k_case(), m)


@pytest.mark.parametrize("m", dc.MOMENTA)
def test_ties_across_an_item_seam(m):
    run(dc.tie_case(), m)


@pytest.mark.parametrize("m", dc.MOMENTA)
def test_zeros_subnormals_infinities_and_nans_in_gradient_and_state(m):
    run(dc.special_case(), m)


def test_garbage_in_every_scratch_buffer():
    run(dc.seam_case(), 0.9, garbage=True)


def test_misaligned_gradient_view_and_state():
    """The gradients 4 bytes past a 16-byte boundary (the scalar path of the accumulate launch), then the state as well."""
    run(dc.seam_case(), 0.9, g_off=1)
    sizes, ks, steps = dc.seam_case()
    G = make_group(sizes, ks)
    user = User(G, 0.5, off=3)
    for gs in steps:
        user.record(gs, g_off=2)


def test_seventy_tensors_and_the_dense_copies():
    sizes, ks, steps = dc.many_case()
    dense = [tc.ordinary(n, 90 + n) for n in (10, 256, 1000)]
    G = make_group(sizes, ks, dense_sizes=[a.size for a in dense])
    user = User(G, 0.9)
    for gs in steps:
        user.record(gs, dense_src=dense)


def test_two_user_slots_recorded_alternately():
    sizes, ks, steps = dc.seam_case()
    G = make_group(sizes, ks)
    a, b = User(G, 0.9), User(G, 0.9)
    other = [[tc.heavy_tailed(n, 7000 + n + s) for n in sizes] for s in range(dc.STEPS)]
    for gs, hs in zip(steps, other):
        a.record(gs)
        b.record(hs)      # (each compares its own state with a restatement that has never seen the other's gradients)


def test_refusals():
    from gq_amd import native
    G = make_group([2000, 3000], [10, 20])
    b = G.g._batch
    with pytest.raises(native.GQNativeError, match="null state table"):
        b.accumulate(0.9)
    wire = torch.zeros(G.ub, dtype=torch.uint8, device=G.dev)
    with pytest.raises(native.GQNativeError, match="null state table"):
        b.mask(wire)
    user = User(G, 0.9)
    user.record([tc.ordinary(2000, 1), tc.ordinary(3000, 2)])
    b.d.struct_bytes -= 1
    with pytest.raises(native.GQNativeError, match="another size"):
        b.accumulate(0.9)
    with pytest.raises(native.GQNativeError, match="another size"):
        b.mask(wire)
    b.d.struct_bytes += 1
    with pytest.raises(native.GQNativeError, match="NaN"):
        b.accumulate(float("nan"))
    torch.cuda.synchronize()
    assert np.array_equal(dc.canon(user.u[0][0].cpu().numpy()), dc.canon(user.want.u[0]))      # a refused call launched nothing


# ---- graphs: the records of a PSQuantizer, replayed ---------------------------------------------------------------------------
def _quantizer(users, **kw):
    from argparse import Namespace
    from gq_amd.compressors import TopKSparsificationCompressor
    from gq_amd.quantizers import PSQuantizer
    shapes = [(n,) for n in dc.SEAM_SIZES] + [(10,), (300,)]
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes]
    args = Namespace(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="1.0", num_users=users,
                     mode="ps", cr=dc.SEAM_CR, momentum_correction=0.9, **kw)
    return PSQuantizer(TopKSparsificationCompressor, params, args), params, shapes


def _graph_run(users, steps, fresh_addresses):
    q, params, shapes = _quantizer(users)
    nbig = len(dc.SEAM_SIZES)
    ks = [n // dc.SEAM_CR for n in dc.SEAM_SIZES]
    want = [dc.State(dc.SEAM_SIZES, ks, 0.9) for _ in range(users)]
    held = []      # fresh_addresses: every gradient tensor stays alive, so no address comes back
    fixed = [[torch.empty(s, device="cuda") for s in shapes] for _ in range(users)]
    for step in range(steps):
        secs, dense = [], []
        for user in range(users):
            gs = [tc.heavy_tailed(int(np.prod(s)), 8000 + 100 * step + 10 * user + j) for j, s in enumerate(shapes)]
            for j, (p, a) in enumerate(zip(params, gs)):
                if fresh_addresses:
                    p.grad = torch.from_numpy(a).to("cuda").view(p.shape)
                    held.append(p.grad)
                else:
                    fixed[user][j].copy_(torch.from_numpy(a).view(p.shape))
                    p.grad = fixed[user][j].detach()      # (a tensor object of its own: apply() rebinds p.grad.data)
            q.record(user, 0)
            secs.append(want[user].record(gs[:nbig]))
            dense.append(gs[nbig:])
        torch.cuda.synchronize()
        for user in range(users):
            w = q._wire[user].cpu().numpy()
            for i, k in enumerate(ks):
                off = q.offsets[i]
                what = "step %d, user %d, tensor %d" % (step, user, i)
                assert np.array_equal(dc.canon_section(w[off:off + 8 * k], k), dc.canon_section(secs[user][i], k)), what + ": wire"
                assert np.array_equal(dc.canon(params[i].dgc_u[user].cpu().numpy()), dc.canon(want[user].u[i])), what + ": u"
                assert np.array_equal(dc.canon(params[i].dgc_v[user].cpu().numpy()), dc.canon(want[user].v[i])), what + ": v"
        q.apply()
        torch.cuda.synchronize()
        for i, (n, k) in enumerate(zip(dc.SEAM_SIZES, ks)):
            mean = tc.decode_mean([tc.split_section(secs[u][i], k) for u in range(users)], n, k, users)
            assert np.array_equal(dc.canon(params[i].grad.cpu().numpy()), dc.canon(mean)), "step %d, tensor %d: the aggregate" % (step, i)
        for j in range(nbig, len(shapes)):
            acc = np.zeros(shapes[j], np.float32)
            for u in range(users):
                acc = (acc + dense[u][j - nbig]).astype(np.float32)
            assert np.array_equal(tc.bits(params[j].grad.cpu().numpy()), tc.bits(acc / np.float32(users))), "step %d: dense tensor %d" % (step, j)
    return q


def test_graph_replay_equals_the_contract_whole_step():
    q = _graph_run(1, 6, fresh_addresses=False)
    p = q.record_paths
    assert p["eager"] >= 1 and p["graph"] + p["whole_step"] >= 1, p
    assert [g[0].__name__ for g in q._groups] == ["BatchedDGC"]


def test_graph_replay_equals_the_contract_two_users():
    q = _graph_run(2, 5, fresh_addresses=False)
    p = q.record_paths
    assert p["eager"] >= 2 and p["graph"] >= 2, p


@pytest.mark.parametrize("users", [1, 2])
def test_address_free_graph_with_gradients_at_new_addresses(users):
    q = _graph_run(users, 6, fresh_addresses=True)
    p = q.record_paths
    assert p["graph_any_address"] + p["whole_step_any_address"] >= users, p
    assert p["graph"] + p["whole_step"] == 0, p
