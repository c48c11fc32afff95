"""Top-k sparsification on the MI355X (libgq_topk.so): the reference's fixtures bit for bit, the kernels against a CPU torch
restatement of the contract (include/gq_topk.h: lowest indices among boundary ties), deterministic wire bytes eagerly and under
graph replay, the one documented deviation, and a training run on the kernels."""
import glob
import hashlib
import json
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="1.0",
                num_users=1, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _same(a, b):
    """Bitwise equal (zeros with their sign), except that any NaN equals any NaN."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    b = np.ascontiguousarray(b, np.float32).reshape(-1)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


def _canon(a):
    """NaNs as one bit pattern (the digests of the fixtures are of NaN-free data; this keeps a stray NaN from hiding)."""
    a = np.ascontiguousarray(a, np.float32).copy()
    a[np.isnan(a)] = np.float32("nan")
    return a


# ---- the contract restated on the CPU ----------------------------------------------------------------------------------
def ref_kept(x, k):
    """Kept indices (ascending): the k largest keys, the lowest indices among boundary ties."""
    x = torch.as_tensor(x, dtype=torch.float32).reshape(-1).cpu()
    key = (x.view(torch.int32).to(torch.int64) & 0x7fffffff)
    key[key > 0x7f800000] = 0x7fffffff
    order = torch.sort(-key, stable=True)[1][:k]
    return torch.sort(order)[0]


def ref_decoded(x, k):
    x = torch.as_tensor(x, dtype=torch.float32).reshape(-1).cpu()
    mask = torch.zeros_like(x)
    mask[ref_kept(x, k)] = 1
    return x * mask


def _group(tensors, ks, dev):
    """A BatchedTopK over `tensors` (device f32) with k per tensor, its wire laid out as the quantizer lays it out."""
    from gq_amd.codecs import BatchedTopK, TopKCodec, _up

    class _C(object):
        def __init__(self, k):
            self.k = k
    codecs = [TopKCodec(_C(k), t.numel(), t.shape) for t, k in zip(tensors, ks)]
    offs, off = [], 0
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes)
    user_bytes = max(16, _up(off))
    return BatchedTopK(codecs, offs, list(range(len(codecs))), dev, 1, user_bytes), codecs, offs, user_bytes


def _check_group(tensors, ks, dev):
    g, codecs, offs, ub = _group(tensors, ks, dev)
    wire = torch.zeros(ub, dtype=torch.uint8, device=dev)
    out = torch.full((g.out_floats,), 7.0, dtype=torch.float32, device=dev)
    assert g.encode(tensors, wire, 0, 0, out=out)
    torch.cuda.synchronize()
    w = wire.cpu()
    o = out.cpu()
    for t, k, cd, off, oo in zip(tensors, ks, codecs, offs, g.out_off):
        x = t.cpu()
        kept = ref_kept(x, k)
        idx = w[off:off + 4 * k].view(torch.int32).to(torch.int64)
        val = w[off + 4 * k:off + 8 * k].view(torch.float32)
        assert torch.equal(idx, kept), "indices differ (n = %d, k = %d)" % (x.numel(), k)
        assert _same(val.numpy(), x[kept].numpy())
        assert _same(o[oo:oo + x.numel()].numpy(), ref_decoded(x, k).numpy())
    return g, wire


# ---- fixtures of the reference --------------------------------------------------------------------------------------
SINGLE = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "topk_*.npz")))


def _input(g):
    if "x" in g.files:
        return g["x"]
    assert str(g["kind"]) == "randn"
    x = np.random.RandomState(int(g["seed"])).standard_normal(int(g["n"])).astype(np.float32)
    assert sha(x) == str(g["x_sha"])
    return x


def test_fixture_list():
    assert len(SINGLE) >= 7 and len(glob.glob(os.path.join(GOLDEN, "topkpsq_*.npz"))) == 4
    assert len(glob.glob(os.path.join(GOLDEN, "topkd_*.npz"))) == 2


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", SINGLE)
def test_compressor_matches_fixture(name):
    """TopKSparsificationCompressor.compress / decompress on a device tensor: the reference's dense tensor, bit for bit."""
    from gq_amd.compressors import TopKSparsificationCompressor
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x = _input(g)
    n, cr = int(g["n"]), int(g["cr"])
    c = TopKSparsificationCompressor(n, torch.Size([n]), make_args(cr=cr))
    assert c.k == int(g["k"])
    dec = c.decompress(c.compress(torch.from_numpy(x).cuda())).cpu().numpy()
    if "dec" in g.files:
        assert _same(dec, g["dec"])
    else:
        assert sha(dec) == str(g["dec_sha"])
    # the wire of the same tensor (checked against the restatement inside): the same keys as the reference's kept set -- the
    # indices themselves may differ among ties on a zero (or NaN) key, where either choice decodes to the same tensor
    grp, wire = _check_group([torch.from_numpy(x).cuda()], [c.k], torch.device("cuda"))
    ours = wire.cpu()[:4 * c.k].view(torch.int32).numpy().astype(np.int64)
    key = np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0x7fffffff)
    key = np.where(key > 0x7f800000, np.uint32(0x7fffffff), key)
    assert np.array_equal(np.sort(key[ours]), np.sort(key[g["kept"].astype(np.int64)]))


@pytest.mark.timeout(600)
def test_25m_digest():
    from gq_amd.compressors import TopKSparsificationCompressor
    g = np.load(os.path.join(GOLDEN, "topkd_25m.npz"))
    x = _input(g)
    n, k = int(g["n"]), int(g["k"])
    c = TopKSparsificationCompressor(n, torch.Size([n]), make_args(cr=int(g["cr"])))
    xd = torch.from_numpy(x).cuda()
    dec = c.decompress(c.compress(xd)).cpu().numpy()
    assert sha(dec) == str(g["dec_sha"])
    grp = _group([xd], [k], xd.device)[0]
    w = torch.zeros(max(16, 8 * k), dtype=torch.uint8, device=xd.device)
    assert grp.encode([xd], w, 0, 0)
    torch.cuda.synchronize()
    assert sha(w.cpu()[:4 * k].numpy().view(np.uint32)) == str(g["kept_sha"])


def _run_psq(g, shapes, steps_grads, ef, two_phase, users):
    from gq_amd.compressors import TopKSparsificationCompressor
    from gq_amd.quantizers import PSQuantizer
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes]
    q = PSQuantizer(TopKSparsificationCompressor, params, make_args(cr=int(g["cr"]), ef=ef, two_phase=two_phase, num_users=users))
    aggs = []
    for step in steps_grads:
        for u, gs in enumerate(step):
            for p, a in zip(params, gs):
                p.grad = torch.from_numpy(a).cuda()
            q.record(u, 0)
        q.apply()
        aggs.append([_canon(p.grad.detach().cpu().numpy()) for p in params])
    return q, params, aggs


def _grads(seed, shapes, users, steps, scale):
    rs = np.random.RandomState(seed)
    return [[[(rs.standard_normal(int(np.prod(s))) * scale).astype(np.float32).reshape(s) for s in shapes]
             for _ in range(users)] for _ in range(steps)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "topkpsq_*.npz"))))
def test_psquantizer_matches_fixture(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    shapes = [tuple(s) for s in json.loads(str(g["shapes"]))]
    users, steps, ef, tp = int(g["users"]), int(g["steps"]), bool(int(g["ef"])), bool(int(g["two_phase"]))
    grads = _grads(int(g["seed"]), shapes, users, steps, float(g["scale"]))
    assert sha(np.concatenate([a.reshape(-1) for st in grads for us in st for a in us])) == str(g["grads_sha"])
    q, params, aggs = _run_psq(g, shapes, grads, ef, tp, users)
    assert [g_[0].__name__ for g_ in q._groups] == ["BatchedTopK"]
    for s in range(steps):
        for i in range(len(shapes)):
            assert sha(aggs[s][i]) == str(g["agg_sha"][s][i]), "step %d parameter %d" % (s, i)
    if ef:
        for i, p in enumerate(params):
            for u in range(users):
                assert sha(_canon(p.error[u].detach().cpu().numpy())) == str(g["err_sha"][i][u]), "residual %d / %d" % (i, u)
    if ef and tp:
        for i, p in enumerate(params):
            assert sha(_canon(p.server_error.detach().cpu().numpy())) == str(g["serr_sha"][i])


@pytest.mark.timeout(600)
def test_resnet50_digest():
    g = np.load(os.path.join(GOLDEN, "topkd_resnet50_u2.npz"))
    shapes = [tuple(s) for s in json.loads(str(g["shapes"]))]
    grads = _grads(int(g["seed"]), shapes, int(g["users"]), 1, float(g["scale"]))
    q, params, aggs = _run_psq(g, shapes, grads, False, False, int(g["users"]))
    assert q.wire_bytes_per_user() == 823_968
    for i in range(len(shapes)):
        assert sha(aggs[0][i]) == str(g["agg_sha"][0][i]), "parameter %d" % i


# ---- kernels against the CPU restatement ---------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_random_tables_with_a_25m_tensor():
    rs = np.random.RandomState(11)
    dev = torch.device("cuda")
    sizes = [1001, 1001, 4096, 4097, 25_000_000, 1001, 70_000, 123_457]
    ts = [torch.from_numpy(rs.standard_normal(n).astype(np.float32)).to(dev) for n in sizes]
    ks = [n // 256 for n in sizes[:-2]] + [1, 123_457]
    _check_group(ts, ks, dev)


@pytest.mark.timeout(300)
def test_forced_ties_and_all_equal():
    rs = np.random.RandomState(12)
    dev = torch.device("cuda")
    small = (rs.randint(-3, 4, size=50_000)).astype(np.float32)          # seven magnitudes: every boundary is a tie
    small[rs.rand(small.size) < 0.3] = np.float32(-0.0)
    equal = np.full(9_000, 0.25, np.float32)
    equal[::2] = -0.25
    zeros = np.zeros(5_000, np.float32)
    zeros[1::3] = np.float32(-0.0)
    nonfin = rs.standard_normal(3_000).astype(np.float32)
    nonfin[rs.choice(3_000, 50, replace=False)] = np.nan
    nonfin[rs.choice(3_000, 50, replace=False)] = np.inf
    ts = [torch.from_numpy(a).to(dev) for a in (small, equal, zeros, nonfin, small, equal)]
    ks = [12_345, 4_500, 17, 60, 50_000, 0]
    _check_group(ts, ks, dev)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("R", range(1, 9))
def test_decode_mean_against_stack_mean(R):
    rs = np.random.RandomState(100 + R)
    dev = torch.device("cuda")
    sizes, cr = [1001, 20_000, 4096, 300_000], 16
    ks = [n // cr for n in sizes]
    g = None
    rows, decs = [], []
    for r in range(R):
        xs = [rs.standard_normal(n).astype(np.float32) * 10 ** rs.uniform(-3, 1) for n in sizes]
        ts = [torch.from_numpy(x).to(dev) for x in xs]
        if g is None:
            g, codecs, offs, ub = _group(ts, ks, dev)
        wire = torch.zeros(ub, dtype=torch.uint8, device=dev)
        assert g.encode(ts, wire, 0, 0)
        rows.append(wire)
        decs.append([ref_decoded(x, k) for x, k in zip(xs, ks)])
    gathered = torch.stack(rows)
    views = g.decode_mean(gathered, R)
    torch.cuda.synchronize()
    for i in range(len(sizes)):
        want = torch.stack([d[i] for d in decs]).mean(0)
        assert _same(views[i].cpu().numpy(), want.numpy()), "tensor %d, R = %d" % (i, R)
    if R == 1:      # plain: the payload's values as they are
        views = g.decode_mean(gathered, 1, plain=True)
        for i in range(len(sizes)):
            got = views[i].cpu()
            kept = ref_kept(decs[0][i], ks[i])
            assert _same(got[kept].numpy(), decs[0][i][kept].numpy())


# ---- determinism, graphs ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_wire_bytes_are_deterministic_eager_and_replayed():
    from gq_amd.compressors import TopKSparsificationCompressor
    from gq_amd.quantizers import PSQuantizer
    torch.manual_seed(3)
    shapes = [(256, 784), (256,), (10, 256), (10,), (300, 300)]
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes]
    grads = [torch.randn(s, device="cuda") for s in shapes]
    for gr in grads:      # a fifth of every tensor ties at 3.0: the boundary of k = n / 64 falls inside the ties
        gr.view(-1)[::5] = 3.0
    q = PSQuantizer(TopKSparsificationCompressor, params, make_args(cr=64))
    wires, outs = [], []
    for step in range(6):
        for p, gr in zip(params, grads):
            p.grad = gr.clone()      # (apply() rebinds p.grad.data to the aggregate)
        q.record(0, 0)
        q.apply()
        torch.cuda.synchronize()
        wires.append(q._wire[0].cpu().clone())
        outs.append([p.grad.detach().cpu().clone() for p in params])
    paths = q.record_paths
    assert paths["eager"] >= 1 and sum(paths.values()) - paths["eager"] >= 1, paths
    for w in wires[1:]:
        assert torch.equal(w, wires[0])
    for o in outs[1:]:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(o, outs[0]))
    # the same bytes from a second quantizer (fresh scratch)
    q2 = PSQuantizer(TopKSparsificationCompressor, params, make_args(cr=64, gq_graph=False))
    for p, gr in zip(params, grads):
        p.grad = gr.clone()
    q2.record(0, 0)
    torch.cuda.synchronize()
    assert torch.equal(q2._wire[0].cpu(), wires[0])


@pytest.mark.timeout(300)
def test_training_loop_replays_after_the_first_steps():
    """driver.FCN trained with the top-k quantizer: gradients are re-allocated every step, the record replays a graph."""
    from gq_amd.compressors import TopKSparsificationCompressor
    from gq_amd.driver import FCN
    from gq_amd.quantizers import PSQuantizer
    torch.manual_seed(0)
    model = FCN().cuda()
    q = PSQuantizer(TopKSparsificationCompressor, model.parameters(), make_args(cr=256))
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    x = torch.randn(32, 784, device="cuda")
    y = torch.randint(0, 10, (32,), device="cuda")
    for _ in range(12):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(x), y).backward()
        q.record(0, 0)
        q.apply()
        opt.step()
    torch.cuda.synchronize()
    p = q.record_paths
    replayed = p["graph"] + p["whole_step"] + p["graph_any_address"] + p["whole_step_any_address"]
    assert p["eager"] <= 3 and replayed >= 9, p
    assert [g[0].__name__ for g in q._groups] == ["BatchedTopK"]


@pytest.mark.timeout(600)
def test_train_py_runs_topk():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "topk", "--network", "fcn", "--dataset", "mnist",
           "--num-users", "1", "--epochs", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip(), "no log lines"


# ---- the documented deviation ------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_nonfinite_beyond_k_aggregates_to_zero():
    """More than k non-finite values in a tensor: the unkept +-inf / NaN entries decode to NaN in the reference (v * 0), but
    the wire does not carry them -- the aggregate has +0 / R there.  Kept entries and the residual
    under error feedback stay exact."""
    from gq_amd.compressors import TopKSparsificationCompressor
    from gq_amd.quantizers import PSQuantizer
    n, cr = 4000, 400       # k = 10
    x = torch.randn(n)
    bad = torch.arange(5, n, 97)[:30]      # 30 > k non-finite values
    x[bad[:10]] = float("nan")
    x[bad[10:20]] = float("inf")
    x[bad[20:]] = float("-inf")
    params = [torch.nn.Parameter(torch.zeros(n, device="cuda")), torch.nn.Parameter(torch.zeros(n, device="cuda"))]
    q = PSQuantizer(TopKSparsificationCompressor, params, make_args(cr=cr, num_users=2))
    for u in range(2):
        for p in params:
            p.grad = x.cuda()
        q.record(u, 0)
    q.apply()
    got = params[0].grad.cpu()
    dec = ref_decoded(x, n // cr)
    ref = torch.stack([dec, dec]).mean(0)
    kept = ref_kept(x, n // cr)
    unkept_nonfinite = torch.tensor([i for i in bad.tolist() if i not in set(kept.tolist())])
    assert len(unkept_nonfinite) == 20
    assert torch.isnan(ref[unkept_nonfinite]).all()
    assert torch.equal(got[unkept_nonfinite].view(torch.int32), torch.zeros(20, dtype=torch.int32))      # +0
    rest = torch.ones(n, dtype=torch.bool)
    rest[unkept_nonfinite] = False
    assert _same(got[rest].numpy(), ref[rest].numpy())


@pytest.mark.timeout(300)
def test_ring_keeps_the_reference_result():
    """RingQuantizer with top-k: user u compresses grad_u + the decoded running sum (ring_quantizer.py:31-40); the hop is
    the decoded dense tensor (GenericCodec over the device kernels), so the result is the reference's bit for bit."""
    from gq_amd.compressors import TopKSparsificationCompressor
    from gq_amd.quantizers import RingQuantizer
    torch.manual_seed(5)
    n, cr, users = 6000, 50, 3
    grads = [torch.randn(n) for _ in range(users)]
    for gr in grads:
        gr[::7] = -0.0
    params = [torch.nn.Parameter(torch.zeros(n, device="cuda")), torch.nn.Parameter(torch.zeros(n, device="cuda"))]
    q = RingQuantizer(TopKSparsificationCompressor, params, make_args(cr=cr, num_users=users, mode="ring"))
    for u in range(users):
        for p in params:
            p.grad = grads[u].cuda()
        q.record(u, 0)
    q.apply()
    running = None
    for u in range(users):
        v = grads[u] if running is None else grads[u] + running
        running = ref_decoded(v, n // cr)
    for p in params:
        assert _same(p.grad.cpu().numpy(), running.numpy())
