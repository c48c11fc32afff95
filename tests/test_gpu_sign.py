"""signSGD on the MI355X (libgq_sign.so), bit for bit: the kernels against torch.sign on the same device and a numpy restatement of
the 2-bit wire (include/gq_sign.h), the decode-mean against gq_mean_rows over the dense signs, PSQuantizer / RingQuantizer against
the dense-f32 path they replace (GenericCodec over torch.sign) and the reference's fixtures, the same wire eagerly and replayed,
training, and two ranks on one GPU."""
import glob
import hashlib
import json
import math
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
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp",
                num_users=1, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _eq(a, b):
    """Bitwise equal float32 tensors (signed zeros and NaN payloads included)."""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same(a, b):
    """Bitwise equal, except that any NaN equals any NaN (the project's bar for arithmetic on NaN)."""
    a, b = a.detach().reshape(-1).cpu(), b.detach().reshape(-1).cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


# ---- the wire restated in numpy ------------------------------------------------------------------------------------------
def np_pack(signs):
    """The section of one tensor: 2-bit codes (+0 -> 00, +1 -> 01, -1 -> 11), element i in bits 2*(i%16) of LE word i/16,
    zero pad up to a multiple of 16 bytes."""
    s = np.ascontiguousarray(signs, np.float32).reshape(-1)
    n = s.size
    c = np.zeros(n, np.uint64)
    c[s > 0] = 1
    c[s < 0] = 3
    assert np.all((s == 0) | (s == 1) | (s == -1)) and not np.any(np.signbit(s) & (s == 0))
    words = -(-n // 16)
    c = np.concatenate([c, np.zeros(words * 16 - n, np.uint64)]).reshape(words, 16)
    w = (c << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype("<u4")
    out = np.zeros(-(-(words * 4) // 16) * 16, np.uint8)
    out[:words * 4] = w.view(np.uint8)
    return out


class TorchSign(object):
    """The compressor as it was before the kernels: torch.sign, identity decompress (signsgd_compressor.py:4-12)."""

    def compress(self, vec):
        return torch.sign(vec)

    def decompress(self, signature):
        return signature


def generic_factory(compressor, numel, shape, packed6=False):
    """The dense-f32 path: GenericCodec over torch.sign for every sign tensor, the PS codecs for the others."""
    from gq_amd.codecs import GenericCodec, default_codec_factory
    from gq_amd.compressors import SignSGDCompressor
    if isinstance(compressor, SignSGDCompressor):
        return GenericCodec(TorchSign(), numel, shape)
    return default_codec_factory(compressor, numel, shape, packed6)


def _group(tensors, dev):
    """A BatchedSign over `tensors`, its wire laid out as the quantizer lays it out."""
    from gq_amd.codecs import BatchedSign, SignCodec, _up
    codecs = [SignCodec(None, t.numel(), t.shape) for t in tensors]
    offs, off = [], 0
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes)
    ub = max(16, _up(off))
    return BatchedSign(codecs, offs, list(range(len(codecs))), dev, 1, ub), codecs, offs, ub


EDGE_BITS = [0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800123, 0x7fbfffff, 0x7fc0beef, 0x7f800000,
             0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x7f7fffff, 0xff7fffff]


def edge_input(n, seed):
    """Random data over the whole exponent range with a quarter of the entries replaced by ±0, ±NaN with payloads, ±inf,
    subnormals, ±FLT_MIN and ±FLT_MAX."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal(n).astype(np.float32) * np.exp2(rs.randint(-140, 120, n)).astype(np.float32)
    pos = rs.rand(n) < 0.25
    x[pos] = np.array(EDGE_BITS, np.uint32)[rs.randint(0, len(EDGE_BITS), int(pos.sum()))].view(np.float32)
    return x


# ---- kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("n", [1001, 4095, 4096, 4097, 1_000_000, 25_000_000])
def test_compress_equals_torch_sign_on_the_device(n):
    dev = torch.device("cuda")
    x = edge_input(n, n)
    t = torch.from_numpy(x).to(dev)
    g, codecs, offs, ub = _group([t], dev)
    wire = torch.full((ub,), 0xA5, dtype=torch.uint8, device=dev)      # (every byte of the section is written, the pad too)
    out = torch.full((g.out_floats,), 7.0, dtype=torch.float32, device=dev)
    assert g.encode([t], wire, 0, 0, out=out)
    want = torch.sign(t)
    torch.cuda.synchronize()
    assert _eq(out[:n], want)
    assert np.array_equal(wire.cpu().numpy(), np_pack(want.cpu().numpy()))
    assert _eq(t, torch.from_numpy(x))      # (no error feedback: the source is only read)
    assert _eq(g.decode_mean(wire.view(1, -1), 1, plain=True)[0].view(-1), want)


@pytest.mark.timeout(300)
def test_group_with_unaligned_views_and_dense_copy():
    """Tensors at 4-byte (not 16-byte) aligned addresses take the element-wise path; the dense tensors ride in the launch."""
    dev = torch.device("cuda")
    base = torch.from_numpy(edge_input(300_017, 3)).to(dev)
    ts = [base[1:4098], base[4100:5101], base[5103:5103 + 70_001], base[80_000:80_000 + 200_000]]
    from gq_amd.codecs import BatchedSign, SignCodec, _up
    codecs = [SignCodec(None, t.numel(), t.shape) for t in ts]
    offs, off = [], 0
    for cd in codecs:
        offs.append(off)
        off = _up(off + cd.nbytes)
    dense = [torch.randn(s, device=dev) for s in (10, 1000, 7)]
    dspec, doff = [], off
    for d in dense:
        dspec.append((doff, d.numel()))
        doff += 4 * d.numel()
    ub = _up(doff)
    g = BatchedSign(codecs, offs, list(range(len(ts))), dev, 1, ub, dense=dspec)
    wire = torch.full((ub,), 0x5A, dtype=torch.uint8, device=dev)
    out = torch.full((g.out_floats,), 7.0, dtype=torch.float32, device=dev)
    assert g.encode(ts, wire, 0, 0, dense=dense, out=out)
    torch.cuda.synchronize()
    w = wire.cpu().numpy()
    for t, cd, o, oo in zip(ts, codecs, offs, g.out_off):
        want = torch.sign(t)
        assert _eq(out[oo:oo + t.numel()], want)
        assert np.array_equal(w[o:o + cd.nbytes], np_pack(want.cpu().numpy()))
    for d, (o, k) in zip(dense, dspec):
        assert np.array_equal(w[o:o + 4 * k].view(np.float32).view(np.uint32), d.cpu().numpy().view(np.uint32))


@pytest.mark.timeout(300)
def test_error_feedback_in_the_launch():
    """w = v + RN(scale * err) stored back into the source, err = w - sign(w): torch's own arithmetic on the device."""
    dev = torch.device("cuda")
    sizes = [1001, 4096, 4097, 123_457]
    vs = [torch.from_numpy(edge_input(n, 10 + n)).to(dev) for n in sizes]
    errs = [torch.from_numpy(edge_input(n, 20 + n)).to(dev) for n in sizes]
    scale = 2 / (math.exp(-1) + 1) - 1
    want_w = [v + scale * e for v, e in zip(vs, errs)]
    want_s = [torch.sign(w) for w in want_w]
    want_e = [w - s for w, s in zip(want_w, want_s)]
    g, codecs, offs, ub = _group(vs, dev)
    wire = torch.zeros(ub, dtype=torch.uint8, device=dev)
    out = torch.empty(g.out_floats, dtype=torch.float32, device=dev)
    assert g.encode(vs, wire, 0, 0, errs=errs, ef_scale=scale, out=out)
    torch.cuda.synchronize()
    for v, e, ww, ws, we, o in zip(vs, errs, want_w, want_s, want_e, g.out_off):
        assert _same(v, ww) and _same(e, we) and _eq(out[o:o + v.numel()], ws)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("R", range(1, 9))
def test_decode_mean_equals_mean_rows_of_the_dense_signs(R):
    from gq_amd import native
    dev = torch.device("cuda")
    sizes = [1001, 20_000, 4096, 300_001]
    g = None
    rows, signs = [], []
    for r in range(R):
        ts = [torch.from_numpy(edge_input(n, 1000 * R + 10 * r + i)).to(dev) for i, n in enumerate(sizes)]
        if g is None:
            g, codecs, offs, ub = _group(ts, dev)
            big = torch.zeros((R, ub + 48), dtype=torch.uint8, device=dev)      # rows at a stride longer than a payload
        assert g.encode(ts, big[r, :ub], 0, 0)
        signs.append([torch.sign(t) for t in ts])
    gathered = big[:, :ub]
    for plain in ((False, True) if R == 1 else (False,)):
        views = g.decode_mean(gathered, R, plain=plain)
        for i, n in enumerate(sizes):
            want = torch.empty(n, dtype=torch.float32, device=dev)
            native.mean_rows(torch.stack([s[i] for s in signs]), want)
            assert _eq(views[i].view(-1), want), "tensor %d, R = %d, plain %s" % (i, R, plain)
            if R == 1:
                assert _eq(views[i].view(-1), signs[0][i])


# ---- quantizers against the dense path and the reference --------------------------------------------------------------------
def _grads(seed, shapes, users, steps, scale):
    """tests/golden/make_golden_sign.py's grads_of."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        st = []
        for _ in range(users):
            us = []
            for s in shapes:
                n = int(np.prod(s))
                a = (rs.standard_normal(n) * scale).astype(np.float32)
                z = rs.rand(n)
                a[z < 0.05] = np.float32(0.0)
                a[(z >= 0.05) & (z < 0.1)] = np.float32(-0.0)
                us.append(a.reshape(s))
            st.append(us)
        out.append(st)
    return out


def _run(cls, shapes, grads, factory=None, **kw):
    from gq_amd.compressors import SignSGDCompressor
    users = len(grads[0])
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes]
    q = cls(SignSGDCompressor, params, make_args(num_users=users, **kw), codec_factory=factory)
    aggs = []
    for epoch, step in enumerate(grads):
        for u, gs in enumerate(step):
            for p, a in zip(params, gs):
                p.grad = torch.from_numpy(a).cuda()
            q.record(u, epoch)
        q.apply()
        aggs.append([p.grad.detach().clone() for p in params])
    return q, params, aggs


def _check_pair_and_fixture(g, cls, **kw):
    shapes = [tuple(s) for s in json.loads(str(g["shapes"]))]
    users, steps = int(g["users"]), int(g["steps"])
    ef, tp = bool(int(g["ef"])), bool(int(g["two_phase"]))
    grads = _grads(int(g["seed"]), shapes, users, steps, float(g["scale"]))
    assert sha(np.concatenate([a.reshape(-1) for st in grads for us in st for a in us])) == str(g["grads_sha"])
    q, params, aggs = _run(cls, shapes, grads, ef=ef, two_phase=tp, **kw)
    q0, params0, aggs0 = _run(cls, shapes, grads, factory=generic_factory, ef=ef, two_phase=tp, **kw)
    assert [x[0].__name__ for x in q._groups] == ["BatchedSign"] and not q0._groups
    for s in range(steps):
        for i in range(len(shapes)):
            assert _eq(aggs[s][i], aggs0[s][i]), "step %d parameter %d: the 2-bit wire differs from the dense path" % (s, i)
            assert sha(aggs[s][i].cpu().numpy()) == str(g["agg_sha"][s][i]), "step %d parameter %d" % (s, i)
    if ef:
        for i, (p, p0) in enumerate(zip(params, params0)):
            for u in range(users):
                assert _eq(p.error[u], p0.error[u])
                assert sha(p.error[u].cpu().numpy()) == str(g["err_sha"][i][u]), "residual %d / %d" % (i, u)
    if ef and tp:
        for i, (p, p0) in enumerate(zip(params, params0)):
            assert _eq(p.server_error, p0.server_error)
            assert sha(p.server_error.cpu().numpy()) == str(g["serr_sha"][i])
    return q


def test_fixture_list():
    assert len(glob.glob(os.path.join(GOLDEN, "sign_*.npz"))) == 4 and len(glob.glob(os.path.join(GOLDEN, "signpsq_*.npz"))) == 4
    assert os.path.exists(os.path.join(GOLDEN, "signring_fcn_u3.npz")) and os.path.exists(os.path.join(GOLDEN, "signd_resnet50_u2.npz"))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "sign_*.npz"))))
def test_compressor_matches_fixture(name):
    """SignSGDCompressor.compress / decompress on a device tensor: the reference's tensor, bit for bit."""
    from gq_amd.compressors import SignSGDCompressor
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    n = int(g["n"])
    if "x" in g.files:
        x = g["x"]
    else:
        x = np.random.RandomState(int(g["seed"])).standard_normal(n).astype(np.float32)
    assert sha(x) == str(g["x_sha"])
    c = SignSGDCompressor(n, torch.Size([n]), make_args())
    dec = c.decompress(c.compress(torch.from_numpy(x).cuda())).cpu().numpy()
    assert sha(dec) == str(g["dec_sha"])
    assert hasattr(c, "_codecs")      # (the kernels ran)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "signpsq_*.npz"))))
def test_psquantizer_equals_dense_path_and_fixture(name):
    from gq_amd.quantizers import PSQuantizer
    _check_pair_and_fixture(np.load(os.path.join(GOLDEN, name + ".npz")), PSQuantizer)


@pytest.mark.timeout(300)
def test_ring_equals_dense_path_and_fixture():
    from gq_amd.quantizers import RingQuantizer
    _check_pair_and_fixture(np.load(os.path.join(GOLDEN, "signring_fcn_u3.npz")), RingQuantizer, mode="ring")


@pytest.mark.timeout(600)
def test_resnet50_digest():
    from gq_amd.quantizers import PSQuantizer
    g = np.load(os.path.join(GOLDEN, "signd_resnet50_u2.npz"))
    q = _check_pair_and_fixture(g, PSQuantizer)
    assert q.wire_bytes_per_user() == 5_964_256


# ---- determinism, graphs, training ---------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_wire_bytes_are_the_same_eager_and_replayed():
    from gq_amd.compressors import SignSGDCompressor
    from gq_amd.quantizers import PSQuantizer
    torch.manual_seed(3)
    shapes = [(256, 784), (256,), (10, 256), (10,), (300, 300)]
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes]
    grads = [torch.from_numpy(edge_input(int(np.prod(s)), i).reshape(s)).cuda() for i, s in enumerate(shapes)]
    q = PSQuantizer(SignSGDCompressor, params, make_args())
    wires, outs = [], []
    for step in range(6):
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
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
        assert all(_eq(a, b) for a, b in zip(o, outs[0]))
    w = wires[0].numpy()
    for cd, off, gr in zip(q.codecs, q.offsets, grads):
        if cd.numel > 1000:
            assert np.array_equal(w[off:off + cd.nbytes], np_pack(torch.sign(gr).cpu().numpy()))
    q2 = PSQuantizer(SignSGDCompressor, params, make_args(gq_graph=False))
    for p, gr in zip(params, grads):
        p.grad = gr.clone()
    q2.record(0, 0)
    torch.cuda.synchronize()
    assert torch.equal(q2._wire[0].cpu(), wires[0])


@pytest.mark.timeout(300)
def test_training_loop_with_moving_gradients_replays_address_free():
    """driver.FCN trained with the sign quantizer, gradients at new addresses every step: the address-free graphs replay."""
    from gq_amd.compressors import SignSGDCompressor
    from gq_amd.driver import FCN
    from gq_amd.quantizers import PSQuantizer
    torch.manual_seed(0)
    model = FCN().cuda()
    q = PSQuantizer(SignSGDCompressor, model.parameters(), make_args())
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    x = torch.randn(32, 784, device="cuda")
    y = torch.randint(0, 10, (32,), device="cuda")
    hold = []
    for it in range(12):
        opt.zero_grad(set_to_none=True)
        hold.append(torch.empty(1 + 4096 * it, device="cuda"))      # (kept alive: the next gradients land elsewhere)
        torch.nn.functional.cross_entropy(model(x), y).backward()
        q.record(0, 0)
        q.apply()
        opt.step()
    torch.cuda.synchronize()
    p = q.record_paths
    replayed = p["graph"] + p["whole_step"] + p["graph_any_address"] + p["whole_step_any_address"]
    assert p["eager"] <= 3 and replayed >= 9, p
    assert p["graph_any_address"] + p["whole_step_any_address"] >= 1, p
    assert [g[0].__name__ for g in q._groups] == ["BatchedSign"]
    assert all(torch.isfinite(t).all() for t in model.parameters())


@pytest.mark.timeout(600)
def test_train_py_runs_sign():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--quantizer", "sign", "--network", "fcn", "--dataset", "mnist",
           "--num-users", "2", "--epochs", "1", "--train-size", "1024", "--log-interval", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    losses = [rec["loss"] for rec in recs if "loss" in rec]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode,ef", [("ps", True), ("ring", False)])
def test_two_ranks_on_one_gpu_equal_single_process(tmp_path, mode, ef):
    """Two ranks (two local users each) exchange the 2-bit wire over gloo on cuda:0; == four users in one process, bit for bit."""
    script = os.path.join(HERE, "_dist_worker_sign.py")
    out = str(tmp_path / "res")
    port = 31700 + (os.getpid() % 1500) + (0 if mode == "ps" else 5) + (11 if ef else 0)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    procs = [subprocess.Popen([sys.executable, script, str(r), "2", out, mode, "1" if ef else "0"], env=env) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    for k in r0.files:
        assert np.array_equal(r0[k].view(np.uint32), r1[k].view(np.uint32)), "ranks disagree on " + k
    sys.path.insert(0, HERE)
    import _dist_worker_sign as w
    single = w.run_single_process(4, mode, ef)
    assert sorted(single) == sorted(r0.files)
    for k in single:
        assert np.array_equal(single[k].view(np.uint32), r0[k].view(np.uint32)), k
