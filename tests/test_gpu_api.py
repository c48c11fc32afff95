"""GPU tests of the reference-shaped Python API (Compressor / Quantizer classes) running on
the HIP kernels: signatures and results against the golden vectors captured from the reference."""
import contextlib
import glob
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _capture(graph):
    """torch.cuda.graph(graph) with the garbage collector held off: a CUDAGraph of an earlier test that the collector finalizes
    INSIDE a capture raises in its destructor and takes the process down (see gq_amd.quantizers._capturing)."""
    import gc
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield
    finally:
        if was:
            gc.enable()

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
HSQ_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "hsq_*.npz")))
QSGD_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "qsgd_*.npz")))
PSQ = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "psq_*.npz")))
RING = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "ring_*.npz")))


@pytest.fixture(scope="module", autouse=True)
def _env():
    os.environ["GQ_CODEBOOK_DIR"] = os.path.join(GOLDEN, "codebooks")
    assert torch.cuda.is_available()
    yield


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp",
                num_users=4, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """Bitwise equal, except that any NaN equals any NaN (sign / payload of a NaN are not part of the contract:
    x86 generates -qNaN, gfx950 +qNaN)."""
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _args_for(g, name):
    d, K = int(g["dim"]), int(g["K"]) if "K" in g.files else 0
    kw = dict(n_bit=int(g["n_bit"]), random=int(g["random"]), gq_rng="reference")
    if name.startswith("hsq"):
        kw["k_bit"] = int(np.log2(K))
        kw["c_dim"] = {"hsq_d24_k64_repair_det": 16, "hsq_d24_k256_repair_det": 16, "hsq_d12_k256_repair_det": 8, "hsq_d12_k32_repair_rand": 8}.get(name, d)
    return make_args(**kw)


@pytest.mark.parametrize("name", HSQ_CASES)
def test_nearest_neighbor_compressor_signature_and_values(name):
    from gq_amd.compressors import NearestNeighborCompressor
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    args = _args_for(g, name)
    x = torch.from_numpy(g["x"]).cuda()
    comp = NearestNeighborCompressor(x.numel(), x.shape, args)
    assert comp.dim == int(g["dim"]) and comp.K == int(g["K"])
    if args.random:
        # reference-parity RNG: the same CPU draw the fixture recorded
        seeds = {"hsq_randn_s1_rand": 4321, "hsq_randn_s1_n2_rand": 99, "hsq_randn_s1e-3_rand": 777,
                 "hsq_small_48_rand": 5, "hsq_zeros_rand": 1, "hsq_constant_u_rand": 2, "hsq_d8_k256_rand": 11,
                 "hsq_d12_k256_rand": 61, "hsq_d24_k256_rand": 62, "hsq_d16_k64_rand": 71, "hsq_d12_k32_repair_rand": 72}
        torch.manual_seed(seeds[name])
    sig = comp.compress(x)
    norms, codes = sig
    assert isinstance(sig, list) and codes.dtype == (torch.uint8 if comp.K <= 256 else torch.int32)
    assert np.array_equal(codes.cpu().numpy(), g["codes"])
    if x.numel() // comp.dim == 1:
        return  # M == 1: MKL sgemv deviation (test_oracle_golden.py)
    if args.n_bit == 32:
        assert _same(norms.cpu().numpy(), g["u"])
    else:
        lb, ub, levels = norms
        assert lb.dim() == 0 and ub.dim() == 0 and levels.dtype == torch.int32
        assert _same(lb.item(), g["lb"]) and _same(ub.item(), g["ub"])
        assert np.array_equal(levels.cpu().numpy(), g["levels"])
    dec = comp.decompress(sig)
    assert dec.shape == x.shape and dec.device == x.device
    assert _same(dec.cpu().numpy(), g["decoded"])
    if not args.random and args.n_bit != 32:
        rt = comp.roundtrip(x)
        if np.isfinite(g["x"]).all():
            assert torch.equal(rt, dec)
        else:
            # the wire carries byte levels, which cannot hold the reference's level INT_MIN of an infinite projection:
            # the 16 values of that subvector decode to NaN instead of +-inf (known deviations); every value
            # that is not finite in the reference is not finite here, and vice versa
            assert np.array_equal(np.isfinite(rt.cpu().numpy()), np.isfinite(g["decoded"]))


@pytest.mark.parametrize("name", QSGD_CASES)
def test_qsgd_compressor_signature_and_values(name):
    from gq_amd.compressors import QSGDCompressor
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    c_dim = {"qsgd_repair_1728_rand": 128, "qsgd_cdim0_n1_rand": 0}.get(name, int(g["dim"]))
    args = make_args(c_dim=c_dim, n_bit=int(g["n_bit"]), random=int(g["random"]), gq_rng="reference")
    x = torch.from_numpy(g["x"]).cuda()
    comp = QSGDCompressor(x.numel(), x.shape, args)
    assert comp.dim == int(g["dim"])
    seeds = {"qsgd_d128_n2_rand": 31, "qsgd_d128_n4_rand": 32, "qsgd_repair_1728_rand": 33, "qsgd_cdim0_n1_rand": 34}
    if args.random:
        torch.manual_seed(seeds[name])
    norm, signs, l = comp.compress(x)
    assert norm.shape == (comp.M, 1) and signs.dtype == torch.bool and l.dtype == torch.int32
    assert signs.shape == x.shape and l.shape == x.shape
    assert _same(norm.cpu().numpy(), g["norm"])        # NaN-propagating bucket norm (torch.max, qsgd_compressor.py:49)
    assert np.array_equal(signs.cpu().numpy(), g["signs"])
    assert np.array_equal(l.cpu().numpy(), g["levels"])
    dec = comp.decompress([norm, signs, l])
    assert np.array_equal(dec.cpu().numpy(), g["decoded"], equal_nan=True)
    if not np.isfinite(g["x"]).all():
        # the same buckets are NaN through the packed multi-tensor wire (a byte code cannot hold the reference's level
        # INT_MIN, so an infinite element decodes to NaN instead of +-inf: finite / not finite is what is compared)
        from gq_amd.quantizers import Quantizer
        ps = [torch.nn.Parameter(torch.zeros(x.shape, device="cuda")), torch.nn.Parameter(torch.zeros(2048, device="cuda"))]
        q = Quantizer(QSGDCompressor, ps, make_args(c_dim=c_dim, n_bit=int(g["n_bit"]), random=0, num_users=1))
        ps[0].grad, ps[1].grad = x.clone(), torch.ones(2048, device="cuda")
        q.record(0, epoch=1)
        q.apply()
        assert q._groups and q._groups[0][2].ready
        assert np.array_equal(np.isfinite(ps[0].grad.cpu().numpy()), np.isfinite(g["decoded"]))


def test_probabilistic_scalar_compressor_standalone(oracle):
    from gq_amd.compressors import ProbabilisticScalarCompressor
    rng = np.random.RandomState(8)
    v = rng.standard_normal(100001).astype(np.float32)
    r = rng.random_sample(100001).astype(np.float32)
    for random in (0, 1):
        c = ProbabilisticScalarCompressor(5, make_args(random=random, gq_rng="reference"))
        if random:
            torch.manual_seed(77)
            r = torch.rand(100001).numpy()
            torch.manual_seed(77)
        lb, ub, l = c.compress(torch.from_numpy(v).cuda())
        elb, eub, el = oracle.scalar_levels(v, 5, random, r)
        assert _bits(lb.item()) == _bits(elb) and _bits(ub.item()) == _bits(eub)
        assert np.array_equal(l.cpu().numpy(), el)
        dec = c.decompress((lb, ub, l)).cpu().numpy()
        # mul, then / 2^n (exact), then add: three separately rounded torch kernels, like the reference's CPU ops
        assert np.array_equal(_bits(dec), _bits(oracle.scalar_decode(el, 5, elb, eub)))


def test_device_rng_default_is_unbiased_and_seeded():
    from gq_amd.compressors import NearestNeighborCompressor
    x = torch.randn(16 * 50000, device="cuda")
    comp = NearestNeighborCompressor(x.numel(), x.shape, make_args(random=1))
    torch.manual_seed(5)
    a = comp.compress(x)
    b = comp.compress(x)
    assert torch.equal(a[1], b[1]) and not torch.equal(a[0][2], b[0][2])   # fresh draws every call
    det = NearestNeighborCompressor(x.numel(), x.shape, make_args(random=0)).compress(x)
    diff = (a[0][2] - det[0][2])
    assert int(diff.min()) >= 0 and int(diff.max()) <= 1 and 0.3 < float(diff.float().mean()) < 0.7


@pytest.mark.parametrize("name", PSQ)
def test_psquantizer_on_gpu_matches_reference(name):
    from test_host_logic import run_psq_fixture
    q = run_psq_fixture(name, None, device="cuda", tol=0.0)
    assert q.codecs[0].__class__.__name__ in ("HSQCodec", "QSGDCodec") or name.endswith("_sgd")
    if "_rand" in name and "qsgd" not in name:     # the reference's own draws, through the multi-tensor kernels (gq_hsq_levels_batched's r_flat)
        assert q._groups and q._groups[0][2].ready and q._groups[0][2].reference_draws


@pytest.mark.parametrize("name", PSQ)
def test_psquantizer_on_gpu_with_packed6_levels_matches_reference(name, monkeypatch):
    """GQ_WIRE_LEVELS=packed6: wherever the configuration allows it (d = 16, K <= 256, top level <= 63) the levels travel
    as four 6-bit values per three bytes; the aggregates (and error-feedback residuals) still equal the reference's
    fixtures at tolerance 0 -- record, error feedback, two-phase round trips, the ring's plain decodes."""
    from test_host_logic import run_psq_fixture
    monkeypatch.setenv("GQ_WIRE_LEVELS", "packed6")
    q = run_psq_fixture(name, None, device="cuda", tol=0.0)
    packed = [c for c in q.codecs if getattr(c, "packed6", False)]
    if name in ("psq_fcn_u4_det", "psq_fcn_u4_ef", "psq_fcn_u4_ef_twophase", "psq_fcn_u4_twophase"):      # d16 k8 n6, deterministic levels
        assert packed, "no tensor of %s took the packed form" % name
    for c in packed:
        assert c.nbytes < c.M * 2 + 16 + 32


def test_resnet50_list_with_packed6_levels_equals_the_byte_wire(monkeypatch):
    """The ResNet-50 parameter list (76 codebook-compressed tensors) through the multi-tensor kernels, two users, with
    and without packed levels: same aggregates bit for bit, 12 % fewer wire bytes; error feedback + two-phase too."""
    import json
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    shapes = json.load(open(os.path.join(GOLDEN, "resnet50_cifar_shapes.json")))["parameter_shapes"]
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    grads = [[torch.randn(s, device=dev) * 1e-3 for s in shapes] for _ in range(2)]
    for ef, two_phase in ((False, False), (True, True)):
        outs, sizes = [], []
        for mode in ("bytes", "packed6"):
            monkeypatch.setenv("GQ_WIRE_LEVELS", mode)
            params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]
            q = Quantizer(NearestNeighborCompressor, params, make_args(c_dim=16, k_bit=8, n_bit=6, random=0, num_users=2, ef=ef,
                                                                       two_phase=two_phase))
            for step in range(2):
                for u in range(2):
                    for p, gr in zip(params, grads[u]):
                        p.grad = gr.clone()
                    q.record(u, epoch=1)
                q.apply()
            assert q._groups and q._groups[0][2].ready
            outs.append([p.grad.data.clone() for p in params] + ([e.clone() for p in params for e in p.error] if ef else []))
            sizes.append(q.wire_bytes_per_user())
        assert sizes[1] < 0.9 * sizes[0], sizes
        for a, b in zip(*outs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "psqd_*.npz"))))
def test_psquantizer_full_parameter_lists_match_reference_digests_on_gpu(name):
    """The real FCN / ResNet-50 parameter lists (161 tensors, 23.5 M elements, two users) through the multi-tensor HIP
    kernels: codes, levels, (lb, ub) of every tensor and user read back from the wire, and every aggregate, equal the
    reference's digests (tests/golden/psqd_*.npz) -- bit for bit by construction of a digest."""
    from test_host_logic import run_psq_digest_fixture

    def signature_of(q, u, i, x):
        codec = q.codecs[i]
        codes, levels, lb_ub = codec._views(q._wire[u], q.offsets[i])
        lb_ub = lb_ub.cpu().numpy()
        return codes.cpu().numpy(), levels.cpu().numpy(), lb_ub[0], lb_ub[1]
    q = run_psq_digest_fixture(name, None, "cuda", signature_of)
    if "qsgd" not in name and "terngrad" not in name:     # QSGD with the reference's draws: per-tensor launches
        assert q._groups and q._groups[0][2].ready


HSQD = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "hsqd_*.npz")))


@pytest.mark.parametrize("name", HSQD)
def test_compressor_at_baseline_size_matches_reference_digests(name):
    """BASELINE configs[1] through the compressor class on the GPU: 25 M float32, c_dim 16 / k_bit 8 / n_bit 6 (with and
    without the reference's stochastic rounding draws), and K = 1024 / 4096 on 4 M / 2 M elements (the fused paged
    prefilter) -- codes, levels, (lb, ub) and the decompressed tensor hash to the digests of the reference's own output."""
    import hashlib
    from gq_amd.compressors import NearestNeighborCompressor
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x = (np.random.RandomState(int(g["seed"])).standard_normal(int(g["n"])) * float(g["scale_in"])).astype(np.float32)
    assert sha(x) == str(g["x_sha"])
    K = int(g["K"])
    comp = NearestNeighborCompressor(x.size, x.shape, make_args(n_bit=int(g["n_bit"]), random=int(g["random"]), gq_rng="reference",
                                                                k_bit=int(np.log2(K))))
    if "seed_r" in g.files:
        torch.manual_seed(int(g["seed_r"]))
    (lb, ub, l), codes = comp.compress(torch.from_numpy(x).cuda())
    dec = comp.decompress([(lb, ub, l), codes])
    assert sha(codes.cpu().numpy().astype(np.uint8 if K <= 256 else np.int32)) == str(g["codes_sha"])
    assert sha(l.cpu().numpy().astype(np.int32)) == str(g["levels_sha"])
    assert _same(np.array([lb.item(), ub.item()], np.float32), g["lbub"])
    assert sha(dec.cpu().numpy()) == str(g["decoded_sha"])


TRAJ = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "traj_*.npz")))


@pytest.mark.parametrize("name", TRAJ)
def test_training_iterations_follow_the_reference_trajectory(name):
    """The caller of the path, main.py:216-233: a few whole iterations of the reference's FCN (forward, backward,
    record per user, apply, SGD step) -- here the model runs on the GPU through gq_amd.driver.one_iter and the HIP
    quantizer, the fixture holds the reference's CPU run (tests/golden/make_golden.py: trajectory_case).  The
    quantizer is bit-exact on equal inputs (psq_* fixtures); the inputs are not equal here -- GPU matmuls round
    differently from MKL -- so this is a tolerance-level pin: losses to 1e-5, the weight UPDATE after one and after all
    iterations to 1e-3 in relative L2 (measured on MI355X: 1e-7 and 3e-7 ... 7e-7 -- no code or level differs; one
    argmax flipped by a last-bit difference would move a 16-element subvector and show up as ~1e-2)."""
    import hashlib
    from gq_amd import driver
    from gq_amd.compressors import NearestNeighborCompressor, QSGDCompressor
    from gq_amd.quantizers import Quantizer
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    users, iters, batch, seed, hidden = (int(g[k]) for k in ("users", "iters", "batch", "seed", "hidden"))
    kw = {"traj_fcn_hsq_u2_rand": dict(random=1), "traj_fcn_hsq_u2_ef2p": dict(random=0, ef=True, two_phase=True),
          "traj_fcn_qsgd_u3": dict(random=0, c_dim=128, n_bit=2)}[name]
    comp = QSGDCompressor if "qsgd" in name else NearestNeighborCompressor

    class FCN(torch.nn.Module):          # the constructor order of models/fcn.py: the same draws initialise it
        def __init__(self):
            super().__init__()
            self.linear1 = torch.nn.Linear(784, hidden)
            self.linear2 = torch.nn.Linear(hidden, 10)

        def forward(self, x):
            return self.linear2(self.linear1(x.view(-1, 784)).clamp(min=0))

    torch.manual_seed(seed)
    model = FCN()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.cuda()
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((iters, users, batch, 1, 28, 28)).astype(np.float32)
    y = rng.randint(0, 10, size=(iters, users, batch)).astype(np.int64)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    assert sha(x) == str(g["x_sha"]) and sha(y) == str(g["y_sha"])
    q = Quantizer(comp, model.parameters(), make_args(num_users=users, gq_rng="reference", **kw))
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-4)
    loss_func = torch.nn.CrossEntropyLoss()
    if "seed_r" in g.files:
        torch.manual_seed(int(g["seed_r"]))

    def update_error(prefix):
        num = den = 0.0
        for k, v in model.state_dict().items():
            want = torch.from_numpy(g[prefix + k]) - init[k]
            got = v.cpu() - init[k]
            num += float((got - want).double().pow(2).sum())
            den += float(want.double().pow(2).sum())
        return (num / den) ** 0.5

    losses = []
    for it in range(iters):
        data = [(torch.from_numpy(x[it, u]).cuda(), torch.from_numpy(y[it, u]).cuda()) for u in range(users)]
        losses.append(float(driver.one_iter(model, loss_func, opt, q, data, epoch=1)))
        if it == 0:
            e1 = update_error("w1_")
    eN = update_error("w_")
    print(name, "loss error", np.abs(np.array(losses) / g["losses"] - 1).max(), "update error", e1, eN)
    assert np.allclose(losses, g["losses"], rtol=1e-5)
    assert e1 < 1e-3 and eN < 1e-3


@pytest.mark.parametrize("name", RING)
def test_ring_quantizer_on_gpu_matches_reference(name):
    """quantizers/ring_quantizer.py on the HIP path (batched kernels, fused error feedback)."""
    from test_host_logic import run_psq_fixture
    q = run_psq_fixture(name, None, device="cuda", tol=0.0)
    assert type(q).__name__ == "RingQuantizer" and q._groups and q._groups[0][2].ready


def test_psquantizer_bit_exact_single_phase():
    """No EF, one phase: the aggregate is bit-identical to the reference's."""
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    g = np.load(os.path.join(GOLDEN, "psq_fcn_u4_det.npz"))
    U, P = int(g["users"]), int(g["n_params"])
    params = [torch.nn.Parameter(torch.zeros(*g["grad_s0_u0_p%d" % i].shape, device="cuda")) for i in range(P)]
    q = Quantizer(NearestNeighborCompressor, params, make_args(num_users=U))
    for u in range(U):
        for i, p in enumerate(params):
            p.grad = torch.from_numpy(g["grad_s0_u%d_p%d" % (u, i)].copy()).cuda()
        q.record(u, epoch=1)
    q.aggregate()
    for i, p in enumerate(params):
        assert np.array_equal(_bits(p.grad.data.cpu().numpy()), _bits(g["agg_s0_p%d" % i]))
    assert q.wire_bytes_per_user() < sum(p.numel() for p in params) * 4 / 20    # >20x smaller than fp32


def test_psquantizer_more_records_than_num_users_and_partial():
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    p = torch.nn.Parameter(torch.zeros(64, 64, device="cuda"))
    q = Quantizer(NearestNeighborCompressor, [p], make_args(num_users=2))
    comp = NearestNeighborCompressor(4096, p.shape, make_args())
    decs = []
    for u in range(3):     # one more than num_users: the wire grows
        gr = torch.randn(64, 64, device="cuda")
        decs.append(comp.roundtrip(gr))
        p.grad = gr
        q.record(u % 2, epoch=1)
    q.apply()
    # the reference's CPU arithmetic: sequential sum, then a true division (torch's GPU mean
    # multiplies by 1/N instead, which differs in the last bit for N = 3)
    want = torch.stack([d.cpu() for d in decs], 0).mean(0)
    assert torch.equal(p.grad.data.cpu(), want)
    q.apply()  # nothing recorded: no-op
    assert torch.equal(p.grad.data.cpu(), want)


def test_nccl_single_rank_group_path():
    """world_size 1 over RCCL: the process-group branch is exercised end to end on one GPU."""
    import torch.distributed as dist
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29611")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        p = torch.nn.Parameter(torch.zeros(128, 64, device="cuda"))
        q = Quantizer(NearestNeighborCompressor, [p], make_args(num_users=1))
        gr = torch.randn(128, 64, device="cuda")
        p.grad = gr.clone()
        q.record(0, epoch=1)
        q.apply()
        comp = NearestNeighborCompressor(8192, p.shape, make_args())
        assert torch.equal(p.grad.data, comp.roundtrip(gr))
    finally:
        dist.destroy_process_group()


def test_kernels_launch_on_pytorch_current_stream():
    """The library takes the stream PyTorch would launch on (raw handle), also inside a stream context."""
    from gq_amd import native
    assert (native._stream().value or 0) == torch.cuda.current_stream().cuda_stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert native._stream().value == side.cuda_stream
        x = torch.randn(4096 * 16, device="cuda")
        from gq_amd.compressors import NearestNeighborCompressor
        comp = NearestNeighborCompressor(x.numel(), x.shape, make_args())
        y = comp.decompress(comp.compress(x))
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(y, comp.decompress(comp.compress(x)))


RESNET50_COMPRESSED = ([(64, 3, 3, 3)] + [(64, 64, 1, 1), (64, 64, 3, 3), (256, 64, 1, 1)] * 2 + [(1024,)] * 4
                       + [(128, 256, 1, 1), (128, 128, 3, 3), (512, 128, 1, 1), (512, 256, 1, 1)]
                       + [(256, 512, 1, 1), (256, 256, 3, 3), (1024, 256, 1, 1), (2048,)]
                       + [(512, 1024, 1, 1), (512, 512, 3, 3), (2048, 512, 1, 1), (2048, 1024, 1, 1)])
RESNET50_SMALL = [(64,), (64,), (256,), (256,), (128,), (512,), (10, 64), (10,)]


def _run_quantizer(shapes, users, seed, grad_scale=1e-2, **argkw):
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    params = [torch.nn.Parameter(torch.zeros(*s, device="cuda")) for s in shapes]
    q = Quantizer(NearestNeighborCompressor, params, make_args(num_users=users, **argkw))
    g = torch.Generator(device="cuda").manual_seed(seed)
    for st in range(2):
        for u in range(users):
            for p in params:
                p.grad = torch.randn(p.shape, device="cuda", generator=g) * grad_scale
            q.record(u, epoch=1)
        q.apply()
    return q, [p.grad.data.clone() for p in params]


@pytest.mark.parametrize("c_dim", [16, 32])
def test_many_small_tensors_in_one_workgroups_run_equal_per_tensor_path(c_dim):
    """The multi-tensor encodes fold (min, max) per workgroup in a 64-tensor table in LDS, tensors beyond it straight into
    the global words (hsq_encode_pf.hip / hsq_encode_pfd.hip, s_mm).  150 one-tile tensors in front of a 20 M-element one:
    the first workgroup's run of ~76 tiles covers 76 tensors -- 64 through the table, the rest through the fallback -- and the
    big tensor is met by every other workgroup.  Wire (codes, levels, lb / ub) and aggregate equal the per-tensor kernels."""
    shapes = [(64 * c_dim,)] * 150 + [(19531 * 64 * c_dim,)] + [(64 * c_dim,)] * 3
    qb, gb = _run_quantizer(shapes, 1, 5, c_dim=c_dim)
    qp, gp = _run_quantizer(shapes, 1, 5, c_dim=c_dim, gq_no_batch=True)
    assert qb._groups and qb._groups[0][2].ready and not qp._groups
    assert torch.equal(qb._wire, qp._wire)
    for a, b in zip(gb, gp):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("kw", [dict(), dict(c_dim=32, n_bit=8), dict(c_dim=8), dict(users=3), dict(ef=True),
                                dict(quant="qsgd", c_dim=128, n_bit=2), dict(quant="qsgd", c_dim=128, n_bit=2, users=2), dict(quant="qsgd", c_dim=0, n_bit=1)])
def test_step_tail_in_the_decode_launch_equals_a_launch_of_its_own(monkeypatch, kw):
    """gq_hsq_decode_sum_batched_tail: the dense tensors' mean, the step of the draws' { seed, step } words and (whole-step
    graphs) the accumulators' reset ride in the decode-mean launch by default; $GQ_STEP_TAIL=0 keeps gq_mean_rows as a launch
    of its own.  Eight steps with stochastic rounding on the device draws (graphs are captured on the way): the same
    gradients bit for bit, i.e. the same means AND the same sequence of draws."""
    from gq_amd import native
    from gq_amd.compressors import NearestNeighborCompressor, QSGDCompressor
    from gq_amd.quantizers import Quantizer
    kw = dict(kw)
    users = kw.pop("users", 1)
    Comp = QSGDCompressor if kw.pop("quant", "hsq") == "qsgd" else NearestNeighborCompressor
    shapes = RESNET50_COMPRESSED[:7] + RESNET50_SMALL[:4]

    def run(tail, fuse_levels=False):
        monkeypatch.setenv("GQ_STEP_TAIL", "1" if tail else "0")
        monkeypatch.setenv("GQ_FUSE_LEVELS", "1" if fuse_levels else "0")      # (under error feedback the step keeps its level launch and its decode either way)
        torch.manual_seed(77)
        from gq_amd import compressors
        compressors._seed_counter[0] = 0      # (the pairs' seeds come from torch's seed and a per-process call counter)
        params = [torch.nn.Parameter(torch.zeros(*s, device="cuda")) for s in shapes]
        q = Quantizer(Comp, params, make_args(num_users=users, random=1, **kw))
        g = torch.Generator(device="cuda").manual_seed(5)
        inputs = [[[torch.randn(p.shape, device="cuda", generator=g) * 1e-2 for p in params] for _ in range(users)] for _ in range(2)]
        outs, calls, bufs = [], 0, {}
        for st in range(8):
            c0 = native.CALLS[0]
            for u in range(users):
                for p, x in zip(params, inputs[st % 2][u]):
                    if st == 0:
                        p.grad = x.clone()
                    else:
                        p.grad.data = bufs[id(p)]      # apply() rebinds .grad.data to the mean: back to the parameter's own buffer,
                        p.grad.data.copy_(x)           # as autograd writes into the same storage every step (graphs need recurring addresses)
                    if st == 0:
                        bufs[id(p)] = p.grad.data
                q.record(u, epoch=1)
            q.apply()
            calls = native.CALLS[0] - c0
            outs.append([p.grad.data.clone() for p in params])
        return outs, calls, q
    with_tail, calls_tail, q1 = run(True)
    own_launch, calls_own, q0 = run(False)
    for a, b in zip(with_tail, own_launch):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(q1._rng_state, q0._rng_state) and int(q1._rng_state[0, 1]) == 8      # one step per aggregate either way
    # ... and the one-rank step's two-kernel form (gq_hsq_levels_decode_batched: level launch + decode of the payload + tail as
    # ONE launch in the whole-step graph; one user only): the same gradients, the same sequence of draws, the wire complete
    fused, calls_fused, q2 = run(True, fuse_levels=True)
    for a, b in zip(fused, own_launch):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(q2._rng_state, q0._rng_state) and torch.equal(q2._wire, q0._wire)
    if users == 1:
        assert any(e[1] is not None for e in q2._step_graphs.values()), "no whole-step graph was captured"
        assert int(q2._ticket.abs().sum()) == 0                                                  # the ticket counters are back at zero
        if kw.get("ef"):
            for p2, p0 in zip(q2.parameters, q0.parameters):
                assert torch.equal(p2.error[0], p0.error[0])


def test_batched_quantizer_equals_per_tensor_path():
    """One launch for all tensors (segment table) == the per-tensor kernels, bit for bit."""
    shapes = RESNET50_COMPRESSED + RESNET50_SMALL
    qb, gb = _run_quantizer(shapes, 3, 7)
    qp, gp = _run_quantizer(shapes, 3, 7, gq_no_batch=True)
    assert qb._groups and qb._groups[0][2] is not None and qb._groups[0][2].ready and not qp._groups
    assert len(qb.batch_idx) == len(RESNET50_COMPRESSED)
    for a, b, s in zip(gb, gp, shapes):
        assert a.shape == torch.Size(s)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), s
    # and the wire itself is identical (codes, levels, lb/ub, dense region)
    assert torch.equal(qb._wire, qp._wire)


@pytest.mark.parametrize("users,kw", [(5, {}), (8, {}), (8, dict(gq_wire_levels="packed6")), (11, {}), (16, dict(gq_wire_levels="packed6")),
                                      (19, {})])
def test_batched_quantizer_many_users_equal_per_tensor_path(users, kw):
    """The multi-tensor decode-mean for every payload count: compile-time-R pipelined kernels up to 8 (768-thread workgroups
    from 6 on), the chunked form above, byte and packed 6-bit levels -- against the per-tensor kernels, bit for bit."""
    shapes = RESNET50_COMPRESSED[:10] + RESNET50_SMALL[:3]
    qb, gb = _run_quantizer(shapes, users, 23, **kw)
    qp, gp = _run_quantizer(shapes, users, 23, gq_no_batch=True, **kw)
    assert qb._groups and qb._groups[0][2].ready and not qp._groups
    for a, b, s in zip(gb, gp, shapes):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), s
    assert torch.equal(qb._wire, qp._wire)


@pytest.mark.parametrize("users", [3, 5, 7, 9, 17])
@pytest.mark.parametrize("grad_scale", [1e-39, 8e37])
def test_batched_quantizer_odd_user_counts_at_the_ends_of_the_float_range(users, grad_scale):
    """The mean over an odd number of users is a four-operation quotient by the constant (csrc/gq_common.hpp): sums that are
    subnormal (gradients of 1e-39) and sums that overflow (8e37 times a few users: +-inf) through the multi-tensor kernels,
    against the per-tensor ones (which tests/test_gpu_kernels.py holds against the oracle's true division)."""
    shapes = RESNET50_COMPRESSED[:6] + RESNET50_SMALL[:2]
    qb, gb = _run_quantizer(shapes, users, 31, grad_scale=grad_scale)
    qp, gp = _run_quantizer(shapes, users, 31, grad_scale=grad_scale, gq_no_batch=True)
    assert qb._groups and qb._groups[0][2].ready and not qp._groups
    for a, b, s in zip(gb, gp, shapes):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), s
    big = torch.cat([a.reshape(-1) for a in gb])
    if grad_scale < 1:
        assert (big != 0).any() and big.abs().max() < 1.2e-38          # subnormal means, not flushed
    elif users >= 9:
        assert torch.isinf(big).any()


@pytest.mark.parametrize("c_dim", [32, 8])
def test_batched_quantizer_other_subdimensions_equal_per_tensor_path(c_dim):
    """The multi-tensor kernels for the other prefilter sub-dimensions (main.py's default --c-dim 32, and 8):
    aggregates, wire, per-user residuals and the server residual identical to the per-tensor kernels."""
    shapes = RESNET50_COMPRESSED[:14] + RESNET50_SMALL[:3]
    qb, gb = _run_quantizer(shapes, 2, 11, c_dim=c_dim)
    qp, gp = _run_quantizer(shapes, 2, 11, c_dim=c_dim, gq_no_batch=True)
    assert qb._groups and qb._groups[0][2] is not None and qb._groups[0][2].ready and not qp._groups
    assert qb._groups[0][2].codebook.shape == (256, c_dim)
    for a, b, s in zip(gb, gp, shapes):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), s
    assert torch.equal(qb._wire, qp._wire)
    # error feedback / two-phase ride in the same launches for these dimensions too
    for kw in (dict(ef=True), dict(ef=True, two_phase=True, scale="0.5")):
        qe, ge = _run_quantizer(shapes, 2, 11, c_dim=c_dim, **kw)
        qf, gf = _run_quantizer(shapes, 2, 11, c_dim=c_dim, gq_no_batch=True, **kw)
        assert qe._groups[0][2].ready
        for a, b in zip(ge, gf):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        for pb, pp in zip(qe.parameters, qf.parameters):
            for eb, ep in zip(pb.error, pp.error):
                assert torch.equal(eb, ep)
            if kw.get("two_phase"):
                assert torch.equal(pb.server_error, pp.server_error)


@pytest.mark.parametrize("c_dim,repaired", [(16, 24), (8, 12)])
def test_repaired_dimensions_run_on_the_prefilter_kernels_and_equal_the_reference(c_dim, repaired, oracle):
    """nearest_neighbor_compressor.py:23-29: a tensor whose size --c-dim does not divide gets c_dim * 3 / 2 (16 -> 24, 8 -> 12).
    Round 6: K = 256 with d = 12 / 24 runs on the f16 prefilter encode (rows of 12 / 24 floats through the d = 16 / 32 kernels, the
    missing elements zeros) instead of the exact f32 MFMA kernel -- multi-tensor and per-tensor forms, error feedback and
    two-phase included -- and the wire's codes and projections equal the oracle's, bit for bit."""
    from gq_amd import native
    from gq_amd.quantizers import BatchedHSQ
    shapes = [(repaired * 501,), (repaired, 3, 43), (c_dim * 1024,), (repaired * 64 * 9 + repaired,), (c_dim, 130), (10,), (repaired * 3,), (64,)]
    assert all(int(np.prod(s)) % c_dim != 0 or i in (2, 4, 7) for i, s in enumerate(shapes))
    qb, gb = _run_quantizer(shapes, 2, 13, c_dim=c_dim)
    qp, gp = _run_quantizer(shapes, 2, 13, c_dim=c_dim, gq_no_batch=True)
    dims = sorted({c.c.dim for c in qb.codecs if hasattr(c, "c")})
    assert dims == [c_dim, repaired], dims
    grp = [g[2] for g in qb._groups if isinstance(g[2], BatchedHSQ) and g[2].codecs[0].c.dim == repaired]
    assert grp and grp[0].ready and grp[0]._batch.path == native.BATCH_PREFILTER and not qp._groups
    for a, b, sh in zip(gb, gp, shapes):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), sh
    assert torch.equal(qb._wire, qp._wire)
    # codes and lb / ub of every repaired tensor on the wire against the oracle (one user's last record)
    g = torch.Generator(device="cuda").manual_seed(13)
    grads = [[[torch.randn(sh, device="cuda", generator=g) * 1e-2 for sh in shapes] for _ in range(2)] for _ in range(2)][1]
    cbn = qb.codecs[0].c._codebook_on(torch.device("cuda:0")).cpu().numpy()
    for u in range(2):
        for i, sh in enumerate(shapes):
            cd = qb.codecs[i]
            if not hasattr(cd, "c") or cd.c.dim != repaired:
                continue
            codes, levels, lb_ub = cd._views(qb._wire[u], qb.offsets[i])
            ref = oracle.hsq_compress(grads[u][i].cpu().numpy().reshape(-1), cd.c._codebook_on(torch.device("cuda:0")).cpu().numpy(), 6, 0)
            assert np.array_equal(codes.cpu().numpy().astype(np.int32), ref["codes"]), (u, sh)
            assert np.array_equal(levels.cpu().numpy().astype(np.int32), ref["levels"]), (u, sh)
            assert _bits(lb_ub[0].item()) == _bits(ref["lb"]) and _bits(lb_ub[1].item()) == _bits(ref["ub"])
    for kw in (dict(ef=True), dict(ef=True, two_phase=True, scale="0.5"), dict(random=1, gq_rng="reference")):
        torch.manual_seed(99)      # (gq_rng = "reference": the draws are torch.rand's, per tensor in parameter order)
        qe, ge = _run_quantizer(shapes, 2, 13, c_dim=c_dim, **kw)
        torch.manual_seed(99)
        qf, gf = _run_quantizer(shapes, 2, 13, c_dim=c_dim, gq_no_batch=True, **kw)
        for a, b in zip(ge, gf):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        if kw.get("ef"):
            for pb, pp in zip(qe.parameters, qf.parameters):
                for eb, ep in zip(pb.error, pp.error):
                    assert torch.equal(eb, ep)


def _shapes_for(d):
    """Tensors whose sizes the sub-dimension d divides (no repair), with ragged last tiles, plus identity ones."""
    return [(d, 130), (3 * d, 3, 3, 7), (d * 1000 + d,), (d * 64,), (d, 64, 9), (2 * d, 77), (10,), (64,), (d * 20 + d,)]


def _write_unit_codebook(root, d, K, seed):
    """A synthetic codebook file in the reference's format and place (./codebooks/learned_codebook/...)."""
    rng = np.random.default_rng(seed)
    cb = rng.standard_normal((K, d)).astype(np.float32)
    rows = np.empty((K, d + 1), dtype="<i4")
    rows[:, 0] = d
    rows[:, 1:] = cb.view("<i4")
    path = os.path.join(root, "codebooks", "learned_codebook")
    os.makedirs(path, exist_ok=True)
    rows.tofile(os.path.join(path, "angular_dim_%d_Ks_%d.fvecs" % (d, K)))


ANY_CASES = [dict(c_dim=32, k_bit=8, n_bit=9),     # prefilter encode, 16-bit levels
             dict(c_dim=16, k_bit=6, n_bit=6),     # round 6: K = 64 / 32 on the prefilter encode (two / one row blocks) and the K <= 256 level / decode kernels
             dict(c_dim=32, k_bit=6, n_bit=9),
             dict(c_dim=16, k_bit=5, n_bit=5),
             dict(c_dim=12, k_bit=9, n_bit=6),     # K = 512: int32 codes
             dict(c_dim=24, k_bit=6, n_bit=4),     # (the repaired dimension 24 on the padded d = 32 kernel, two row blocks; levels / decode generic)
             dict(c_dim=8, k_bit=5, n_bit=8),
             dict(c_dim=10, k_bit=5, n_bit=6),     # d % 4 != 0: scalar loads / stores
             dict(c_dim=48, k_bit=11, n_bit=17),   # 384 KiB codebook (chunked in LDS), int32 codes and levels
             dict(c_dim=16, k_bit=8, n_bit=32),    # uncompressed norms: the projections travel as f32
             dict(c_dim=24, k_bit=6, n_bit=32),
             dict(c_dim=16, k_bit=9, n_bit=6),     # K = 512 ... : the prefilter kernel once per page of 256 codewords
             dict(c_dim=32, k_bit=10, n_bit=8),
             dict(c_dim=8, k_bit=9, n_bit=4)]


@pytest.mark.parametrize("case", ANY_CASES, ids=lambda c: "d%d_k%d_n%d" % (c["c_dim"], c["k_bit"], c["n_bit"]))
def test_batched_quantizer_any_shape_equals_per_tensor_path(case, tmp_path, monkeypatch):
    """The multi-tensor kernels for every other (d, K, code width, level width): aggregates, wire, per-user
    residuals and the server residual identical to the per-tensor kernels."""
    d, K = case["c_dim"], 2 ** case["k_bit"]
    if not os.path.exists(os.path.join(GOLDEN, "codebooks", "learned_codebook", "angular_dim_%d_Ks_%d.fvecs" % (d, K))):
        _write_unit_codebook(str(tmp_path), d, K, 5)
        monkeypatch.chdir(tmp_path)
    shapes = _shapes_for(d)
    qb, gb = _run_quantizer(shapes, 2, 13, **case)
    qp, gp = _run_quantizer(shapes, 2, 13, gq_no_batch=True, **case)
    assert qb._groups and qb._groups[0][2] is not None and qb._groups[0][2].ready and not qp._groups
    grp = qb._groups[0][2]
    assert grp.codebook.shape == (K, d) and len(qb.batch_idx) == sum(int(np.prod(s)) > 1000 for s in shapes) >= 5
    from gq_amd import native
    want = (native.BATCH_PREFILTER if (K <= 256 and K % 4 == 0 and d in (8, 12, 16, 24, 32)) else
            native.BATCH_PAGED if (K > 256 and K % 256 == 0 and d in (8, 16, 32)) else native.BATCH_EXACT)
    assert grp._batch.path == want      # the library's choice of kernels for this shape (gq_hsq_batched_path)
    for a, b, s in zip(gb, gp, shapes):
        assert a.shape == torch.Size(s)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), s
    assert torch.equal(qb._wire, qp._wire)
    for kw in (dict(ef=True), dict(ef=True, two_phase=True, scale="0.5")):
        qe, ge = _run_quantizer(shapes, 2, 13, **case, **kw)
        qf, gf = _run_quantizer(shapes, 2, 13, gq_no_batch=True, **case, **kw)
        assert qe._groups[0][2].ready
        for a, b in zip(ge, gf):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        for pb, pp in zip(qe.parameters, qf.parameters):
            for eb, ep in zip(pb.error, pp.error):
                assert torch.equal(eb, ep)
            if kw.get("two_phase"):
                assert torch.equal(pb.server_error, pp.server_error)


def test_batched_quantizer_reference_default_flags():
    """main.py:90-94's defaults (--c-dim 32 --k-bit 8 --n-bit 8 --random 1): stochastic rounding reaches level
    256, so the levels travel as int16 -- still one launch per stage, and every level within one step of the
    deterministic rounding."""
    shapes = RESNET50_COMPRESSED[:8] + RESNET50_SMALL[:3]
    q, g = _run_quantizer(shapes, 2, 9, c_dim=32, n_bit=8, random=1)
    det, gd = _run_quantizer(shapes, 2, 9, c_dim=32, n_bit=8, random=0)
    grp = q._groups[0][2]
    from gq_amd import native
    assert grp.ready and grp._batch.path == native.BATCH_PREFILTER and grp.level_dtype == torch.int16
    assert det._groups[0][2].level_dtype == torch.uint8
    for a, b, p in zip(g, gd, q.parameters):
        if p.numel() > 1000:
            assert not torch.equal(a, b)
        assert (a - b).abs().max() <= b.abs().max() * 0.1 + 1e-12   # one step = (ub - lb)/256 of the projection


@pytest.mark.parametrize("c_dim", [16, 32])
def test_batched_quantizer_long_tensor_lists(c_dim):
    """More tensors than the kernels keep segment records for in LDS (384): the prefilter kernel (d = 16 and, since
    round 5, d = 32 / 8 as well) switches to the instantiation that reads the records from global memory; same results as
    per-tensor launches."""
    shapes = [(1024,)] * 300 + [(32, 64)] * 100 + [(10,)] * 3
    qb, gb = _run_quantizer(shapes, 1, 4, c_dim=c_dim)
    qp, gp = _run_quantizer(shapes, 1, 4, c_dim=c_dim, gq_no_batch=True)
    assert qb._groups and len(qb._groups[0][1]) == 400
    from gq_amd import native
    assert qb._groups[0][2].ready
    assert qb._groups[0][2]._batch.path == native.BATCH_PREFILTER
    for a, b in zip(gb, gp):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(qb._wire, qp._wire)


def test_batched_quantizer_device_rng_and_misaligned_fallback():
    shapes = RESNET50_COMPRESSED[:6] + RESNET50_SMALL[:3]
    q, g = _run_quantizer(shapes, 2, 9, random=1)
    det, gd = _run_quantizer(shapes, 2, 9, random=0)
    for a, b in zip(g, gd):
        # stochastic rounding moves every level by at most one step
        assert (a - b).abs().max() <= (b.abs().max() * 2.5 + 1e-12)
    # a non-contiguous gradient makes the step fall back to the per-tensor path
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    params = [torch.nn.Parameter(torch.zeros(64, 64, device="cuda")) for _ in range(3)]
    q = Quantizer(NearestNeighborCompressor, params, make_args(num_users=1))
    ref = Quantizer(NearestNeighborCompressor, [torch.nn.Parameter(torch.zeros(64, 64, device="cuda")) for _ in range(3)],
                    make_args(num_users=1, gq_no_batch=True))
    grads = [torch.randn(64, 64, device="cuda") for _ in range(3)]
    for p, pr, gr in zip(params, ref.parameters, grads):
        p.grad = gr.t().contiguous().t()          # same values, column-major storage
        pr.grad = gr.clone()
    q.record(0, epoch=1)
    ref.record(0, epoch=1)
    q.apply()
    ref.apply()
    for p, pr in zip(params, ref.parameters):
        assert torch.equal(p.grad.data, pr.grad.data)


@pytest.mark.parametrize("kw", [dict(ef=True), dict(two_phase=True), dict(ef=True, two_phase=True, scale="0.5")])
def test_batched_error_feedback_and_two_phase_equal_per_tensor_path(kw):
    """Error feedback / two-phase on the batched kernels == the per-tensor path, bit for bit
    (aggregates, per-user residuals and the server residual)."""
    shapes = RESNET50_COMPRESSED[:9] + RESNET50_SMALL[:4]
    qb, gb = _run_quantizer(shapes, 2, 21, **kw)
    qp, gp = _run_quantizer(shapes, 2, 21, gq_no_batch=True, **kw)
    assert qb._groups and qb._groups[0][2].ready
    for a, b in zip(gb, gp):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if kw.get("ef"):
        for pb, pp in zip(qb.parameters, qp.parameters):
            for eb, ep in zip(pb.error, pp.error):
                assert torch.equal(eb, ep)
            if kw.get("two_phase"):
                assert torch.equal(pb.server_error, pp.server_error)


@pytest.mark.parametrize("c_dim", [16, 8, 32])
def test_error_feedback_encode_on_large_tensors_matches_the_oracle(oracle, c_dim):
    """Regression: the error-feedback instantiation of the d16/K256 encode once produced ONE wrong projection in
    ~1e5 subvectors (right code, u off by ~1e-3 relative, always lanes 48-63 of a tile): a packed FMA whose
    destination pair was also its multiplicand pair (hsq_pf_common.hpp).  Small fixtures never met it; two million
    subvectors per record do.  Codes and levels of every record must equal the oracle's."""
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    from gq_amd.codebook import load_codebook
    cb = load_codebook(c_dim, 256)
    shapes = [(80000, c_dim), (120000 * c_dim,), (10,)]
    for seed in range(1, 17 if c_dim == 16 else 7):     # the old build failed about one seed in twelve (d = 16)
        params = [torch.nn.Parameter(torch.zeros(*s, device="cuda")) for s in shapes]
        q = Quantizer(NearestNeighborCompressor, params, make_args(num_users=1, ef=True, scale="0.5", c_dim=c_dim))
        g = torch.Generator(device="cuda").manual_seed(seed)
        grads = [torch.randn(p.shape, device="cuda", generator=g) * 1e-2 for p in params]
        for p, x in zip(params, grads):
            p.grad = x.clone()
        q.record(0, epoch=1)
        torch.cuda.synchronize()
        assert q._groups and q._groups[0][2].ready
        w = q._wire.cpu().numpy()
        for k in (0, 1):
            M = grads[k].numel() // c_dim
            off, cd = q.offsets[k], q.codecs[k]
            codes, u = oracle.hsq_encode(grads[k].cpu().numpy().reshape(-1), cb)
            lb, ub, lv = oracle.scalar_levels(u, 6, 0, None)
            assert np.array_equal(w[0, off + cd.codes_off: off + cd.codes_off + M], codes.astype(np.uint8)), (seed, k)
            assert np.array_equal(w[0, off + cd.levels_off: off + cd.levels_off + M].astype(np.int64), lv.astype(np.int64)), (seed, k)


@pytest.mark.parametrize("which", ["hsq", "qsgd"])
def test_fused_error_feedback_updates_grad_and_error_in_place(which):
    """ps_quantizer.py:35,39 inside the batched launches: after record() the gradient tensor holds
    grad + scale*error_old (the reference's in-place add_) and error holds grad_new - decoded, where
    decoded is what a single-user apply() returns."""
    from gq_amd.compressors import NearestNeighborCompressor, QSGDCompressor
    from gq_amd.quantizers import Quantizer
    shapes = [(1024,), (64, 3, 3, 3), (72, 16), (128, 128, 3, 3)]
    params = [torch.nn.Parameter(torch.zeros(*s, device="cuda")) for s in shapes]
    kw = dict(c_dim=128, n_bit=2) if which == "qsgd" else {}
    q = Quantizer(QSGDCompressor if which == "qsgd" else NearestNeighborCompressor, params,
                  make_args(num_users=1, ef=True, scale="0.75", random=1, **kw))
    gen = torch.Generator(device="cuda").manual_seed(3)
    for p in params:
        p.error[0] = torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
    grads = [torch.randn(p.shape, device="cuda", generator=gen) * 1e-2 for p in params]
    old_err = [p.error[0].clone() for p in params]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    q.record(0, epoch=1)
    assert q._groups and q._groups[0][2].ready
    folded = [p.grad.data.clone() for p in params]
    for f, g, e in zip(folded, grads, old_err):
        assert torch.equal(f, g + 0.75 * e)
    q.apply()
    for p, f in zip(params, folded):
        assert torch.equal(p.error[0], f - p.grad.data)


def _run_qsgd(shapes, users, seed, grad_fn=None, **argkw):
    from gq_amd.compressors import QSGDCompressor
    from gq_amd.quantizers import Quantizer
    params = [torch.nn.Parameter(torch.zeros(*s, device="cuda")) for s in shapes]
    q = Quantizer(QSGDCompressor, params, make_args(**dict(dict(num_users=users, c_dim=128, n_bit=2), **argkw)))
    g = torch.Generator(device="cuda").manual_seed(seed)
    for st in range(2):
        for u in range(users):
            for p in params:
                p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-2
                if grad_fn is not None:
                    p.grad = grad_fn(p.grad)
            q.record(u, epoch=1)
        q.apply()
    return q, [p.grad.data.clone() for p in params]


QSGD_RANGES = {
    "below": lambda t: t * 1e-23,            # bucket norms around 2^-81
    "low": lambda t: t * 2e-22,              # ... 2^-77, elements down to 2^-90
    "high": lambda t: t * 2e7,               # ... 2^19.6
    "above": lambda t: t * 2e8,              # ... 2^23
    "zeros": lambda t: torch.where(t.abs() < 3e-3, torch.zeros_like(t), t),   # exact zeros inside most buckets
    "tiny": lambda t: torch.where(t.abs() < 1e-3, t * 1e-33, t),             # elements under 2^-102 beside ordinary ones
}


@pytest.mark.parametrize("span", sorted(QSGD_RANGES))
def test_batched_qsgd_compress_divides_like_the_reference_at_every_scale(span, oracle):
    """v / norm at the ends of the range (qsgd_compressor.py:52): the 4-bit multi-tensor compress against the per-tensor
    kernels and against the oracle's decompress(compress(g)) for the deterministic rounding -- tiny and huge bucket norms,
    exact zeros, elements forty orders of magnitude under their bucket's norm."""
    shapes = RESNET50_COMPRESSED[:8] + RESNET50_SMALL[:2]
    fn = QSGD_RANGES[span]
    qb, gb = _run_qsgd(shapes, 1, 9, grad_fn=fn)
    qp, gp = _run_qsgd(shapes, 1, 9, grad_fn=fn, gq_no_batch=True)
    assert qb._groups and qb._groups[0][2].ready and not qp._groups
    for a, b, s in zip(gb, gp, shapes):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), s
    g = torch.Generator(device="cuda").manual_seed(9)
    grads = [[fn(torch.randn(s, device="cuda", generator=g) * 1e-2) for s in shapes] for _ in range(2)][1]
    for k, s in enumerate(shapes):
        if int(np.prod(s)) <= 1000:
            continue
        d = qb.codecs[k].d
        with np.errstate(all="ignore"):
            norm, signs, levels = oracle.qsgd_compress(grads[k].cpu().numpy().reshape(-1), d, 2, 0)
            want = oracle.qsgd_decompress(norm, signs, levels, d, 2).reshape(-1)
        assert np.array_equal(gb[k].cpu().numpy().reshape(-1), want), s


@pytest.mark.parametrize("d,n_bit", [(128, 2), (128, 1), (32, 2), (8, 4), (256, 6), (512, 2), (64, 8), (16, 5), (2048, 2), (24, 2)])
def test_batched_qsgd_shared_quotient_equals_the_division_over_the_exponent_range(d, n_bit, oracle):
    """Round 6: |v| / norm comes from ONE reciprocal per bucket and Markstein's correction inside the operand window
    (2^-64 <= norm <= 2^20 -- norm / s >= 2^-80 --, every |v| of the lane >= 2^-102) and from the true division outside it
    (qsgd_batched.hip: qsgd_code<FAST>, quotient_window).  Buckets with norms from 2^-140 to 2^60 -- 2^-80 and the window's upper
    end to the ulp among them; the lower end, 2^-64, to the ulp: tests/test_gpu_qsgd_contract.py --, elements up to 2^-70 below their bucket's norm, exact zeros, zero buckets, NaN: the wire's
    decode equals the oracle's decompress(compress(g)) (qsgd_compressor.py:49-53,66-71) bit for bit, NaN for NaN."""
    from gq_amd.compressors import QSGDCompressor
    from gq_amd.quantizers import QSGDCodec
    rng = np.random.RandomState(1000 * d + n_bit)
    Mb = 6000 if d <= 256 else 700
    x = rng.standard_normal((Mb, d)).astype(np.float32)
    x *= np.exp2(rng.uniform(-140, 60, (Mb, 1))).astype(np.float32)                          # the bucket's scale
    small = rng.random_sample((Mb, d)) < 0.2
    x = np.where(small, x * np.exp2(-rng.uniform(0, 70, (Mb, d))).astype(np.float32), x)     # elements far below the norm
    x = np.where(rng.random_sample((Mb, d)) < 0.05, np.float32(0), x).astype(np.float32)     # exact zeros
    edges = np.array([2.0 ** -80, np.nextafter(np.float32(2.0 ** -80), np.float32(0)), 2.0 ** 20, np.nextafter(np.float32(2.0 ** 20), np.float32(np.inf)),
                      2.0 ** -102, 2.0 ** -126, 1e-45], dtype=np.float32)
    for k, e in enumerate(edges):      # a bucket whose norm IS the value, and one that holds it next to a norm of 1 / 2^-80
        x[k] = np.clip(x[k] / np.abs(x[k]).max(), -1, 1) * e
        x[k, 0] = e
        x[20 + k, 1] = e if e <= 1 else 1.0
        x[20 + k, 0] = 1.0 if k % 2 else np.float32(2.0 ** -80)
    x[40] = 0.0
    x[43, 0] = np.nan      # (a bucket with an infinite element: the packed wire has no code for the reference's INT_MIN level -- DESIGN.md section 2)
    codec = QSGDCodec(QSGDCompressor(x.size, x.shape, make_args(c_dim=d, n_bit=n_bit)), x.size, x.shape)
    assert codec.bits in (4, 8, 16)
    got = codec.roundtrip(torch.from_numpy(x).cuda(), 0).cpu().numpy()
    with np.errstate(all="ignore"):
        norm, signs, levels = oracle.qsgd_compress(x.reshape(-1), d, n_bit, 0)
        want = oracle.qsgd_decompress(norm, signs, levels, d, n_bit).reshape(x.shape)
    assert _same(got, want)


def test_batched_qsgd_device_draws_round_without_bias():
    """The draws of the bucketed kernels (round 6: one full hash per bucket, one multiply-xorshift round per element): the level of
    every element is floor or floor + 1 of |v| / norm * s, and over many elements the share rounded up equals the mean
    fractional part -- overall, per position inside the bucket, and for two seeds that share no draws."""
    from gq_amd.compressors import QSGDCompressor
    from gq_amd.quantizers import QSGDCodec
    d, n_bit, Mb = 128, 2, 40000
    torch.manual_seed(11)
    x = torch.randn(Mb, d, device="cuda")
    det = QSGDCodec(QSGDCompressor(x.numel(), x.shape, make_args(c_dim=d, n_bit=n_bit, random=0)), x.numel(), x.shape)
    rnd = QSGDCodec(QSGDCompressor(x.numel(), x.shape, make_args(c_dim=d, n_bit=n_bit, random=1)), x.numel(), x.shape)
    norm = x.abs().max(dim=1, keepdim=True)[0]
    s = float(2 ** n_bit)
    scaled = (x / norm).abs() * s
    floor = torch.clamp(scaled, 0, s - 1).floor()
    frac = (scaled - floor).double()
    lv0 = (det.roundtrip(x, 0).abs() * s / norm).round()
    assert torch.equal(lv0, floor)
    ups = []
    for salt in (1, 2):
        lv = (rnd.roundtrip(x, salt).abs() * s / norm).round()
        up = lv - floor
        assert float(up.min()) >= 0 and float(up.max()) <= 1
        assert abs(float(up.double().mean()) - float(frac.mean())) < 2e-3
        per_pos = (up.double().mean(0) - frac.mean(0)).abs().max()      # 40,000 draws per position: sigma ~ 2e-3
        assert float(per_pos) < 1.2e-2, float(per_pos)
        ups.append(up)
    agree = float((ups[0] == ups[1]).double().mean())
    assert 0.5 < agree < 0.9, agree      # independent draws agree where both round the same way by chance, not everywhere


@pytest.mark.parametrize("kw", [dict(n_bit=8), dict(n_bit=8, c_dim=512, ef=True), dict(n_bit=5), dict(n_bit=8, c_dim=32), dict(n_bit=2, c_dim=32),
                                dict(n_bit=5, c_dim=64), dict(n_bit=2, c_dim=16), dict(n_bit=8, c_dim=16, ef=True), dict(n_bit=4, c_dim=256),
                                dict(n_bit=2, c_dim=8), dict(n_bit=8, c_dim=64, ef=True), dict(n_bit=2, c_dim=512), dict(n_bit=4, c_dim=512, ef=True)])
def test_batched_packed_qsgd_wider_codes(kw, oracle):
    """8- and 16-bit packed codes (e.g. the usual "8-bit QSGD") and every lanes-per-bucket form of the bucketed kernels
    (bucket widths 8 ... 256: 2, 4, 8 or 16 lanes per bucket, picked from the descriptor's bucket_hint; the list's 1,728-element
    tensor brings widths that are no power of two): batched launch == per-tensor path and, for the deterministic
    rounding, the mean of the oracle's decompress(compress(g))."""
    shapes = RESNET50_COMPRESSED[:10] + RESNET50_SMALL[:3]
    qb, gb = _run_qsgd(shapes, 2, 5, **kw)
    qp, gp = _run_qsgd(shapes, 2, 5, gq_no_batch=True, **kw)
    assert qb._groups and qb._groups[0][2].ready and qb.codecs[0].bits == (16 if kw["n_bit"] == 8 else 8 if kw["n_bit"] > 2 else 4)
    for a, b in zip(gb, gp):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if kw.get("ef"):
        for pb, pp in zip(qb.parameters, qp.parameters):
            for eb, ep in zip(pb.error, pp.error):
                assert torch.equal(eb, ep)
        return
    g = torch.Generator(device="cuda").manual_seed(5)
    grads = [[[torch.randn(s, device="cuda", generator=g) * 1e-2 for s in shapes] for _ in range(2)] for _ in range(2)][1]
    for k, s in enumerate(shapes):
        if int(np.prod(s)) <= 1000:
            continue
        d = qb.codecs[k].d
        dec = []
        for u in range(2):
            norm, signs, levels = oracle.qsgd_compress(grads[u][k].cpu().numpy().reshape(-1), d, kw["n_bit"], 0)
            dec.append(oracle.qsgd_decompress(norm, signs, levels, d, kw["n_bit"]).reshape(-1))
        want = (torch.from_numpy(np.stack(dec)).sum(0) / 2).numpy()
        assert np.array_equal(gb[k].cpu().numpy().reshape(-1), want), s


@pytest.mark.parametrize("kw", [dict(), dict(ef=True), dict(two_phase=True)])
def test_batched_packed_qsgd_equals_per_tensor_and_reference_arithmetic(kw, oracle):
    """QSGD on the packed 4-bit wire: batched launch == per-tensor path, and the single-user decode
    equals the oracle's decompress(compress(g)) (the reference's arithmetic)."""
    shapes = RESNET50_COMPRESSED[:10] + RESNET50_SMALL[:3]
    qb, gb = _run_qsgd(shapes, 2, 5, **kw)
    qp, gp = _run_qsgd(shapes, 2, 5, gq_no_batch=True, **kw)
    assert qb._groups and qb._groups[0][0].__name__ == "BatchedQSGD" and qb._groups[0][2].ready
    for a, b in zip(gb, gp):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if kw.get("ef"):
        for pb, pp in zip(qb.parameters, qp.parameters):
            for eb, ep in zip(pb.error, pp.error):
                assert torch.equal(eb, ep)
    assert qb.codecs[0].bits == 4
    # 0.5 B per element + one f32 per 128-element bucket
    n = sum(p.numel() for p in qb.parameters if p.numel() > 1000)
    assert qb.wire_bytes_per_user() < n * 0.56 + 4 * 4096
    if not kw:
        from gq_amd.compressors import QSGDCompressor
        x = torch.randn(256, 128, device="cuda") * 3
        x[5] = 0.0   # a zero bucket
        codec = qb.codecs[0].__class__(QSGDCompressor(x.numel(), x.shape, make_args(c_dim=128, n_bit=2)), x.numel(), x.shape)
        got = codec.roundtrip(x, 0).cpu().numpy()
        norm, signs, levels = oracle.qsgd_compress(x.cpu().numpy(), 128, 2, 0)
        want = oracle.qsgd_decompress(norm, signs, levels, 128, 2).reshape(256, 128)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n_bit", [2, 4, 7])
def test_qsgd_extreme_bucket_scales_match_the_oracle(n_bit, oracle):
    """The packed QSGD compress on bucket scales from 1e-38 (subnormal elements) to 1e30, elements 30 orders of magnitude
    below their bucket's norm, zero and single-spike buckets, NaN / inf buckets: levels, signs and norms equal the
    oracle's (the reference's `v / norm`).  (Round 6: inside its operand window the quotient comes from one reciprocal per bucket
    and Markstein's correction, with ONE window test per lane -- round 5's per-element test cost what it saved.)"""
    from gq_amd.compressors import QSGDCompressor
    from gq_amd.quantizers import QSGDCodec
    rng = np.random.RandomState(n_bit)
    B, d = 4096, 128
    x = rng.standard_normal((B, d)).astype(np.float32)
    scale = (np.float32(10.0) ** rng.randint(-38, 31, size=B)).astype(np.float32)
    scale[:1024] = np.float32(1e-3)                                   # plain waves: every lane on the quick path
    x *= scale[:, None]
    tiny = rng.randint(0, B, size=600)
    x[tiny, 3:40] *= np.float32(1e-35)                                 # elements far below the bucket's norm (some underflow)
    x[7] = 0.0
    x[9, 1:] = 0.0                                                     # one spike, the rest exact zeros
    x[11, 5] = np.float32("nan")
    x[13, 6] = np.float32("inf")
    x[15] = np.float32(1e-45)                                          # a bucket of the smallest subnormal
    xt = torch.from_numpy(x).cuda()
    codec = QSGDCodec(QSGDCompressor(x.size, x.shape, make_args(c_dim=d, n_bit=n_bit, random=0)), x.size, x.shape)
    assert codec.bits in (4, 8)
    wire = torch.zeros(codec.nbytes, dtype=torch.uint8, device="cuda")
    codec.encode_into(xt, wire, 0, 0)
    norm, signs, levels = oracle.qsgd_compress(x.reshape(-1), d, n_bit, 0)
    got_norm = wire[codec.norm_off:codec.norm_off + 4 * B].view(torch.float32).cpu().numpy()
    assert _same(got_norm, norm)
    raw = wire[codec.codes_off:codec.codes_off + x.size * codec.bits // 8].cpu().numpy()
    if codec.bits == 4:
        codes = np.empty(x.size, np.uint8)
        codes[0::2], codes[1::2] = raw & 15, raw >> 4
    else:
        codes = raw
    lv = np.where(levels < 0, 0, levels)                               # INT_MIN (NaN quotient) is level 0 on the packed wire
    assert np.array_equal(codes & ((1 << (codec.bits - 1)) - 1), lv.astype(np.uint8))
    # a NaN quotient's level (INT_MIN in the reference: negative) carries its sign in the sign bit, so that level 0 decodes to
    # the zero the reference decodes (-2^31)(2 sign - 1)(norm) / s to: +0 for a zero bucket
    assert np.array_equal(codes >> (codec.bits - 1), np.where(levels < 0, 1 - signs.astype(np.uint8), signs))
    dec = torch.empty(x.size, dtype=torch.float32, device="cuda")
    codec.decode_wire(wire, 0, dec)
    with np.errstate(all="ignore"):
        want = oracle.qsgd_decompress(norm, signs, levels, d, n_bit).reshape(-1)
    finite_norm = np.repeat(np.isfinite(norm), d)      # (an infinite norm: the reference's INT_MIN level times inf has no code on the packed wire)
    assert _same(dec.cpu().numpy()[finite_norm], want[finite_norm])


@pytest.mark.parametrize("kw", [dict(c_dim=128, n_bit=2), dict(c_dim=0, n_bit=1), dict(c_dim=512, n_bit=8)],
                         ids=lambda k: "d%d_n%d" % (k["c_dim"], k["n_bit"]))
def test_qsgd_large_tensors_match_the_oracle(kw, oracle):
    """Rare-event check at size: 2 x 12.6 M elements per user through the packed kernels (bucketed, wide and
    16-bit forms), the aggregate of two users against the oracle's decompress(compress(g)) mean, bit for bit."""
    shapes = [(2048, 4096), (4_194_304 + 2048,), (10,)]
    qb, gb = _run_qsgd(shapes, 2, 9, **kw)
    assert qb._groups and qb._groups[0][2].ready
    g = torch.Generator(device="cuda").manual_seed(9)
    grads = [[[torch.randn(s, device="cuda", generator=g) * 1e-2 for s in shapes] for _ in range(2)] for _ in range(2)][1]
    for k in (0, 1):
        d = qb.codecs[k].d
        dec = []
        for u in range(2):
            norm, signs, levels = oracle.qsgd_compress(grads[u][k].cpu().numpy().reshape(-1), d, kw["n_bit"], 0)
            dec.append(oracle.qsgd_decompress(norm, signs, levels, d, kw["n_bit"]).reshape(-1))
        want = oracle.mean_users(np.stack(dec, 0))     # (+0 + dec0 + dec1) / 2: torch's sum starts from +0
        assert np.array_equal(gb[k].cpu().numpy().reshape(-1).view(np.uint32), want.view(np.uint32)), k


WIDE_SHAPES = [(64, 3, 3, 3), (128, 128, 3, 3), (1024,), (2048,), (512, 128, 1, 1), (9000,), (5, 1001, 2), (10,), (64,),
               (2, 4099)]


@pytest.mark.parametrize("kw", [dict(c_dim=0, n_bit=1), dict(c_dim=0, n_bit=1, random=1), dict(c_dim=0, n_bit=1, ef=True),
                                dict(c_dim=0, n_bit=1, ef=True, two_phase=True, scale="0.5"), dict(c_dim=0, n_bit=5),
                                dict(c_dim=4098, n_bit=2), dict(c_dim=8192, n_bit=2, ef=True), dict(c_dim=0, n_bit=8),
                                dict(c_dim=4098, n_bit=9, ef=True)],
                         ids=lambda k: "_".join("%s%s" % kv for kv in k.items()))
def test_wide_bucket_qsgd_terngrad_equals_reference_arithmetic(kw, oracle):
    """TernGrad (`--quantizer qsgd --c-dim 0 --n-bit 1`: the tensor is ONE bucket) and other wide buckets on the
    chunked kernels: the multi-tensor launch == one launch per tensor, and -- deterministic rounding -- the aggregate
    equals the mean of the oracle's decompress(compress(g)) per user, the residuals the oracle's g - decoded."""
    users = 2
    if kw["c_dim"]:
        shapes = [(kw["c_dim"], 3), (kw["c_dim"] * 2,), (7, kw["c_dim"]), (10,)]
    else:
        shapes = WIDE_SHAPES
    qb, gb = _run_qsgd(shapes, users, 5, **kw)
    qp, gp = _run_qsgd(shapes, users, 5, gq_no_batch=True, **kw)
    wide = [g for g in qb._groups if g[0].__name__ == "BatchedQSGD" and g[2] is not None and g[2].wide]
    assert wide and wide[0][2].ready and not qp._groups
    if kw.get("random"):
        # the draws are indexed by (bucket, element) of the launch: the two layouts round differently, each within
        # one level (max|v| / 2^n_bit) of the deterministic rounding
        _, gd = _run_qsgd(shapes, users, 5, **dict(kw, random=0))
        for a, b, d in zip(gb, gp, gd):
            step = d.abs().max() * 1.0001 + 1e-12       # n_bit = 1, deterministic levels {0, 1}: max|decoded| = norm/2
            assert (a - d).abs().max() <= step and (b - d).abs().max() <= step
            assert a.numel() <= 1000 or not torch.equal(a, d)
        return
    for a, b in zip(gb, gp):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if kw.get("ef"):
        for pb, pp in zip(qb.parameters, qp.parameters):
            for eb, ep in zip(pb.error, pp.error):
                assert torch.equal(eb, ep)
    if kw.get("ef") or kw.get("two_phase"):
        return
    # the same gradients as _run_qsgd's second step, through the oracle
    g = torch.Generator(device="cuda").manual_seed(5)
    grads = [[[torch.randn(s, device="cuda", generator=g) * 1e-2 for s in shapes] for _ in range(users)] for _ in range(2)][1]
    for k, s in enumerate(shapes):
        n = int(np.prod(s))
        if n <= 1000:
            continue
        d = qb.codecs[k].d
        dec = []
        for u in range(users):
            x = grads[u][k].cpu().numpy().reshape(-1)
            norm, signs, levels = oracle.qsgd_compress(x, d, kw["n_bit"], 0)
            dec.append(oracle.qsgd_decompress(norm, signs, levels, d, kw["n_bit"]).reshape(-1))
        want = (torch.from_numpy(np.stack(dec)).sum(0) / users).numpy() if users > 1 else dec[0]
        assert np.array_equal(gb[k].cpu().numpy().reshape(-1), want), s


def test_probabilistic_vector_compressor_matches_oracle_and_is_unbiased(oracle):
    """a12 (intended semantics, parity unpinned vs the reference -- its class cannot run):
    GPU == CPU restatement bit for bit for the same draws r; the decode is unbiased."""
    from gq_amd.compressors import ProbabilisticVectorCompressor
    rng = np.random.RandomState(4)
    M = 20000
    x = rng.standard_normal(16 * M).astype(np.float32)
    args = make_args(n_bit=32, gq_rng="reference")
    comp = ProbabilisticVectorCompressor(x.size, torch.Size([x.size]), args)
    assert comp.c_dagger.shape == (256, 16)
    torch.manual_seed(123)
    r = torch.rand(M).numpy()
    torch.manual_seed(123)
    u, codes = comp.compress(torch.from_numpy(x).cuda())
    rc, ru = oracle.pvq_encode(x, comp.c_dagger.cpu().numpy(), r)
    assert np.array_equal(codes.cpu().numpy().astype(np.int32), rc)
    assert np.array_equal(_bits(u.cpu().numpy()), _bits(ru))
    dec = comp.decompress([u, codes])
    assert np.array_equal(dec.cpu().numpy().reshape(-1, 16),
                          comp.codewords.cpu().numpy()[rc] * ru[:, None])
    # unbiasedness with the in-kernel generator: mean decode of one repeated subvector -> that subvector
    v = rng.standard_normal(16).astype(np.float32)
    rep = 100000
    c2 = ProbabilisticVectorCompressor(16 * rep, torch.Size([16 * rep]), make_args(n_bit=32))
    out = c2.decompress(c2.compress(torch.from_numpy(np.tile(v, rep)).cuda())).view(rep, 16).double().mean(0).cpu().numpy()
    assert np.linalg.norm(out - v) / np.linalg.norm(v) < 3e-2
    # quantised norms (n_bit=6) go through the same level quantiser as HSQ
    c3 = ProbabilisticVectorCompressor(x.size, torch.Size([M, 16]), make_args(n_bit=6, random=0))
    sig = c3.compress(torch.from_numpy(x).cuda().view(M, 16))
    (lb, ub, l), cds = sig
    assert l.dtype == torch.int32 and int(l.max()) == 63 and c3.decompress(sig).shape == (M, 16)
    # K == dim: random orthogonal codebook, c_dagger == codewords
    c4 = ProbabilisticVectorCompressor(16 * 100, torch.Size([1600]), make_args(k_bit=4, n_bit=32))
    assert torch.allclose(c4.c_dagger, c4.codewords, atol=1e-5)


@pytest.mark.parametrize("quant", ["hsq", "qsgd", "terngrad"])
def test_batched_quantizer_gradients_updated_in_place_between_steps(quant):
    """Gradients that KEEP their storage from step to step (the pointer table is then not rewritten) but change their
    values, shrinking: the per-tensor (min, max) accumulators must start afresh every step.  Multi-tensor path ==
    per-tensor path over three steps, bit for bit."""
    from gq_amd.compressors import NearestNeighborCompressor, QSGDCompressor
    from gq_amd.quantizers import Quantizer
    shapes = [(96, 112), (96,), (64, 64, 3, 3), (40, 128), (12,), (1024,)]
    kw = {"hsq": {}, "qsgd": dict(c_dim=128, n_bit=2), "terngrad": dict(c_dim=0, n_bit=1)}[quant]
    comp = NearestNeighborCompressor if quant == "hsq" else QSGDCompressor
    outs = []
    for no_batch in (False, True):
        torch.manual_seed(3)
        params = [torch.nn.Parameter(torch.zeros(*s, device="cuda")) for s in shapes]
        q = Quantizer(comp, params, make_args(num_users=1, gq_no_batch=no_batch, **kw))
        grads = [torch.randn(s, device="cuda") for s in shapes]
        res = []
        for step in range(3):
            for p, g in zip(params, grads):
                p.grad = g
            q.record(0, epoch=1)
            q.apply()
            res.append([p.grad.data.clone() for p in params])
            for g in grads:
                g.mul_(0.25)            # same storage, smaller range: a stale (min, max) would show
        outs.append(res)
        assert bool(q._groups) != no_batch
    for a, b in zip(outs[0], outs[1]):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


PVQ_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "pvq_*.npz")))
RESIDUAL_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "residual_*.npz")))


def _inject(comp, codewords, c_dagger):
    """The fixture's codebook and pseudo-inverse (LAPACK output / ortho_group draws of the generating run)."""
    comp.codewords = torch.from_numpy(np.ascontiguousarray(codewords))
    if c_dagger is not None:
        comp.c_dagger = torch.from_numpy(np.ascontiguousarray(c_dagger))


def _check_sig(sig, g, prefix, n_bit):
    norms, codes = sig
    assert np.array_equal(codes.cpu().numpy().astype(np.int32), g[prefix + "codes"].astype(np.int32)), prefix + "codes"
    if n_bit == 32:
        assert np.array_equal(_bits(norms.cpu().numpy()), _bits(g[prefix + "u"])), prefix + "u"
    else:
        lb, ub, l = norms
        assert _bits(lb.cpu().numpy()) == _bits(g[prefix + "lb"]) and _bits(ub.cpu().numpy()) == _bits(g[prefix + "ub"])
        assert l.dtype == torch.int32 and np.array_equal(l.cpu().numpy(), g[prefix + "levels"]), prefix + "levels"


@pytest.mark.parametrize("name", PVQ_CASES)
def test_probabilistic_vector_compressor_matches_reference(name):
    """a12 against the reference's own output (tests/golden/pvq_*.npz; make_golden.py explains the one operation it
    had to define): codes, magnitudes / levels, lb, ub and the decode, bit for bit, for the reference's draws r."""
    from gq_amd.compressors import ProbabilisticVectorCompressor
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    d, K, n_bit = int(g["dim"]), int(g["K"]), int(g["n_bit"])
    x = torch.from_numpy(g["x"])
    comp = ProbabilisticVectorCompressor(x.numel(), x.shape, make_args(c_dim=d, k_bit=int(np.log2(K)), n_bit=n_bit,
                                                                       random=0, gq_rng="reference"))
    _inject(comp, g["codewords"], g["c_dagger"])
    torch.manual_seed({"pvq_d16_k256_n32": 51, "pvq_d16_k256_n6": 52, "pvq_d16_k16_n32": 53, "pvq_d8_k32_n32": 54,
                       "pvq_d16_k256_zero_rows": 55}[name])
    sig = comp.compress(x.cuda())
    _check_sig(sig, g, "", n_bit)
    assert np.array_equal(_bits(comp.decompress(sig).cpu().numpy()), _bits(g["decoded"]))


PVQD = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "pvqd_*.npz")))


@pytest.mark.parametrize("name", PVQD)
def test_probabilistic_vector_compressor_at_size_matches_reference_digests(name):
    """a12 on 4 M elements through the MFMA kernel (shared-divisor quotient, double threshold: pvq.hip): codes, magnitudes /
    levels, (lb, ub) and the decode hash to the digests of the reference's own output."""
    import hashlib
    from gq_amd.compressors import ProbabilisticVectorCompressor
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x = (np.random.RandomState(int(g["seed"])).standard_normal(int(g["n"])) * float(g["scale_in"])).astype(np.float32)
    assert sha(x) == str(g["x_sha"])
    d, K, n_bit = int(g["dim"]), int(g["K"]), int(g["n_bit"])
    comp = ProbabilisticVectorCompressor(x.size, x.shape, make_args(c_dim=d, k_bit=int(np.log2(K)), n_bit=n_bit, random=0,
                                                                    gq_rng="reference"))
    _inject(comp, g["codewords"], g["c_dagger"])
    torch.manual_seed(int(g["seed_r"]))
    norms, codes = comp.compress(torch.from_numpy(x).cuda())
    assert sha(codes.cpu().numpy().astype(np.int32)) == str(g["codes_sha"])
    if n_bit == 32:
        assert sha(norms.cpu().numpy()) == str(g["u_sha"])
    else:
        lb, ub, l = norms
        assert sha(l.cpu().numpy().astype(np.int32)) == str(g["levels_sha"])
        assert _same(np.array([lb.item(), ub.item()], np.float32), g["lbub"])
    assert sha(comp.decompress([norms, codes]).cpu().numpy()) == str(g["decoded_sha"])


@pytest.mark.parametrize("name", RESIDUAL_CASES)
def test_residual_compressor_matches_reference(name):
    """a11 against the reference's own output (tests/golden/residual_*.npz): both stage signatures and the summed
    decode, bit for bit."""
    from gq_amd.compressors import ResidualCompressor
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    d, K, n_bit = int(g["dim"]), int(g["K"]), int(g["n_bit"])
    x = torch.from_numpy(g["x"])
    np.random.seed(0)
    comp = ResidualCompressor(x.numel(), x.shape, make_args(c_dim=d, k_bit=int(np.log2(K)), n_bit=n_bit, random=0,
                                                            gq_rng="reference"))
    _inject(comp.compressors[0], g["codewords1"], None)
    _inject(comp.compressors[1], g["codewords2"], g["c_dagger"])
    torch.manual_seed({"residual_d16_k256_n6": 56, "residual_d16_k256_n32": 57, "residual_d16_k16_n32": 58}[name])
    sigs = comp.compress(x.cuda())
    _check_sig(sigs[0], g, "s1_", n_bit)
    _check_sig(sigs[1], g, "s2_", n_bit)
    assert np.array_equal(_bits(comp.decompress(sigs).cpu().numpy()), _bits(g["decoded"]))


@pytest.mark.parametrize("name", sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "residuald_*.npz"))))
def test_residual_compressor_at_size_matches_reference_digests(name):
    """a11 on 4 M elements: stage 1 (prefilter encode), stage 2 on `grad - decode(stage 1)` inside the kernel
    (gq_pvq_encode_residual) and the summed decode hash to the digests of the reference's own output."""
    import hashlib
    from gq_amd.compressors import ResidualCompressor
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x = (np.random.RandomState(int(g["seed"])).standard_normal(int(g["n"])) * float(g["scale_in"])).astype(np.float32)
    assert sha(x) == str(g["x_sha"])
    d, K, n_bit = int(g["dim"]), int(g["K"]), int(g["n_bit"])
    np.random.seed(0)
    comp = ResidualCompressor(x.size, x.shape, make_args(c_dim=d, k_bit=int(np.log2(K)), n_bit=n_bit, random=0, gq_rng="reference"))
    _inject(comp.compressors[0], g["codewords1"], None)
    _inject(comp.compressors[1], g["codewords2"], g["c_dagger"])
    torch.manual_seed(int(g["seed_r"]))
    sigs = comp.compress(torch.from_numpy(x).cuda())
    for k, (norms, codes) in enumerate(sigs, 1):
        assert sha(codes.cpu().numpy().astype(np.int32)) == str(g["s%d_codes_sha" % k]), k
        if n_bit == 32:
            assert sha(norms.cpu().numpy()) == str(g["s%d_u_sha" % k]), k
        else:
            lb, ub, l = norms
            assert sha(l.cpu().numpy().astype(np.int32)) == str(g["s%d_levels_sha" % k]), k
            assert _same(np.array([lb.item(), ub.item()], np.float32), g["s%d_lbub" % k]), k
    assert sha(comp.decompress(sigs).cpu().numpy()) == str(g["decoded_sha"])


def test_residual_compressor_two_stages():
    """a11: stage 1 (nearest neighbour) + stage 2 (probabilistic vector) on the residual."""
    from gq_amd.compressors import ResidualCompressor, NearestNeighborCompressor
    x = torch.randn(4096, 16, device="cuda")
    args = make_args(n_bit=32)
    rc = ResidualCompressor(x.numel(), x.shape, args)
    sigs = rc.compress(x)
    assert len(sigs) == 2
    dec = rc.decompress(sigs)
    s1 = rc.compressors[0].decompress(sigs[0])
    assert torch.equal(s1, NearestNeighborCompressor(x.numel(), x.shape, args).decompress(
        NearestNeighborCompressor(x.numel(), x.shape, args).compress(x)))
    # stage 1 removes energy; the two-stage decode is the sum of the stage decodes
    assert (x - s1).norm() < x.norm()
    assert torch.allclose(dec, s1 + rc.compressors[1].decompress(sigs[1]))
    # averaged over draws the second stage is unbiased on the residual, so the mean error shrinks
    acc = torch.zeros_like(x)
    for _ in range(40):
        acc += rc.decompress(rc.compress(x))
    assert (acc / 40 - x).norm() < 0.5 * (x - s1).norm()


def test_training_driver_fcn_hsq_learns():
    """BASELINE config 1 (plumbing): hsq, fcn, MNIST-shaped synthetic data, c-dim 16 k-bit 8 n-bit 6,
    num-users 1 -- the loss goes down through the quantized gradients, and matches plain SGD closely."""
    from gq_amd.driver import build_parser, train
    base = ["--network", "fcn", "--dataset", "mnist", "--c-dim", "16", "--k-bit", "8", "--n-bit", "6",
            "--num-users", "2", "--batch-size", "32", "--epochs", "2", "--train-size", "2048", "--lr", "0.05",
            "--log-interval", "4"]
    _, q, hist = train(build_parser().parse_args(base + ["--quantizer", "hsq"]))
    assert hist[-1]["loss"] < 0.7 * hist[0]["loss"]
    assert q._groups and q._groups[0][2].ready          # the batched HIP path did the work
    _, _, hist_sgd = train(build_parser().parse_args(base + ["--quantizer", "sgd"]))
    assert abs(hist[-1]["loss"] - hist_sgd[-1]["loss"]) < 0.35 * hist_sgd[0]["loss"]
    # error feedback variant runs too
    _, _, hist_ef = train(build_parser().parse_args(base + ["--quantizer", "hsq", "--ef"]))
    assert hist_ef[-1]["loss"] < 0.7 * hist_ef[0]["loss"]


def test_training_driver_resnet50_shapes_and_one_step():
    """BASELINE config 3 shape: the driver's ResNet-50 has the reference's parameter list."""
    import json
    from gq_amd.driver import ResNet50, build_parser, train
    shapes = json.load(open(os.path.join(HERE, "golden", "resnet50_cifar_shapes.json")))["parameter_shapes"]
    assert [list(p.shape) for p in ResNet50().parameters()] == shapes
    args = build_parser().parse_args(["--network", "resnet50", "--dataset", "cifar10", "--quantizer", "hsq", "--c-dim", "16",
                                      "--k-bit", "8", "--n-bit", "6", "--num-users", "1", "--batch-size", "16",
                                      "--epochs", "1", "--train-size", "64", "--log-interval", "1"])
    _, q, hist = train(args)
    assert len(hist) >= 2 and all(np.isfinite(h["loss"]) for h in hist)
    assert len(q._groups[0][1]) == 76 and len(q.dense_idx) == 85


def test_prefilter_on_real_resnet50_gradients_equals_exact_kernel(oracle):
    """BASELINE config 3: REAL back-propagated ResNet-50 gradients (not Gaussian noise) -- every compressed
    tensor's codes and projections from the prefilter path equal the exact f32 MFMA kernel's, a sampled tensor
    equals the oracle's, and only a small fraction of subvectors needs the exact recomputation."""
    from gq_amd import native
    from gq_amd.codebook import load_codebook
    from gq_amd.driver import ResNet50
    torch.manual_seed(5)
    dev = torch.device("cuda:0")
    model = ResNet50().to(dev)
    x = torch.randn(16, 3, 32, 32, device=dev)
    y = torch.randint(0, 10, (16,), device=dev)
    torch.nn.functional.cross_entropy(model(x), y).backward()
    cb_np = load_codebook(16, 256)
    cb = torch.from_numpy(cb_np).to(dev)
    total, fixed, checked_oracle = 0, 0, False
    for p in model.parameters():
        if p.numel() <= 1000:
            continue
        g = p.grad.data.contiguous().view(-1)
        M = g.numel() // 16
        res = {}
        for impl in (1, 4):
            codes = torch.empty(M, dtype=torch.uint8, device=dev)
            u = torch.empty(M, dtype=torch.float32, device=dev)
            ws = native.new_workspace(dev, M)
            native.mark_worklist(ws, M)
            native.hsq_encode(g, cb, codes, u, ws, impl=impl)
            res[impl] = (codes, u, ws)
        torch.cuda.synchronize()
        assert torch.equal(res[1][0], res[4][0]), tuple(p.shape)
        assert torch.equal(res[1][1].view(torch.int32), res[4][1].view(torch.int32)), tuple(p.shape)
        total += M
        fixed += native.fixup_count(res[4][2], M)
        if not checked_oracle and 4096 <= M <= 40000:
            rc, ru = oracle.hsq_encode(g.cpu().numpy(), cb_np)
            assert np.array_equal(res[4][0].cpu().numpy().astype(np.int32), rc)
            assert np.array_equal(res[4][1].cpu().numpy().view(np.uint32), ru.view(np.uint32))
            checked_oracle = True
    assert checked_oracle and total > 1_400_000
    print("real ResNet-50 gradients: %d of %d subvectors (%.3f%%) took the exact fix-up path" % (fixed, total, 100.0 * fixed / total))
    assert fixed < 0.02 * total


@pytest.mark.parametrize("mode,quant,ef", [("ps", "hsq", False), ("ps", "hsq", True), ("ring", "hsq", True), ("ps", "qsgd", False),
                                           ("ring", "qsgd", False), ("ring", "terngrad", False)])
def test_two_ranks_on_one_gpu_equal_single_process(tmp_path, mode, quant, ef):
    """The distributed product path with the REAL kernels: two ranks (two local users each) drive the HIP library
    on cuda:0 and exchange the wire over gloo (RCCL refuses two ranks on one GPU); the result equals four users
    in one process, bit for bit -- parameter-server mean and ring sum, HSQ and QSGD, with and without error feedback."""
    import subprocess
    import sys
    script = os.path.join(HERE, "_dist_worker_gpu.py")
    out = str(tmp_path / "res")
    port = 29800 + (os.getpid() % 1500) + {"ps": 0, "ring": 3}[mode] + {"hsq": 0, "qsgd": 5, "terngrad": 17}[quant] + (11 if ef else 0)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    procs = [subprocess.Popen([sys.executable, script, str(r), "2", out, mode, quant, "1" if ef else "0"], env=env) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    for k in r0.files:
        assert np.array_equal(r0[k].view(np.uint32), r1[k].view(np.uint32)), "ranks disagree on " + k
    sys.path.insert(0, HERE)
    import _dist_worker_gpu as w
    single = w.run_single_process(4, mode, quant, ef=ef)
    for k in single:
        assert np.array_equal(single[k].view(np.uint32), r0[k].view(np.uint32)), k


def test_failed_capture_leaves_no_graph_table_behind():
    """A launch that raises between _graph_tables() and _graph_tables_done() (an invalidated capture, a launch error) must not
    leave the group's descriptor pointing at the graph's own header: the eager launches the quantizer falls back to would read
    their gradient pointers from it.  After the failure the descriptor reads the shared device header again, the next eager
    encode re-sends it, and the step's result equals a fresh quantizer's."""
    sys.path.insert(0, HERE)
    import _dist_worker_gpu as w
    q, params = w.build(1, "ps", "hsq")
    ref_q, ref_params = w.build(1, "ps", "hsq")
    def step(qq, pp, st):
        for p, gr in zip(pp, w.grads_for(0, st)):
            p.grad = gr.cuda()
        qq.record(0, epoch=1)
        qq.apply()
        return [p.grad.data.clone() for p in pp]
    step(q, params, 0)
    obj = q._groups[0][2]
    shared = obj._dev.data_ptr()
    assert obj._batch.s.seg_table == shared
    header = obj._host[obj._last_slot].to("cuda")
    real_levels = obj._batch.levels
    def boom(*a, **k):
        raise RuntimeError("injected launch failure")
    obj._batch.levels = boom
    grads = [params[i].grad for i in obj.idxs]
    dense = list(q._pick_dense([p.grad for p in params])) if obj.ndense else None
    with pytest.raises(RuntimeError, match="injected"):
        obj.encode(grads, q._wire[0], 0, 0, graph_header=header, dense=dense)
    obj._batch.levels = real_levels
    assert obj._batch.s.seg_table == shared and obj._last_ptrs is None and not obj._acc_clean
    for st in (1, 2, 3):
        a, b = step(q, params, st), step(ref_q, ref_params, st)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("quant,ef,steps", [("hsq", False, 2), ("hsq", True, 5), ("qsgd", True, 5)])
def test_two_ranks_two_phase_stochastic_rounding_agrees_across_ranks(tmp_path, quant, ef, steps):
    """--two-phase --random 1 on two ranks: the second phase (ps_quantizer.py:52-61) is replicated on every rank, so its
    stochastic rounding must draw the SAME numbers everywhere -- the { seed, step } pair of the two-phase slot leaves the
    rank out (PSQuantizer._rng_pairs_for) -- or the replicas apply different gradients and, under error feedback, carry
    different server residuals.  The applied gradients of every step are bit-equal on both ranks; steps >= 3 replay graphs."""
    import subprocess
    import sys
    script = os.path.join(HERE, "_dist_worker_gpu.py")
    out = str(tmp_path / "res")
    port = 29700 + (os.getpid() % 1500) + {"hsq": 0, "qsgd": 7}[quant] + (13 if ef else 0)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GQ_TEST_STEPS=str(steps))
    procs = [subprocess.Popen([sys.executable, script, str(r), "2", out, "ps", quant, "1" if ef else "0", "2", "two_phase=1,random=1"],
                              env=env) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    assert len(r0.files) == steps * 6
    for k in r0.files:
        assert np.array_equal(r0[k].view(np.uint32), r1[k].view(np.uint32)), "ranks disagree on " + k


@pytest.mark.parametrize("exchange,users", [("direct", 2), ("split", 1), ("auto", 1), ("pipelined", 1)])
def test_two_ranks_on_one_gpu_every_exchange_transport(tmp_path, exchange, users):
    """gq_amd/exchange.py with the real kernels: direct all-pairs, split (the tensors below the cut are decoded by the
    multi-tensor kernels' "head" launch while the rest of the wire is in flight, then the "tail" launch), pipelined (the same
    with $GQ_PIPELINE_CHUNKS ranges: a launch over the group's tensors of each range as it arrives) and auto ==
    the same users in one process, bit for bit (HSQ and the small dense tensors; error feedback on)."""
    import subprocess
    import sys
    script = os.path.join(HERE, "_dist_worker_gpu.py")
    out = str(tmp_path / "res")
    port = 29900 + (os.getpid() % 1500) + len(exchange)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GQ_EXCHANGE=exchange)
    procs = [subprocess.Popen([sys.executable, script, str(r), "2", out, "ps", "hsq", "1", str(users)], env=env) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    for k in r0.files:
        assert np.array_equal(r0[k].view(np.uint32), r1[k].view(np.uint32)), "ranks disagree on " + k
    sys.path.insert(0, HERE)
    import _dist_worker_gpu as w
    single = w.run_single_process(2 * users, "ps", "hsq", ef=True)
    for k in single:
        assert np.array_equal(single[k].view(np.uint32), r0[k].view(np.uint32)), k


def test_bench_two_rank_code_path_on_one_gpu():
    """bench.py --gpus 2 as the driver launches it (torch.distributed.run, one JSON line from rank 0), with the
    GQ_BENCH_BACKEND=gloo test hook so that both ranks can share this box's one GPU: barriers, all-gather of the
    wire, decode-mean over two payloads, aggregate value."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    env = dict(os.environ, GQ_BENCH_BACKEND="gloo")
    port = 29650 + (os.getpid() % 300)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["ranks"] == 2 and "cpu_baseline" not in d and d["roofline"]["kernel_ms"] > 0



@pytest.mark.parametrize("workload", ["hsq", "qsgd"])
def test_bench_plain_run_times_its_steps_and_dumps_the_same_outputs_twice(workload, tmp_path, oracle):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` without --full: one JSON line with the headline keys only
    (none of --full's objects), `steps` == K, and DIR/<name>.npy in float32 / float64 under 64 MB -- bit-identical from one
    run to the next.  hsq: the dumped wire decodes (CPU oracle) to the dumped sample of the decoded gradient."""
    import json
    import subprocess
    root = os.path.dirname(HERE)
    sys.path.insert(0, root)
    import bench
    dumps = []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--workload", workload,
               "--dump-outputs", d]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-1500:]
        line = json.loads(lines[0])
        assert line["steps"] == 7 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["dtype"] == "f32"
        assert line["higher_is_better"] is True and line["unit"] == "elements/s" and line["value"] > 0 and line["ms_per_step"] > 0
        assert abs(line["value"] * line["ms_per_step"] * 1e-3 - line["config"]["elements_per_rank"]) < 1e-6 * line["value"]
        for extra in ("roofline", "phases_ms", "cpu_baseline", "workloads", "variants", "timed_windows", "ranks_bit_identical"):
            assert extra not in line, extra
        files = sorted(os.listdir(d))
        got = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
        assert files and all(f.endswith(".npy") for f in files)
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
        dumps.append(got)
    assert set(dumps[0]) == set(dumps[1])
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name].view(np.uint8), dumps[1][name].view(np.uint8)), name
    got = dumps[0]
    if workload == "hsq":
        from gq_amd.codebook import load_codebook
        assert set(got) == {"codes", "levels", "lb_ub", "decoded_sample", "decoded_checksums"}
        M = bench.SIZE // bench.C_DIM
        assert got["codes"].shape == (M,) and got["levels"].shape == (M,) and got["lb_ub"].shape == (2,)
        dec = oracle.hsq_decompress(got["codes"].astype(np.int32), got["levels"].astype(np.int32), got["lb_ub"][0], got["lb_ub"][1],
                                    load_codebook(bench.C_DIM, 1 << bench.K_BIT), bench.N_BIT)
        want = dec.reshape(M, bench.C_DIM)[bench.sample_index(np, M)].reshape(-1)
        assert np.array_equal(got["decoded_sample"].view(np.uint32), want.view(np.uint32))
        assert got["decoded_checksums"].shape == (1, 2)
    else:
        assert set(got) == {"grads_sample", "grads_checksums"} and got["grads_checksums"].shape == (161, 2)
        assert np.isfinite(got["grads_sample"]).all() and got["grads_sample"].size == bench.DUMP_SAMPLE_BLOCKS * 16


def test_integration_example_runs():
    """tools/integration_example.py -- INTEGRATION.md section 3's ctypes stubs (per-tensor calls, the gq_hsq_batch descriptor
    and gq_step_tail with every table built by hand) -- against the package's own classes and torch.stack().mean(0)."""
    import subprocess
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "integration_example.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DIFFERS" not in r.stdout and r.stdout.count("equal") >= 8, r.stdout[-2000:] + r.stderr[-2000:]


def test_bench_watchdog_ends_a_hung_transport_and_fresh_ranks_finish_on_the_all_gather():
    """A rank that never joins the first collective of `--exchange direct` ($GQ_BENCH_TEST_HANG): the other rank's watchdog
    ends the job after $GQ_BENCH_TIMEOUT_S with exit code 3 and what was in flight on stderr; the self-launched parent
    then starts FRESH ranks (new processes, no exec) on the all-gather, which print the one JSON line."""
    import json
    import subprocess
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GQ_BENCH_BACKEND="gloo", GQ_BENCH_TIMEOUT_S="20", GQ_BENCH_TEST_HANG="direct")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--exchange", "direct"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "bench_watchdog" in r.stderr and "first exchange" in r.stderr and "starting fresh ranks with --exchange allgather" in r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["exchange"]["transport"] == "allgather" and d["exchange"]["rccl_ranks"] == 2


def test_bench_fails_when_the_collectives_joined_fewer_ranks_than_were_launched():
    """`bench.py --gpus 2` whose collective library reports one joined rank ($GQ_BENCH_TEST_RANKS): the line is printed, the
    exchange object is repeated on stderr, and the exit code is 4 -- such a line is not a 2-GPU measurement."""
    import subprocess
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GQ_BENCH_BACKEND="gloo", GQ_BENCH_TEST_RANKS="1")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode != 0
    assert "the collectives joined 1 ranks, not 2" in r.stderr and '"rccl_ranks": 1' in r.stderr


@pytest.mark.parametrize("extra", [[], ["--exchange", "split"], ["--exchange", "auto"], ["--workload", "qsgd"], ["--workload", "resnet50"],
                                   ["--exchange", "pipelined"], ["--exchange", "pipelined", "--workload", "resnet50"]])
def test_bench_launches_its_own_ranks(extra):
    """`python bench.py --gpus 2 --full` from a bare shell (no RANK / WORLD_SIZE): bench.py starts its own two ranks before
    anything touches the GPU and rank 0 prints the one JSON line (GQ_BENCH_BACKEND=gloo: both ranks share this GPU)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["GQ_BENCH_BACKEND"] = "gloo"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--full"] + extra
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["value"] > 0 and d["ranks_bit_identical"] is True
    assert d["exchange"]["ranks"] == 2 and d["exchange"]["backend"] == "gloo"
    # the self-explaining part of a first multi-GPU run: ranks COUNTED by a collective, and both transports timed in every run
    assert d["exchange"]["rccl_ranks"] == 2 and "rccl_version" in d["exchange"]
    assert set(d["exchange"]["ms_by_transport"]) == {"allgather", "direct"}
    assert all(isinstance(v, float) and v > 0 for v in d["exchange"]["ms_by_transport"].values()), d["exchange"]["ms_by_transport"]
    if extra[:1] == ["--exchange"]:
        assert d["exchange"]["transport"] == (extra[1] if extra[1] in ("split", "pipelined") else d["exchange"]["transport"])
        if extra[1] == "auto":     # opt-in: every transport timed before the timed region, all ranks decide alike
            assert d["exchange"]["transport"] in ("allgather", "direct", "split")
            assert set(d["exchange"]["autotune_ms"]) == {"allgather", "direct", "split"}
    elif not extra:     # the default is the in-place all-gather, nothing is auto-tuned
        assert d["exchange"]["transport"] == "allgather" and d["exchange"]["autotune_ms"] is None
        assert d["exchange"]["ms"] > 0


def test_a_gradient_replaced_at_the_same_address_is_revalidated():
    """Round-2 advisor: the pointer-table fast path returned before the dtype / contiguity checks.  A gradient that comes
    back at the SAME address as a strided view must not be read as if it were contiguous: the group refuses it and the
    step takes the per-tensor path (which makes it contiguous), with the reference's result."""
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    dev = torch.device("cuda:0")
    shapes = [(64, 64), (64, 64), (32, 64)]
    params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]
    q = Quantizer(NearestNeighborCompressor, params, make_args(num_users=1))
    torch.manual_seed(11)
    store = [torch.randn(s, device=dev) for s in shapes]

    def step(grads):
        for p, g in zip(params, grads):
            p.grad = g
        q.record(0, epoch=1)
        q.apply()
        return [p.grad.data.clone() for p in params]
    first = step([g.view(g.shape) for g in store])
    assert q._groups[0][2].ready
    # same storage, same data_ptr, but a transposed (non-contiguous) view for tensor 0.  (apply() rebinds .data of the
    # tensor objects it was given, like the reference's `param.grad.data = g`: the expected input is copied first.)
    t0 = store[0].t()
    assert t0.data_ptr() == store[0].data_ptr() and not t0.is_contiguous()
    expect_in = [t0.contiguous().clone(), store[1].clone(), store[2].clone()]
    second = step([t0, store[1].view(shapes[1]), store[2].view(shapes[2])])
    qp = Quantizer(NearestNeighborCompressor, [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes],
                   make_args(num_users=1, gq_no_batch=True))
    for p, g in zip(qp.parameters, expect_in):
        p.grad = g
    qp.record(0, epoch=1)
    qp.apply()
    for a, p in zip(second, qp.parameters):
        assert torch.equal(a.view(torch.int32), p.grad.data.view(torch.int32))
    assert not torch.equal(first[0], second[0])


@pytest.mark.parametrize("kw", [dict(random=0), dict(random=1), dict(random=1, gq_rng="keyed"), dict(random=0, ef=True, scale="0.5"),
                                dict(qsgd=True, c_dim=128, n_bit=2, random=1), dict(random=1, ef=True, scale="0.5"),
                                dict(random=1, gq_rng="keyed", gq_wire_levels="packed6", n_bit=5),
                                dict(qsgd=True, c_dim=128, n_bit=2, random=1, gq_rng="keyed"),
                                dict(qsgd=True, c_dim=0, n_bit=1, random=1, gq_rng="keyed", ef=True, scale="0.5")])
def test_record_replayed_from_a_hip_graph_equals_the_eager_launches(kw):
    """gq_graph: from the second sighting of a set of gradient addresses on, record() replays its device work (header copy,
    encode, levels, the dense tensors' copy) as ONE graph launch, and apply() its decode-mean launches (one graph per output
    buffer).  Same aggregates, wire and residuals as the eager launches, over steps that alternate between two address sets
    and then move to a third."""
    from gq_amd.compressors import NearestNeighborCompressor, QSGDCompressor
    from gq_amd.quantizers import Quantizer
    kw = dict(kw)
    Comp = QSGDCompressor if kw.pop("qsgd", False) else NearestNeighborCompressor
    shapes = RESNET50_COMPRESSED[:12] + RESNET50_SMALL[:4]
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    store = [[torch.randn(s, device=dev) * 1e-2 for s in shapes] for _ in range(3)]      # three address sets
    fills = [[torch.randn(s, device=dev) * 1e-2 for s in shapes] for _ in range(9)]      # what the gradients hold, step by step
    order = [0, 1, 0, 1, 0, 1, 2, 2, 2]

    def run(graph):
        from gq_amd import compressors
        compressors._seed_counter[0] = 0      # gq_rng = "device": both runs start from the same { seed, step } words
        params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]
        q = Quantizer(Comp, params, make_args(num_users=1, gq_graph=graph, **kw))
        outs = []
        for step, k in enumerate(order):
            for t, f in zip(store[k], fills[step]):
                t.copy_(f)
            for p, t in zip(params, store[k]):
                p.grad = t.view(t.shape)      # a fresh object at the same address (apply() rebinds .data of the object)
            q.record(0, epoch=1)
            q.apply()
            outs.append([p.grad.data.clone() for p in params])
        return q, outs

    qg, og = run(True)
    qe, oe = run(False)
    counts = qg.graph_counts()      # one graph per address set + the address-free one (round 6) that serves a set's first sightings
    assert counts["record"] == 3 and counts["record_any_address"] == 1 and not qe._rec_graphs, counts
    assert counts["apply"] == 2 and not qe._apply_graphs     # the two output buffers in turn
    for a, b in zip(og, oe):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(qg._wire, qe._wire)
    if kw.get("ef"):
        for pg, pe in zip(qg.parameters, qe.parameters):
            assert torch.equal(pg.error[0], pe.error[0])


def test_switching_graphs_off_after_captures_runs_eager_launches_again():
    """`q.use_graphs = False` on a quantizer that has been replaying whole-step graphs (bench.py does it to arm the encode's profile
    events; a failed capture does it too): the next records run their launches eagerly -- the short way through record()
    (PSQuantizer._replay_known_step) looks at the switch every time -- and give the replayed steps' bits."""
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    shapes = RESNET50_COMPRESSED[:8] + RESNET50_SMALL[:3]
    dev = torch.device("cuda:0")
    torch.manual_seed(9)
    store = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    fills = [[torch.randn(s, device=dev) * 1e-2 for s in shapes] for _ in range(16)]

    def run(switch_at):
        params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]
        q = Quantizer(NearestNeighborCompressor, params, make_args(num_users=1, random=0))
        outs = []
        for step in range(16):
            if step == switch_at:
                q.use_graphs = False
            for t, f in zip(store, fills[step]):
                t.copy_(f)
            for p, t in zip(params, store):
                p.grad = t.view(t.shape)
            q.record(0, epoch=1)
            q.apply()
            outs.append([p.grad.data.clone() for p in params])
        return q, outs
    qa, oa = run(None)
    qb, ob = run(10)
    assert qa.record_paths["whole_step"] >= 8 and qa.record_paths["eager"] <= 3
    assert qb.record_paths["eager"] >= 6 + 2, qb.record_paths      # the six steps after the switch ran eagerly
    for a, b in zip(oa, ob):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("kw", [dict(random=1), dict(random=0, ef=True, scale="0.5"), dict(qsgd=True, c_dim=128, n_bit=2, random=1),
                                dict(random=1, num_users=3), dict(random=0, two_phase=True)])
def test_gradients_at_new_addresses_every_step_replay_the_address_free_graph(kw):
    """A training loop whose backward allocates the gradients anew (optimizer.zero_grad() sets them to None) shows record() a new
    set of gradient addresses nearly every step: no per-address graph ever pays.  Round 6: ONE address-free graph per (slot, user)
    -- the launches read the shared device header, refreshed by one pinned copy in front of the replay -- serves every set, the
    whole step included at one user.  24 steps with every gradient in freshly allocated storage: from the third step on nothing
    runs eagerly, and aggregates, wire and residuals equal the eager quantizer's bit for bit."""
    from gq_amd.compressors import NearestNeighborCompressor, QSGDCompressor
    from gq_amd.quantizers import Quantizer
    kw = dict(kw)
    users = kw.pop("num_users", 1)
    Comp = QSGDCompressor if kw.pop("qsgd", False) else NearestNeighborCompressor
    shapes = RESNET50_COMPRESSED[:12] + RESNET50_SMALL[:4]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)

    def run(graph):
        from gq_amd import compressors
        compressors._seed_counter[0] = 0
        gen.manual_seed(77)
        params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]
        q = Quantizer(Comp, params, make_args(num_users=users, gq_graph=graph, **kw))
        outs, hold, seen = [], [], set()
        for step in range(24):
            for u in range(users):
                hold.append(torch.empty(1000 + 4096 * ((7 * step + u) % 5), device=dev))      # (shifts what the allocator hands out next)
                for p, s in zip(params, shapes):
                    p.grad = torch.randn(s, device=dev, generator=gen) * 1e-2               # new storage, as autograd's first write into a None grad
                seen.add(tuple(p.grad.data_ptr() for p in params))
                q.record(u, epoch=1)
            q.apply()
            outs.append([p.grad.data.clone() for p in params])
            if len(hold) > 6:
                del hold[:3]
        return q, outs, len(seen)

    qg, og, sets = run(True)
    qe, oe, _ = run(False)
    assert sets >= 12, "the test's allocation pattern no longer moves the gradients (%d address sets)" % sets
    paths, counts = qg.record_paths, qg.graph_counts()
    assert counts["record_any_address"] == users, counts
    assert paths["eager"] <= 2 * users + 1, paths      # (two sightings per slot, one more for the very first record, which builds the groups)
    if users == 1 and not kw.get("two_phase"):
        assert counts["whole_step_any_address"] >= 1 and paths["whole_step_any_address"] >= 12, (counts, paths)
    for a, b in zip(og, oe):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(qg._wire, qe._wire)
    if kw.get("ef"):
        for pg, pe in zip(qg.parameters, qe.parameters):
            assert torch.equal(pg.error[0], pe.error[0])


@pytest.mark.parametrize("kw", [dict(random=1), dict(random=0, ef=True, scale="0.5"), dict(qsgd=True, c_dim=128, n_bit=2, random=1)])
def test_whole_step_replayed_as_one_graph_equals_the_eager_launches(kw, monkeypatch):
    """One rank, args.num_users == 1: once a set of gradient addresses has its record graph, record() replays the compress AND
    the decode-mean launches of the step as ONE graph (PSQuantizer._step_graphs) and apply() only rebinds the gradients.
    Same aggregates, wire and residuals as eager launches over 14 steps on two alternating address sets; $GQ_FUSE_STEP=0 keeps
    the two graphs per step and gives the same bits too."""
    from gq_amd.compressors import NearestNeighborCompressor, QSGDCompressor
    from gq_amd.quantizers import Quantizer
    kw = dict(kw)
    Comp = QSGDCompressor if kw.pop("qsgd", False) else NearestNeighborCompressor
    shapes = RESNET50_COMPRESSED[:10] + RESNET50_SMALL[:4]
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    store = [[torch.randn(s, device=dev) * 1e-2 for s in shapes] for _ in range(2)]
    order = [0, 1] * 7
    fills = [[torch.randn(s, device=dev) * 1e-2 for s in shapes] for _ in order]

    def run(graph, fuse="1"):
        from gq_amd import compressors
        compressors._seed_counter[0] = 0
        monkeypatch.setenv("GQ_FUSE_STEP", fuse)
        params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]
        q = Quantizer(Comp, params, make_args(num_users=1, gq_graph=graph, **kw))
        outs, fused_steps = [], 0
        for step, k in enumerate(order):
            for t, f in zip(store[k], fills[step]):
                t.copy_(f)
            for p, t in zip(params, store[k]):
                p.grad = t.view(t.shape)
            q.record(0, epoch=1)
            fused_steps += q._fused is not None
            q.apply()
            outs.append([p.grad.data.clone() for p in params])
        return q, outs, fused_steps

    qf, of, nf = run(True)
    q2, o2, n2 = run(True, fuse="0")
    qe, oe, ne = run(False)
    assert qf.graph_counts()["whole_step"] == 2 and nf >= 4, (qf.graph_counts(), nf)
    assert not q2._step_graphs and n2 == 0 and ne == 0
    for other in (of, o2):
        for a, b in zip(other, oe):
            for x, y in zip(a, b):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(qf._wire, qe._wire) and torch.equal(q2._wire, qe._wire)
    if kw.get("ef"):
        for pf, pe in zip(qf.parameters, qe.parameters):
            assert torch.equal(pf.error[0], pe.error[0])


def test_launch_plan_replays_a_chain_of_kernels_and_refuses_other_graphs():
    """gq_launch_plan_*: the kernel nodes of a captured graph issued as plain launches give what the graph's own replay gives; a
    graph that is not ONE chain of kernel launches (a copy node, two branches, no node) is refused with an error text and no plan."""
    from gq_amd import native
    dev = torch.device("cuda:0")
    x = torch.zeros(4096, device=dev)
    y, z = torch.empty_like(x), torch.empty_like(x)
    torch.cuda.synchronize()

    def chain():
        torch.add(x, 1.0, out=y)
        torch.mul(y, 2.0, out=z)
    chain()                                     # (first calls outside a capture)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with _capture(g):
        chain()
    plan = native.LaunchPlan(g)
    assert plan.nodes == 2
    for v in (3.0, -1.5):
        x.fill_(v)
        z.zero_()
        plan.replay()
        torch.cuda.synchronize()
        assert torch.equal(z, (x + 1.0) * 2.0)
    g.instantiate()
    x.fill_(7.0)
    g.replay()                                  # the graph itself still replays next to its plan
    torch.cuda.synchronize()
    assert float(z[0]) == 16.0
    # a copy node in the chain
    g2 = torch.cuda.CUDAGraph(keep_graph=True)
    with _capture(g2):
        torch.add(x, 1.0, out=y)
        z.copy_(y)
    with pytest.raises(native.GQNativeError) as e:
        native.LaunchPlan(g2)
    assert "gq_launch_plan_create" in str(e.value)
    # two branches
    side = torch.cuda.Stream()
    g3 = torch.cuda.CUDAGraph(keep_graph=True)
    with _capture(g3):
        torch.add(x, 1.0, out=y)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            torch.mul(x, 2.0, out=z)
        torch.add(y, 1.0, out=y)
        torch.cuda.current_stream().wait_stream(side)
    with pytest.raises(native.GQNativeError) as e:
        native.LaunchPlan(g3)
    assert "chain" in str(e.value) or "dependents" in str(e.value) or "root" in str(e.value)
    L = native.lib()
    import ctypes
    pl = ctypes.c_void_p(0)
    assert L.gq_launch_plan_create(None, ctypes.byref(pl), None) != 0 and b"null pointer" in L.gq_last_error()
    assert L.gq_launch_plan_run(None, None) != 0 and b"null plan" in L.gq_last_error()
    L.gq_launch_plan_destroy(None)              # (a no-op)


@pytest.mark.parametrize("kw", [dict(random=1), dict(random=1, ef=True, two_phase=True, scale="0.5"), dict(qsgd=True, c_dim=128, n_bit=2, random=1)])
def test_direct_replay_of_captured_steps_equals_the_graphs_own_replay(kw, monkeypatch):
    """$GQ_DIRECT_REPLAY (default 1): a captured record / apply / whole step is replayed as plain launches of its kernel nodes
    (native.LaunchPlan); 0 keeps the graph's own replay.  Twelve steps on two alternating sets of gradient addresses: the same
    aggregates, wire and residuals bit for bit, and the replayed objects are what the switch says."""
    from gq_amd import native
    from gq_amd.compressors import NearestNeighborCompressor, QSGDCompressor
    from gq_amd.quantizers import Quantizer
    kw = dict(kw)
    Comp = QSGDCompressor if kw.pop("qsgd", False) else NearestNeighborCompressor
    shapes = RESNET50_COMPRESSED[:8] + RESNET50_SMALL[:3]
    dev = torch.device("cuda:0")
    torch.manual_seed(9)
    store = [[torch.randn(s, device=dev) * 1e-2 for s in shapes] for _ in range(2)]
    order = [0, 1] * 6
    fills = [[torch.randn(s, device=dev) * 1e-2 for s in shapes] for _ in order]

    def run(direct):
        from gq_amd import compressors
        compressors._seed_counter[0] = 0
        monkeypatch.setenv("GQ_DIRECT_REPLAY", direct)
        params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]
        q = Quantizer(Comp, params, make_args(num_users=1, gq_graph=True, **kw))
        outs = []
        for step, k in enumerate(order):
            for t, f in zip(store[k], fills[step]):
                t.copy_(f)
            for p, t in zip(params, store[k]):
                p.grad = t.view(t.shape)
            q.record(0, epoch=1)
            q.apply()
            outs.append([p.grad.data.clone() for p in params])
        replayed = [e[1] for cache in (q._rec_graphs, q._apply_graphs, q._step_graphs) for e in cache.values() if e[1] is not None]
        return q, outs, replayed

    qd, od, rd = run("1")
    qg, og, rg = run("0")
    assert rd and all(isinstance(r, native.LaunchPlan) for r in rd), [type(r) for r in rd]
    assert rg and not any(isinstance(r, native.LaunchPlan) for r in rg)
    assert qd.graph_counts() == qg.graph_counts()
    for a, b in zip(od, og):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(qd._wire, qg._wire)
    if kw.get("ef"):
        for pd, pg in zip(qd.parameters, qg.parameters):
            assert torch.equal(pd.error[0], pg.error[0]) and torch.equal(pd.server_error, pg.server_error)


def test_garbage_collection_is_held_off_during_a_capture():
    """torch's CUDAGraph destructor raises inside a stream capture and the process aborts (at::cuda::CUDAGraph::~CUDAGraph ->
    c10_hip_check; seen once in round 6 when the interpreter's own collection, started by an allocation count in the middle of
    gq_hsq_levels_decode_batched's capture, finalized an older quantizer's graphs; torch.cuda.graph no longer collects before a
    capture by itself).  The quantizer's captures run with the collector held off (quantizers._capturing).  In a child process: a
    quantizer with captured graphs becomes cyclic garbage, and while a second one captures, a call inside the capture does what
    an automatic collection would do there -- collect if the collector is enabled.  It is not: the process survives, the garbage
    is collected afterwards, and the collector is back on after every capture."""
    import subprocess
    import sys
    code = r"""
import gc, os, sys, weakref
sys.path.insert(0, os.path.join(%r, "gradient-quantization_amd"))
import torch
from argparse import Namespace
from gq_amd import native
from gq_amd.compressors import NearestNeighborCompressor
from gq_amd.quantizers import Quantizer
dev = torch.device("cuda:0")
shapes = [(64, 64, 3, 3), (256, 64), (512, 128), (64,), (10,)]
store = [[torch.randn(s, device=dev) * 1e-2 for s in shapes] for _ in range(2)]
def run(steps):
    params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]
    q = Quantizer(NearestNeighborCompressor, params, Namespace(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=1, ef=False, two_phase=False,
                                                               scale="exp", num_users=1, mode="ps", cr=256, gq_graph=True))
    for st in range(steps):
        for p, t in zip(params, store[st %% 2]):
            p.grad = t.view(t.shape)
        q.record(0, epoch=1)
        q.apply()
    torch.cuda.synchronize()
    return q
gc.set_threshold(10 ** 9)        # no collection by itself: the hook below decides
old = run(8)
assert old.graph_counts()["whole_step"] >= 1
alive = weakref.ref(old)
old.myself = old                 # a cycle: only the collector frees it
del old
assert alive() is not None
seen = []
inner = native.HSQBatch.levels_decode
def hooked(self, *a, **kw):
    if torch.cuda.is_current_stream_capturing():
        seen.append(gc.isenabled())
        if gc.isenabled():       # what an automatic collection at this point would do
            gc.collect()
    return inner(self, *a, **kw)
native.HSQBatch.levels_decode = hooked
new = run(8)
assert new.graph_counts()["whole_step"] >= 1 and seen and not any(seen), seen
assert gc.isenabled() and alive() is not None
gc.collect()
assert alive() is None
print("ok")
""" % (os.path.dirname(HERE),)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-500:], r.stderr[-3000:])


@pytest.mark.parametrize("users", [2, 4, 3])
def test_quantizer_fma_aggregate_is_opt_in_and_within_tolerance(users, monkeypatch):
    """$GQ_AGGREGATE=fma / args.gq_aggregate: the multi-tensor decode-mean accumulates with fused multiply-adds for R >= 2
    payloads (R = 2, 4, 8, 16; other R stay exact).  The wire -- codes, levels, (lb, ub) -- is the exact run's bit for bit, the
    aggregate within 1e-6 relative L2; without the option nothing changes."""
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    dev = torch.device("cuda:0")
    shapes = RESNET50_COMPRESSED[:6] + RESNET50_SMALL[:3]
    torch.manual_seed(31)
    grads = [[torch.randn(s, device=dev) * 1e-2 for s in shapes] for _ in range(users)]

    def run(**kw):
        params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]
        q = Quantizer(NearestNeighborCompressor, params, make_args(num_users=users, random=0, **kw))
        for u in range(users):
            for p, g in zip(params, grads[u]):
                p.grad = g.clone()
            q.record(u, epoch=1)
        wire = q._wire[:users].clone()
        q.apply()
        return wire, [p.grad.data.clone() for p in params]
    w_exact, a_exact = run()
    w_fma, a_fma = run(gq_aggregate="fma")
    assert torch.equal(w_exact, w_fma)
    for x, y in zip(a_exact, a_fma):
        if users == 3:
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        else:
            rel = float((x.double() - y.double()).norm() / x.double().norm())
            assert rel <= 1e-6, rel


def test_device_counter_draws_are_fresh_every_step_reproducible_and_unbiased():
    """gq_rng = "device" on the multi-tensor launches (GQ_RANDOM_DEVICE_COUNTER): the launch arguments never change, the
    stream is keyed by a { seed, step } pair in device memory that every aggregate steps.  The SAME gradient recorded in
    two consecutive steps is rounded with different draws (the keyed variant of round 3 repeated them: ADVICE r3), a second
    quantizer built from the same torch seed reproduces the sequence, and the rounding is unbiased."""
    from gq_amd import compressors
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    dev = torch.device("cuda:0")
    shapes = [(40000, 16), (30000, 16), (10,)]
    torch.manual_seed(22)
    g = [torch.randn(s, device=dev) * 1e-2 for s in shapes]

    def run(random, steps=3):
        compressors._seed_counter[0] = 0
        params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]
        q = Quantizer(NearestNeighborCompressor, params, make_args(num_users=1, random=random))
        out = []
        for _ in range(steps):
            for p, t in zip(params, g):
                p.grad = t.clone()
            q.record(0, epoch=1)
            torch.cuda.synchronize()
            grp = q._groups[0][2]
            out.append([q._wire[0, q.offsets[i] + cd.levels_off:q.offsets[i] + cd.levels_off + cd.M].clone().to(torch.int32)
                        for i, cd in zip(grp.idxs, grp.codecs)])
            q.apply()
        return q, out
    q1, a = run(1)
    q2, b = run(1)
    _, t = run(0, steps=1)
    assert q1._groups[0][2].counter and q1._rng_state is not None and int(q1._rng_state[0, 1]) == 3     # three aggregates, three steps
    for s1, s2 in zip(a, b):
        for x, y in zip(s1, s2):
            assert torch.equal(x, y)                                  # same torch seed: the same sequence of draws
    for x0, x1, x2, w in zip(a[0], a[1], a[2], t[0]):
        assert (x0 != x1).float().mean() > 0.2 and (x1 != x2).float().mean() > 0.2     # the same gradient, new draws every step
        for x in (x0, x1, x2):
            d = (x - w).float()
            assert bool(((d == 0) | (d == 1)).all()) and 0.47 < float(d.mean()) < 0.53


def test_keyed_draws_are_new_for_every_gradient_and_round_without_bias():
    """gq_rng = "keyed" (GQ_RANDOM_DEVICE_KEYED): the seed never changes, every tensor's stream is keyed by its (lb, ub).
    The same gradient gives the same levels, another gradient other draws, and the rounding is unbiased: against the
    truncated levels the stochastic ones are half a level higher on average."""
    from gq_amd.compressors import NearestNeighborCompressor
    from gq_amd.quantizers import Quantizer
    dev = torch.device("cuda:0")
    shapes = [(40000, 16), (30000, 16)]

    def levels_of(grads, **kw):
        params = [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]
        q = Quantizer(NearestNeighborCompressor, params, make_args(num_users=1, **kw))
        for p, g in zip(params, grads):
            p.grad = g.clone()
        q.record(0, epoch=1)
        torch.cuda.synchronize()
        grp = q._groups[0][2]
        out = []
        for i, cd in zip(grp.idxs, grp.codecs):
            off = q.offsets[i]
            out.append(q._wire[0, off + cd.levels_off:off + cd.levels_off + cd.M].clone().to(torch.int32))
        return out
    torch.manual_seed(21)
    g1 = [torch.randn(s, device=dev) * 1e-2 for s in shapes]
    g2 = [g + 1e-6 * torch.randn_like(g) for g in g1]
    a = levels_of(g1, random=1, gq_rng="keyed")
    b = levels_of(g1, random=1, gq_rng="keyed")
    c = levels_of(g2, random=1, gq_rng="keyed")
    t = levels_of(g1, random=0)
    for x, y, z, w in zip(a, b, c, t):
        assert torch.equal(x, y)                                  # same gradient, same draws
        assert (x != z).float().mean() > 0.2                       # another gradient (1e-4 relative away): other draws
        d = (x - w).float()
        assert bool(((d == 0) | (d == 1)).all()) and 0.47 < float(d.mean()) < 0.53


def test_training_driver_with_graph_replay_learns_like_the_eager_run():
    """A real training loop (fcn, synthetic MNIST-shaped data, two users): backward allocates new gradient tensors every
    iteration, the allocator hands the same blocks out again, and from the second sighting on the quantizer's launches are
    replayed from HIP graphs (--gq-graph with --gq-rng keyed).  Deterministic rounding: the same losses as the eager run."""
    from gq_amd.driver import build_parser, train
    base = ["--network", "fcn", "--dataset", "mnist", "--c-dim", "16", "--k-bit", "8", "--n-bit", "6", "--num-users", "2",
            "--batch-size", "32", "--epochs", "2", "--train-size", "2048", "--lr", "0.05", "--log-interval", "4", "--quantizer", "hsq"]
    _, qg, hist_g = train(build_parser().parse_args(base + ["--gq-graph", "--gq-rng", "keyed"]))
    assert hist_g[-1]["loss"] < 0.7 * hist_g[0]["loss"]
    assert any(e[1] is not None for e in qg._rec_graphs.values()), "no record was ever replayed from a graph"
    _, qe, hist_e = train(build_parser().parse_args(base + ["--no-gq-graph", "--gq-rng", "keyed"]))
    assert not qe._rec_graphs
    assert [h["loss"] for h in hist_g] == [h["loss"] for h in hist_e]


@pytest.mark.parametrize("quant,ef", [("hsq", False), ("hsq", True)])
def test_two_ranks_on_one_gpu_with_graph_replay(tmp_path, quant, ef):
    """gq_graph with more than one rank: every rank's record() and the decode after the exchange replay from graphs
    (the exchange itself stays outside); five steps, == the same users in one eager process, bit for bit."""
    import subprocess
    import sys
    script = os.path.join(HERE, "_dist_worker_gpu.py")
    out = str(tmp_path / "res")
    port = 30100 + (os.getpid() % 1500) + (7 if ef else 0)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GQ_GRAPH="1", GQ_TEST_STEPS="5")
    procs = [subprocess.Popen([sys.executable, script, str(r), "2", out, "ps", quant, "1" if ef else "0"], env=env) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    for k in r0.files:
        assert np.array_equal(r0[k].view(np.uint32), r1[k].view(np.uint32)), "ranks disagree on " + k
    rec, app = map(int, open(out + "_rank0_graphs.txt").read().split())
    assert rec >= 1 and app >= 1, "no graph was captured on rank 0 (%d records, %d applies)" % (rec, app)
    sys.path.insert(0, HERE)
    import _dist_worker_gpu as w
    assert "GQ_GRAPH" not in os.environ
    q, params = w.build(4, "ps", quant, ef=ef)
    single = w.run(q, params, 4, 0, steps=5)
    assert len(single) == len(r0.files)
    for k in single:
        assert np.array_equal(single[k].view(np.uint32), r0[k].view(np.uint32)), k


def test_rccl_single_rank_exchange_calls():
    """The non-staged exchange on the REAL collective library (RCCL cannot put two ranks on one GPU, so: one rank): an
    all_gather_into_tensor of uint8 wire rows -- out of place for fewer rows than slots, in place for all of them -- queued
    behind a kernel of the current stream, Work.wait(), a kernel reading the result, forty times over 3 MB rows; the grouped
    point-to-point transport with no peers; the collectives bench.py uses around its windows (tests/_rccl_one_rank.py)."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    port = 29500 + (os.getpid() % 400)
    r = subprocess.run([sys.executable, os.path.join(here, "_rccl_one_rank.py"), str(port)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rccl one rank ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
