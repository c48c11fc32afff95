"""tests/kmeans_contract.py against the C fmaf, scipy and the exact mean (no GPU), and the host side of codebook training:
the library's ABI, write_fvecs, the command line, and the failure without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import kmeans_contract as kc
from gq_amd import codebook, native

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


# ---- the fmaf restatement ---------------------------------------------------------------------------------------------------
def test_fmaf_breaks_a_double_rounding_tie_by_the_exact_sum():
    """1 + 2^-23 + (2^-24 - 2^-70): the f64 sum lands on the f32 tie 1 + 2^-23 + 2^-24, which round-to-even would send UP to
    1 + 2^-22; the exact sum is below the tie, so fmaf gives 1 + 2^-23.  And the mirrored case."""
    eps = 2.0 ** -23
    a, b, c = F(2.0 ** -24 * (1 + eps)), F(1 - eps), F(1 + eps)
    assert float(a) * float(b) == 2.0 ** -24 * (1 - 2.0 ** -46)
    got = kc.fmaf(np.array([a, a, -a]), np.array([b, -b, b]), np.array([c, -c, -c]))
    assert np.array_equal(got, np.array([c, -c, -c], F))
    # a true tie (the exact sum IS the midpoint) rounds to even
    assert kc.fmaf(np.array([F(2.0 ** -24)]), np.array([F(1)]), np.array([c]))[0] == F(1 + 2 * eps)
    # the subnormal range: 2^-149 * 0.75 + 2^-149 = 1.75 * 2^-149 -> 2 * 2^-149; * 0.5 -> a tie at 1.5 -> even = 2
    tiny = F(2.0 ** -149)
    assert kc.fmaf(np.array([tiny, tiny]), np.array([F(0.75), F(0.5)]), np.array([tiny, tiny])).tolist() == [2 * float(tiny)] * 2


def _tie_rows(cb, rng):
    """Rows whose two best |<x, c>| nearly tie (sums and differences of two codewords), lattice rows whose chains hit f32
    rounding ties, and the engineered double-rounding pair of the test above in the first two coordinates."""
    K, d = cb.shape
    a, b = rng.randint(0, K, 200), rng.randint(0, K, 200)
    near = np.concatenate([cb[a] + cb[b], cb[a] - cb[b], cb[a] + cb[b] * F(1 + 2.0 ** -20)])
    lattice = (rng.randint(-4096, 4097, (300, d)) * 2.0 ** -12).astype(F)
    eng = np.zeros((2, d), F)
    eps = 2.0 ** -23
    eng[:, 0] = 1 + eps
    if d > 1:
        eng[:, 1] = [2.0 ** -24 * (1 + eps), -(2.0 ** -24) * (1 + eps)]
    return np.concatenate([near, lattice, eng]).astype(F)


@pytest.mark.parametrize("d", [8, 12, 16, 24, 32])
def test_absdot_assignment_equals_the_scalar_oracle(oracle, d):
    """The C fmaf chain (oracle.hsq_encode_scalar) and the restatement: codes == labels, u == dot, bit for bit."""
    rng = np.random.RandomState(100 + d)
    shipped = codebook.load_codebook(d, 256)
    lattice_cb = (rng.randint(-4096, 4097, (64, d)) * 2.0 ** -12).astype(F)
    lattice_cb[0, :2] = [1, 1 - 2.0 ** -23][:min(2, d)]
    lattice_cb[1] = lattice_cb[0]      # a duplicate: the lower index wins
    for cb in (shipped, lattice_cb):
        X = np.concatenate([
            rng.standard_normal((600, d)).astype(F),
            codebook.normalize_rows(rng.standard_normal((300, d)).astype(F))[1],
            _tie_rows(cb, rng),
            (rng.standard_normal((100, d)) * 1e-41).astype(F),      # subnormal entries
            (rng.standard_normal((100, d)) * 1e-20).astype(F),      # products in the subnormal range
            np.zeros((1, d), F),
        ])
        labels, signs, dot = kc.assign(X, cb, kc.ABSDOT)
        codes, u = oracle.hsq_encode_scalar(X.reshape(-1), cb)
        assert np.array_equal(labels, codes)
        assert np.array_equal(dot.view(np.uint32), u.view(np.uint32))
        assert np.array_equal(signs, np.where(u < 0, -1, 1).astype(np.int8))


# ---- euclid against scipy and the exact mean --------------------------------------------------------------------------------
CASES = [(16, 64, 20000), (8, 32, 4099), (12, 256, 20000)]
_inputs = {}


def euclid_input(d, K, N):
    """Unit Gaussians and K of them as initial centroids; points whose two best scores are closer than 1e-5 are left out, so
    that an f32 rounding cannot decide a label (scipy computes distances another way)."""
    if (d, K, N) not in _inputs:
        X = kc.unit_gaussians(N, d, 808)
        init = np.ascontiguousarray(codebook.initial_centroids(X, K, 808))
        _, _, _, t = kc.assign(X, init, kc.EUCLID, with_scores=True)
        top = np.sort(t, axis=1)[:, -2:]
        X = np.ascontiguousarray(X[(top[:, 1] - top[:, 0]) > 2e-5])
        _inputs[(d, K, N)] = (X, init)
    return _inputs[(d, K, N)]


@pytest.mark.parametrize("d,K,N", CASES)
def test_euclid_iteration_against_scipy(d, K, N):
    import scipy.cluster.vq as vq
    X, init = euclid_input(d, K, N)
    assert X.shape[0] > 0.99 * N
    labels, _, _, t = kc.assign(X, init, kc.EUCLID, with_scores=True)
    top = np.sort(t, axis=1)[:, -2:]
    gap = float((top[:, 1] - top[:, 0]).min())
    print("d%d K%d N%d: smallest gap between the best two scores %.3g" % (d, K, X.shape[0], gap))
    assert gap > 1e-5      # the precondition of the comparison
    C1, labels1, _, counts = kc.run(X, init, kc.EUCLID, 1)
    ref_C, ref_labels = vq.kmeans2(X, init.copy(), iter=1, minit="matrix")
    assert np.array_equal(labels1, labels) and np.array_equal(counts, np.bincount(labels, minlength=K))
    assert np.array_equal(labels1, ref_labels.astype(np.int32))
    err = float(np.abs(C1.astype(np.float64) - ref_C.astype(np.float64)).max())
    print("d%d K%d N%d: max |centroid - scipy's| %.3g" % (d, K, X.shape[0], err))
    assert err <= 1e-6
    # the exact mean: quantisation <= 2^-41 per point, then one f32 rounding of a value below 1 (half an ulp <= 2^-25)
    for k in range(K):
        mean = X[labels == k].astype(np.float64).mean(axis=0)
        assert np.abs(C1[k].astype(np.float64) - mean).max() <= 2.0 ** -24


@pytest.mark.parametrize("d,K,N,iters", [(8, 32, 4099, 5), (8, 32, 4099, 20), (16, 64, 20000, 5)])
def test_euclid_inertia_after_several_iterations_against_scipy(d, K, N, iters):
    """The trajectories part in a few labels (a near-tie decided differently), so only the objective is compared."""
    import scipy.cluster.vq as vq
    X, init = euclid_input(d, K, N)
    C, labels, _, _ = kc.run(X, init, kc.EUCLID, iters)
    ref_C, ref_labels = vq.kmeans2(X, init.copy(), iter=iters, minit="matrix")
    a, b = kc.inertia(X, C, labels), kc.inertia(X, ref_C, ref_labels)
    print("d%d K%d N%d iters %d: inertia %.12g against scipy's %.12g (relative difference %.3g), %d labels differ"
          % (d, K, X.shape[0], iters, a, b, abs(a - b) / b, int((labels != ref_labels).sum())))
    assert abs(a - b) / b <= 1e-6


def test_absdot_update_and_unchanged_rows():
    """Step 5 on hand-made sums: an empty row and a row whose mirrored points cancel keep their bits; the others are S / |S|
    in f64, rounded once."""
    C = np.array([[1, 0], [0, 1], [-0.0, 0.5], [0.6, 0.8]], F)
    X = np.array([[1, 0], [-1, 0], [0, 1], [0, 1]], F)
    labels, signs = np.array([0, 0, 1, 1], np.int32), np.array([1, 1, 1, 1], np.int8)
    S, n = kc.accumulate(X, labels, signs, 4)
    assert S.tolist() == [[0, 0], [0, 2 ** 41], [0, 0], [0, 0]] and n.tolist() == [2, 2, 0, 0]
    out = kc.update(C, S, n, kc.ABSDOT)
    assert np.array_equal(out.view(np.uint32), np.array([[1, 0], [0, 1], [-0.0, 0.5], [0.6, 0.8]], F).view(np.uint32))
    out = kc.update(C, S, n, kc.EUCLID)
    assert np.array_equal(out.view(np.uint32), np.array([[0, 0], [0, 1], [-0.0, 0.5], [0.6, 0.8]], F).view(np.uint32))
    assert kc.quantise(np.array([[2.0 ** -42, -(2.0 ** -41), 3 * 2.0 ** -41, 1, -1]], F)).tolist() == [[0, 0, 2, 2 ** 40, -2 ** 40]]


# ---- the host side ----------------------------------------------------------------------------------------------------------
def test_kmeans_library_is_built_and_exports_its_abi(tmp_path):
    if not os.path.exists(native.KMEANS_LIB_PATH):
        pytest.fail("libgq_kmeans.so is not built (build() makes it)")
    L = native.kmeans_lib()
    assert L.gq_kmeans_abi_version() == native.KMEANS_ABI_VERSION
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "gq_kmeans.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)      # declarations only: the comments name the entry points too
    declared = sorted(set(re.findall(r"\b(gq_kmeans_\w+)\s*\(", code)))
    assert declared == sorted(native.KMEANS_EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", native.KMEANS_LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("gq"))
    assert exported == declared
    for name, value in (("ABI_VERSION", native.KMEANS_ABI_VERSION), ("MAX_D", native.KMEANS_MAX_D), ("MAX_K", native.KMEANS_MAX_K),
                        ("MAX_N", native.KMEANS_MAX_N), ("EUCLID", native.KMEANS_EUCLID), ("ABSDOT", native.KMEANS_ABSDOT),
                        ("THREADS", native.KMEANS_THREADS), ("BLOCKS_PER_CU", native.KMEANS_BLOCKS_PER_CU)):
        assert re.search(r"#define GQ_KMEANS_%s %d\b" % (name, value), hdr), name
    assert "#define GQ_KMEANS_GLOBAL_ATOMICS 0x%x" % native.KMEANS_GLOBAL_ATOMICS in hdr
    assert native.kmeans_workspace_bytes(256, 16) == 8 * 256 * 17
    assert native.kmeans_workspace_bytes(4097, 16) == 0 and native.kmeans_workspace_bytes(4, 65) == 0
    # the loader's two failures, as for the other libraries
    desc = native.KMEANS_LIBRARY
    saved = (desc.path, desc.abi, desc.handle)
    try:
        desc.handle, desc.path = None, str(tmp_path / "libgq_kmeans.so")
        with pytest.raises(native.GQNativeError, match="libgq_kmeans.so not found"):
            native.kmeans_lib()
        desc.path, desc.abi = saved[0], saved[1] + 1
        with pytest.raises(native.GQNativeError, match="rebuild it"):
            native.kmeans_lib()
    finally:
        desc.path, desc.abi, desc.handle = saved
    assert native.kmeans_lib() is not None


def test_write_fvecs_round_trip_and_truncation(tmp_path):
    rng = np.random.RandomState(3)
    a = rng.standard_normal((37, 12)).astype(F)
    a[0, 0], a[1, 1], a[2, 2] = -0.0, np.float32(1e-42), np.inf
    p = str(tmp_path / "a.fvecs")
    codebook.write_fvecs(p, a)
    assert os.path.getsize(p) == 37 * 13 * 4
    assert np.array_equal(codebook.read_fvecs(p).view(np.uint32), a.view(np.uint32))
    codebook.write_fvecs(p, a[:5])      # a second write replaces the file
    assert np.array_equal(codebook.read_fvecs(p).view(np.uint32), a[:5].view(np.uint32))
    codebook.write_fvecs(p, a[:, ::2])  # a strided view
    assert np.array_equal(codebook.read_fvecs(p).view(np.uint32), np.ascontiguousarray(a[:, ::2]).view(np.uint32))
    with pytest.raises(ValueError):
        codebook.write_fvecs(p, a[0])


def test_cli_arguments_and_overwrite_refusal(tmp_path, capsys, monkeypatch):
    for argv in (["--ks", "4", "--out", str(tmp_path)], ["--dim", "4", "--out", str(tmp_path)], ["--dim", "4", "--ks", "4"],
                 ["--dim", "4", "--ks", "4", "--out", str(tmp_path), "--metric", "cosine"],
                 ["--dim", "0", "--ks", "4", "--out", str(tmp_path)], ["--dim", "4", "--ks", "4", "--iters", "0", "--out", str(tmp_path)],
                 ["--dim", "4", "--ks", "9", "--train-size", "8", "--out", str(tmp_path)]):
        with pytest.raises(SystemExit) as e:
            codebook.main(argv)
        assert e.value.code == 2, argv
    calls = []

    def fake_train(dim, K, **kw):
        calls.append((dim, K, kw))
        return np.full((K, dim), 0.5, F)

    monkeypatch.setattr(codebook, "train_codebook", fake_train)
    argv = ["--dim", "4", "--ks", "3", "--metric", "absdot", "--iters", "7", "--train-size", "50", "--seed", "9", "--out", str(tmp_path)]
    assert codebook.main(argv) == 0
    path = str(tmp_path / "learned_codebook" / "angular_dim_4_Ks_3.fvecs")
    assert capsys.readouterr().out.strip() == path
    assert calls == [(4, 3, dict(train_size=50, iters=7, seed=9, metric="absdot"))]
    assert np.array_equal(codebook.read_fvecs(path), np.full((3, 4), 0.5, F))
    with pytest.raises(SystemExit) as e:      # the file exists: refused before any training
        codebook.main(argv)
    assert e.value.code == 2 and len(calls) == 1 and "--force" in capsys.readouterr().err
    assert codebook.main(argv + ["--force"]) == 0 and len(calls) == 2
    monkeypatch.setenv("GQ_CODEBOOK_DIR", str(tmp_path))
    monkeypatch.chdir(tmp_path)
    assert codebook.codebook_path(4, 3) == path


def test_train_codebook_needs_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(native.GQNativeError):
        codebook.train_codebook(8, 4, train_size=100, iters=1)
    with pytest.raises(native.GQNativeError):
        codebook.train_codebook(8, 4, iters=1, points=np.ones((10, 8), F))
    with pytest.raises(ValueError):
        codebook.train_codebook(8, 4, train_size=100, metric="cosine")
    with pytest.raises(ValueError):      # zero rows are dropped: three points are left for four centroids
        codebook.train_codebook(8, 4, points=np.concatenate([np.ones((3, 8), F), np.zeros((5, 8), F)]))
    with pytest.raises(native.GQNativeError):
        native.kmeans_assign(torch.zeros(4, 8), torch.zeros(2, 8), native.KMEANS_EUCLID, torch.zeros(4, dtype=torch.int32))
