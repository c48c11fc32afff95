"""Codebook training through the public interface on the MI355X: train_codebook against the numpy restatement
(tests/kmeans_contract.py), the command line, and a trained codebook found through GQ_CODEBOOK_DIR and used by
NearestNeighborCompressor, against the CPU oracle bit for bit."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import kmeans_contract as kc
from gq_amd import codebook

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp",
                num_users=1, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("metric", ["euclid", "absdot"])
def test_train_codebook_equals_the_restatement(metric):
    got = codebook.train_codebook(16, 64, train_size=20000, iters=5, seed=1, metric=metric)
    X = codebook.train_points(16, 20000, 1)
    want = kc.run(X, codebook.initial_centroids(X, 64, 1), kc.METRICS[metric], 5)[0]
    assert got.dtype == np.float32 and same_bits(got, want)
    # points given, on the device and on the host, unnormalised and with zero rows: normalised, the zero rows dropped
    raw = np.concatenate([X[:3000] * np.float32(3.0), np.zeros((7, 16), np.float32)])
    norms, unit = codebook.normalize_rows(raw)
    unit = np.ascontiguousarray(unit[norms != 0])
    want = kc.run(unit, codebook.initial_centroids(unit, 64, 1), kc.METRICS[metric], 2)[0]
    for pts in (torch.from_numpy(raw).cuda(), torch.from_numpy(raw), raw):
        assert same_bits(codebook.train_codebook(16, 64, iters=2, seed=1, metric=metric, points=pts), want)


def _use_trained(monkeypatch, out, empty, d, K, k_bit, c_dim, oracle):
    """With GQ_CODEBOOK_DIR = out and an empty cwd: load_codebook finds the file, the compressor builds on it and equals the
    oracle on that codebook."""
    from gq_amd.compressors import NearestNeighborCompressor
    monkeypatch.setenv("GQ_CODEBOOK_DIR", str(out))
    monkeypatch.chdir(empty)
    path = os.path.join(str(out), "learned_codebook", "angular_dim_%d_Ks_%d.fvecs" % (d, K))
    assert codebook.codebook_path(d, K) == path
    cb = codebook.load_codebook(d, K)
    assert cb.shape == (K, d) and same_bits(cb, codebook.normalize_rows(codebook.read_fvecs(path))[1])
    x = (np.random.RandomState(11).standard_normal(d * 4001) * 1e-2).astype(np.float32)
    comp = NearestNeighborCompressor(x.size, torch.Size([x.size]), make_args(c_dim=c_dim, k_bit=k_bit, n_bit=6, random=False))
    assert comp.dim == d and comp.K == K
    xt = torch.from_numpy(x).cuda()
    (lb, ub, levels), codes = comp.compress(xt)
    dec = comp.decompress([(lb, ub, levels), codes])
    ref = oracle.hsq_compress(x, cb, 6, 0)
    assert np.array_equal(codes.cpu().numpy().astype(np.int32), ref["codes"])
    assert np.array_equal(levels.cpu().numpy().astype(np.int32), ref["levels"])
    assert same_bits(np.array([lb.item(), ub.item()], np.float32), np.array([ref["lb"], ref["ub"]], np.float32))
    want = oracle.hsq_decompress(ref["codes"], ref["levels"], ref["lb"], ref["ub"], cb, 6)
    assert same_bits(dec.cpu().numpy().reshape(-1), want)
    return cb


def test_cli_writes_a_codebook_the_compressor_uses(tmp_path, monkeypatch, oracle, capsys):
    out, empty = tmp_path / "books", tmp_path / "empty"
    empty.mkdir()
    argv = ["--dim", "16", "--ks", "64", "--iters", "3", "--train-size", "20000", "--seed", "5", "--out", str(out)]
    assert codebook.main(argv) == 0
    path = str(out / "learned_codebook" / "angular_dim_16_Ks_64.fvecs")
    assert capsys.readouterr().out.strip() == path and os.path.getsize(path) == 64 * 17 * 4
    assert same_bits(codebook.read_fvecs(path), codebook.train_codebook(16, 64, train_size=20000, iters=3, seed=5))
    with pytest.raises(SystemExit):      # no --force: refused
        codebook.main(argv)
    _use_trained(monkeypatch, out, empty, 16, 64, 6, 16, oracle)


def test_a_dimension_and_size_that_ship_nowhere(tmp_path, monkeypatch, oracle):
    """d = 36 (what repaired_dim makes of c_dim 24 on 36 * 4001 elements), K = 32: trained, found and used; the encode takes the
    exact kernel."""
    out, empty = tmp_path / "books", tmp_path / "empty"
    empty.mkdir()
    assert codebook.repaired_dim(36 * 4001, 24) == 36
    with pytest.raises(FileNotFoundError):
        codebook.codebook_path(36, 32)
    assert codebook.main(["--dim", "36", "--ks", "32", "--metric", "absdot", "--iters", "5", "--train-size", "20000", "--out", str(out)]) == 0
    _use_trained(monkeypatch, out, empty, 36, 32, 5, 24, oracle)


def _max_abs_cos(cb):
    unit = codebook.normalize_rows(cb)[1].astype(np.float64)
    cos = unit @ unit.T
    np.fill_diagonal(cos, 0.0)
    return cos


def test_absdot_leaves_no_antipodal_pairs():
    """The Euclidean objective is blind to the sign HSQ ignores: the reference's d16 K32 book holds nearly antipodal pairs
    (cos < -0.99), which are one codeword to the encode.  The absdot objective merges such pairs: 20 iterations on 20000 unit
    Gaussians leave no pair with |cos| > 0.9."""
    ref = codebook.read_fvecs(os.path.join(GOLDEN, "codebooks", "learned_codebook", "angular_dim_16_Ks_32.fvecs"))
    assert _max_abs_cos(ref).min() < -0.99
    cb = codebook.train_codebook(16, 32, train_size=20000, iters=20, seed=808, metric="absdot")
    worst = float(np.abs(_max_abs_cos(cb)).max())
    print("largest |cos| between two trained codewords: %.3f" % worst)
    assert worst <= 0.9
    assert np.allclose(np.linalg.norm(cb.astype(np.float64), axis=1), 1.0, atol=1e-6)
