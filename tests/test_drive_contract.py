"""tests/drive_contract.py checked on the CPU (no GPU): the restatement of include/gq_drive.h against an explicit 256 x 256 Hadamard
matrix in float64 / longdouble, the order of its additions, its edges, the wire layout, and the error figures the README quotes."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402
import mxr_contract as mxr  # noqa: E402
import drive_contract as dc  # noqa: E402

f32 = np.float32
SMALL = [1, 10, 255, 257]


def exact(w, mode, signs):
    """The contract in longdouble over the explicit matrix -> (x', S, D) per block [nb, 256]."""
    wb = dc.pad_blocks(w).astype(np.longdouble)
    sg = 1.0 - 2.0 * (mxr.sign_mask(signs) >> np.uint32(31)).astype(np.longdouble)
    H = mxr.hadamard_matrix().astype(np.longdouble)
    xp = (wb * sg[None, :]) @ H.T / 16
    L1 = np.abs(xp).sum(axis=1)
    S = (xp * xp).sum(axis=1) / L1 if mode == dc.UNBIASED else L1 / 256
    y = np.where(np.signbit(xp), -S[:, None], S[:, None])
    D = (y @ H.T / 16) * sg[None, :]
    return xp, S, D


@pytest.mark.parametrize("mode", [dc.UNBIASED, dc.MSE])
def test_restatement_against_the_explicit_matrix(mode):
    """x', S and D of the float32 restatement within float32 rounding of the longdouble ones; the codes equal wherever x' is not
    within rounding of zero."""
    for n, seed in ((4096 + 300, 1), (257, 2), (10, 3)):
        for signs in (dc.SEEDED, mxr.ZERO_SIGNS):
            w = dc.student(n, seed)
            sec, D, _, _, xp, S = dc.compress(w, mode, signs)
            exp, eS, eD = exact(w, mode, signs)
            scale = float(np.abs(exp).max())
            assert np.abs(xp - exp).max() <= 16 * 2.0 ** -24 * scale
            assert np.all(np.abs(S - eS) <= 2.0 ** -20 * eS)
            assert np.abs(D - eD.reshape(-1)[:n]).max() <= 2.0 ** -18 * float(np.abs(eD).max())
            sure = np.abs(exp) > 32 * 2.0 ** -24 * scale
            assert sure.mean() > 0.99 and np.array_equal(dc.code_bits(xp)[sure], np.signbit(exp)[sure].astype(np.uint32))


def test_integer_blocks_are_exact():
    """Integer-valued blocks: every sum of the transform and of L1 is exact, so x', the codes and the mse scale equal the matrix's."""
    w = mxr.integers(3, 5, top=1 << 10).reshape(-1)
    _, _, _, _, xp, S = dc.compress(w, dc.MSE, dc.SEEDED)
    exp, eS, _ = exact(w, dc.MSE, dc.SEEDED)
    assert np.array_equal(xp.astype(np.longdouble), exp) and np.array_equal(S.astype(np.longdouble), eS.astype(f32).astype(np.longdouble))


def test_the_tree_order_is_visible():
    """A sequential or a descending-stride order of the additions changes bits of S on the test inputs."""
    w = dc.student(dc.ITEM, 11)
    xp = mxr.forward_blocks(dc.pad_blocks(w), dc.SEEDED)
    for mode in (dc.UNBIASED, dc.MSE):
        S = dc.scales(xp, mode)[0]
        for other in (dc.sequential_sum, dc.reversed_tree_sum):
            assert not np.array_equal(mx.bits_of(S), mx.bits_of(dc.scales(xp, mode, other)[0]))
    v = np.arange(256, dtype=f32)[None, :]
    assert dc.tree_sum(v)[0] == dc.sequential_sum(v)[0] == dc.reversed_tree_sum(v)[0] == 255 * 128


def test_zero_blocks_and_nonfinite_blocks():
    for mode in (dc.UNBIASED, dc.MSE):
        z = dc.zeros_mixed(600, 3)
        sec, D, _, _, xp, S = dc.compress(z, mode, dc.SEEDED)
        assert not mx.bits_of(S).any(), "L1 == 0: S = +0"
        assert not (mx.bits_of(D) & np.uint32(0x7fffffff)).any() and dc.code_bits(xp).any() and not dc.code_bits(xp).all()
        w, bad = dc.nonfinite()
        sec, D, _, _, xp, S = dc.compress(w, mode, dc.SEEDED)
        for b in range(S.size):
            blk = D[b * 256:(b + 1) * 256]
            if b in bad:
                assert mx.bits_of(S[b:b + 1])[0] == mx.QNAN and np.isnan(blk).all()
            else:
                assert np.isfinite(S[b]) and np.isfinite(blk).all()
        h = dc.huge(512, 4)
        S = dc.compress(h, mode, dc.SEEDED)[5]
        assert np.isposinf(S).all() if mode == dc.UNBIASED else np.isfinite(S).all()
        s = dc.subnormals(512, 5)
        S = dc.compress(s, mode, dc.SEEDED)[5]
        assert not mx.bits_of(S).any() if mode == dc.UNBIASED else (S > 0).all()


@pytest.mark.parametrize("kind", ["gaussian", "student", "subnormal_free_mixed"])
def test_unbiased_scale_is_exact_in_the_direction_of_x(kind):
    """|<D, x> / <x, x> - 1| <= 1e-5 (float64 accumulation) on every finite input with a scale to speak of (all-zero blocks have
    <x, x> = 0, all-subnormal ones S = +0 and the 2^63 ones S = +inf: test_zero_blocks_and_nonfinite_blocks), n = 1, 10, 255, 257
    among them."""
    for n in SMALL + [2048, 4097, 8193]:
        if kind == "subnormal_free_mixed":
            x = dc.gaussian(n, n)
            x[::3] = dc.student(n, n + 1)[::3]
            x[1::5] = 0
        else:
            x = dc.FINITE_KINDS[kind](n, 40 + n)
        for signs in (dc.SEEDED, mxr.ZERO_SIGNS, dc.SIGN_SETS["seed2"]):
            D = dc.compress(x, dc.UNBIASED, signs)[1].astype(np.float64)
            x64 = x.astype(np.float64)
            assert abs(np.dot(D, x64) / np.dot(x64, x64) - 1) <= 1e-5, (kind, n)


def test_wire_layout_and_pad_bytes():
    for n in (1, 255, 256, 257, 1024, 1025, 4097):
        nb = -(-n // 256)
        assert dc.section_bytes(n) == nb * 32 + (4 * nb + 15) // 16 * 16 and dc.section_bytes(n) % 16 == 0
        x = dc.student(n, n)
        sec, D, _, _, xp, S = dc.compress(x, dc.UNBIASED, dc.SEEDED)
        assert sec.size == dc.section_bytes(n) and not sec[nb * 36:].any()
        for b, j in ((0, 0), (nb - 1, 255), (nb - 1, 9), (nb // 2, 130)):
            assert (sec[32 * b + (j >> 3)] >> (j & 7)) & 1 == mx.bits_of(xp[b, j:j + 1])[0] >> 31
        assert np.array_equal(sec[nb * 32:nb * 36].view("<f4"), S)
        bits, S2 = dc.unpack(sec, n)
        assert np.array_equal(bits, dc.code_bits(xp)) and np.array_equal(mx.bits_of(S2), mx.bits_of(S))
        assert np.array_equal(mx.bits_of(dc.decode_mean([sec], n, dc.SEEDED, plain=True)), mx.bits_of(D))
    # the code bits behind element n - 1 of a last block are the transform's outputs: they depend on the input
    a, b = dc.student(300, 1), dc.student(300, 2)
    assert not np.array_equal(dc.compress(a, 0, dc.SEEDED)[0][32 + 8:64], dc.compress(b, 0, dc.SEEDED)[0][32 + 8:64])
    offs, dense, ub = dc.layout([300, 5000], [10])
    assert offs == [0, dc.section_bytes(300)] and dense == [(offs[1] + dc.section_bytes(5000), 10)] and ub % 16 == 0


def test_mean_first_then_one_inverse():
    """The decode-mean is the mean in the rotated domain and ONE inverse: rotating every payload back first changes bits."""
    n = 4096
    secs = dc.payloads(n, 8, seed=3)[2:7]      # (payloads without the NaN scale)
    a, b = dc.decode_mean(secs, n, dc.SEEDED), dc.decode_mean_inverse_first(secs, n, dc.SEEDED)
    ok = np.isfinite(a) & np.isfinite(b)
    assert ok.mean() > 0.5 and not np.array_equal(mx.bits_of(a[ok]), mx.bits_of(b[ok]))
    assert np.abs(a[ok] - b[ok]).max() <= 1e-5 * np.abs(a[ok]).max()
    one = dc.decode_mean(secs[:1], n, dc.SEEDED)
    assert np.array_equal(one[ok] == 0, dc.decode_mean(secs[:1], n, dc.SEEDED, plain=True)[ok] == 0)


def test_error_table_of_the_readme():
    """N(0, 1) * 1e-3 at 262,144 elements, sign seed 1, numpy.random.default_rng(3): sqrt(pi/2 - 1) for `unbiased`,
    sqrt(1 - 2/pi) for `mse`, each within 0.01; the mean of 256 decodes of one 4,096-element vector under the seeds 100 ... 355 is
    <= 0.06 of the vector for `unbiased` (0.756 / 16 = 0.047) and stays >= 0.30 for `mse`."""
    x = (np.random.default_rng(3).standard_normal(262144) * 1e-3).astype(f32)
    got = {m: dc.rel_l2(x, dc.compress(x, dc.MODES[m], mxr.sign_words(1))[1]) for m in ("unbiased", "mse")}
    print("single shot:", got)
    assert abs(got["unbiased"] - math.sqrt(math.pi / 2 - 1)) <= 0.01
    assert abs(got["mse"] - math.sqrt(1 - 2 / math.pi)) <= 0.01
    v = (np.random.default_rng(3).standard_normal(4096) * 1e-3).astype(f32)
    mean = {}
    for m in ("unbiased", "mse"):
        acc = np.zeros(4096)
        for k in range(256):
            acc += dc.compress(v, dc.MODES[m], mxr.sign_words(100 + k))[1]
        mean[m] = dc.rel_l2(v, acc / 256)
    print("mean of 256 seeds:", mean)
    assert mean["unbiased"] <= 0.06 and mean["mse"] >= 0.30
