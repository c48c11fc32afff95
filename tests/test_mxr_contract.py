"""tests/mxr_contract.py held to account on the CPU: the stage-wise transform against an explicit 256 x 256 +-1 matrix, the sign
words against a scalar splitmix64, the preconditions every GPU input claims, the teeth of the GPU comparison (what the kernels
must not compute would change bits on every input), and the property the rotation is there for."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402
import mxr_contract as mxr  # noqa: E402

f32 = np.float32
SIGNS = sorted(mxr.SIGN_SETS)


def bits(a):
    return mx.bits_of(a)


@pytest.mark.parametrize("signs", SIGNS)
def test_stages_equal_the_explicit_matrix_on_integers(signs):
    """On integer-valued inputs below 2^14 every float32 sum is exact: the eight stages are H * diag(s) * x, and the scaled
    result that over 16, computed here in int64."""
    s = mxr.SIGN_SETS[signs]
    x = mxr.integers(5, 1)
    H = mxr.hadamard_matrix()
    assert np.array_equal(H @ H, 256 * np.eye(256, dtype=np.int64))
    sg = np.where(mxr.sign_mask(s) != 0, -1, 1).astype(np.int64)
    want = (x.astype(np.int64) * sg[None, :]) @ H.T
    assert np.abs(want).max() < 1 << 23
    got = mxr.stages(mxr.flip(x, s))
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(f32))
    assert np.array_equal(mxr.forward_blocks(x, s).astype(np.float64), want / 16.0)
    # the stride of stage t is 2^t: stage 0 alone pairs neighbours
    one = mxr.stage(x, 0)
    assert np.array_equal(one[:, 0::2], x[:, 0::2] + x[:, 1::2]) and np.array_equal(one[:, 1::2], x[:, 0::2] - x[:, 1::2])


@pytest.mark.parametrize("signs", SIGNS)
def test_forward_then_inverse_is_the_identity_on_integers(signs):
    s = mxr.SIGN_SETS[signs]
    x = mxr.integers(4, 2, top=1 << 10) * f32(16)       # (multiples of 16: the two scalings stay integers)
    x[x == 0] = 16                                      # (a zero's sign is the sum's, not the input's)
    back = mxr.inverse_blocks(mxr.forward_blocks(x, s), s)
    assert np.array_equal(bits(back), bits(x))
    flat = np.concatenate([x.reshape(-1), mx.randn(77, 3)])
    xp = mxr.forward(flat, s)
    assert np.array_equal(bits(xp[-77:]), bits(flat[-77:])), "the tail is not rotated"
    assert np.array_equal(bits(mxr.inverse(xp, s)), bits(flat))
    small = mx.randn(255, 4)
    assert np.array_equal(bits(mxr.forward(small, s)), bits(small)), "a tensor below 256 elements is plain MX"


def test_sign_words_equal_a_scalar_splitmix64():
    def splitmix(seed):
        M = (1 << 64) - 1
        state, out = seed & M, []
        for _ in range(4):
            state = (state + 0x9E3779B97F4A7C15) & M
            z = state
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            out.append(z ^ (z >> 31))
        return tuple(out)

    for seed in (0, 1, 2, 12345, (1 << 64) - 1):
        assert mxr.sign_words(seed) == splitmix(seed)
    assert splitmix(0)[0] == 0xE220A8397B1DCDAF      # the generator's published first output for seed 0
    from gq_amd.compressors import MXCompressor
    assert MXCompressor.sign_words(1) == mxr.SEEDED == splitmix(1)
    m = mxr.sign_mask((1 | (1 << 63), 2, 0, 1 << 63))
    assert set(np.nonzero(m)[0]) == {0, 63, 65, 255} and np.all(m[m != 0] == 0x80000000)


def _inputs():
    """Every tensor the GPU contract tests compress: (name, values)."""
    out = [("size_%d" % n, mxr.gradients(n, 100 + n)) for n in mxr.SIZES]
    out.append(("edge_finite", mxr.edge_finite()[0]))
    out.append(("edge_nonfinite", mxr.edge_nonfinite()[0]))
    return out


def test_preconditions_of_the_inputs():
    for n in mxr.SIZES:
        g = mxr.gradients(n, 100 + n)
        assert g.size == n and np.all(np.isfinite(g))
        for s in mxr.SIGN_SETS.values():
            assert np.all(np.isfinite(mxr.forward(g, s))), "no overflow in the butterflies of the size tests"
    w, at = mxr.edge_finite()
    assert np.all(np.isfinite(w)) and w.size == 4 * 256 + 40
    blk = lambda x, name: x[at[name]:at[name] + 256]
    assert np.all(blk(w, "zeros") == 0) and np.signbit(blk(w, "zeros")).any() and not np.signbit(blk(w, "zeros")).all()
    sub = blk(w, "subnormals")
    assert np.all(np.abs(sub) < 2.0 ** -126) and (sub != 0).sum() > 100 and (sub == 0).sum() > 10
    for s in mxr.SIGN_SETS.values():
        xp = mxr.forward(w, s)
        raw = mxr.stages(mxr.flip(blk(w, "tiny")[None, :], s))[0]      # before the scaling
        t = blk(xp, "tiny")
        assert np.all(np.abs(raw) >= 2.0 ** -126) or np.all(np.isfinite(raw))
        assert np.all(np.abs(t) < 2.0 ** -126) and (t != 0).sum() > 200, "x' = x * 2^-4 is subnormal"
        assert (t.astype(np.float64) != raw.astype(np.float64) / 16).sum() > 50, "and the multiplication rounds"
        o = blk(xp, "overflow")
        assert np.isinf(o).sum() == 128 and not np.isnan(o).any(), "inf from a finite input, and no inf meets another"
        sb, _, _, _ = mx.codes_of(o, mx.FP4)
        assert np.all(sb == 255)
        assert np.array_equal(bits(xp[-40:]), bits(w[-40:]))
    w, at = mxr.edge_nonfinite()
    for s in mxr.SIGN_SETS.values():
        xp = mxr.forward(w, s)
        for name, a in at.items():
            if name == "tail":
                continue
            b = xp[a:a + 256]
            if name.startswith("finite"):
                assert np.all(np.isfinite(b))
            else:
                assert not np.isfinite(b).any(), "%s: an inf or NaN reaches all 256 outputs" % name
        sb, _, _, _ = mx.codes_of(xp, mx.FP8)
        want = np.repeat([255, 0, 255, 255, 0, 255], 8)
        assert np.array_equal(sb[:48] == 255, want == 255)
        assert [int(x == 255) for x in sb[48:]] == [1, 0, 0, 1], "the tail: only the MX blocks that hold the inf and the NaN"


@pytest.mark.parametrize("name,g", _inputs(), ids=[n for n, _ in _inputs()])
def test_the_gpu_comparison_has_teeth(name, g):
    """On every size input with a rotated block, what the kernels must not compute changes what the GPU tests compare.
    Descending stage order, and a scale applied before the stages (the inputs' first block is small enough for w * 2^-4 to
    round): bits of x', and of the wire under the draws r = frac(x') (mxr_contract.frac_draws: the wire then shows the last bit
    of x' -- a quantiser to nearest would swallow it).  The decoded values of a rotated block share their scale, so their sums
    are exact in any order: the inverse transform's order shows in the decode-mean of the hand-built payloads (next test).
    The edge tensors are exact by construction (zeros, multiples of 2^-149, infinities): they test values, not order.
    (Tensors below 256 elements are plain MX: nothing to tell apart.)"""
    s = mxr.SEEDED
    if not name.startswith("size"):
        return
    if g.size < 256:
        assert np.array_equal(bits(mxr.forward(g, s)), bits(g))
        return
    xp = mxr.forward(g, s)
    nr = g.size // 256 * 256
    for fmt in (mx.FP4, mx.FP8):
        r = mxr.frac_draws(xp, fmt)
        ref = mxr.compress(g, fmt, s, r)
        assert np.array_equal(ref[0], mxr.compress(g, fmt, s, np.zeros_like(r))[0]) or np.any(r > 0)
        for kw in ({"order": range(7, -1, -1)}, {"scale_first": True}):
            alt = mxr.compress(g, fmt, s, r, **kw)
            assert not np.array_equal(bits(ref[4][:nr]), bits(alt[4][:nr])) or name == "edge_nonfinite", (name, kw, "x'")
            if name != "edge_nonfinite":
                assert not np.array_equal(ref[0], alt[0]), (name, kw, "the wire under r = frac")
    if name.startswith("size") and g.size >= 4096:
        d = mxr.forward(g, s, order=range(7, -1, -1))
        assert (bits(xp[:nr]) != bits(d[:nr])).mean() > 0.3, "ascending against descending order: a large part of the words differ"


@pytest.mark.parametrize("fmt", [mx.FP4, mx.FP8])
def test_mean_then_inverse_differs_from_inverse_then_mean(fmt):
    """The decode-mean payloads of the GPU tests: rotating every payload back and then taking the mean changes bits."""
    n = 4096 + 255
    for R in (2, 3, 8, 16):
        secs = [mxr.payloads(n, fmt, R, seed=n)[r] for r in range(R)]
        a = mxr.decode_mean(secs, n, fmt, mxr.SEEDED)
        b = mxr.decode_mean_inverse_first(secs, n, fmt, mxr.SEEDED)
        assert not mx.same(a, b, nan_as_one=True), "R = %d" % R
        m = mx.decode_mean(secs, n, fmt)
        assert not mx.same(a, mxr.inverse(m, mxr.SEEDED, order=range(7, -1, -1)), nan_as_one=True), "the inverse's stage order shows"
        assert np.array_equal(bits(a[4096:]), bits(mx.decode_mean(secs, n, fmt)[4096:])), "the tail is the plain mean"
    one = mxr.payloads(n, fmt, 1, seed=n)
    plain = mxr.decode_mean(one, n, fmt, mxr.ZERO_SIGNS, plain=True)
    assert mx.same(plain, mxr.inverse(mx.decode_mean(one, n, fmt, True), mxr.ZERO_SIGNS), nan_as_one=True)


def test_compress_is_mx_on_the_rotated_tensor():
    g = mxr.gradients(4097, 7)
    err = mxr.gradients(4097, 8)
    r = np.random.RandomState(1).rand(4097).astype(f32)
    sec, D, w, ne, xp = mxr.compress(g, mx.FP4, mxr.SEEDED, r, err, 0.5)
    assert np.array_equal(bits(w), bits((g + (f32(0.5) * err).astype(f32)).astype(f32)))
    sec2, Dx, _, _ = mx.compress(xp, mx.FP4, r)
    assert np.array_equal(sec, sec2) and np.array_equal(bits(D), bits(mxr.inverse(Dx, mxr.SEEDED)))
    assert np.array_equal(bits(ne), bits((w - D).astype(f32)))
    assert np.array_equal(bits(mxr.decode_mean([sec], 4097, mx.FP4, mxr.SEEDED, plain=True)), bits(D))
    assert mxr.rel_l2(w, D) < 0.5


def test_rotation_lowers_the_error_on_heavy_tails():
    """FP4, 16,384 elements, np.random.default_rng(1): over Student-t with 3 d.o.f. and over Gaussian x exp(1.5 Gaussian) the
    relative L2 error with rotation is strictly smaller than without, under nearest rounding and under one fixed draw vector.
    A condition, not a tolerance (nothing is claimed for Gaussian or sparse input)."""
    rng = np.random.default_rng(1)
    n = 16384
    inputs = {"student_t3": mxr.student_t(n, 3, rng), "lognormal_gaussian": mxr.lognormal_gaussian(n, rng)}
    draws = rng.random(n, dtype=np.float32)
    for name, g in inputs.items():
        for r in (None, draws):
            plain = mxr.rel_l2(g, mx.compress(g, mx.FP4, r)[1])
            rot = mxr.rel_l2(g, mxr.compress(g, mx.FP4, mxr.SEEDED, r)[1])
            print("%s, %s: plain %.4f, rotated %.4f" % (name, "nearest" if r is None else "stochastic", plain, rot))
            assert rot < plain, (name, r is None, plain, rot)
