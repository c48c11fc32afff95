"""The bf16 tensor-side type of the microscaling compressor on the CPU (no GPU): tests/mx_bf16_contract.py's narrow against torch's
own float32 -> bfloat16 cast as an independent witness, the header's exactness statements over every code and scale byte, the
preconditions the decode-mean and error-feedback cases claim (asserted on the reference alone), and a mutation check -- truncation,
round-half-up and a w narrowed before the residual must each change bits on the cases the GPU tests run.

One precondition cannot exist and is replaced by its proof: a decode-mean never narrows a FINITE float32 to +-inf.  With R >= 2
the accumulator is finite only below 2^128, so the mean lies below 2^127, and bf16's halfway point to infinity is (2 - 2^-8) * 2^127;
with R = 1 the mean is one decoded value, which bf16 holds exactly; behind a rotation the eight stages stay finite only below
2^128, so the output, scaled by 2^-4, lies below 2^124 (test_no_decode_mean_reaches_infinity_from_a_finite_value).  The finite value
that narrows to infinity is therefore placed where it can occur -- the source written back under error feedback (ef_case)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx6_contract as m6  # noqa: E402
import mx_bf16_contract as bx  # noqa: E402
import mxr_contract as mxr  # noqa: E402

f32, U16, U32 = np.float32, np.uint16, np.uint32
LOWS = np.array([0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF], U32)


def _torch_narrow(bits):
    x = torch.from_numpy(np.ascontiguousarray(bits.astype(U32)).view(np.int32).copy()).view(torch.float32)
    return x.to(torch.bfloat16).view(torch.int16).numpy().view(U16)


def _against_torch(bits):
    x = bits.view(f32)
    got, witness = bx.narrow(x), _torch_narrow(bits)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], witness[~nan])
    assert np.all(got[nan] == bx.BF16_NAN)                      # the contract's NaN
    assert np.all(np.isnan(bx.widen(witness[nan])))             # torch's is a NaN too, whichever


def test_narrow_is_torchs_cpu_cast_on_every_high_half():
    hi = np.arange(65536, dtype=U32) << U32(16)
    for lo in LOWS:
        _against_torch(hi | lo)


def test_narrow_is_torchs_cpu_cast_on_random_patterns():
    rs = np.random.RandomState(1)
    _against_torch(rs.randint(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(U32))


def test_widen_narrow_round_trip():
    h = np.arange(65536, dtype=U32).astype(U16)
    w = bx.widen(h)
    ok = ~np.isnan(w)
    assert np.array_equal(bx.narrow(w)[ok], h[ok])
    assert np.array_equal(m6.bits_of(bx.widen(bx.narrow(w)))[ok], m6.bits_of(w)[ok])
    assert np.all(bx.narrow(w)[~ok] == bx.BF16_NAN)


def test_narrow_named_values():
    x = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2 - 2.0 ** -9, 2.0 ** 128 - 2.0 ** 119, -(2.0 ** 128 - 2.0 ** 119), 2.0 ** 128 - 2.0 ** 120,
                  2.0 ** -134, -2.0 ** -135, 3 * 2.0 ** -134, 2.0 ** -149, -0.0], np.float64).astype(f32)
    assert bx.narrow(x).tolist() == [0x3F80, 0x3F82, 0x4000, 0x7F80, 0xFF80, 0x7F7F, 0x0000, 0x8000, 0x0002, 0x0000, 0x8000]


@pytest.mark.parametrize("fmt", bx.FMTS)
def test_a_single_decode_is_exact_in_bf16(fmt):
    """Every code under every scale byte 0 ... 253: the value has at most 2 (FP4) or 4 (FP6, E4M3) significant bits, so narrowing
    changes nothing -- unless the value has a bit below 2^-133, bf16's subnormal grid, which then rounds it.  With 4 significant
    bits that can happen only below 2^-130 (2^-132 for FP4): "below 2^-133" alone would be too narrow a bound -- E4M3's
    1.125 * 2^-133 is above it and not a bf16 value."""
    F = m6.FORMATS[fmt]
    codes = np.arange(1 << F.bits)
    sig_bits = 0
    for sb in range(254):
        nblk = -(-codes.size // 32)
        code = np.zeros(nblk * 32, np.int64)
        code[:codes.size] = codes
        d = m6.decode_values(np.full(nblk, sb, np.uint8), code, fmt)[:codes.size]
        back = bx.widen(bx.narrow(d))
        exact = m6.bits_of(back) == m6.bits_of(d)
        d64 = d.astype(np.float64)
        off_grid = np.isfinite(d64) & (np.mod(np.abs(np.where(np.isfinite(d64), d64, 0)) * 2.0 ** 133, 1.0) != 0)
        assert np.array_equal(exact, ~off_grid), "scale byte %d" % sb
        assert not np.any(off_grid & (np.abs(d64) >= 2.0 ** (-132 if fmt == m6.FP4 else -130))), "scale byte %d" % sb
        fin = np.isfinite(d) & (d != 0) & (np.abs(d) >= 2.0 ** -126)
        mant = m6.bits_of(d)[fin] & U32(0x7fffff)
        for m in np.unique(mant):
            sig_bits = max(sig_bits, 24 - (int(m) & -int(m)).bit_length() + 1 if m else 1)
    assert sig_bits == {m6.FP4: 2, m6.FP8: 4, m6.FP6_E2M3: 4, m6.FP6_E3M2: 3}[fmt]
    assert sig_bits <= 8


@pytest.mark.parametrize("fmt", bx.FMTS)
def test_decode_mean_case_preconditions(fmt):
    """What the hand-built payloads claim, on the reference alone (R = 2 unless said)."""
    two = bx.special_means(fmt, 2)
    assert two["tie_down"] == (m6.bits_of(f32(1 + 2.0 ** -8)).item(), 0x3F80)          # a tie, the even neighbour below
    assert two["tie_up"] == (m6.bits_of(f32(1 + 3 * 2.0 ** -8)).item(), 0x3F82)        # a tie, the even neighbour above
    assert two["carry"] == (m6.bits_of(f32(2 - 2.0 ** -9)).item(), 0x4000)             # the round-up carries into the exponent
    assert two["subnormal"] == (m6.bits_of(f32(2.0 ** -127)).item(), 0x0040)           # a bf16 subnormal
    assert two["minus_zero"] == (0, 0)                                                  # +0 + -0 + -0
    assert bx.special_means(fmt, 1, plain=True)["minus_zero"] == (0x80000000, 0x8000)   # plain: the -0 stays
    assert two["nan_block"][1] == bx.BF16_NAN
    assert two["largest"] == (m6.bits_of(f32(1.75 * 2.0 ** 126)).item(), 0x7EE0)
    m, h = two["underflow"]
    assert m == m6.bits_of(f32(-bx.min_mag(fmt) * 2.0 ** -128)).item()
    if fmt == m6.FP8:
        assert h == 0x8000      # -2^-137 lies below half of bf16's smallest subnormal: a -0 made by narrowing
    # the inputs themselves hold a -0 and a 0xFF scale byte
    secs = bx.decode_payloads(fmt, 2)
    sb, code = m6.unpack(secs[0][bx.SPECIAL_AT], bx.SPECIAL_N, fmt)
    assert sb[5] == 0xFF and code[32 * 4] == m6.FORMATS[fmt].sign
    # three payloads: the R = 3 division is inexact, and some bf16-subnormal result is NOT on bf16's grid before narrowing
    pl = bx.decode_payloads(fmt, 3)
    seen = False
    for i, n in enumerate(bx.DEC_SIZES):
        m3 = m6.decode_mean([p[i] for p in pl], n, fmt)
        sub = np.isfinite(m3) & (m3 != 0) & (np.abs(m3) < 2.0 ** -126)
        seen |= bool(np.any(m6.bits_of(bx.widen(bx.narrow(m3[sub]))) != m6.bits_of(m3[sub])))
    assert seen


@pytest.mark.parametrize("fmt", bx.FMTS)
def test_no_decode_mean_reaches_infinity_from_a_finite_value(fmt):
    """The module docstring's proof, at its edge: the largest finite accumulator of two payloads."""
    top = np.finfo(f32).max
    assert np.isfinite(bx.widen(bx.narrow(np.array([top / f32(2), top / f32(3), top / f32(16)], f32)))).all()
    assert bx.narrow(np.array([top], f32))[0] == 0x7F80          # (the value itself would: no mean of R >= 2 payloads reaches it)
    # R = 1, not plain: (+0 + d_0) / 1 = d_0, one decoded value -- exact in bf16 (test_a_single_decode_is_exact_in_bf16), or inf already
    top_codes = m6.decode_values(np.full(1, 253, np.uint8), np.full(32, m6.FORMATS[fmt].cmax, np.int64), fmt)
    assert np.array_equal(m6.bits_of(bx.widen(bx.narrow(top_codes))), m6.bits_of(top_codes))
    # behind a rotation: every stage finite means the unscaled sum is at most FLT_MAX, the output at most FLT_MAX / 16
    assert np.isfinite(bx.widen(bx.narrow(mxr.scale(np.array([top], f32))))).all()


@pytest.mark.parametrize("fmt", bx.FMTS)
def test_error_feedback_case_preconditions(fmt):
    gs, err, s = bx.ef_case(4097, 900)
    steps = bx.run_ef(gs, err, s, fmt)
    w0 = (bx.widen(gs[0]) + err).astype(f32)
    assert np.isfinite(w0[0]) and np.isfinite(w0[1]) and w0[0] == f32(2.0 ** 128 - 2.0 ** 119)
    assert steps[0][1][0] == 0x7F80 and steps[0][1][1] == 0xFF80          # a finite float32 w narrows to +-inf
    assert steps[0][1][2] == 0x3F80 and steps[0][1][3] == 0x3F82                 # the two ties, each to its even neighbour
    assert steps[0][2][0] != np.inf                                        # ... and the residual was taken from the finite w
    g_all = np.concatenate(gs)
    for h in (0x0000, 0x8000, 0x0001, 0x807F, 0x7F80, 0xFF80, 0x7FC0):
        assert np.any(g_all == h), hex(h)
    assert np.any(np.isnan(err)) and np.any(np.isinf(err)) and np.any(m6.bits_of(err) == 0x80000000)
    # the residual keeps precision bf16 has not: after the first record most w are not bf16 values
    with np.errstate(invalid="ignore", over="ignore"):
        w1 = (bx.widen(gs[1]) + steps[0][2]).astype(f32)
    fin = np.isfinite(w1)
    assert np.mean(m6.bits_of(bx.widen(bx.narrow(w1[fin]))) != m6.bits_of(w1[fin])) > 0.5


@pytest.mark.parametrize("signs", [None, mxr.SEEDED], ids=["plain", "rotated"])
@pytest.mark.parametrize("fmt", bx.FMTS)
def test_mutations_change_bits(fmt, signs):
    """The cases tell the contract from its three nearest mistakes."""
    if signs is None:
        n, secs = bx.SPECIAL_N, [p[bx.SPECIAL_AT] for p in bx.decode_payloads(fmt, 2)]
    else:
        n, secs = 4097, bx.rotated_payloads(4097, fmt, 2, 31)
    right = bx.decode_mean(secs, n, fmt, signs=signs)
    if signs is not None:      # the rotated payloads' hand-built tie: +-(1 + 2^-8) before narrowing, +-1 after it, 256 times
        assert set(right[512:768].tolist()) <= {0x3F80, 0xBF80}
        assert set(m6.bits_of(m6.decode_mean_rotated(secs, n, fmt, signs))[512:768].tolist()) <= {0x3F808000, 0xBF808000}
    for mode in ("trunc", "half_up"):
        assert not np.array_equal(right, bx.decode_mean(secs, n, fmt, signs=signs, mode=mode)), mode
    gs, err, s = bx.ef_case(4097, 900)
    good = bx.run_ef(gs, err, s, fmt, signs=signs)
    for mode in ("trunc", "half_up"):
        bad = bx.run_ef(gs, err, s, fmt, signs=signs, mode=mode)
        assert any(not np.array_equal(a[1], b[1]) for a, b in zip(good, bad)), mode
    bad = bx.run_ef(gs, err, s, fmt, signs=signs, narrow_w_first=True)
    assert not m6.same(good[0][2], bad[0][2], nan_as_one=True), "err from a narrowed w"
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(good[1:], bad[1:])), "... and the next record's wire"


@pytest.mark.parametrize("fmt", bx.FMTS)
def test_wire_of_a_bf16_source_is_the_f32_wire_of_the_widened_tensor(fmt):
    """(By construction of the reference -- stated so that a change to it is noticed.)"""
    g = bx.edge_gradient(4097, 5)
    r = np.random.RandomState(3).rand(g.size).astype(f32)
    assert np.array_equal(bx.compress(g, fmt, r)[0], m6.compress(bx.widen(g), fmt, r)[0])
    out = bx.compress(g, fmt, r)[1]
    assert np.array_equal(bx.widen(out).view(U32)[~np.isnan(bx.widen(out))],
                          m6.bits_of(m6.compress(bx.widen(g), fmt, r)[1])[~np.isnan(bx.widen(out))]), "a plain decode is exact in bf16"
