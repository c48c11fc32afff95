"""tests/mx_contract.py -- the numpy restatement of include/gq_mx.h -- checked against an independent witness: a brute-force search
of the explicit value table (8 and 127 magnitudes) in float64 / longdouble and exact integers (fractions).  No GPU."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402

f32 = np.float32
FMTS = [mx.FP4, mx.FP8]
# the value tables, written out independently of mx.mag: E2M1 and E4M3 (OCP) magnitudes in ascending order
TABLE = {
    mx.FP4: [Fraction(x).limit_denominator() for x in (0, 0.5, 1, 1.5, 2, 3, 4, 6)],
    mx.FP8: [Fraction(m, 8) * Fraction(2) ** -6 for m in range(8)]
            + [Fraction(8 + m, 8) * Fraction(2) ** (ex - 7) for ex in range(1, 16) for m in range(8)][:119],
}


def test_value_tables():
    assert len(TABLE[mx.FP4]) == 8 and len(TABLE[mx.FP8]) == 127 and TABLE[mx.FP8][-1] == 448 and TABLE[mx.FP4][-1] == 6
    for fmt in FMTS:
        got = mx.mag(np.arange(len(TABLE[fmt])), fmt)
        assert [Fraction(float(x)) for x in got] == TABLE[fmt]
        assert all(a < b for a, b in zip(TABLE[fmt], TABLE[fmt][1:]))


def _inputs(fmt):
    w, _ = mx.edge_tensor(fmt)
    return np.concatenate([w, mx.randn(4096, 1), mx.randn(2048, 2, 6.0), (mx.randn(1024, 3) * f32(1e-38)).astype(f32),
                           (mx.randn(1024, 4) * f32(1e35)).astype(f32)])


def _witness_bracket(y, fmt):
    """(lo index, hi index) of the table around y (float64, exact): the largest value <= y and the smallest >= y."""
    tab = np.array([float(v) for v in TABLE[fmt]], np.float64)
    lo = np.searchsorted(tab, y, side="right") - 1
    hi = np.searchsorted(tab, y, side="left")
    return tab, lo, hi


@pytest.mark.parametrize("fmt", FMTS)
def test_bracket_nothing_clamped_and_nearest_even(fmt):
    w = _inputs(fmt)
    F = mx.FORMATS[fmt]
    wb = mx.pad_blocks(w)
    sb, e, bad = mx.block_exponents(wb, fmt)
    assert sb[~bad].max() <= 253 and np.all(sb[bad] == 255) and bad.sum() == 2
    ok = ~bad
    y = mx.scaled(wb[ok], e[ok]).astype(np.float64)            # (float32 values, exact in float64)
    tab, lo, hi = _witness_bracket(y, fmt)
    assert y.max() <= tab[-1], "an element above mag(cmax): it would have to be clamped"
    assert np.all(lo >= 0) and np.all(hi <= F.cmax)
    c_lo, frac, q = mx.split_element(y.astype(f32), fmt)
    assert np.array_equal(c_lo, lo), "c_lo is not the largest table value <= y"
    assert np.all((tab[lo] <= y) & (y <= tab[hi]))
    # frac and q against the table in exact arithmetic: y = tab[lo] + frac * q, and q is the table's step at lo
    step = np.where(lo < F.cmax, tab[np.minimum(lo + 1, F.cmax)] - tab[lo], q)
    assert np.array_equal(q.astype(np.float64)[lo < F.cmax], step[lo < F.cmax])
    assert np.array_equal(tab[lo] + frac.astype(np.float64) * q.astype(np.float64), y)
    assert np.all(frac[lo == F.cmax] == 0)
    # deterministic mode: the nearest table value, ties to the even code (brute force over the whole table, in longdouble)
    yl = y.reshape(-1).astype(np.longdouble)
    dist = np.abs(yl[:, None] - tab.astype(np.longdouble)[None, :])
    best = dist.min(axis=1)
    cand = dist == best[:, None]
    even_first = np.where(cand & (np.arange(len(tab)) % 2 == 0)[None, :], 1, 0) * 2 + cand
    want = even_first.argmax(axis=1)
    assert np.all(cand.sum(axis=1) <= 2)
    _, code, _, _ = mx.codes_of(w, fmt, None)
    got = (code.reshape(wb.shape)[ok] & (F.sign - 1)).reshape(-1)
    assert np.array_equal(got, want)
    # the scale is the smallest that fits: one step smaller and the block's maximum exceeds the table (unless e is clamped at -127)
    ymax = y.max(axis=1)
    assert np.all((2 * ymax > tab[-1]) | (e[ok] == -127) | (ymax == 0))


@pytest.mark.parametrize("fmt", FMTS)
def test_signs_zero_and_nonfinite_blocks(fmt):
    F = mx.FORMATS[fmt]
    w, where = mx.edge_tensor(fmt)
    sb, code, e, bad = mx.codes_of(w, fmt, None)
    sign = (mx.bits_of(mx.pad_blocks(w)).reshape(-1) >> 31).astype(np.int64)
    okel = np.repeat(~bad, mx.BLOCK)
    assert np.array_equal((code >> (F.bits - 1))[okel], sign[okel]), "an element's own sign bit, +-0 included"
    at, m = where["nonfinite"]
    b0 = at // mx.BLOCK
    assert list(bad[b0:b0 + 5]) == [False, True, False, True, False]
    assert np.all(code.reshape(-1, mx.BLOCK)[bad] == 0)
    D = mx.decode_values(sb, code, fmt)
    assert np.all(mx.bits_of(D).reshape(-1, mx.BLOCK)[bad] == mx.QNAN)
    for name in ("zeros", "signed_zeros"):
        at, m = where[name]
        assert sb[at // mx.BLOCK] == 0 and np.array_equal(mx.bits_of(D[at:at + m]), mx.bits_of(w[at:at + m]))
    at, _ = where["min_subnormal"]
    assert sb[at // mx.BLOCK] == 0 and e[at // mx.BLOCK] == -127


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_is_exact_for_every_code_and_scale(fmt):
    F = mx.FORMATS[fmt]
    ncode = 1 << F.bits
    for sb in range(256):
        code = np.zeros(256, np.int64)
        code[:ncode] = np.arange(ncode)
        d = mx.decode_values(np.full(8, sb, np.uint8), code, fmt)[:ncode]
        if sb == 255:
            assert np.all(mx.bits_of(d) == mx.QNAN)
            continue
        for c in range(ncode):
            m = c & (F.sign - 1)
            exact = (TABLE[fmt][m] if m < len(TABLE[fmt]) else Fraction(480)) * Fraction(2) ** (sb - 127)
            neg = bool(c >> (F.bits - 1))
            if exact >= Fraction(2) ** 128:
                assert np.isinf(d[c]) and (d[c] < 0) == neg
            else:
                assert Fraction(float(d[c])) == (-exact if neg else exact), (sb, c)
                assert bool(mx.bits_of(d[c:c + 1])[0] >> 31) == neg
    # what a compress writes never reaches 2^128 except by rounding up from within half a step of it
    top = mx.block_with_max(np.finfo(f32).max, [])
    sbt, codet, _, _ = mx.codes_of(top, fmt, None)
    assert np.isinf(mx.decode_values(sbt, codet, fmt)[0])
    sbt, codet, _, _ = mx.codes_of(top, fmt, np.full(32, 0.9999999, f32))
    assert np.isfinite(mx.decode_values(sbt, codet, fmt)[0])


@pytest.mark.parametrize("fmt", FMTS)
def test_unbiased_to_2_pow_minus_24_of_a_step(fmt):
    """With the generator's draws r = j * 2^-24, P(up) = ceil(frac * 2^24) / 2^24; the mean of the decode is then within
    2^-24 * q of y (exact fractions)."""
    w = _inputs(fmt)
    wb = mx.pad_blocks(w)
    sb, e, bad = mx.block_exponents(wb, fmt)
    y = mx.scaled(wb[~bad], e[~bad]).reshape(-1)[::7]
    c_lo, frac, q = mx.split_element(y, fmt)
    tab = TABLE[fmt]
    for yy, c, fr, qq in zip(y[:3000], c_lo[:3000], frac[:3000], q[:3000]):
        fr, qq, yy = Fraction(float(fr)), Fraction(float(qq)), Fraction(float(yy))
        p_up = Fraction(-((-fr.numerator * 2 ** 24) // fr.denominator), 2 ** 24)      # ceil(frac * 2^24) / 2^24
        # the count of j in 0 .. 2^24 - 1 with frac > j * 2^-24 is ceil(frac * 2^24)
        assert 0 <= p_up <= 1 and p_up - fr < Fraction(1, 2 ** 24) and p_up >= fr
        hi = tab[c + 1] if p_up > 0 else tab[c]
        mean = tab[c] * (1 - p_up) + hi * p_up
        assert abs(mean - yy) <= qq / 2 ** 24
    # and the restated comparison does what the count says, at the edges of a draw
    one = np.array([0.25, 0.25, 0.25, 0.0, 2.0 ** -30], f32)
    r = np.array([0.25, 0.25 - 2.0 ** -24, 0.25 + 2.0 ** -24, 0.0, 0.0], f32)
    assert list(mx.round_up(np.zeros(5, np.int64), one, r)) == [False, True, False, False, True]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 511, 512, 513, 4097])
def test_section_layout(fmt, n):
    F = mx.FORMATS[fmt]
    nb = -(-n // 32)
    assert mx.section_bytes(n, fmt) == (nb + 15) // 16 * 16 + nb * (16 if fmt == mx.FP4 else 32)
    assert mx.section_bytes(n, fmt) % 16 == 0
    w = mx.randn(n, n)
    sec, D, _, _ = mx.compress(w, fmt)
    assert sec.size == mx.section_bytes(n, fmt) and sec.dtype == np.uint8
    sb, code, _, _ = mx.codes_of(w, fmt, None)
    assert np.array_equal(sec[:nb], sb) and np.all(sec[nb:(nb + 15) // 16 * 16] == 0)
    body = sec[(nb + 15) // 16 * 16:]
    for i in (0, 1, n - 1, min(n, nb * 32 - 1)):
        if fmt == mx.FP4:
            assert (int(body[i // 2]) >> (4 * (i % 2))) & 15 == code[i], "element 2i in the low nibble"
        else:
            assert body[i] == code[i]
    assert np.all(code[n:] == 0), "the padding elements' codes"
    sb2, code2 = mx.unpack(sec, n, fmt)
    assert np.array_equal(sb2, sb) and np.array_equal(code2, code)
    assert mx.same(mx.decode_mean([sec], n, fmt, plain=True), D)
    assert 8 * mx.section_bytes(1 << 20, fmt) / (1 << 20) == (4.25 if fmt == mx.FP4 else 8.25)


@pytest.mark.parametrize("fmt", FMTS)
def test_edge_inputs_hold_their_preconditions(fmt):
    F = mx.FORMATS[fmt]
    # 7: on every grid value and every midpoint, both parities of the tie
    for s in (-3, -127, 100):
        w = mx.grid_and_midpoints(fmt, s)
        wb = mx.pad_blocks(w)
        sb, e, bad = mx.block_exponents(wb, fmt)
        assert np.all(e == s) and not bad.any()
        c_lo, frac, _ = mx.split_element(mx.scaled(wb, e), fmt)
        assert set(np.unique(frac)) == {f32(0), f32(0.5)}
        on_grid = set(c_lo[frac == 0].tolist())
        assert on_grid == set(range(F.cmax + 1)), "every grid value"
        ties = c_lo[frac == 0.5]
        assert set(ties.tolist()) == set(range(F.cmax)), "every midpoint"
        assert (ties % 2 == 0).any() and (ties % 2 == 1).any()
    # 8: frac equals the draw exactly
    w, r, frac = mx.frac_equals_draw(fmt, -5)
    wb = mx.pad_blocks(w)
    sb, e, _ = mx.block_exponents(wb, fmt)
    assert e[0] == -5
    c_lo, fr, _ = mx.split_element(mx.scaled(wb, e), fmt)
    assert np.array_equal(fr.reshape(-1), frac) and np.all(c_lo.reshape(-1)[1:] == F.cmax - 1)
    up = mx.round_up(c_lo.reshape(-1), fr.reshape(-1), r)
    assert not up[:10].any() and up[11:21].all() and np.array_equal(up[21:], frac[21:] > 0)
    assert np.all(r[1:10] == frac[1:10]) and np.all(r[21:] == 0)
    # 9: y subnormal (or rounded to zero), and the two ties onto the subnormal grid go to even
    w = mx.subnormal_y(fmt)
    wb = mx.pad_blocks(w)
    sb, e, _ = mx.block_exponents(wb, fmt)
    assert e[0] == 8
    y = mx.scaled(wb, e).reshape(-1)
    assert np.all(y[1:12] < f32(2.0 ** -126)) and (y[1:12] > 0).sum() >= 8 and (y[1:12] == 0).sum() >= 2
    assert y[3] == f32(2 * 2.0 ** -149) and y[4] == f32(2 * 2.0 ** -149), "1.5 and 2.5 ulp: ties to even"
    # 2 ... 5 of edge_blocks
    blocks = mx.edge_blocks(fmt)
    assert mx.bits_of(blocks["min_subnormal"]).max() & 0x7fffffff == 1
    assert (mx.bits_of(blocks["all_subnormal"]) & 0x7fffffff).max() == 0x7fffff
    assert np.abs(blocks["flt_max"]).max() == np.finfo(f32).max
    for E in (1, 100, 254):
        a = (mx.bits_of(blocks["at_mthr_E%d" % E]) & 0x7fffffff).max()
        b = (mx.bits_of(blocks["above_mthr_E%d" % E]) & 0x7fffffff).max()
        assert a == (E << 23) | F.mthr and b == a + 1
        ea = mx.block_exponents(blocks["at_mthr_E%d" % E][None], fmt)[1][0]
        eb = mx.block_exponents(blocks["above_mthr_E%d" % E][None], fmt)[1][0]
        assert eb == max(E - 127 - F.emax + 1, -127) and ea == max(E - 127 - F.emax, -127)


@pytest.mark.parametrize("fmt", FMTS)
def test_error_feedback_and_mean_arithmetic(fmt):
    g, err = mx.randn(100, 1), mx.randn(100, 2)
    sec, D, w, ne = mx.compress(g, fmt, None, err, 0.3)
    p = (f32(0.3) * err).astype(f32)
    assert mx.same(w, g + p) and mx.same(ne, w - D)
    fused = (g.astype(np.float64) + np.float64(f32(0.3)) * err.astype(np.float64)).astype(f32)
    assert not mx.same(w, fused), "the two roundings are visible in this input"
    secs = [mx.compress(mx.randn(100, 10 + r), fmt)[0] for r in range(3)]
    ds = [mx.decode_mean([s], 100, fmt, plain=True) for s in secs]
    assert mx.same(mx.decode_mean(secs, 100, fmt), (((np.zeros(100, f32) + ds[0]) + ds[1]) + ds[2]) / f32(3))
    neg0 = mx.compress(np.full(40, -0.0, f32), fmt)[0]
    assert np.all(mx.bits_of(mx.decode_mean([neg0], 40, fmt, plain=True)) == 0x80000000)
    assert np.all(mx.bits_of(mx.decode_mean([neg0], 40, fmt)) == 0)
