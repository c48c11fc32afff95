"""tests/mx6_contract.py checked on the CPU (no GPU): the generic restatement against tests/mx_contract.py on FP4 / FP8, the two 6-bit
formats against explicit value tables in exact fractions, the 6-bit wire against a bit string built with Python integers, the section
sizes, the preconditions the hand-built inputs claim, the error table of the README -- and the host side of the two formats: the
driver's names, the ResNet-50 wire, the ABI numbers."""
import json
import os
import re
import sys
from argparse import Namespace
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx6_contract as m6  # noqa: E402
import mx_contract as mx  # noqa: E402

f32 = np.float32
FP6 = list(m6.FP6)
# every magnitude code's value, written out (OCP Microscaling v1.0, tables 3 and 4)
TABLE = {
    m6.FP6_E2M3: [0, .125, .25, .375, .5, .625, .75, .875, 1, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
                  2, 2.25, 2.5, 2.75, 3, 3.25, 3.5, 3.75, 4, 4.5, 5, 5.5, 6, 6.5, 7, 7.5],
    m6.FP6_E3M2: [0, .0625, .125, .1875, .25, .3125, .375, .4375, .5, .625, .75, .875, 1, 1.25, 1.5, 1.75,
                  2, 2.5, 3, 3.5, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28],
}


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp",
                num_users=1, mode="ps", cr=256)
    base.update(kw)
    return Namespace(**base)


def test_the_shared_table_is_left_alone():
    assert sorted(mx.FORMATS) == [mx.FP4, mx.FP8] and m6.FORMATS is not mx.FORMATS
    for fmt in (mx.FP4, mx.FP8):
        assert vars(m6.FORMATS[fmt]) == vars(mx.FORMATS[fmt])


@pytest.mark.parametrize("fmt", [mx.FP4, mx.FP8])
def test_generic_restatement_equals_mx_contract(fmt):
    """FP4 / FP8 through the format-table form: every intermediate and every byte, on the edge tensor and on heavy-tailed values,
    to nearest and with draws."""
    edge, _ = mx.edge_tensor(fmt)
    for w, seed in ((edge, 1), (mx.randn(5000, 21), 2), (mx.randn(4097, 22, spread=6.0), 3)):
        wb = mx.pad_blocks(w)
        for a, b in zip(m6.block_exponents(wb, fmt), mx.block_exponents(wb, fmt)):
            assert np.array_equal(a, b)
        r = np.random.RandomState(seed).rand(w.size).astype(f32)
        for rr in (None, r):
            for a, b in zip(m6.codes_of(w, fmt, rr), mx.codes_of(w, fmt, rr)):
                assert np.array_equal(a, b)
            err = mx.randn(w.size, 40 + seed)
            for args in ((w, fmt, rr), (w, fmt, rr, err, 0.5)):
                got, want = m6.compress(*args), mx.compress(*args)
                assert np.array_equal(got[0], want[0]), "the section's bytes"
                for a, b in zip(got[1:], want[1:]):
                    assert (a is None and b is None) or np.array_equal(mx.bits_of(a), mx.bits_of(b))
        sec = m6.compress(w, fmt, r)[0]
        sb, code = m6.unpack(sec, w.size, fmt)
        sb2, code2 = mx.unpack(sec, w.size, fmt)
        assert np.array_equal(sb, sb2) and np.array_equal(code, code2)
        assert np.array_equal(mx.bits_of(m6.decode_values(sb, code, fmt)), mx.bits_of(mx.decode_values(sb, code, fmt)))
    secs = mx.payload_set(300, fmt, 5)
    assert all(np.array_equal(a, b) for a, b in zip(secs, m6.payload_set(300, fmt, 5)))
    for R in (1, 2, 5):
        for plain in (False, True):
            assert np.array_equal(mx.bits_of(m6.decode_mean(secs[:R], 300, fmt, plain)), mx.bits_of(mx.decode_mean(secs[:R], 300, fmt, plain)))
    for n in (1, 31, 32, 33, 511, 4097, 25000000):
        assert m6.section_bytes(n, fmt) == mx.section_bytes(n, fmt)


@pytest.mark.parametrize("fmt", FP6)
def test_value_tables(fmt):
    F = m6.FORMATS[fmt]
    T = TABLE[fmt]
    assert (F.bits, F.cmax, F.sign) == (6, 31, 32) and len(T) == 32 == 1 << (F.bits - 1)
    assert m6.mag(np.arange(32), fmt).tolist() == T and all(a < b for a, b in zip(T, T[1:]))
    assert T[31] == (2 - 2.0 ** -F.mb) * 2.0 ** F.emax and T[1 << F.mb] == 2.0 ** (1 - F.bias)
    assert (F.mthr | 0x800000) * 2.0 ** -23 == T[31] / 2.0 ** F.emax, "MTHR is the mantissa of mag(cmax)"
    # the decode of every code at scale byte 127, both signs
    got = m6.decode_values(np.array([127, 127], np.uint8), np.arange(64), fmt)
    assert got.tolist() == T + [-t for t in T] and np.signbit(got[32])


def _exact_codes(w, e, fmt, r=None):
    """Scalar witness in exact fractions: the bracket from the explicit table, nearest with ties to the even code / frac > r."""
    T = [Fraction(t) for t in TABLE[fmt]]
    out = []
    for i, x in enumerate(w):
        y = Fraction(abs(float(x))) / Fraction(2) ** int(e[i // 32])
        c = max(k for k in range(32) if T[k] <= y)
        if c == 31:
            assert y == T[31]
            up = False
        else:
            frac = (y - T[c]) / (T[c + 1] - T[c])
            up = (frac > Fraction(1, 2) or (frac == Fraction(1, 2) and c % 2 == 1)) if r is None else frac > Fraction(float(r[i]))
        out.append((c + up) | (32 if np.signbit(x) else 0))
    return np.array(out, np.int64)


@pytest.mark.parametrize("fmt", FP6)
def test_codes_against_the_table_in_exact_fractions(fmt):
    """Blocks where y is exact (no subnormal y): heavy-tailed values, every grid value and midpoint, the frac == draw block."""
    w = np.concatenate([mx.randn(1536, 31, spread=2.0), m6.grid_and_midpoints(fmt, -3), m6.grid_and_midpoints(fmt, 90),
                        m6.frac_equals_draw(fmt, -5)[0]])
    wb = mx.pad_blocks(w)
    _, e, bad = m6.block_exponents(wb, fmt)
    y = mx.scaled(wb, e)
    assert not bad.any() and np.all((y == 0) | (y >= f32(2.0 ** -126))), "every y exact"
    r = np.random.RandomState(5).rand(w.size).astype(f32)
    r[-32:] = m6.frac_equals_draw(fmt, -5)[1]
    for rr in (None, r):
        _, code, _, _ = m6.codes_of(w, fmt, rr)
        assert np.array_equal(code[:w.size], _exact_codes(w, e, fmt, rr))
    # the decode is the table's value times the scale, exactly
    sb, code, _, _ = m6.codes_of(w, fmt, r)
    D = m6.decode_values(sb, code, fmt).astype(np.float64)
    T = np.array(TABLE[fmt])
    assert np.array_equal(D, np.where(code >= 32, -1.0, 1.0) * T[code & 31] * np.repeat(np.ldexp(1.0, e), 32))


@pytest.mark.parametrize("fmt", FP6)
def test_codes_never_exceed_cmax_on_the_edge_tensor(fmt):
    w, _ = m6.edge_tensor(fmt)
    F = m6.FORMATS[fmt]
    ones = np.zeros(w.size, f32)      # r = 0: everything with frac > 0 goes up
    for r in (None, ones, np.random.RandomState(1).rand(w.size).astype(f32)):
        sb, code, e, bad = m6.codes_of(w, fmt, r)
        assert (code & (F.sign - 1)).max() == F.cmax and code.max() < 64 and code.min() >= 0
        assert np.all(code.reshape(-1, 32)[bad] == 0) and np.all(sb[bad] == 255) and sb[~bad].max() <= 253
        # and the scaled values never pass mag(cmax): nothing is clamped
        wb = mx.pad_blocks(w)
        with np.errstate(invalid="ignore", over="ignore"):
            y = mx.scaled(np.where(bad[:, None], f32(0), wb), e)
        assert y.max() <= f32(m6.mag(F.cmax, fmt))


def _bitstring_section(sb, code, nb):
    """The header's words with Python integers: block b's codes as one little-endian 192-bit number, element i at bit 6i."""
    out = bytearray(sb.tobytes()) + bytes(m6._up(nb) - nb)
    for b in range(nb):
        v = 0
        for i in range(32):
            v |= int(code[32 * b + i]) << (6 * i)
        out += v.to_bytes(24, "little")
    out += bytes(-len(out) % 16)
    return np.frombuffer(bytes(out), np.uint8)


@pytest.mark.parametrize("fmt", FP6)
@pytest.mark.parametrize("nb", [1, 2, 3, 16, 17, 129])
def test_pack_and_unpack_against_a_bit_string(fmt, nb):
    rs = np.random.RandomState(nb)
    code = rs.randint(0, 64, 32 * nb)
    code[:64] = np.arange(64)[:32 * nb]
    sb = rs.randint(0, 256, nb).astype(np.uint8)
    sec = m6.pack(sb, code, fmt)
    assert np.array_equal(sec, _bitstring_section(sb, code, nb))
    assert sec.size == m6.section_bytes(32 * nb, fmt) == m6._up(nb) + m6._up(24 * nb) and sec.size % 16 == 0
    pad = sec[m6._up(nb) + 24 * nb:]
    assert pad.size == (8 if nb % 2 else 0) and not pad.any(), "the code bytes' zero pad"
    assert not sec[nb:m6._up(nb)].any(), "the scale bytes' zero pad"
    sb2, code2 = m6.unpack(sec, 32 * nb, fmt)
    assert np.array_equal(sb2, sb) and np.array_equal(code2, code)
    # element i of block b from the bytes alone: bits 6i .. 6i+5
    body = sec[m6._up(nb):]
    for b, i in ((0, 0), (0, 5), (nb - 1, 10), (nb - 1, 31)):
        bit = 192 * b + 6 * i
        two = int(body[bit // 8]) | (int(body[bit // 8 + 1]) << 8 if bit // 8 + 1 < body.size else 0)
        assert (two >> (bit % 8)) & 63 == code[32 * b + i]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 4096, 4097, 25000000])
def test_section_sizes(n):
    from gq_amd import native
    from gq_amd.codecs import MXCodec, mx_section_bytes
    from gq_amd.compressors import MXCompressor
    nb = (n + 31) // 32
    for fmt, per_block in ((m6.FP4, 16), (m6.FP6_E2M3, 24), (m6.FP6_E3M2, 24), (m6.FP8, 32)):
        want = (nb + 15) // 16 * 16 + (per_block * nb + 15) // 16 * 16
        name = m6.NAMES[fmt]
        assert m6.section_bytes(n, fmt) == want == mx_section_bytes(n, name) == mx_section_bytes(n, fmt) and want % 16 == 0
        assert native.MX_FORMATS[name] == fmt and native.MX_CODE_BITS[fmt] * 4 == per_block
        cd = MXCodec(MXCompressor(n, (n,), make_args(mx_format=name)), n, (n,))
        assert cd.nbytes == want and cd.format == fmt
    assert m6.section_bytes(n, m6.FP4) < m6.section_bytes(n, m6.FP6_E2M3) == m6.section_bytes(n, m6.FP6_E3M2) <= m6.section_bytes(n, m6.FP8)
    assert m6.section_bytes(n, m6.FP6_E2M3) - (24 * nb + (nb + 15) // 16 * 16) == (8 if nb % 2 else 0)


@pytest.mark.parametrize("fmt", FP6)
def test_edge_inputs_hold_their_preconditions(fmt):
    F = m6.FORMATS[fmt]
    # on every grid value and every midpoint, both parities of the tie
    for s in (-3, -127, 100):
        w = m6.grid_and_midpoints(fmt, s)
        wb = mx.pad_blocks(w)
        sb, e, bad = m6.block_exponents(wb, fmt)
        assert np.all(e == s) and not bad.any()
        c_lo, frac, _ = m6.split_element(mx.scaled(wb, e), fmt)
        assert set(np.unique(frac)) == {f32(0), f32(0.5)}
        assert set(c_lo[frac == 0].tolist()) == set(range(F.cmax + 1)), "every grid value"
        ties = c_lo[frac == 0.5]
        assert set(ties.tolist()) == set(range(F.cmax)), "every midpoint"
        assert (ties % 2 == 0).any() and (ties % 2 == 1).any()
    # frac equals the draw exactly
    for s in (-5, 0, -127, 100):
        w, r, frac = m6.frac_equals_draw(fmt, s)
        wb = mx.pad_blocks(w)
        sb, e, _ = m6.block_exponents(wb, fmt)
        assert e[0] == s
        c_lo, fr, _ = m6.split_element(mx.scaled(wb, e), fmt)
        assert np.array_equal(fr.reshape(-1), frac) and np.all(c_lo.reshape(-1)[1:] == F.cmax - 1)
        up = mx.round_up(c_lo.reshape(-1), fr.reshape(-1), r)
        assert not up[:10].any() and up[11:21].all() and np.array_equal(up[21:], frac[21:] > 0)
        assert np.all(r[1:10] == frac[1:10]) and np.all(r[21:] == 0)
        assert np.all(r[11:21] < frac[11:21]) and np.all(frac[11:21].astype(np.float64) - r[11:21] == 2.0 ** -24)
    # y subnormal (or rounded to zero), and the two ties onto the subnormal grid go to even
    w = m6.subnormal_y(fmt)
    wb = mx.pad_blocks(w)
    sb, e, _ = m6.block_exponents(wb, fmt)
    assert e[0] == 8
    y = mx.scaled(wb, e).reshape(-1)
    assert np.all(y[1:12] < f32(2.0 ** -126)) and (y[1:12] > 0).sum() >= 8 and (y[1:12] == 0).sum() >= 2
    assert y[3] == f32(2 * 2.0 ** -149) and y[4] == f32(2 * 2.0 ** -149), "1.5 and 2.5 ulp: ties to even"
    # the blocks around MTHR, with this format's threshold
    blocks = m6.edge_blocks(fmt)
    assert mx.bits_of(blocks["min_subnormal"]).max() & 0x7fffffff == 1
    assert (mx.bits_of(blocks["all_subnormal"]) & 0x7fffffff).max() == 0x7fffff
    assert np.abs(blocks["flt_max"]).max() == np.finfo(f32).max
    assert F.mthr == {m6.FP6_E2M3: 0x700000, m6.FP6_E3M2: 0x600000}[fmt]
    for E in (1, 100, 254):
        a = (mx.bits_of(blocks["at_mthr_E%d" % E]) & 0x7fffffff).max()
        b = (mx.bits_of(blocks["above_mthr_E%d" % E]) & 0x7fffffff).max()
        assert a == (E << 23) | F.mthr and b == a + 1
        ea = m6.block_exponents(blocks["at_mthr_E%d" % E][None], fmt)[1][0]
        eb = m6.block_exponents(blocks["above_mthr_E%d" % E][None], fmt)[1][0]
        assert eb == max(E - 127 - F.emax + 1, -127) and ea == max(E - 127 - F.emax, -127)
        # at MTHR the maximum lands on mag(cmax) exactly; one ulp above it would pass it without the bump
        top = float(mx.from_bits([a])[0])
        assert top * 2.0 ** -float(ea) == m6.mag(F.cmax, fmt) or ea == -127
    # the hand-built payloads hold every code and every special scale byte
    sec = m6.payload_set(2 * 4096, fmt, 1)[0]
    sb, code = m6.unpack(sec, 2 * 4096, fmt)
    assert set(code.tolist()) == set(range(64)) and {0, 1, 126, 127, 253, 255} <= set(sb.tolist())


# relative L2 error of decode(compress(w)), 262,144 elements, to nearest / stochastic (uniform float32 draws): the README's table
N_TABLE = 262144
# gauss: RandomState(0).randn * 1e-3; student: RandomState(1).standard_t(3) * 1e-3; heavy: mx_contract.randn(n, 7); the draws:
# RandomState(2).rand.  The to-nearest figures of `heavy` depend on no seed chosen here.
ERROR_TABLE = {
    "gauss": {"fp4": (0.1158, 0.1650), "fp6_e2m3": (0.0283, 0.0401), "fp6_e3m2": (0.0529, 0.0749), "fp8": (0.0266, 0.0376)},
    "student": {"fp4": (0.1506, 0.2155), "fp6_e2m3": (0.0346, 0.0491), "fp6_e3m2": (0.0523, 0.0755), "fp8": (0.0267, 0.0378)},
    "heavy": {"fp4": (0.0852, 0.1265), "fp6_e2m3": (0.0309, 0.0361), "fp6_e3m2": (0.0496, 0.0583), "fp8": (0.0305, 0.0351)},
}


def _table_inputs():
    rs = np.random.RandomState(0)
    gauss = (rs.randn(N_TABLE) * 1e-3).astype(f32)
    student = (m6.student_t(N_TABLE, 3, 1).astype(np.float64) * 1e-3).astype(f32)
    heavy = mx.randn(N_TABLE, 7)
    r = np.random.RandomState(2).rand(N_TABLE).astype(f32)
    return {"gauss": gauss, "student": student, "heavy": heavy}, r


def measured_error_table():
    inputs, r = _table_inputs()
    return {name: {m6.NAMES[fmt]: (round(m6.rel_l2(w, fmt), 4), round(m6.rel_l2(w, fmt, r), 4)) for fmt in (m6.FP4, m6.FP6_E2M3, m6.FP6_E3M2, m6.FP8)}
            for name, w in inputs.items()}


def test_error_table_of_the_readme():
    got = measured_error_table()
    assert got == ERROR_TABLE, got
    readme = open(os.path.join(os.path.dirname(HERE), "README.md")).read()
    for fmt in ("fp4", "fp6_e2m3", "fp6_e3m2", "fp8"):
        cells = " | ".join("%.4f / %.4f" % got[name][fmt] for name in ("gauss", "student", "heavy"))
        assert cells in readme, "the README's row for %s: %s" % (fmt, cells)
    # what the table is quoted for: E2M3 within 10 % of FP8's error on Gaussian blocks, E3M2 flat across the three inputs
    assert got["gauss"]["fp6_e2m3"][0] < 1.1 * got["gauss"]["fp8"][0] and got["gauss"]["fp6_e2m3"][0] < 0.3 * got["gauss"]["fp4"][0]


# ---- the host side ---------------------------------------------------------------------------------------------------------------------
def test_driver_accepts_the_two_names_and_still_rejects_fp6():
    from gq_amd import driver
    from gq_amd.compressors import MXCompressor
    p = driver.build_parser()
    for name in ("fp6_e2m3", "fp6_e3m2"):
        assert p.parse_args(["--quantizer", "mx", "--mx-format", name]).mx_format == name
        assert MXCompressor(2000, (2000,), make_args(mx_format=name)).format == name
    for bad in ("fp6", "fp6_e5m2", "e2m3", "FP6_E2M3"):
        with pytest.raises(SystemExit):
            p.parse_args(["--quantizer", "mx", "--mx-format", bad])
        with pytest.raises(ValueError):
            MXCompressor(2000, (2000,), make_args(mx_format=bad))
    assert p.parse_args(["--quantizer", "mx"]).mx_format == "fp4"


def test_groups_by_format():
    from gq_amd.codecs import BatchedMX, BatchedMXR, MXCodec, MXRCodec
    from gq_amd.compressors import MXCompressor
    keys = {BatchedMX.group_key(MXCodec(MXCompressor(5000, (5000,), make_args(mx_format=f)), 5000, (5000,))) for f in MXCompressor.FORMATS}
    assert len(keys) == 4
    keys = {BatchedMXR.group_key(MXRCodec(MXCompressor(5000, (5000,), make_args(mx_format=f, mx_rotate="hadamard")), 5000, (5000,)))
            for f in MXCompressor.FORMATS}
    assert len(keys) == 4


def test_resnet50_wire_bytes():
    """Host arithmetic: the ResNet-50 list's wire per user for the 6-bit formats equals the contract's sections, and lies strictly
    between the fp4 and the fp8 wire."""
    from gq_amd.compressors import MXCompressor
    from gq_amd.quantizers import PSQuantizer
    with open(os.path.join(HERE, "golden", "resnet50_cifar_shapes.json")) as f:
        shapes = json.load(f)["parameter_shapes"]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    got = {}
    for fmt in (m6.FP4, m6.FP6_E2M3, m6.FP6_E3M2, m6.FP8):
        q = PSQuantizer(MXCompressor, params, make_args(mx_format=m6.NAMES[fmt]))
        dense = sum(4 * p.numel() for p in params if p.numel() <= 1000)
        want = sum(m6.section_bytes(p.numel(), fmt) for p in params if p.numel() > 1000) + dense
        assert q.wire_bytes_per_user() == (want + 15) // 16 * 16
        got[fmt] = q.wire_bytes_per_user()
    assert got[m6.FP4] < got[m6.FP6_E2M3] == got[m6.FP6_E3M2] < got[m6.FP8]
    assert 6.25 / 32 < got[m6.FP6_E2M3] / 94083376 < 6.3 / 32
    readme = open(os.path.join(os.path.dirname(HERE), "README.md")).read()
    assert "{:,}".format(got[m6.FP6_E2M3]) in readme, "the README quotes the fp6 wire: %d bytes" % got[m6.FP6_E2M3]


def test_abi_numbers_in_headers_and_binding_agree():
    from gq_amd import native
    inc = os.path.join(os.path.dirname(HERE), "include")
    hdr, hdr_r = open(os.path.join(inc, "gq_mx.h")).read(), open(os.path.join(inc, "gq_mxr.h")).read()
    assert native.MX_ABI_VERSION == native.MXR_ABI_VERSION == 2
    assert int(re.search(r"#define GQ_MX_ABI_VERSION (\d+)", hdr).group(1)) == native.MX_ABI_VERSION
    assert int(re.search(r"#define GQ_MXR_ABI_VERSION (\d+)", hdr_r).group(1)) == native.MXR_ABI_VERSION
    assert "#define GQ_MX_FP6_E2M3 0x%x" % native.MX_FP6_E2M3 in hdr and "#define GQ_MX_FP6_E3M2 0x%x" % native.MX_FP6_E3M2 in hdr
    assert (native.MX_FP6_E2M3, native.MX_FP6_E3M2) == (0x23, 0x32) == (m6.FP6_E2M3, m6.FP6_E3M2)
    assert native.mx_lib().gq_mx_abi_version() == 2 and native.mxr_lib().gq_mxr_abi_version() == 2
    # an older library fails at the accessor, not at the first launch
    desc = native.MX_LIBRARY
    saved = (desc.abi, desc.handle)
    try:
        desc.handle, desc.abi = None, 3
        with pytest.raises(native.GQNativeError, match="ABI version 2, this binding is written for 3"):
            native.mx_lib()
    finally:
        desc.abi, desc.handle = saved
    assert native.mx_lib() is not None
