"""What PACKED16 (include/gq_ctk.h) promises, on tests/ctk_packed_contract.py and without a GPU: the levels and bounds as integers, the
section size against the header's macro, and the README's error table from fixed seeds."""
import os
import re

import numpy as np
import pytest

import ctk_contract as cc
import ctk_packed_contract as pc
import topk_contract as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_levels_and_bounds():
    """Over every kind of input at four ratios: levels in 0 ... 7, T <= dk <= H and 14 |dk - k| <= D + 6 on every kept element; both end
    levels, an item of equal keys (D == 0) and an item that keeps nothing occur."""
    seen_levels, seen = set(), set()
    for cr in cc.CRS:
        for i, kind in enumerate(cc.KINDS):
            w = cc.make(kind, 2 * 4096 + cr - 1, 40 + i)
            bounds, words, dec, idx = pc.encode(w, cr)
            T, H = (bounds[idx // 4096, j].astype(np.int64) for j in (0, 1))
            k, lev, dk = tc.keys(w)[idx].astype(np.int64), words.astype(np.int64) >> 12 & 7, (tc.bits(dec)[idx] & 0x7fffffff).astype(np.int64)
            assert np.all(T <= dk) and np.all(dk <= H) and np.all(14 * np.abs(dk - k) <= H - T + 6), (kind, cr)
            assert np.array_equal(words & 0xfff, idx % 4096) and np.array_equal(words >> 15, tc.bits(w)[idx] >> 31)
            seen_levels |= set(lev.tolist())
            seen |= {"D == 0"} if np.any((H == T) & (T > 0)) else set()
            seen |= {"k_t == 0"} if not np.any(idx >= 2 * 4096) and not bounds[2].any() else set()
    assert seen_levels == set(range(8)) and seen == {"D == 0", "k_t == 0"}


@pytest.mark.parametrize("cr", [2, 3, 16, 256, 1000, 4096])
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 3 * 4096, 3 * 4096 + 17, 25_000_000])
def test_section_bytes_equal_the_headers_macro(n, cr):
    """n of one, two, three and four items (odd counts: the 8-byte pad behind the bounds) against the macro's own text, evaluated."""
    from gq_amd.codecs import ctk_packed_section_bytes
    with open(os.path.join(ROOT, "include", "gq_ctk.h")) as f:
        macros = dict(re.findall(r"^#define (GQ_CTK_\w+)(?:\(n, cr\))? +(.+?)(?: +/\*.*)?$", f.read(), re.M))
    text = macros["GQ_CTK_PACKED_SECTION_BYTES"].replace("GQ_CTK_KEPT(n, cr)", macros["GQ_CTK_KEPT"])
    text = text.replace("GQ_CTK_CHUNK", macros["GQ_CTK_CHUNK"]).replace("(int64_t)", "").replace("/", "//")
    assert ctk_packed_section_bytes(n, cr) == pc.section_size(n, cr) == eval(text, {"n": n, "cr": cr})
    assert pc.section_size(n, cr) == cc.up16(8 * -(-n // 4096)) + cc.up16(2 * cc.kept_count(n, cr))


def error_table():
    """[(README row, [(this format's error, the one-magnitude rule's)] at cr = 16 / 64 / 256)]: relative L2 error over the kept set against
    float64 of the true values, 262,144 elements.  One magnitude: sign(w) times the mean |w| of the tensor's kept set (STC's rule)."""
    n, rs = 262144, np.random.RandomState(2025)
    scale = np.repeat(np.exp(rs.standard_normal(n // 4096)), 4096)
    inputs = [("N(0, 1) * 1e-3", rs.standard_normal(n) * 1e-3), ("Student-t(3) * 1e-3", rs.standard_t(3, n) * 1e-3),
              ("per-item log-normal scale", rs.standard_normal(n) * scale)]
    rows = []
    for name, x in inputs:
        w, cells = x.astype(np.float32), []
        for cr in (16, 64, 256):
            _, _, dec, idx = pc.encode(w, cr)
            true = w[idx].astype(np.float64)
            one = np.sign(true) * np.abs(true).mean()
            cells.append(tuple(float(np.linalg.norm(d - true) / np.linalg.norm(true)) for d in (dec[idx].astype(np.float64), one)))
        rows.append(("| %s | %s | %s |" % (name, " / ".join("%.4f" % a for a, _ in cells), " / ".join("%.4f" % b for _, b in cells)), cells))
    return rows


def test_the_readme_carries_the_error_table_and_the_resnet50_wire():
    from gq_amd.codecs import ctk_packed_section_bytes
    from gq_amd.driver import ResNet50
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    for row, cells in error_table():
        print(row)
        assert all(a < b for a, b in cells), row
        assert row in readme, row
    wire = cc.up16(sum(ctk_packed_section_bytes(p.numel(), 256) if p.numel() > 1000 else 4 * p.numel() for p in ResNet50().parameters()))
    print(wire)
    assert re.search(r"packed16[^\n]*\b%s B" % format(wire, ","), readme), wire
