"""tests/ctk_contract.py against independent witnesses, without a GPU: torch.topk per item on tie-free input, a scalar loop on ties, the
section-size formula against gq_amd.codecs and the header's macro, and the README's error table from fixed seeds.  Every claim an input
makes about itself (tie-free; a tie block that straddles `need` at a named seam) is asserted here before a GPU test relies on it."""
import os
import re

import numpy as np
import pytest
import torch

import ctk_contract as cc
import topk_contract as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _items(w):
    return [(b, w[b:b + cc.CHUNK]) for b in range(0, w.size, cc.CHUNK)]


@pytest.mark.parametrize("cr", cc.CRS)
@pytest.mark.parametrize("kind", ["gauss", "student"])
def test_against_torch_topk_per_item(kind, cr):
    w = cc.make(kind, 2 * 4096 + cr + 1, 1)
    assert all(np.unique(tc.keys(x)).size == x.size for _, x in _items(w)), "the input is not tie-free"
    want = [b + np.sort(torch.topk(torch.from_numpy(x).abs(), x.size // cr).indices.numpy()) for b, x in _items(w)]
    idx, pos = cc.kept(w, cr)
    assert np.array_equal(idx, np.concatenate(want)) and np.array_equal(pos, idx % 4096) and idx.size == cc.kept_count(w.size, cr)
    sec = cc.section_bytes(w, cr)
    assert sec.size == cc.section_size(w.size, cr) and np.array_equal(sec[cc.up16(2 * idx.size):][:4 * idx.size].view(np.float32), w[idx])
    assert np.array_equal(cc.decode_mean([sec], w.size, cr, plain=True), cc.dense(w, cr))      # (finite input: -0 == +0 where dropped)


@pytest.mark.parametrize("w,cr", [(cc.tie_input(last), cc.TIE_CR) for last in cc.TIE_LASTS] + [(cc.make(k, 4096 + 300, 3), 16) for k in ("equal", "low7")])
def test_against_a_scalar_loop_on_ties(w, cr):
    want = []
    for b, x in _items(w):
        ranked = sorted(range(x.size), key=lambda i: (-int(tc.keys(x)[i]), i))
        want += sorted(b + i for i in ranked[:x.size // cr])
    assert list(cc.kept(w, cr)[0]) == want


@pytest.mark.parametrize("last", cc.TIE_LASTS)
def test_the_tie_block_straddles_need_at_its_seam(last):
    s = tc.select(cc.tie_input(last), 4096 // cc.TIE_CR)
    assert (s["T"], s["gt"], s["ties"], s["need"], s["last"]) == (tc.ONE, 100, 196, 156, last)
    assert (last + 1) % 4 == 0 and ((last + 1) % 256 == 0 or last in (259, 1027))      # a lane seam; 255 a wave seam, 1023 a register step


def test_low7_keys_differ_in_the_last_pass_alone():
    k = tc.keys(cc.make("low7", 4096, 5))
    assert np.unique(k >> 7).size == 1 and np.unique(k).size > 100


def test_section_sizes():
    from gq_amd.codecs import ctk_section_bytes
    with open(os.path.join(ROOT, "include", "gq_ctk.h")) as f:
        assert "(2 * GQ_CTK_KEPT(n, cr) + 15) / 16 * 16 + (4 * GQ_CTK_KEPT(n, cr) + 15) / 16 * 16" in f.read()
    for cr in cc.CRS + [3, 1000]:
        for n in cc.SIZES(cr) + [25_000_000]:
            K = sum(min(4096, n - b) // cr for b in range(0, n, 4096))
            assert cc.kept_count(n, cr) == K and ctk_section_bytes(n, cr) == cc.section_size(n, cr) == cc.up16(2 * K) + cc.up16(4 * K)


def _rel_err(w, cr, per_item):
    d = cc.dense(w, cr) if per_item else tc.dense(w, w.size // cr)
    return float(np.linalg.norm((w - d).astype(np.float64)) / np.linalg.norm(w.astype(np.float64)))


def error_table():
    """The README's rows: relative L2 error of decode(compress(x)) at cr = 16 / 64 / 256, global top-k against per-item, 262,144 elements."""
    n, rs = 262144, np.random.RandomState(2024)
    scale = np.repeat(np.exp(rs.standard_normal(n // 4096)), 4096)
    inputs = [("i.i.d. Gaussian", rs.standard_normal(n)), ("Student-t(3)", rs.standard_t(3, n)),
              ("per-item log-normal scale (the bad case)", rs.standard_normal(n) * scale)]
    return ["| %s | %s | %s |" % (name, " / ".join("%.4f" % _rel_err(x.astype(np.float32), cr, False) for cr in (16, 64, 256)),
                                 " / ".join("%.4f" % _rel_err(x.astype(np.float32), cr, True) for cr in (16, 64, 256))) for name, x in inputs]


def test_the_readme_carries_the_error_table_and_the_resnet50_wire():
    from gq_amd.codecs import ctk_section_bytes
    from gq_amd.driver import ResNet50
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    for row in error_table():
        assert row in readme, row
    # (one user's wire as the quantizer lays it out: the sections, multiples of 16 bytes, then the small tensors as they are)
    wire = cc.up16(sum(ctk_section_bytes(p.numel(), 256) if p.numel() > 1000 else 4 * p.numel() for p in ResNet50().parameters()))
    assert re.search(r"chunked top-k[^\n]*\b%s B" % format(wire, ","), readme), wire
