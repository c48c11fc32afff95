"""gq_hsq_decode_sum_batched at every dispatch of csrc/hsq_batched.hip -- hsq_decode_sum_batched4_r_kernel (d = 16, every compile-time
payload count, exact and fused), hsq_decode_sum_batched4_rc_kernel (the chunked one), hsq_decode_sum_batched_tile_kernel (a wave per
tile) and hsq_decode_sum_batched_any_kernel -- against tests/hsq_decode_contract.py: numpy float32, one operation at a time, nothing
from a kernel, tolerance 0 on the uint32 view of the whole `out` (so every float between the tensors' spans is untouched too), and
the gathered buffer byte for byte what was uploaded.  Through native.HSQBatch(...).decode with hand-built tables, no quantizer.
tests/test_hsq_decode_contract.py asserts without a GPU that a wrong order of additions, a multiplication by 1 / R or a fused
multiply-add would show on these inputs.

The steady-state cases (test_steady_state_*) are the long table -- 101 tiles -- and the single-tensor level quantiser at a size
where, with the grids capped at one compute unit's workgroups ($GQ_CU_COUNT=1, read once per process), every wave makes three or
more trips: test_grid_capped_child runs them again in a child pytest process that has the variable set."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hsq_decode_contract as dc  # noqa: E402

pytestmark = pytest.mark.gpu

OFF, GIVEN = 0, 1


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from gq_amd import native
    return native


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _launch(c, fma=False):
    """One decode launch of the case -> (`out` as the launch left it, the wire): the gathered buffer is checked here."""
    native = _gpu()
    w = dc.wire_of(c)
    code_dtype = {1: torch.uint8, 4: torch.int32}[c.code_bytes]
    level_dtype = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 0: torch.float32, dc.P6: native.PACKED6}[c.level]
    dbuf = _t(w.buf)
    gathered = torch.as_strided(dbuf, (c.R, w.P), (w.P, 1), w.lead)
    assert gathered.data_ptr() % 16 == 0
    out = torch.full((w.out_floats,), dc.OUT_FILL, dtype=torch.float32, device="cuda:0")
    b = native.HSQBatch(_t(w.table), _t(w.tile_seg), len(w.Ms), w.ntiles, _t(w.cb), code_dtype, level_dtype, c.n_bit)
    b.decode(gathered, c.R, out, plain=w.plain, fma=fma)
    torch.cuda.synchronize()
    assert np.array_equal(dbuf.cpu().numpy(), w.buf)
    return out.cpu().numpy(), w


def _exact(c, fma=False):
    got, w = _launch(c, fma)
    bad = np.nonzero(got.view(np.uint32) != w.want().view(np.uint32))[0]
    assert bad.size == 0, "%d of %d floats differ, the first at %d: got %r, want %r (in a span: %s)" % (
        bad.size, got.size, bad[0], got[bad[0]], w.want()[bad[0]], bool(w.spans()[bad[0]]))


@pytest.mark.parametrize("c", dc.D16_CASES, ids=dc.case_id)
def test_d16(c):
    _exact(c)


@pytest.mark.parametrize("c", dc.FMA_LOOSE, ids=dc.case_id)
def test_d16_fused(c):
    """GQ_AGGREGATE_FMA at the payload counts that serve it: relative L2 <= 1e-6 of the exact mean, nothing outside the spans."""
    got, w = _launch(c, fma=True)
    m = w.spans()
    assert np.array_equal(got[~m].view(np.uint32), w.want()[~m].view(np.uint32))
    err = dc.rel_l2(got[m], w.want()[m])
    print("relative L2 of the fused aggregate: %.3e" % err)
    assert err <= 1e-6


@pytest.mark.parametrize("c", dc.FMA_EXACT, ids=dc.case_id)
def test_fma_flag_where_it_is_not_served(c):
    _exact(c, fma=True)


@pytest.mark.parametrize("c", dc.TILE_CASES, ids=dc.case_id)
def test_tile(c):
    _exact(c)


@pytest.mark.parametrize("c", dc.ANY_CASES, ids=dc.case_id)
def test_any_shape(c):
    _exact(c)


@pytest.mark.parametrize("c", dc.STEADY_CASES, ids=dc.case_id)
def test_steady_state_decode(c):
    _exact(c)


@pytest.mark.parametrize("misaligned", [0, 1], ids=["aligned", "off_by_a_float"])
@pytest.mark.parametrize("given", [False, True], ids=["off", "given"])
@pytest.mark.parametrize("level,off_bit,given_bit", dc.LEVELS_FORMS, ids=["u8", "u16", "i32", "p6"])
def test_steady_state_levels(level, off_bit, given_bit, given, misaligned):
    """gq_hsq_levels behind gq_minmax_partials at dc.LEVELS_M projections: levels against hsq_dequant_contract.quantise / pack6,
    (lb, ub) against the exact extrema, the 16 bytes in front of and behind the level section untouched.  misaligned: `u` one
    float off a 16-byte boundary (the scalar path)."""
    native = _gpu()
    n_bit = given_bit if given else off_bit
    u, r, _, section, (lb, ub) = dc.levels_case(level, n_bit, given)
    M = u.size
    ubuf = _t(np.concatenate([np.zeros(misaligned, np.float32), u]))
    du = ubuf[misaligned:]
    assert du.data_ptr() % 16 == 4 * misaligned and du.numel() == M
    want = np.concatenate([np.full(16, dc.CANARY, np.uint8), section, np.full(16, dc.CANARY, np.uint8)])
    lbuf = torch.full((want.size,), dc.CANARY, dtype=torch.uint8, device="cuda:0")
    levels = lbuf[16:16 + section.size]
    if level != dc.P6:
        levels = levels.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[level])
    lb_ub = torch.full((2,), dc.OUT_FILL, dtype=torch.float32, device="cuda:0")
    partials = native.new_workspace(torch.device("cuda:0"), M)
    native.minmax_partials(du, partials)
    native.hsq_levels(du, n_bit, GIVEN if given else OFF, _t(r) if given else None, 0, partials, lb_ub, levels, packed6=(level == dc.P6))
    torch.cuda.synchronize()
    assert np.array_equal(lb_ub.cpu().numpy().view(np.uint32), np.array([lb, ub], np.float32).view(np.uint32))
    got = lbuf.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%d bytes differ, the first at %d (the section is bytes 16 .. %d)" % (bad.size, bad[0], 16 + section.size)
    assert np.array_equal(ubuf.cpu().numpy()[misaligned:].view(np.uint32), u.view(np.uint32))


def test_grid_capped_child():
    """The steady-state cases with every grid capped at one compute unit's workgroups: a wave's second and later tiles, the
    re-request into the registers just consumed and the hand-over of `cur` / `nxt` / `aft` across tensors; the level quantiser's
    loads from its third trip on."""
    _gpu()
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__, "-k", "steady_state"],
                       env=dict(os.environ, GQ_CU_COUNT="1"), capture_output=True, text=True, timeout=300)
    tail = r.stdout[-2000:] + r.stderr[-2000:]
    assert r.returncode == 0 and " passed" in r.stdout and " skipped" not in r.stdout, tail
    print(r.stdout.strip().splitlines()[-1])
