"""gq_hsq_encode_batched, gq_hsq_levels_batched and gq_hsq_levels_decode_batched at every dispatch -- the prefilter instantiations of
csrc/hsq_encode_pf.hip (every sub-dimension, one / two / eight row blocks, segment records from LDS and from global memory, error
feedback off and on), the paged form of csrc/hsq_encode_pfd.hip, the exact form of csrc/hsq_encode.hip, the five level routes of
csrc/gq_api.hip and the fused level + decode launch -- against tests/hsq_encode_contract.py: numpy float32, one operation at a
time, nothing from a GPU kernel, tolerance 0 on the uint32 / byte views of the wire, u_flat, seg_minmax, the gradients, the
errors, `out` and the tail's outputs.  Through native.HSQBatch with hand-built tables: no quantizer, no codec.
tests/test_hsq_encode_contract.py asserts without a GPU that the mutations a kernel could carry would show on these inputs.

The steady-state cases (test_steady_state_*) are the `long` table -- 101 tiles -- and the `many` table -- 71 tensors in 75
tiles: with every grid capped at one compute unit's workgroups ($GQ_CU_COUNT=1) one workgroup runs all of them, a wave takes
about twelve tiles across tensors, a ring and a second pass of its own, and the workgroup's 64-entry (min, max) table overflows.
test_grid_capped_child runs them again in a child pytest process that has the variable set."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hsq_encode_contract as ec  # noqa: E402

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from gq_amd import native
    return native


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _same(got, want, what, nan_equal=False):
    """Tolerance 0 on the bits (bytes as they are); nan_equal: any NaN equals any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        if nan_equal:
            got, want = np.where(np.isnan(got), np.float32(np.nan), got), np.where(np.isnan(want), np.float32(np.nan), want)
        gb, wb = got.view(np.uint32), want.view(np.uint32)
    else:
        gb, wb = got, want
    bad = np.nonzero(gb.reshape(-1) != wb.reshape(-1))[0]
    assert bad.size == 0, "%s: %d of %d differ, the first at %d: got %r, want %r" % (
        what, bad.size, gb.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


class Rig(object):
    """The device side of a case: the float buffers, the wire, the tables with their pointers, the batch."""

    def __init__(self, lay, cb, gbuf, ebuf, err_rows, level, n_bit, u_flat, minmax, wire, workspace):
        native = _gpu()
        self.lay = lay
        self.g, self.e, self.wire = _t(gbuf), _t(ebuf), _t(wire)
        self.u, self.mm = _t(u_flat), _t(np.ascontiguousarray(minmax, dtype=np.uint32).view(np.int32))
        table = lay.table.copy()
        table[:, 0] = self.g.data_ptr() + 4 * table[:, 6]
        table[:, 7] = [self.e.data_ptr() + 4 * int(table[s, 6]) if err_rows[s] else 0 for s in range(lay.nseg)]
        assert all(int(p) % (16 if lay.d % 4 == 0 else 4) == 0 for p in table[:, 0])
        self.ws = native.new_workspace(torch.device("cuda:0"), lay.ntiles * 64) if workspace else None
        code_dtype = {1: torch.uint8, 4: torch.int32}[lay.code_bytes]
        level_dtype = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 0: torch.float32, ec.P6: native.PACKED6}[level]
        self.b = native.HSQBatch(_t(table), _t(lay.tile_seg), lay.nseg, lay.ntiles, _t(cb), code_dtype, level_dtype, n_bit,
                                 u_flat=self.u, seg_minmax=self.mm, workspace=self.ws)

    def minmax(self):
        return _np(self.mm).view(np.uint32)


# ---- encode ------------------------------------------------------------------------------------------------------------------------------
def _encode(c):
    e = ec.encode_of(c)
    lay = e.lay
    rig = Rig(lay, e.cb, e.gbuf, e.ebuf, [x is not None for x in e.errs], 1, 8, np.full(lay.ntiles * 64, ec.U_FILL, np.float32),
              np.tile(np.array([ec.M32, 0], np.uint32), (lay.nseg, 1)), lay.new_wire(), True)
    assert rig.b.path == c.path, "routed to %d, the case is for %d" % (rig.b.path, c.path)
    rig.b.encode(rig.wire, e.ef_scale)
    torch.cuda.synchronize()
    return e, rig


def _check_encode(c):
    e, rig = _encode(c)
    want, lay = e.want(), e.lay
    special = c.special is not None
    _same(_np(rig.wire), want["wire"], "wire (codes; every other byte its canary, the sections' padding included)")
    u = _np(rig.u)
    stated = np.zeros(u.size, bool)
    for s in range(lay.nseg):
        stated[lay.slots(s)] = True
    _same(u[stated], want["u_flat"][stated], "u_flat", nan_equal=special)
    pad = u[~stated].view(np.uint32)      # a padding slot keeps its value or becomes +0 (include/gq_hsq.h)
    assert np.isin(pad, [0, int(np.array([ec.U_FILL]).view(np.uint32)[0])]).all(), "u_flat's padding slots"
    mm = rig.minmax()
    keep = slice(1, None) if special else slice(None)      # the non-finite rows lie in tensor 0
    _same(mm[keep], want["minmax"][keep], "seg_minmax")
    _same(_np(rig.g), want["gbuf"], "gradients (v over the rows with an error buffer, the rest and every gap as uploaded)", nan_equal=special)
    _same(_np(rig.e), want["ebuf"], "error buffers (untouched by the encode)")
    return e, rig


@pytest.mark.parametrize("c", ec.PF_CASES, ids=ec.ecase_id)
def test_encode_prefilter(c):
    _check_encode(c)


@pytest.mark.parametrize("c", ec.PAGED_CASES, ids=ec.ecase_id)
def test_encode_paged(c):
    _check_encode(c)


@pytest.mark.parametrize("c", ec.EXACT_CASES, ids=ec.ecase_id)
def test_encode_exact(c):
    _check_encode(c)


@pytest.mark.parametrize("c", ec.NONFINITE_CASES, ids=ec.ecase_id)
def test_encode_nonfinite_rows(c):
    """A row with an infinity and a row with a NaN: codes and u are the oracle's (torch.argmax ranks a NaN first); the tensor's
    seg_minmax words are not part of this comparison (include/gq_hsq.h says what they hold)."""
    _check_encode(c)


@pytest.mark.parametrize("c", ec.STEADY_CASES, ids=ec.ecase_id)
def test_steady_state_encode(c):
    _check_encode(c)


@pytest.mark.parametrize("d,K", ec.LOG_SHAPES, ids=lambda x: str(x))
def test_steady_state_fixup_log(d, K):
    """The flat entry point, impl = prefilter -- the multi-tensor launches share its template and its bound but do not write the
    workspace's log: every near-tie row and every tiny row is in the log (the first pass cannot settle them wherever they lie),
    the zero rows are not.  A huge row is in it on the paged kernel, whose window is absolute.  On the f16 kernel it need not be:
    a wave's first tile takes its scale from its own largest element, and a wave that met a huge row there keeps that scale
    while the sampled rows of its tiles convert to zero -- the huge rows of its later tiles are then inside the window, and
    the rows beside them are the logged ones."""
    native = _gpu()
    g, kinds, codes, u = ec.log_case(d, K)
    M = ec.LOG_M
    paged = K > 256
    dg, dcb = _t(g.reshape(-1)), _t(ec.codebook(d, K))
    dcodes = torch.zeros(M, dtype=torch.int32 if paged else torch.uint8, device="cuda:0")
    du = torch.full((M,), float(ec.U_FILL), dtype=torch.float32, device="cuda:0")
    ws = native.new_workspace(torch.device("cuda:0"), M)
    native.mark_worklist(ws, M)
    native.hsq_encode(dg, dcb, dcodes, du, ws, impl=native.ENCODE_PREFILTER_D16K256)
    torch.cuda.synchronize()
    _same(_np(dcodes).astype(np.int32), codes, "codes")
    _same(_np(du), u, "u")
    log = _np(ws[native.WS_LOG_FIRST:native.WS_LOG_FIRST + M].view(torch.int32))
    logged = log >= 0
    assert np.array_equal(log[logged], np.nonzero(logged)[0])
    is_ = lambda *names: np.isin(kinds, [ec.KIND[n] for n in names])
    must = is_(*ec.LOGGED)
    if paged:
        must |= is_("huge")
    assert must.sum() > 0 and logged[must].all(), "rows the first pass cannot settle are missing from the log: %s" % np.nonzero(must & ~logged)[0][:8]
    assert not logged[is_("zero+", "zero-")].any()
    print("%d of %d rows logged, %d of them required" % (logged.sum(), M, must.sum()))


# ---- levels ------------------------------------------------------------------------------------------------------------------------------
def _level_rig(c):
    native = _gpu()
    lv = ec.levels_of(c)
    rig = Rig(lv.lay, lv.cb, lv.gbuf, lv.ebuf, [s % 3 != 1 for s in range(lv.lay.nseg)], c.level, c.n_bit, lv.u_flat, lv.minmax, lv.wire0, False)
    rig.r = _t(lv.r_flat)
    rig.srcs = [_t(x) for x in lv.dense_src]
    if c.ndense:
        rig.dt = _t(np.array([[t.data_ptr(), at, t.numel()] for t, at in zip(rig.srcs, lv.lay.dense_at)], np.int64))
        rig.b.set_dense(rig.dt, c.ndense)
    return native, lv, rig


def _check_levels(lv, rig, want, out=None):
    _same(_np(rig.wire), want["wire"], "wire (levels, (lb, ub), dense copies; the codes and every other byte as they were)")
    _same(_np(rig.e), want["ebuf"], "error buffers")
    _same(_np(rig.g), lv.gbuf, "gradients (read only)")
    _same(_np(rig.u), lv.u_flat, "u_flat (read only)")
    _same(rig.minmax(), lv.minmax, "seg_minmax (read only)")
    if out is not None:
        _same(_np(out), want["out"], "out")


def _launch_levels(c):
    native, lv, rig = _level_rig(c)
    rig.b.levels(rig.wire, c.mode, 1234, rig.r if c.mode == ec.GIVEN else None, write_error=bool(c.write_error))
    torch.cuda.synchronize()
    return lv, rig


@pytest.mark.parametrize("c", ec.LEVEL_CASES, ids=ec.lcase_id)
def test_levels(c):
    lv, rig = _launch_levels(c)
    _check_levels(lv, rig, lv.want())


@pytest.mark.parametrize("c", ec.LEVEL_STEADY, ids=ec.lcase_id)
def test_steady_state_levels(c):
    lv, rig = _launch_levels(c)
    _check_levels(lv, rig, lv.want())


@pytest.mark.parametrize("c", ec.DRAW_CASES, ids=ec.lcase_id)
def test_levels_device_draws(c):
    """GQ_RANDOM_DEVICE / _KEYED: every level is the truncated one or one more, the same seed replays the same wire, and the
    rest of the contract holds exactly for the levels actually written."""
    lv, rig = _launch_levels(c)
    wire = _np(rig.wire)
    got = [ec.levels_in(lv.lay, wire, s) for s in range(lv.lay.nseg)]
    for s, (l, l0) in enumerate(zip(got, lv.levels(r=[None] * lv.lay.nseg))):
        assert np.isin(l - l0, (0, 1)).all(), "tensor %d: a level is not the truncated one or one more" % s
    assert sum(int((l != l0).sum()) for l, l0 in zip(got, lv.levels(r=[None] * lv.lay.nseg))) > 0, "no level was rounded up"
    _check_levels(lv, rig, lv.want(levels=got))
    _, rig2 = _launch_levels(c)
    _same(_np(rig2.wire), wire, "the same seed's wire")


# ---- fused level + decode ------------------------------------------------------------------------------------------------------------------
def _launch_fused(f, fused=True):
    native, lv, rig = _level_rig(f.l)
    c, lay = f.l, lv.lay
    out = torch.full((lay.floats,), float(ec.FILL), dtype=torch.float32, device="cuda:0")
    tail = None
    if f.tail:
        n = sum(lay.dense)
        rows = rig.wire[lay.dense_off: lay.dense_off + 4 * n].view(torch.float32).view(1, n)
        rig.dense_out = torch.full((n + 16,), float(ec.FILL), dtype=torch.float32, device="cuda:0")
        rig.rng = _t(np.array([[11 + i, 100 * (i + 1)] for i in range(ec.RNG_PAIRS)], np.int64))
        rig.reset_src = _t(np.arange(1, ec.RESET_WORDS + 1, dtype=np.int64) * 0x0101010101)
        rig.reset_dst = torch.zeros(ec.RESET_WORDS, dtype=torch.int64, device="cuda:0")
        rig.ticket = torch.zeros(native.TICKET_WORDS, dtype=torch.int32, device="cuda:0")
        tail = native.StepTail(rows=rows, out=rig.dense_out[8:8 + n], rng_state=rig.rng, reset=(rig.reset_dst, rig.reset_src), ticket=rig.ticket)
    r = rig.r if c.mode == ec.GIVEN else None
    if fused:
        rig.b.levels_decode(rig.wire, c.mode, 1234, r, bool(c.write_error), out, plain=bool(f.plain), tail=tail)
    else:
        rig.b.levels(rig.wire, c.mode, 1234, r, write_error=bool(c.write_error))
        rig.b.decode(rig.wire[:lay.P].view(1, lay.P), 1, out, plain=bool(f.plain), tail=tail)
    torch.cuda.synchronize()
    return lv, rig, out


def _check_fused(f, fused=True):
    lv, rig, out = _launch_fused(f, fused)
    want = lv.want(plain=bool(f.plain))
    _check_levels(lv, rig, want, out)
    if f.tail:
        n = sum(lv.lay.dense)
        dense = np.full(n + 16, ec.FILL, np.float32)
        dense[8:8 + n] = want["dense_out"]
        _same(_np(rig.dense_out), dense, "the dense rows' mean, (+0 + x) / 1")
        _same(_np(rig.rng), np.array([[11 + i, 100 * (i + 1) + 1] for i in range(ec.RNG_PAIRS)], np.int64), "{ seed, step } pairs")
        _same(_np(rig.reset_dst), _np(rig.reset_src), "reset words")
        assert not _np(rig.ticket).any(), "the ticket words are not zero after the launch"
    return lv, rig, out


@pytest.mark.parametrize("f", ec.FUSED_SERVED, ids=ec.fcase_id)
def test_fused_served(f):
    _check_fused(f)


@pytest.mark.parametrize("f", ec.FUSED_UNSERVED, ids=ec.fcase_id)
def test_fused_unserved_equals_the_two_launches(f):
    _, a, out_a = _check_fused(f)
    _, b, out_b = _check_fused(f, fused=False)
    _same(_np(a.wire), _np(b.wire), "wire")
    _same(_np(out_a), _np(out_b), "out")


@pytest.mark.parametrize("f", ec.FUSED_STEADY, ids=ec.fcase_id)
def test_steady_state_fused(f):
    _check_fused(f)


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ec.CHAIN_CASES, ids=ec.ecase_id)
def test_steady_state_chain(c):
    """encode -> levels (write_error) -> decode with R = 1 on the long table, every stage against the reference."""
    e, rig = _check_encode(c)
    lay = e.lay
    want = ec.chain_want(e, 8)
    enc = e.want()
    rig.b.levels(rig.wire, ec.OFF, 0, None, write_error=True)
    torch.cuda.synchronize()
    _same(_np(rig.wire), want["wire"], "wire behind the level launch")
    _same(_np(rig.e), want["ebuf"], "error buffers behind the level launch")
    _same(_np(rig.g), enc["gbuf"], "gradients behind the level launch")
    out = torch.full((lay.floats,), float(ec.FILL), dtype=torch.float32, device="cuda:0")
    rig.b.decode(rig.wire[:lay.P].view(1, lay.P), 1, out, plain=False)
    torch.cuda.synchronize()
    _same(_np(out), want["out"], "out")
    _same(_np(rig.wire), want["wire"], "wire behind the decode")


def test_grid_capped_child():
    """The steady-state cases with every grid capped at one compute unit's workgroups: one encode workgroup whose waves take about
    twelve tiles each across tensor boundaries, with a ring and a second pass per wave and more tensors than its (min, max) table
    holds; the level kernels' later trips."""
    _gpu()
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__, "-k", "steady_state"],
                       env=dict(os.environ, GQ_CU_COUNT="1"), capture_output=True, text=True, timeout=600)
    tail = r.stdout[-2000:] + r.stderr[-2000:]
    assert r.returncode == 0 and " passed" in r.stdout and " skipped" not in r.stdout, tail
    print(r.stdout.strip().splitlines()[-1])
