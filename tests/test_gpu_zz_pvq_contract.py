"""The ProbabilisticVectorCompressor's encode kernels held to tests/pvq_contract.py at tolerance 0 on draws that sit ON the
sampler's thresholds and a ladder of ulps to both sides of them (tests/test_pvq_contract.py shows without a GPU that a wrong kernel
would be seen on them): gq_pvq_encode -- the one-sweep kernel pvq_encode_walk_kernel, the two-sweep matrix-core kernel
pvq_encode_lds_kernel and, in a child process with $GQ_PVQ_VALU, the VALU kernel pvq_encode_kernel --, its stage1 form,
gq_pvq_encode_batched with error feedback off and on, and gq_rq_encode2_batched, the last three through pw_encode_tile of
csrc/pvq_walk.hpp.  Codes byte for byte (uint8 and int32), u and (lb, ub) bit for bit; where a row holds inf or NaN, any NaN equals
any NaN.  The library reads $GQ_PVQ_EPS, $GQ_PVQ_TWO_SWEEPS, $GQ_PVQ_VALU and $GQ_CU_COUNT once, so the flat cases run again in one
child pytest process per setting.
(The file's name sorts behind the other GPU files: see the docstring of tests/test_gpu_z_mx6_api.py.)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import hsq_encode_contract as ec  # noqa: E402
import pvq_contract as pc  # noqa: E402
import rq_contract as rc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def nat(oracle):
    from gq_amd import native
    native.lib()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return native


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _same(got, want, what):
    """Tolerance 0 on the bits; any NaN equals any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        nan = np.float32(np.nan)
        got, want = np.where(np.isnan(got), nan, got).view(np.uint32), np.where(np.isnan(want), nan, want).view(np.uint32)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, "%s: %d of %d differ, the first at %d: got %r, want %r" % (
        what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def _flat(nat, tab, grad=None, stage1=None, code_np=None, first=0, count=None):
    """gq_pvq_encode over rows [first, first + count) of a table (grad: what the kernel reads in their place, with stage1) ->
    codes, the bits of u and the (lb, ub) gq_hsq_levels folds from the workspace against the contract."""
    count = tab.M - first if count is None else count
    sl = slice(first, first + count)
    code_np = code_np or tab.code_np
    dev = torch.device("cuda:0")
    g = _t(rc.f32(tab.x[sl] if grad is None else grad).reshape(-1))
    codes = torch.full((count,), 77, dtype=torch.uint8 if code_np == np.uint8 else torch.int32, device=dev)
    u = torch.full((count,), -3.0, dtype=torch.float32, device=dev)
    ws = nat.new_workspace(dev, count)
    nat.pvq_encode(g, _t(tab.cdag), codes, u, ws, nat.RANDOM_GIVEN, _t(tab.r[sl]), 0, stage1=stage1)
    lb_ub = torch.empty(2, dtype=torch.float32, device=dev)
    levels = torch.empty(count, dtype=torch.uint8, device=dev)
    nat.hsq_levels(u, 6, 0, None, 0, ws, lb_ub, levels)
    torch.cuda.synchronize()
    got = codes.cpu().numpy().astype(np.int32)
    bad = np.flatnonzero(got != tab.codes[sl])
    where = {int(i) + first: (k, j) for i, k, j in tab.entries + tab.extra}
    assert bad.size == 0, "codes: %d of %d differ; (row, got, want, (k, j) of an on-threshold draw): %r" % (
        bad.size, count, [(int(i) + first, int(got[i]), int(tab.codes[sl][i]), where.get(int(i) + first)) for i in bad[:12]])
    _same(u.cpu().numpy(), tab.u[sl], "u")
    _same(lb_ub.cpu().numpy(), np.array(pc.lb_ub(tab.u[sl]), np.float32), "(lb, ub)")


# ---- gq_pvq_encode: the tests whose names hold `flat` run again in the children -------------------------------------------------------
@pytest.mark.parametrize("dk", pc.ONE_SWEEP, ids=pc.table_id)
def test_flat_one_sweep(nat, dk):
    _flat(nat, pc.table(*dk))


def test_flat_one_sweep_int32_codes(nat):
    _flat(nat, pc.table(16, 256), code_np=np.int32)


@pytest.mark.parametrize("dk", pc.TWO_SWEEP, ids=pc.table_id)
def test_flat_two_sweep(nat, dk):
    _flat(nat, pc.table(*dk))


@pytest.mark.parametrize("dk", pc.CAPPED, ids=pc.table_id)
def test_flat_grid_capped(nat, dk):
    """Forty-one tiles: with the grids capped at one compute unit's workgroups a wave walks several tiles, each fetched while the
    one before it is encoded."""
    _flat(nat, pc.table(dk[0], dk[1], pc.M_CAPPED))


def _child(env, select):
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__, "-k", select],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=os.path.dirname(HERE))
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0 and " passed" in r.stdout and " skipped" not in r.stdout and " deselected" in r.stdout, tail
    print(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("env,select", [
    ({"GQ_PVQ_EPS": "1e-3"}, "flat"),             # most lanes unsettled: the wave's prefix-sum walk
    ({"GQ_PVQ_EPS": "-1e-3"}, "flat"),            # ... the term-by-term walk
    ({"GQ_PVQ_TWO_SWEEPS": "1"}, "flat"),         # the two-sweep kernel on the one-sweep kernel's tables
    ({"GQ_PVQ_VALU": "1"}, "flat and not d10- and not d48-"),      # pvq_encode_kernel, at every d it is built for
    ({"GQ_CU_COUNT": "1"}, "flat_grid_capped"),
], ids=["wave_walk", "term_by_term", "two_sweeps", "valu", "one_cu"])
def test_children(env, select):
    assert all(d in pc.VALU_D for d, _ in pc.ONE_SWEEP + pc.TWO_SWEEP if d not in (10, 48))
    _child(env, select)


# ---- gq_pvq_encode_batched ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.MULTI_CASES, ids=pc.multi_id)
def test_multi_tensor(nat, c):
    """Tensors of 1, 63, 64, 65 and 337 subvectors, draws through r_flat: the codes sections of the wire with every other byte
    its canary, u_flat's valid slots, seg_minmax, the gradients (v over those with an error buffer; the others, the gaps and the
    error buffers as uploaded)."""
    m = pc.multi_case(*c)
    lay = m.lay
    g, e, wire = _t(m.gbuf), _t(m.ebuf), _t(lay.new_wire())
    u = _t(np.full(lay.ntiles * 64, ec.U_FILL, np.float32))
    mm = _t(np.tile(np.array([ec.M32, 0], np.uint32), (lay.nseg, 1)).view(np.int32))
    table = lay.table.copy()
    table[:, 0] = g.data_ptr() + 4 * table[:, 6]
    table[:, 7] = [e.data_ptr() + 4 * int(table[s, 6]) if m.has_err[s] else 0 for s in range(lay.nseg)]
    assert all(int(p) % 16 == 0 for p in table[:, 0]) and all(int(p) % 16 == 0 for p in table[:, 7])
    cdag = _t(m.cdag)
    b = nat.PVQBatch(_t(table), _t(lay.tile_seg), lay.nseg, lay.ntiles, cdag, cdag, torch.uint8, torch.uint8, 6, u_flat=u, seg_minmax=mm)
    assert b.path != 0 and nat.pvq_batched_serves(lay.d, m.tab.K, torch.uint8)
    b.encode(wire, m.ef, nat.RANDOM_GIVEN, 0, _t(m.r_flat))
    torch.cuda.synchronize()
    _same(wire.cpu().numpy(), m.want_wire, "wire (codes; every other byte its canary)")
    got_u = u.cpu().numpy()
    for s in range(lay.nseg):
        _same(got_u[lay.slots(s)], m.want_u[s], "u_flat of tensor %d" % s)
    _same(mm.cpu().numpy().view(np.uint32), m.want_minmax, "seg_minmax")
    _same(g.cpu().numpy(), m.want_gbuf, "gradients")
    _same(e.cpu().numpy(), m.ebuf, "error buffers")


# ---- the residual compressor's second stage ---------------------------------------------------------------------------------------------
def test_residual_stage1_form(nat):
    """gq_pvq_encode(stage1): the kernel forms v - RN(cb1[code1] * norm1) itself; the draws were built on that."""
    G, T, tab = pc.residual_case()
    cb1 = _t(rc.codebooks(G.d, G.K)[0])
    at = 0
    for t in T:
        _flat(nat, tab, grad=t["v"], stage1=(_t(t["codes1"]), _t(t["norm1"]), cb1), first=at, count=t["M"])
        at += t["M"]


def test_residual_encode2_batched(nat):
    import test_gpu_rq_contract as rqt
    G, T, _ = pc.residual_case()
    rqt.check_encode(G, T, rqt.run_encode(G, T))
