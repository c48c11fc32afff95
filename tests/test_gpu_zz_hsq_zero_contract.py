"""The HSQ encode kernels on subvectors whose projection is a SIGNED zero (tests/hsq_zero_contract.py): the prefilter kernel's padded
shapes (csrc/hsq_encode_pf.hip, 12 in 16 and 24 in 32), the exact LDS kernel (csrc/hsq_encode.hip, d rounded up to 8, the running
best that starts from +0), flat and multi-tensor, plain and with error feedback, and what travels behind them: u_flat, seg_minmax,
(lb, ub), the level-form-0 section, the plain decode.  Every comparison is on the bits, against numpy and the CPU oracle; no
tolerance, no row left out.  tests/test_hsq_zero_contract.py asserts without a GPU that a chain that goes on over zero padding
(+0 where the contract says -0) changes every expectation used here on the padded shapes.

test_grid_capped_child runs the steady-state cases again with every grid capped at one compute unit's workgroups: a wave then
meets these rows in a later trip of its loop, with a ring and a second pass of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hsq_encode_contract as ec  # noqa: E402
import hsq_zero_contract as zc  # noqa: E402
import rq_contract as rc  # noqa: E402
import test_gpu_hsq_encode_contract as te  # noqa: E402  (its Rig, _same, _t, _np)

pytestmark = pytest.mark.gpu
_same, _t, _np = te._same, te._t, te._np


def _flat(native, g, cb, K, impl):
    M = g.shape[0]
    dg, dcb = _t(g.reshape(-1)), _t(cb)
    codes = torch.zeros(M, dtype=torch.int32 if K > 256 else torch.uint8, device="cuda:0")
    u = torch.full((M,), float(ec.U_FILL), dtype=torch.float32, device="cuda:0")
    ws = native.new_workspace(torch.device("cuda:0"), M)
    native.hsq_encode(dg, dcb, codes, u, ws, impl=impl)
    lb_ub = torch.zeros(2, dtype=torch.float32, device="cuda:0")
    levels = torch.zeros(M, dtype=torch.uint8, device="cuda:0")
    native.hsq_levels(u, 8, 0, None, 0, ws, lb_ub, levels)
    torch.cuda.synchronize()
    return _np(codes).astype(np.int32), _np(u), _np(lb_ub)


@pytest.mark.parametrize("shape,impl", zc.FLAT, ids=lambda x: "-".join(str(v) for v in x) if isinstance(x, tuple) else "impl%d" % x)
def test_flat_encode(shape, impl):
    """gq_hsq_encode on all tensors of the case as one, then on the tensor of only the new rows ((lb, ub) = (-0, +0)) and on the
    one of only neg_* rows ((-0, -0)): codes, u and the (min, max) gq_hsq_levels derives."""
    native = te._gpu()
    d, K, shipped = shape
    g, names, codes, u = zc.flat_case(d, K, shipped)
    cb = zc.codebook(d, K, shipped)
    first = np.cumsum((0,) + zc.MS)
    for what, rows in (("all", slice(None)), ("only new rows", slice(first[zc.ONLY_NEW], first[zc.ONLY_NEW + 1])),
                       ("only neg rows", slice(first[zc.ONLY_NEG], first[zc.ONLY_NEG + 1]))):
        got_codes, got_u, got_lbub = _flat(native, g[rows], cb, K, impl)
        bad = np.nonzero(rc.bits(got_u) != rc.bits(u[rows]))[0]
        print("%s: %d of %d projections differ%s" % (what, bad.size, got_u.size, "" if not bad.size else ", rows %s" % sorted({str(names[rows][i]) for i in bad})))
        _same(got_codes, codes[rows], what + ": codes")
        _same(got_u, u[rows], what + ": u")
        mm = rc.fold_minmax(u[rows])
        _same(got_lbub, np.array([ec.order_unmap(mm[0]), ec.order_unmap(mm[1])], np.float32), what + ": (lb, ub)")


def _rig(z, level, n_bit):
    lay = z.lay
    rig = te.Rig(lay, z.cb, z.gbuf, z.ebuf, [x is not None for x in z.errs], level, n_bit, np.full(lay.ntiles * 64, ec.U_FILL, np.float32),
                 np.tile(np.array([ec.M32, 0], np.uint32), (lay.nseg, 1)), lay.new_wire(), True)
    assert rig.b.path == z.path, "routed to %d, the case is for %d" % (rig.b.path, z.path)
    return rig


def _check_encode(c, n_bit=8):
    z = zc.zero_of(c)
    rig = _rig(z, c.level, n_bit)
    rig.b.encode(rig.wire, z.ef_scale)
    torch.cuda.synchronize()
    want, lay = z.want(), z.lay
    _same(_np(rig.wire), want["wire"], "wire (codes; every other byte its canary, the sections' padding included)")
    u = _np(rig.u)
    stated = np.zeros(u.size, bool)
    for s in range(lay.nseg):
        stated[lay.slots(s)] = True
    _same(u[stated], want["u_flat"][stated], "u_flat")
    pad = u[~stated].view(np.uint32)      # a padding slot keeps its value or becomes +0 (include/gq_hsq.h)
    assert np.isin(pad, [0, int(np.array([ec.U_FILL]).view(np.uint32)[0])]).all(), "u_flat's padding slots"
    _same(rig.minmax(), want["minmax"], "seg_minmax")
    _same(_np(rig.g), want["gbuf"], "gradients (v over the rows with an error buffer, the rest and every gap as uploaded)")
    _same(_np(rig.e), want["ebuf"], "error buffers (untouched by the encode)")
    return z, rig


@pytest.mark.parametrize("c", zc.BATCHED, ids=zc.zcase_id)
def test_batched_encode(c):
    _check_encode(c)


@pytest.mark.parametrize("c", zc.STEADY, ids=zc.zcase_id)
def test_steady_state_encode(c):
    _check_encode(c)


def _chain(c, n_bit):
    z, rig = _check_encode(c, n_bit)
    lay, want = z.lay, zc.chain_want(z, n_bit)
    rig.b.levels(rig.wire, ec.OFF, 0, None, write_error=c.ef is not None)
    torch.cuda.synchronize()
    _same(_np(rig.wire), want["wire"], "wire behind the level launch (levels, (lb, ub); level form 0: the projections)")
    _same(_np(rig.e), want["ebuf"], "error buffers behind the level launch")
    _same(_np(rig.g), z.want()["gbuf"], "gradients behind the level launch")
    out = torch.full((lay.floats,), float(ec.FILL), dtype=torch.float32, device="cuda:0")
    rig.b.decode(rig.wire[:lay.P].view(1, lay.P), 1, out, plain=True)
    torch.cuda.synchronize()
    _same(_np(out), want["out"], "out (the plain decode: a -0 stays -0)")
    _same(_np(rig.wire), want["wire"], "wire behind the decode")


@pytest.mark.parametrize("c,n_bit", zc.CHAINS, ids=lambda x: zc.zcase_id(x) if isinstance(x, tuple) else "n%d" % x)
def test_chain(c, n_bit):
    """encode -> gq_hsq_levels_batched (level form 0 at n_bit 32, byte levels at 8) -> the plain R = 1 decode."""
    _chain(c, n_bit)


def test_steady_state_chain():
    _chain(zc.ZCase(24, 256, True, 0, 0), 32)


def test_pvq_selected_projection(oracle):
    """csrc/pvq.hip recomputes the selected codeword's projection over the d real elements: the same rows against oracle.pvq_encode
    at (12, 100), a shape its LDS kernel pads to 16."""
    native = te._gpu()
    cd, g, names, r = zc.pvq_case()
    M = g.shape[0]
    codes = torch.zeros(M, dtype=torch.uint8, device="cuda:0")
    u = torch.full((M,), float(ec.U_FILL), dtype=torch.float32, device="cuda:0")
    ws = native.new_workspace(torch.device("cuda:0"), M)
    native.pvq_encode(_t(g.reshape(-1)), _t(cd), codes, u, ws, native.RANDOM_GIVEN, _t(r), 0)
    torch.cuda.synchronize()
    want_codes, want_u = oracle.pvq_encode(g.reshape(-1), cd, r)
    _same(_np(codes).astype(np.int32), want_codes.astype(np.int32), "codes")
    _same(_np(u), rc.f32(want_u), "u", nan_equal=True)


def test_quantizer(oracle):
    """NearestNeighborCompressor c_dim 24 / k_bit 8 / n_bit 32 through PSQuantizer -- the shipped d24 codebook, the projections on
    the wire as float32 -- on a gradient that holds the neg_mid rows, against tests/oracle_codec.py's CPU codec: the wire and the
    aggregate, every step."""
    te._gpu()
    want, got = zc.quantizer_run(False), zc.quantizer_run(True)
    for st in range(len(want["wire"])):
        for t in range(len(zc.Q_SHAPES)):
            _same(got["codes"][st][t], want["codes"][st][t], "step %d, tensor %d: codes" % (st, t))
            _same(got["norms"][st][t], want["norms"][st][t], "step %d, tensor %d: u on the wire" % (st, t))
        _same(got["wire"][st], want["wire"][st], "step %d: the wire" % st)
        for t in range(len(zc.Q_SHAPES)):
            _same(got["grads"][st][t], want["grads"][st][t], "step %d, tensor %d: the aggregate" % (st, t))


def test_grid_capped_child():
    """The steady-state cases with every grid capped at one compute unit's workgroups."""
    te._gpu()
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__, "-k", "steady_state"],
                       env=dict(os.environ, GQ_CU_COUNT="1"), capture_output=True, text=True, timeout=300)
    tail = r.stdout[-2000:] + r.stderr[-2000:]
    assert r.returncode == 0 and " passed" in r.stdout and " skipped" not in r.stdout, tail
    print(r.stdout.strip().splitlines()[-1])
