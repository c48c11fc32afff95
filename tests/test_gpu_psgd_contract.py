"""libgq_psgd.so on the MI355X against the numpy restatement of include/gq_psgd.h (tests/psgd_contract.py), at tolerance 0: the wire,
the warm start, the residual and the dense decode after each of three consecutive records, canaries round every section and every
buffer, garbage in the scratch before every compress.  Equality is the header's: bit for bit, any NaN equal to any NaN
(psgd_contract.same); on inputs without non-finite values that is np.array_equal of the bits."""
import ctypes
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import psgd_contract as pc  # noqa: E402
from psgd_cases import CASES, CASE_IDS, mats as _mats  # noqa: E402

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
CANARY = 0xA5
FCANARY = f32(-7.25)
SEED = 77


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available()
    yield


def _guarded(arrays, lead=0):
    """The arrays back to back in ONE device buffer, a canary float in front of, between and behind them; lead: floats in front of
    the first canary (4-byte but not 16-byte aligned views).  -> (buffer, views)"""
    total = lead + 1 + sum(a.size + 1 for a in arrays)
    host = np.full(total, FCANARY, f32)
    spans, at = [], lead + 1
    for a in arrays:
        host[at:at + a.size] = a.reshape(-1)
        spans.append((at, a.size))
        at += a.size + 1
    buf = torch.from_numpy(host).cuda()
    return buf, [buf[o:o + k] for o, k in spans], spans


def _canaries_ok(buf, spans, lead=0):
    host = buf.cpu().numpy()
    keep = np.ones(host.size, bool)
    for o, k in spans:
        keep[o:o + k] = False
    keep[:lead] = False
    return bool(np.all(host[keep] == FCANARY))


class Group(object):
    """A BatchedPowerSGD over `shapes` at rank r with canaries between the wire sections; per user: warm starts in a guarded buffer."""

    def __init__(self, shapes, r, users=1, lead=0, seed=SEED):
        from gq_amd.codecs import BatchedPowerSGD, PowerSGDCodec
        from gq_amd.compressors import PowerSGDCompressor
        self.shapes, self.r, self.lead, self.seed = shapes, r, lead, seed
        args = Namespace(psgd_rank=r, psgd_seed=seed)
        self.nm = [pc.matrix_of(s) for s in shapes]
        self.codecs = [PowerSGDCodec(PowerSGDCompressor(int(np.prod(s)), s, args), int(np.prod(s)), s, param_index=i) for i, s in enumerate(shapes)]
        self.offsets, off = [], 16
        for cd in self.codecs:
            assert cd.nbytes == pc.section_nbytes(cd.n, cd.m, r)
            self.offsets.append(off)
            off += cd.nbytes + 16
        self.user_bytes = off
        dev = torch.device("cuda", torch.cuda.current_device())
        self.grp = BatchedPowerSGD(self.codecs, self.offsets, list(range(len(shapes))), dev, 1, self.user_bytes)
        self.wire = torch.full((self.user_bytes,), CANARY, dtype=torch.uint8, device=dev)
        self.q0 = [[pc.q0(seed, i, u, m, r) for i, (n, m) in enumerate(self.nm)] for u in range(users)]
        self.qnp = [[q.copy() for q in qs] for qs in self.q0]
        self.qbuf = [_guarded(qs, lead) for qs in self.q0]
        self.enp = [np.zeros(s, f32).reshape(nm) for s, nm in zip(shapes, self.nm)]
        self.ebuf = None
        self.outbuf = torch.full((self.grp.out_floats + 4 + lead,), float(FCANARY), dtype=torch.float32, device=dev)

    def set_state(self, user, qs=None, es=None):
        if qs is not None:
            self.qnp[user] = [np.array(q, f32) for q in qs]
            for v, q in zip(self.qbuf[user][1], qs):
                v.copy_(torch.from_numpy(np.ascontiguousarray(q, f32).reshape(-1)))
        if es is not None:
            self.enp = [np.array(e, f32).reshape(nm) for e, nm in zip(es, self.nm)]

    def scratch_garbage(self):
        for t, v in ((self.grp._pwork, float("nan")), (self.grp._cpart, 3e38)):
            t.fill_(v)
        self.grp._flags.fill_(-1)

    def record(self, mats, user=0, ef=None, want_out=True, launch=True):
        """One record on the device and in numpy; asserts everything.  mats: [n, m] float32 per tensor."""
        r = self.r
        gbuf, gviews, gspans = _guarded(mats, self.lead)
        errs = None
        if ef is not None:
            self.ebuf = _guarded(self.enp, self.lead)
            errs = self.ebuf[1]
        out = self.outbuf[self.lead:self.lead + self.grp.out_floats] if want_out else None
        self.outbuf.fill_(float(FCANARY))
        self.wire.fill_(CANARY)
        self.scratch_garbage()
        if launch:
            assert self.grp.encode(gviews, self.wire, 0, 0, (errs, self.qbuf[user][1], user), ef, out=out)
            torch.cuda.synchronize()
        self.check(mats, user, ef, want_out, gbuf, gspans)
        return gviews, errs, out

    def check(self, mats, user, ef, want_out, gbuf=None, gspans=None):
        r = self.r
        wire = self.wire.cpu().numpy()
        covered = np.zeros(wire.size, bool)
        outh = self.outbuf.cpu().numpy()
        out_cov = np.zeros(outh.size, bool)
        out_cov[:self.lead] = False
        for i, (M, (n, m)) in enumerate(zip(mats, self.nm)):
            rec = pc.record(M, self.qnp[user][i], self.q0[user][i], self.enp[i] if ef is not None else None, ef)
            o = self.offsets[i]
            got = wire[o:o + rec.section.size]
            covered[o:o + rec.section.size] = True
            assert pc.same_section(got, rec.section, n, m, r), "tensor %d %r: the wire section" % (i, self.shapes[i])
            self.qnp[user][i] = rec.Q
            assert pc.same(self.qbuf[user][1][i].cpu().numpy(), rec.Q), "tensor %d %r: the warm start" % (i, self.shapes[i])
            if ef is not None:
                self.enp[i] = rec.e
                assert pc.same(self.ebuf[1][i].cpu().numpy(), rec.e), "tensor %d %r: the residual" % (i, self.shapes[i])
            if want_out:
                a = self.lead + self.grp.out_off[i]
                out_cov[a:a + n * m] = True
                assert pc.same(outh[a:a + n * m], rec.D), "tensor %d %r: the dense decode" % (i, self.shapes[i])
        assert np.all(wire[~covered] == CANARY), "a byte outside the sections was written"
        assert np.all(outh[~out_cov] == FCANARY), "a float outside the decoded tensors was written"
        assert _canaries_ok(self.qbuf[user][0], self.qbuf[user][2], self.lead)
        if ef is not None:
            assert _canaries_ok(self.ebuf[0], self.ebuf[2], self.lead)
        if gbuf is not None:      # the gradients are read only
            host = gbuf.cpu().numpy()
            assert _canaries_ok(gbuf, gspans, self.lead) and all(np.array_equal(host[o:o + k].view(u32), M.reshape(-1).view(u32))
                                                                 for (o, k), M in zip(gspans, mats))


@pytest.mark.parametrize("shape,r", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("ef", [None, 0.75], ids=["plain", "ef"])
def test_three_records(shape, r, ef):
    """Every path: rows shorter than a wave, a multiple of it, across two and three pieces, many rows per item, a row count off
    every block size, n or m equal to r; plain without the dense decode on the first record (no residual launch at all)."""
    g = Group([shape], r)
    for step in range(3):
        g.record(_mats([shape], 100 + step), ef=ef, want_out=not (ef is None and step == 0))


def test_seventy_tensors_in_one_group():
    """Items and tiles of many tensors in one grid (more tensors than a workgroup has waves per CU, items of neighbouring tensors
    in one wave's worth of workgroups), sizes from the CU count so that the count changes the layout."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = [(3 + (i * 7 + cus) % 9, 40 + (i * 13 + cus) % 61) if i % 3 else (40 + (i * 11 + cus) % 90, 4 + i % 5) for i in range(70)]
    g = Group(shapes, 2)
    for step in range(3):
        g.record(_mats(shapes, 200 + step), ef=0.5)


def test_views_at_4_byte_alignment():
    """Gradients, residuals, warm starts and the dense decode one float off 16-byte alignment."""
    shapes = [(33, 31), (20, 260), (5, 4097)]
    g = Group(shapes, 4, lead=1)
    for step in range(3):
        views, errs, out = g.record(_mats(shapes, 300 + step), ef=1.0)
        assert views[0].data_ptr() % 16 == 8 and out.data_ptr() % 16 == 4      # (a canary in front, and the lead)


def test_non_finite_and_tiny_values():
    """+-0, subnormals, +-inf and NaN in the gradient, in e and in the warm start, each on its own and all together."""
    shapes = [(33, 31), (70, 300)]
    for where in ("gradient", "residual", "warm start", "all"):
        g = Group(shapes, 2)
        mats = _mats(shapes, 400)
        tiny = [(m * f32(1e-39)).astype(f32) for m in mats]      # subnormal throughout
        g.record(tiny, ef=1.0)
        if where in ("gradient", "all"):
            mats = [pc.specials(m, 41 + i) for i, m in enumerate(mats)]
        if where in ("residual", "all"):
            g.set_state(0, es=[pc.specials(e, 51 + i) for i, e in enumerate(g.enp)])
        if where in ("warm start", "all"):
            g.set_state(0, qs=[pc.specials(q, 61 + i) for i, q in enumerate(g.qnp[0])])
        for step in range(3):
            g.record(mats, ef=1.0)


def test_linearly_dependent_columns():
    """M of rank one with small integers: P's columns are exact multiples of one another, Gram-Schmidt leaves a column of zeros or
    of rounding dust -- the flags and the bytes are the contract's either way -- and the record after it."""
    rs = np.random.RandomState(5)
    u, v = rs.randint(-3, 4, (40, 1)).astype(f32), rs.randint(-3, 4, (1, 50)).astype(f32)
    M = (u @ v).astype(f32)
    for r in (2, 4):
        g = Group([(40, 50)], r)
        q = np.round(g.qnp[0][0] * 8).astype(f32)      # small integers too: P = M Q is exact
        g.set_state(0, qs=[q])
        g.record([M])
        g.record([M])
        g.record(_mats([(40, 50)], 6))


def test_zero_gradient_and_the_reset():
    shapes = [(33, 31), (5, 4097)]
    g = Group(shapes, 2)
    g.record(_mats(shapes, 7), ef=1.0)
    g.set_state(0, es=[np.zeros_like(e) for e in g.enp])
    g.record([np.zeros(pc.matrix_of(s), f32) for s in shapes], ef=1.0)
    for i in range(len(shapes)):
        assert np.array_equal(g.qnp[0][i], g.q0[0][i])      # (the contract: every column went back to Q0)
    g.record(_mats(shapes, 8), ef=1.0)
    assert all(np.any(pc.parse(g.wire.cpu().numpy()[o:], n, m, 2)[1] != 0) for o, (n, m) in zip(g.offsets, g.nm))


def test_two_user_slots_in_turn():
    shapes = [(33, 31), (20, 260)]
    g = Group(shapes, 2, users=2)
    for step in range(3):
        for user in (0, 1):
            g.record(_mats(shapes, 500 + 2 * step + user), user=user)
    assert not np.array_equal(g.qnp[0][0], g.qnp[1][0])


@pytest.mark.parametrize("r", [1, 2, 4])
def test_decode_mean_of_hand_built_payloads(r):
    """R = 1 ... 16 payloads of arbitrary factors (not orthonormal, signed zeros among them), rows at a stride beyond their bytes."""
    shapes = [(33, 31), (70, 300), (5, 4097), (130, 4)]
    shapes = [s for s in shapes if min(s) >= r]
    g = Group(shapes, r)
    rs = np.random.RandomState(9 + r)
    Rmax = 16
    rows = np.full((Rmax, g.user_bytes + 32), CANARY, np.uint8)
    for rho in range(Rmax):
        for o, (n, m) in zip(g.offsets, g.nm):
            Ph, Qn = rs.standard_normal((n, r)).astype(f32), rs.standard_normal((m, r)).astype(f32)
            Ph[rs.rand(n, r) < 0.1] = f32(-0.0)
            sec = pc.section(Ph, Qn)
            rows[rho, o:o + sec.size] = sec
    dev_rows = torch.from_numpy(rows).cuda()
    for R in range(1, Rmax + 1):
        out = torch.full((g.grp.out_floats + 4,), float(FCANARY), dtype=torch.float32, device="cuda")
        g.grp.decode_into(dev_rows[:R, :g.user_bytes], R, out[:g.grp.out_floats])
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        cov = np.zeros(host.size, bool)
        for i, (o, (n, m)) in enumerate(zip(g.offsets, g.nm)):
            want = pc.decode_mean([rows[rho, o:] for rho in range(R)], n, m, r)
            a = g.grp.out_off[i]
            cov[a:a + n * m] = True
            assert np.array_equal(host[a:a + n * m].view(u32), want.reshape(-1).view(u32)), "R = %d, tensor %d" % (R, i)
        assert np.all(host[~cov] == FCANARY)


def test_graphs_replayed_three_times_equal_the_eager_bytes():
    """The record, the apply and the whole step captured once and replayed three times: the contract's bytes after each replay
    (the warm start and the residual step with every replay, so each replay is checked against its own record)."""
    shapes = [(33, 31), (70, 300), (5, 4097)]
    mats = _mats(shapes, 600)
    for kind in ("record", "apply", "step"):
        g = Group(shapes, 4)
        gviews, errs, out = g.record(mats, ef=0.75)      # eager: tables uploaded, the state table built
        dec = torch.empty(g.grp.out_floats, dtype=torch.float32, device="cuda")
        rows = g.wire.view(1, -1)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            if kind in ("record", "step"):
                assert g.grp.encode(gviews, g.wire, 0, 0, (errs, g.qbuf[0][1], 0), 0.75, out=out, table_current=True)
            if kind in ("apply", "step"):
                g.grp.decode_into(rows, 1, dec)
        for rep in range(3):
            if kind == "apply":
                g.grp.encode(gviews, g.wire, 0, 0, (errs, g.qbuf[0][1], 0), 0.75, out=out)
            graph.replay()
            torch.cuda.synchronize()
            # (the residual buffer is stepped in place: the numpy side follows it; canaries and the gradients as ever)
            g.check(mats, 0, 0.75, True)
            if kind != "record":
                host, wire = dec.cpu().numpy(), g.wire.cpu().numpy()
                for i, (o, (n, m)) in enumerate(zip(g.offsets, g.nm)):
                    a = g.grp.out_off[i]
                    assert pc.same(host[a:a + n * m], pc.decode_mean([wire[o:]], n, m, 4))


def test_refusals():
    from gq_amd import native
    from gq_amd.codecs import PowerSGDCodec
    from gq_amd.compressors import PowerSGDCompressor
    for bad in (0, 3, 8, True, "2"):
        with pytest.raises(ValueError, match="psgd_rank"):
            PowerSGDCompressor(2000, (40, 50), Namespace(psgd_rank=bad))
    with pytest.raises(ValueError, match="psgd_seed"):
        PowerSGDCompressor(2000, (40, 50), Namespace(psgd_rank=2, psgd_seed=-1))
    c = PowerSGDCompressor(2000, (40, 50), Namespace(psgd_rank=2, psgd_seed=1))
    with pytest.raises(TypeError, match="float32"):
        c.compress(torch.zeros(40, 50))
    with pytest.raises(TypeError, match="float32"):
        c.compress(torch.zeros(40, 50, device="cuda", dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="no matrix"):
        PowerSGDCodec(PowerSGDCompressor(2048, (2048,), Namespace(psgd_rank=2)), 2048, (2048,))
    with pytest.raises(ValueError, match="no matrix"):
        PowerSGDCodec(PowerSGDCompressor(1100, (1, 1100), Namespace(psgd_rank=2)), 1100, (1, 1100))
    g = Group([(33, 31), (20, 260)], 2)
    mats = _mats(g.shapes, 1)
    _, views, _ = _guarded(mats)
    with pytest.raises(ValueError, match="warm starts"):
        g.grp.encode(views, g.wire, 0, 0, None, None)
    short = [q[:-1] for q in g.qbuf[0][1]]
    assert g.grp.encode(views, g.wire, 0, 0, (None, short, 0), None) is False            # a warm start of another size
    assert g.grp.encode(views, g.wire, 0, 0, (None, g.qbuf[0][1], 4096), None) is False    # a user beyond the key
    assert g.grp.encode([v.double() for v in views], g.wire, 0, 0, (None, g.qbuf[0][1], 0), None) is False
    b = g.grp._batch
    with pytest.raises(native.GQNativeError, match="state table"):      # no record before: no state table in the descriptor
        native.PSGDBatch(g.grp._dev[:g.grp._table_words], g.grp.item_seg, 2, g.grp._nitems, rank=2, lay=g.grp._lay,
                         aitem_seg=g.grp._aitem_seg, naitems=int(g.grp._aitem_seg.numel()), pwork=g.grp._pwork, cpart=g.grp._cpart,
                         flags=g.grp._flags).compress(g.wire)
    with pytest.raises(native.GQNativeError, match="rank 3"):
        native.PSGDBatch(g.grp._dev[:g.grp._table_words], g.grp.item_seg, 2, g.grp._nitems, rank=3).decode(g.wire.view(1, -1), 1, g.outbuf)
    g.record(mats)
    with pytest.raises(native.GQNativeError, match="4-byte aligned"):
        b.compress(g.wire[1:])
    rc = b._decode(b.ref, native._dev_ptr(g.wire), ctypes.c_int64(0), ctypes.c_int(0), native._dev_ptr(g.outbuf), ctypes.c_int(0),
                   native._stream())
    with pytest.raises(native.GQNativeError, match="R = 0"):
        native._check(rc, "gq_psgd_decode_sum_batched", native.PSGD_LIBRARY)
