"""The multi-tensor kernels of libgq_hsq.so whose de-quantiser is level_to_norm's `* 2^-n_bit` where it used to be the
division by 2^n_bit -- hsq_decode_sum_batched_kernel (the decode-mean of a wire that is not 4-byte aligned),
hsq_levels_ef_batched_kernel (packed 6-bit levels with error feedback) and hsq_levels_ef_tile_kernel (byte levels with error
feedback, a wave per tile) -- against tests/hsq_dequant_contract.py (numpy float32,
one operation at a time; nothing from another kernel), at tolerance 0, through native.HSQBatch with hand-built tables.
d = 16, K = 256, two tensors of 67 and 1 subvectors: a whole tile, a 3-subvector tail and a lone subvector."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hsq_dequant_contract as hc  # noqa: E402
import rq_contract as rc  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY, OUT_FILL, GAP = 0xA5, 7.0, 8
OFF, GIVEN = 0, 1


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from gq_amd import native
    return native


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _cb():
    return rc.codebooks(hc.D, hc.K)[0]


def _layout(level_section_bytes, lbub_mod4):
    """One payload's sections for the tensors hc.MS -> (seg_table rows' wire / out columns, payload bytes, out floats): codes |
    levels | (lb, ub) per tensor with 16 canary bytes between sections; the (lb, ub) offsets are lbub_mod4 modulo 4 (so that they
    are float-aligned in a payload that starts lbub_mod4 bytes short of a 4-byte boundary); every tensor's span of `out` has GAP
    floats that belong to nobody round it."""
    rows, off, tile, out = [], 16, 0, GAP
    for M in hc.MS:
        codes = off
        off = (off + M + 16 + 15) // 16 * 16
        levels = off
        off = (off + level_section_bytes(M) + 16 + 15) // 16 * 16
        lbub = off + lbub_mod4
        off += 32
        rows.append([0, M, tile, codes, levels, lbub, out, 0])
        tile += (M + 63) // 64
        out = (out + M * hc.D + GAP + 3) // 4 * 4
    return np.array(rows, np.int64), (off + 15) // 16 * 16, out, tile


def _tile_seg():
    return np.concatenate([np.full((M + 63) // 64, s, np.int32) for s, M in enumerate(hc.MS)])


# ---- the decode-mean of a wire one byte off a 4-byte boundary ---------------------------------------------------------------------
@pytest.mark.parametrize("regime", sorted(hc.REGIMES))
@pytest.mark.parametrize("n_bit", [6, 8])
@pytest.mark.parametrize("R", [1, 3])
def test_misaligned_wire_decode(R, n_bit, regime):
    native = _gpu()
    cb = _cb()
    lb, ub = hc.REGIMES[regime]
    table, P, out_floats, ntiles = _layout(lambda M: M, lbub_mod4=3)      # payload r starts at 1 (mod 4): 1 + 3 = a float's place
    levels = hc.levels_of_launch(n_bit, R, hc.level_start(regime))
    rs = np.random.RandomState(17 * n_bit + R)
    buf = np.full(1 + R * P + 16, CANARY, np.uint8)
    want = np.full(out_floats, OUT_FILL, np.float32)
    payloads = [[] for _ in hc.MS]
    for r in range(R):
        base = 1 + r * P
        for s, M in enumerate(hc.MS):
            codes = rs.randint(0, hc.K, size=M).astype(np.uint8)
            lbr, ubr = (lb, ub) if r != 1 else (np.float32(lb * np.float32(0.5)), ub)      # payloads of one tensor differ in lb
            if regime == "flat":
                lbr = ubr
            buf[base + table[s, 3]: base + table[s, 3] + M] = codes
            buf[base + table[s, 4]: base + table[s, 4] + M] = levels[r][s]
            buf[base + table[s, 5]: base + table[s, 5] + 8] = np.array([lbr, ubr], np.float32).view(np.uint8)
            payloads[s].append((codes, levels[r][s], (lbr, ubr)))
    for s, M in enumerate(hc.MS):
        want[table[s, 6]: table[s, 6] + M * hc.D] = hc.decode_mean(payloads[s], cb, n_bit, plain=(R == 1)).reshape(-1)
    dbuf = _t(buf)
    gathered = torch.as_strided(dbuf, (R, P), (P, 1), 1)
    assert gathered.data_ptr() % 4 == 1
    out = torch.full((out_floats,), OUT_FILL, dtype=torch.float32, device="cuda:0")
    b = native.HSQBatch(_t(table), _t(_tile_seg()), len(hc.MS), ntiles, _t(cb), torch.uint8, torch.uint8, n_bit)
    b.decode(gathered, R, out, plain=(R == 1))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))      # every span bit for bit, every float round them untouched
    assert np.array_equal(dbuf.cpu().numpy(), buf)


# ---- levels with error feedback: packed 6-bit (one thread per quarter) and bytes (a wave per tile) -------------------------------
@pytest.mark.parametrize("regime", sorted(hc.REGIMES))
@pytest.mark.parametrize("n_bit,mode", [(6, OFF), (5, GIVEN)])
@pytest.mark.parametrize("packed,err_on", [(True, 0), (True, 1), (False, 0), (False, 1)])
def test_error_feedback_levels(packed, err_on, n_bit, mode, regime):
    """err_on: the tensor that has an error buffer; the other has none (err_on = 1: the 67-subvector tensor, whose levels are not
    all 0, goes without)."""
    native = _gpu()
    cb = _cb()
    lb, ub = hc.REGIMES[regime]
    table, P, _, ntiles = _layout((lambda M: 3 * ((M + 3) // 4)) if packed else (lambda M: M), lbub_mod4=0)
    rs = np.random.RandomState(5 * n_bit + mode)
    wire = np.full(P, CANARY, np.uint8)
    u_flat = np.zeros(ntiles * 64, np.float32)
    r_flat = rs.rand(ntiles * 64).astype(np.float32)
    minmax = np.zeros(2 * len(hc.MS), np.uint32)
    grads, errs, want_err = [], [], []
    want = wire.copy()
    for s, M in enumerate(hc.MS):
        t0 = int(table[s, 2]) * 64
        u = hc.projections(M, lb, ub, n_bit, seed=s + 3)
        u_flat[t0:t0 + M] = u
        minmax[2 * s:2 * s + 2] = rc.order_map(np.array([u.min(), u.max()], np.float32))
        tlb, tub = np.float32(u.min()), np.float32(u.max())
        codes = rs.randint(0, hc.K, size=M).astype(np.uint8)
        wire[table[s, 3]: table[s, 3] + M] = codes
        want[table[s, 3]: table[s, 3] + M] = codes
        l = hc.quantise(u, tlb, tub, n_bit, r_flat[t0:t0 + M] if mode == GIVEN else None)
        section = hc.pack6(l) if packed else l.astype(np.uint8)
        want[table[s, 4]: table[s, 4] + len(section)] = section
        want[table[s, 5]: table[s, 5] + 8] = np.array([tlb, tub], np.float32).view(np.uint8)
        scale = np.float32(max(abs(float(tlb)), abs(float(tub)), 1e-30))
        v = rc.f32(rs.randn(M, hc.D)) * scale
        grads.append(_t(np.concatenate([np.full(GAP, OUT_FILL, np.float32), v.reshape(-1)])))
        table[s, 0] = grads[-1].data_ptr() + 4 * GAP
        if s == err_on:
            errs.append(torch.full((GAP + M * hc.D + GAP,), OUT_FILL, dtype=torch.float32, device="cuda:0"))
            table[s, 7] = errs[-1].data_ptr() + 4 * GAP
            with np.errstate(all="ignore"):
                e = v - rc.stage_decode(codes, rc.level_norm(l.astype(np.uint8), 1, n_bit, tlb, tub), cb)
            want_err.append(np.concatenate([np.full(GAP, OUT_FILL, np.float32), e.reshape(-1), np.full(GAP, OUT_FILL, np.float32)]))
    dwire = _t(wire)
    b = native.HSQBatch(_t(table), _t(_tile_seg()), len(hc.MS), ntiles, _t(cb), torch.uint8, native.PACKED6 if packed else torch.uint8, n_bit,
                        u_flat=_t(u_flat), seg_minmax=_t(minmax.view(np.int32)))
    b.levels(dwire, mode, 0, r_flat=_t(r_flat) if mode == GIVEN else None, write_error=True)
    torch.cuda.synchronize()
    assert np.array_equal(dwire.cpu().numpy(), want)      # levels, (lb, ub), the codes as they were, every canary byte
    assert np.array_equal(errs[0].cpu().numpy().view(np.uint32), want_err[0].view(np.uint32))
