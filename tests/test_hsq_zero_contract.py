"""What tests/hsq_zero_contract.py claims, checked without a GPU: every neg_* row's projection is -0 under the contract (the chain
over the d real elements) and +0 under the zero-padded restatement -- the mutation tests/test_gpu_zz_hsq_zero_contract.py must
catch --, every pos_* row's is +0, every such row's code is 0, and the difference travels: u_flat, the seg_minmax words, the
(lb, ub) bytes, the level-form-0 section and the plain decode's zeros.  Conditions, not measurements: no row is left out."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hsq_encode_contract as ec  # noqa: E402
import hsq_zero_contract as zc  # noqa: E402
import rq_contract as rc  # noqa: E402

SHAPES = sorted({s for s, _ in zc.FLAT})
PADDED = [s for s in SHAPES if zc.pad_to(s[0], ec.batch_path(s[0], s[1], 1 if s[1] <= 256 else 4, len(zc.MS))) != s[0]]
CASES = sorted(set(zc.BATCHED + [c for c, _ in zc.CHAINS] + zc.STEADY), key=zc.zcase_id)


def test_the_lists_hold_what_the_gpu_file_promises():
    flat = {(s[0], s[1], impl) for s, impl in zc.FLAT}
    assert {(12, 256, 0), (12, 32, 0), (24, 256, 0), (24, 64, 0)} <= flat                                  # the prefilter, DR < D
    assert {(5, 5, 0), (3, 32, 0), (10, 33, 0), (33, 300, 0), (100, 512, 0), (12, 101, 0), (16, 250, 0)} <= flat      # the exact LDS kernel
    assert {(12, 256, 5), (12, 32, 5), (24, 256, 5), (24, 64, 5)} <= flat                                  # ... forced on the prefilter shapes
    assert {(8, 256, 0), (16, 256, 0), (32, 256, 0)} <= flat                                               # controls without padding
    assert all(sh for (d, K, sh), _ in zc.FLAT if d == 24) and set(PADDED) == {s for s in SHAPES if s[0] not in (8, 16, 32)}
    b = {(c.d, c.K, c.ef is not None) for c in zc.BATCHED}
    assert b == {(d, K, ef) for d, K in ((12, 256), (24, 256), (12, 101), (5, 5), (33, 300)) for ef in (False, True)}
    assert {(c.d, c.level, nb) for c, nb in zc.CHAINS} >= {(d, lv, nb) for d in (12, 24) for lv, nb in ((0, 32), (1, 8))}
    assert {ec.batch_path(c.d, c.K, 1 if c.K <= 256 else 4, len(zc.MS)) for c in zc.STEADY} == {ec.PREFILTER, ec.EXACT}
    assert zc.MS[:4] == ec.TABLES["small"] and zc.MS[4] == 5 * 64
    assert {(12, 101, 2), (5, 5, 2), (130, 8, 0)} <= flat                  # the generic kernel: forced, and the dispatcher's choice at d > 128
    assert {(16, 256, 1), (12, 256, 3), (16, 256, 3), (24, 256, 3)} <= flat           # the d16 MFMA kernel and the VALU cross-check


@pytest.mark.parametrize("d,K,shipped", SHAPES)
def test_codebooks_and_rows(d, K, shipped):
    cb, cat = zc.codebook(d, K, shipped), zc.catalog(d, K, shipped)
    names = [n for n, _ in cat]
    if shipped:
        assert np.array_equal(cb, np.load(os.path.join(rc.GOLDEN, zc.SHIPPED[(d, K)])))
        small = zc.small_columns(cb)
        assert (d, K) != (24, 256) or small == [15, 17]
        assert (d, K) != (24, 64) or len(small) == 12
    else:
        j1, j2, j3 = ec.ties(K)                        # ec's exact ties survive the scaling
        assert np.array_equal(cb[j1], cb[j2]) and np.array_equal(cb[j3], -cb[j1])
        assert "neg_last" in names and "pos_last" in names and "neg_last2" in names
        assert d < 3 or any(n.startswith("neg_mid") for n in names)
    assert any(zc.is_neg(n) for n in names) and any(not zc.is_neg(n) for n in names)
    for n, row in cat:
        j = np.nonzero(row)[0]
        assert j.size == 1 and np.abs(cb[:, j[0]]).max() < (0.25 if n == "neg_last2" else 0.5)
        assert abs(row[j[0]]) == (2 if n == "neg_last2" else 1) * zc.TINY
        assert (j[0] == d - 1) == ("last" in n)
        prod0 = np.float64(cb[0, j[0]]) * np.float64(row[j[0]])
        assert (prod0 < 0) == zc.is_neg(n)
        behind = slice(j[0] + 1, None)                 # zeros whose products with row 0 are -0
        assert np.array_equal(np.signbit(row[behind]), ~np.signbit(cb[0][behind]))


@pytest.mark.parametrize("d,K,shipped", SHAPES)
def test_every_row_is_what_its_name_says_and_the_padded_chain_is_not(oracle, d, K, shipped):
    g, names, codes, u = zc.flat_case(d, K, shipped)
    z = zc.zero_of(zc.ZCase(d, K, shipped, None, 1))
    pad = np.concatenate([uu for _, uu in z.encode(padded=True)])
    pcodes = np.concatenate([cc for cc, _ in z.encode(padded=True)])
    assert np.array_equal(codes, pcodes)               # codes are decided on |p|: the padding cannot move them
    ub, pb = rc.bits(u), rc.bits(pad)
    nneg = 0
    for r, n in enumerate(names):
        if n is None:
            assert ub[r] == pb[r] and u[r] != 0
            continue
        assert codes[r] == 0, (r, n)
        assert ub[r] == (zc.NEG0 if zc.is_neg(n) else zc.POS0), (r, n, hex(ub[r]))
        if (d, K, shipped) in PADDED:
            assert pb[r] == zc.POS0, (r, n)            # the mutation: every neg_* row comes out +0
        nneg += zc.is_neg(n)
    assert nneg >= 40 and len(names) == sum(zc.MS)


@pytest.mark.parametrize("c", CASES, ids=zc.zcase_id)
def test_error_feedback_reaches_the_same_rows(c):
    z, plain = zc.zero_of(c), zc.zero_of(c._replace(ef=None))
    for s in range(len(zc.MS)):
        rows, _ = z.special(s)
        assert rc.same(z.v[s][rows], plain.v[s][rows]) and np.array_equal(rc.bits(z.v[s][rows]), rc.bits(plain.v[s][rows]))
        assert (z.errs[s] is None) == (c.ef is None or s % 3 == 1)
        if z.errs[s] is not None:
            assert np.array_equal(rc.bits(ec.ef_add(z.grads[s], z.errs[s], z.ef_scale)), rc.bits(z.v[s]))
            odd = rows[rows % 2 == 1]
            assert odd.size == 0 or (z.errs[s][odd] != 0).any(axis=1).all()      # there the subnormal comes from the error buffer


@pytest.mark.parametrize("c", [c for c in CASES if c.ef is None], ids=zc.zcase_id)
def test_the_difference_travels(oracle, c):
    z = zc.zero_of(c)
    a, b = z.want(False), z.want(True)
    padded = zc.pad_to(c.d, z.path) != c.d
    for s, want in ((zc.ONLY_NEW, (zc.NEG0, zc.POS0)), (zc.ONLY_NEG, (zc.NEG0, zc.NEG0))):
        lb, ub = ec.order_unmap(a["minmax"][s, 0]), ec.order_unmap(a["minmax"][s, 1])
        assert (int(rc.bits(lb).reshape(-1)[0]), int(rc.bits(ub).reshape(-1)[0])) == want
        if padded:
            assert not np.array_equal(a["minmax"][s], b["minmax"][s])
            assert np.array_equal(b["minmax"][s], rc.fold_minmax(np.zeros(1, np.float32)))
    assert np.array_equal(a["wire"], b["wire"])        # the codes
    if not padded:
        assert np.array_equal(rc.bits(a["u_flat"]), rc.bits(b["u_flat"]))
        return
    assert not np.array_equal(rc.bits(a["u_flat"]), rc.bits(b["u_flat"]))
    for level, n_bit in ((0, 32), (1, 8)):
        zl = zc.zero_of(c._replace(level=level))
        ca, cb_ = zc.chain_want(zl, n_bit, False), zc.chain_want(zl, n_bit, True)
        for s in (zc.ONLY_NEW, zc.ONLY_NEG):
            name = "levels" if level == 0 else "lbub"
            off, n = zl.lay.sections[(s, name)]
            assert not np.array_equal(ca["wire"][off:off + n], cb_["wire"][off:off + n]), (level, s, name)
        if level == 0:                                 # the plain decode: codeword * (-0) flips the sign of every zero it writes
            sp = zl.lay.span(zc.ONLY_NEG)
            assert not np.array_equal(rc.bits(ca["out"][sp]), rc.bits(cb_["out"][sp]))
            assert (ca["out"][sp] == 0).all() and (cb_["out"][sp] == 0).all()


def test_pvq_rows(oracle):
    cd, g, names, r = zc.pvq_case()
    assert np.abs(cd[:, [5, 11]]).max() < 0.5 and sum(n is not None for n in names) >= 60
    assert {n.split("@")[0] for n in names if n} == {"neg", "pos"} and {n.split("@")[1] for n in names if n} == {"5", "11"}


def test_quantizer_case_on_the_cpu_codec(oracle):
    """What tests/test_gpu_zz_hsq_zero_contract.py::test_quantizer compares the HIP path with: NearestNeighborCompressor c_dim 24 /
    k_bit 8 / n_bit 32 through PSQuantizer on the CPU codec.  The compressor's codebook is the shipped d24 one; every neg_mid
    row travels as u = -0 with code 0, every pos_mid row as +0 -- the sign is on the wire --; in the aggregate these rows are +0,
    because the mean over the users starts from +0."""
    res = zc.quantizer_run(False, steps=1)
    assert np.array_equal(res["cb"], zc.codebook(24, 256, True))
    nneg = 0
    for t, names in enumerate(res["names"]):
        u, codes, grad = res["norms"][0][t], res["codes"][0][t], res["grads"][0][t].reshape(-1, 24)
        assert u.size == len(names) == codes.size
        for r, n in enumerate(names):
            if n is None:
                assert u[r] != 0
                continue
            assert codes[r] == 0 and rc.bits(u)[r] == (zc.NEG0 if zc.is_neg(n) else zc.POS0), (t, r, n)
            assert not rc.bits(grad[r]).any()      # the aggregate: the mean sums from +0 (ps_quantizer.py:48), a -0 decode ends as +0
            nneg += zc.is_neg(n)
    assert nneg >= 100 and all(zc.is_neg(n) for n in res["names"][2])
