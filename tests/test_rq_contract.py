"""tests/rq_contract.py against independent witnesses (no GPU): oracle.residual_compress, OracleResidualCodec on ragged tensors,
the reference's residual_*.npz fixtures, oracle.scalar_decode, oracle.mean_users and float64 -- and one assertion for every claim
tests/test_gpu_rq_contract.py makes about its inputs (every code below K, the zero-residual rows have l1 == 0 and come out as code
K - 1 with u = +0, the multi-tile lists exceed the wave bound, the -0 rows decode to -0 in both stages), so that the reference the
kernels are held to cannot be wrong, or its inputs toothless, silently."""
import glob
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import rq_contract as rc  # noqa: E402

F = np.float32
RESIDUAL = sorted(glob.glob(os.path.join(rc.GOLDEN, "residual_*.npz")))
NEG0 = 0x80000000


# ---- witnesses ----------------------------------------------------------------------------------------------------------------
def test_fixtures_found():
    assert len(RESIDUAL) >= 3


def _fixture_stage(g, tag, n_bit):
    """(codes, raw, level_bytes, (lb, ub)) of a fixture's stage signature."""
    if n_bit == 32:
        return g[tag + "codes"], rc.f32(g[tag + "u"]), (F(0), F(0))
    return g[tag + "codes"], g[tag + "levels"].astype(np.uint8), (F(g[tag + "lb"]), F(g[tag + "ub"]))


@pytest.mark.parametrize("path", RESIDUAL, ids=[os.path.basename(p)[:-4] for p in RESIDUAL])
def test_restatement_against_the_reference_fixtures(oracle, path):
    """Stage 2's signature from the fixture's stage 1 through encode2(), `decoded` from both through decode_sum() in PLAIN
    mode -- and the same from oracle.residual_compress."""
    g = np.load(path)
    n_bit = int(g["n_bit"])
    lvb = 0 if n_bit == 32 else 1
    c1, raw1, b1 = _fixture_stage(g, "s1_", n_bit)
    c2, raw2, b2 = _fixture_stage(g, "s2_", n_bit)
    norm1 = rc.level_norm(raw1, lvb, n_bit, *b1)
    codes, u, (mlo, mhi) = rc.encode2(g["x"], c1, norm1, g["codewords1"], g["c_dagger"], g["r"])
    assert np.array_equal(codes, c2.astype(np.uint8))
    s1, s2, d1, d2, dec = oracle.residual_compress(g["x"], g["codewords1"], g["codewords2"], g["c_dagger"], g["r"], n_bit)
    assert np.array_equal(rc.bits(u), rc.bits(s2["u"])) and np.array_equal(codes.astype(np.int32), s2["codes"])
    if n_bit == 32:
        assert np.array_equal(rc.bits(u), rc.bits(g["s2_u"]))
    lo, hi = oracle.minmax(u)
    assert (mlo, mhi) == (int(rc.order_map(lo).item()), int(rc.order_map(hi).item()))
    assert np.array_equal(rc.bits(rc.stage_decode(c1, norm1, g["codewords1"]).reshape(-1)), rc.bits(g["decoded1"].reshape(-1)))
    payload = (c1, raw1, b1, c2, raw2, b2)
    plain = rc.decode_sum([payload], g["codewords1"], g["codewords2"], lvb, n_bit, rc.PLAIN)
    assert np.array_equal(rc.bits(plain), rc.bits(g["decoded"].reshape(-1)))
    assert np.array_equal(rc.bits(plain), rc.bits(dec))
    err = rc.decode_sum([payload], g["codewords1"], g["codewords2"], lvb, n_bit, rc.ERROR, v=g["x"])
    assert np.array_equal(rc.bits(err), rc.bits(rc.f32(g["x"]).reshape(-1) - rc.f32(g["decoded"]).reshape(-1)))


def make_args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=True, random=0, ef=False, two_phase=False, scale="exp",
                num_users=1, mode="ps", cr=256, gq_rng="reference")
    base.update(kw)
    return Namespace(**base)


@pytest.mark.parametrize("d,n_bit", [(16, 6), (8, 6), (32, 32)])
def test_restatement_against_the_oracle_codec_on_ragged_tensors(oracle, d, n_bit):
    """OracleResidualCodec (tests/oracle_codec_rq.py) encodes tensors of 1, 63, 64, 65 and 300 subvectors for three users; stage
    2's codes from stage 1's sections through encode2(), the codec's decode through decode_sum() in MEAN and PLAIN mode."""
    from gq_amd.compressors import ResidualCompressor
    from oracle_codec_rq import OracleResidualCodec
    lvb = 0 if n_bit == 32 else 1
    rs = np.random.RandomState(d)
    for M in (1, 63, 64, 65, 300):
        n = M * d
        cd = OracleResidualCodec(ResidualCompressor(n, torch.Size([n]), make_args(c_dim=d, n_bit=n_bit)), n, torch.Size([n]))
        first, second = cd.c.compressors
        cb1, cb2, cdag = first.codewords.numpy(), second.codewords.numpy(), second.c_dagger.numpy()
        wire = torch.zeros((3, cd.nbytes), dtype=torch.uint8)
        payloads = []
        for r in range(3):
            v = rc.f32(rs.randn(n) * 10.0 ** (r - 2))
            draws = torch.from_numpy(rs.rand(cd.draw_count()).astype(np.float32))
            cd.encode_into(torch.from_numpy(v.copy()), wire[r], 0, 0, r=draws)
            st = []
            for s, o in ((cd.s1, 0), (cd.s2, cd.stage2_off)):
                codes, levels, lb_ub = [t.numpy() for t in s._views(wire[r], o)]
                st += [codes.copy(), levels.copy(), (F(lb_ub[0]), F(lb_ub[1])) if lvb else (F(0), F(0))]
            payloads.append(tuple(st))
            run = cd.draw_runs()[1]
            codes, u, _ = rc.encode2(v, st[0], rc.level_norm(st[1], lvb, n_bit, *st[2]), cb1, cdag, draws.numpy()[run * M:(run + 1) * M])
            assert np.array_equal(codes, st[3]), (M, r)
            if lvb == 0:
                assert np.array_equal(rc.bits(u), rc.bits(st[4])), (M, r)
        for R, plain, mode in ((3, False, rc.MEAN), (1, False, rc.MEAN), (1, True, rc.PLAIN)):
            out = torch.empty(n)
            cd._decode(wire[:R], 0, R, out, plain=plain)
            want = rc.decode_sum(payloads[:R], cb1, cb2, lvb, n_bit, mode)
            assert np.array_equal(rc.bits(out.numpy()), rc.bits(want)), (M, R, plain)


@pytest.mark.parametrize("n_bit", [1, 6, 8])
def test_level_norm_at_every_level(oracle, n_bit):
    """Every level 0 .. 2**n_bit against oracle.scalar_decode (a division by s where level_norm scales by 1 / s), for bounds
    whose range is no power of two, for lb == ub and for lb == ub == 0; in every level width that holds the top level."""
    levels = np.arange((1 << n_bit) + 1)
    for lb, ub in ((F(-0.37), F(1.91)), (F(3e-39), F(7e-39)), (F(-2.5e37), F(3.1e38)), (F(0.75), F(0.75)), (F(0.0), F(0.0))):
        want = oracle.scalar_decode(levels, n_bit, lb, ub)
        for lvb in (1, 2, 4):
            if levels[-1] > np.iinfo(rc.LEVEL_DTYPE[lvb]).max:
                continue
            got = rc.level_norm(levels.astype(rc.LEVEL_DTYPE[lvb]), lvb, n_bit, lb, ub)
            assert got.dtype == np.float32 and np.array_equal(rc.bits(got), rc.bits(want)), (n_bit, lb, ub, lvb)
    raw = rc.f32([0.0, -0.0, 1e-45, np.inf])
    assert np.array_equal(rc.bits(rc.level_norm(raw, 0, 32, F(1), F(2))), rc.bits(raw))      # f32 norms travel as they are


def _decode_f64(payloads, cb1, cb2, lvb, n_bit, R):
    """The mean with every operation in float64, rounded to f32 where the header rounds: a product of two f32 is exact in f64,
    a sum of two f32 and an f32 divided by an integer are safe under double rounding."""
    acc = None
    with np.errstate(all="ignore"):
        for c1, r1, b1, c2, r2, b2 in payloads:
            d = []
            for c, raw, b, cb in ((c1, r1, b1, cb1), (c2, r2, b2, cb2)):
                n = rc.level_norm(raw, lvb, n_bit, *b).astype(np.float64)
                d.append((rc.f32(cb).astype(np.float64)[c.astype(np.intp)] * n[:, None]).astype(np.float32).astype(np.float64))
            x = ((0.0 + d[0]).astype(np.float32).astype(np.float64) + d[1]).astype(np.float32).astype(np.float64)
            acc = x if acc is None else (acc + x).astype(np.float32).astype(np.float64)
        return ((0.0 + acc) / float(R)).astype(np.float32).reshape(-1)


@pytest.mark.parametrize("R", [1, 2, 3, 5, 7, 8, 9, 16])
@pytest.mark.parametrize("lvb", [0, 1, 2, 4])
def test_decode_mean_against_float64_and_mean_users(oracle, R, lvb):
    G, P, cb1, cb2 = rc.decode_case(rc.RAGGED, 16, 256, lvb, R, 40 + R, two_images=bool(R & 1), special="zeros" if not (R & 1) else None)
    for s in range(G.nseg):
        got = rc.decode_sum(P[s], cb1, cb2, lvb, G.n_bit, rc.MEAN)
        assert rc.same(got, _decode_f64(P[s], cb1, cb2, lvb, G.n_bit, R)), (s, R)
        xs = np.stack([rc.decode_sum([p], cb1, cb2, lvb, G.n_bit, rc.PLAIN) for p in P[s]])
        assert np.array_equal(rc.bits(got), rc.bits(oracle.mean_users(xs))), (s, R)


@pytest.mark.parametrize("R", [3, 5, rc.GQ_ODD_DIV_MAX, rc.GQ_ODD_DIV_MAX + 2])
def test_decode_mean_at_the_ends_of_the_float_range(R):
    """The "range" inputs do what they are for: subnormal means, finite sums above 1e38, sums that overflow, NaN from inf - inf;
    the restatement equals float64 on them (any NaN equals any NaN)."""
    G, P, cb1, cb2 = rc.decode_case([5, 64, 131], 16, 256, 0, R, 7 + R, special="range")
    kinds = set()
    for s in range(G.nseg):
        got = rc.decode_sum(P[s], cb1, cb2, 0, 32, rc.MEAN)
        assert rc.same(got, _decode_f64(P[s], cb1, cb2, 0, 32, R)), (s, R)
        a = np.abs(got)
        kinds |= {k for k, m in (("subnormal", (a > 0) & (a < np.finfo(np.float32).tiny)), ("huge", np.isfinite(a) & (a * R > 1e38)),
                                 ("inf", np.isinf(a)), ("nan", np.isnan(a))) if m.any()}
    assert kinds == {"subnormal", "huge", "inf", "nan"}, kinds


def test_uniforms_and_seeds_against_the_pvq_tests_host_forms():
    """resolve_seed here == tests/test_gpu_pvq.py's, whose _uniform01_host the GPU file uses for the device draws."""
    import test_gpu_pvq as tp
    for seed, step in ((0x1234ABCD5678EF01, 5), (0, 0), (rc.M64, 2 ** 40 + 3)):
        assert rc.resolve_seed(seed, step) == tp._resolved_counter_seed(seed, step)
    assert rc.RQ_CODE_SALT == tp.PVQ_STREAM_SALT and rc.RQ_LEVEL2_SALT != rc.RQ_CODE_SALT
    r = tp._uniform01_host(rc.resolve_seed(1, 2) ^ rc.RQ_CODE_SALT, list(range(0, 200000, 997)))
    assert r.dtype == np.float32 and (r >= 0).all() and (r < 1).all() and np.unique(r).size > 190


def test_order_map_is_monotonic_and_has_the_identities():
    x = rc.f32([-np.inf, -3.0, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf])
    m = rc.order_map(x).astype(np.int64)
    assert (np.diff(m) > 0).all() and m.min() > 0 and m.max() < rc.M32
    assert rc.fold_minmax(x[1:4]) == (int(m[1]), int(m[3]))


# ---- preconditions of the GPU tests' inputs ------------------------------------------------------------------------------------
CUS = [256, 304, 64]


def test_bounds_are_the_kernels():
    """PwShape<D>::LDS_BYTES as csrc/pvq_walk.hpp computes it, and the issue's figures at 256 CUs."""
    assert [rc.pw_lds_bytes(d) for d in (8, 16, 32)] == [24832, 41216, 73984]
    assert [rc.encode_wave_bound(d, 256) for d in (8, 16, 32)] == [12288, 6144, 4096]
    assert [rc.decode_pass_slots(d, 256) for d in (8, 16, 32)] == [262144, 131072, 65536]


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("d", [8, 16, 32])
def test_multi_tile_lists_exceed_the_wave_bound(d, cus):
    bound = rc.encode_wave_bound(d, cus)
    for k, total in enumerate(rc.multi_tile_totals(d, cus)):
        Ms = rc.multi_tile_Ms(d, cus, total)
        G = rc.Group(Ms, d, 64, 1, 6)
        assert G.ntiles == total > bound
        assert sum(1 for m in Ms if m <= 200) == 300 and set(rc.SMALL_CYCLE) <= set(Ms) and sum(1 for m in Ms if m > 200) == 5
        for bpc in range(1, 9):      # whatever the occupancy query answers: every wave gets two tiles or more ...
            waves = min((total + 3) // 4, cus * bpc) * rc.ENC_WAVES
            if cus * bpc * rc.ENC_WAVES * 2 > bound:
                continue
            assert total // waves >= 2
            if k == 1:               # ... and of the second total some waves one more, some not
                assert 0 < total - (total // waves) * waves < waves
    Ms = rc.decode_multi_pass_Ms(d, cus)
    G = rc.Group(Ms, d, 64, 1, 6)
    assert G.ntiles * 64 > rc.decode_pass_slots(d, cus) and len(set(Ms)) > 8


def _check_encode_case(G, T, K):
    for t in T:
        assert t["codes"].dtype == np.uint8 and int(t["codes"].max()) < K and int(t["codes1"].max()) < K
        assert not np.isnan(t["u"]).any() and not (rc.bits(t["u"]) == NEG0).any()
        assert t["minmax"][0] <= t["minmax"][1]
    return T


@pytest.mark.parametrize("lvb", [0, 1, 2, 4])
def test_stage1_inputs_hold_what_they_claim(oracle, lvb):
    """Level 0 and the top level, lb == ub, lb == ub == 0 with every norm 0, tensors of 1, 63, 64 and 65 subvectors, draws 0 and
    >= 1, and the rows whose residual is exactly zero: l1 == 0, and the oracle gives code K - 1 with u = +0."""
    K, d = 256, 16
    G, T = rc.encode_case([1, 63, 64, 65, 700, 7, 129, 64, 300], d, K, lvb, 21 + lvb, kinds=("ordinary", "equal", "zero"))
    _check_encode_case(G, T, K)
    cb1, cdag, _ = rc.codebooks(d, K)
    assert {1, 63, 64, 65} <= set(G.Ms)
    seen_zero_rows = 0
    for t in T:
        x = rc.stage2_input(t["v"], t["codes1"], t["norm1"], cb1)
        zr = t["zero"]
        assert zr[0] and not rc.bits(x[zr]).any()                                  # the residual is +0 in every element
        _, _, l1, _, _ = oracle.pvq_encode(x.reshape(-1), cdag, t["r"], sub_rows=1)
        assert not l1[zr].any() and (l1[~zr] > 0).all()
        assert (t["codes"][zr] == K - 1).all() and not rc.bits(t["u"][zr]).any()
        seen_zero_rows += int(zr.sum())
        assert (t["r"] == 0).any() and (t["M"] <= 4 or (t["r"] >= 1).sum() == 2)
        if lvb:
            top = rc.top_level(G.n_bit)
            assert int(t["raw1"].max()) == top and (t["M"] == 1 or int(t["raw1"].min()) == 0) and top <= np.iinfo(t["raw1"].dtype).max
            if t["kind"] == "equal":
                assert t["lb"] == t["ub"] != 0 and (t["norm1"] == t["lb"]).all()
        if t["kind"] == "zero":
            assert not rc.bits(t["norm1"]).any()
    assert seen_zero_rows > 150 and {t["kind"] for t in T} == {"ordinary", "equal", "zero"}


@pytest.mark.parametrize("K,d", rc.SERVED)
def test_served_shape_inputs(oracle, K, d):
    G, T = rc.encode_case(rc.SERVED_MS, d, K, 1, K + d)
    _check_encode_case(G, T, K)
    cb1, cdag, other = rc.codebooks(d, K)
    assert cb1.shape == cdag.shape == other.shape == (K, d) and not np.array_equal(cb1, other)
    assert len({int(c) for t in T for c in t["codes"]}) > K // 2      # the sampler's codes spread over the codebook


def test_signed_zero_inputs_decode_to_minus_zero_in_both_stages():
    for lvb in (0, 1, 2, 4):
        G, P, cb1, cb2 = rc.decode_case(rc.RAGGED, 16, 256, lvb, 3, 5, special="zeros")
        assert cb1 is cb2 and (cb1 < 0).any()
        for p in P[1]:
            d1 = rc.stage_decode(p[0], rc.level_norm(p[1], lvb, G.n_bit, *p[2]), cb1)
            d2 = rc.stage_decode(p[3], rc.level_norm(p[4], lvb, G.n_bit, *p[5]), cb2)
            both = (rc.bits(d1) == NEG0) & (rc.bits(d2) == NEG0)
            assert both.any() and not d1.any() and not d2.any()
        for p in P[2]:
            d1 = rc.stage_decode(p[0], rc.level_norm(p[1], lvb, G.n_bit, *p[2]), cb1)
            d2 = rc.stage_decode(p[3], rc.level_norm(p[4], lvb, G.n_bit, *p[5]), cb2)
            assert d1.any() and np.array_equal(rc.bits(d2), rc.bits(-d1))
        for mode, R in ((rc.MEAN, 3), (rc.MEAN, 1), (rc.PLAIN, 1)):
            for s in (1, 2):
                assert not rc.bits(rc.decode_sum(P[s][:R], cb1, cb2, lvb, G.n_bit, mode)).any()      # +0 everywhere
        v = rc.f32(np.arange(G.Ms[1] * 16) - 7.0)
        assert np.array_equal(rc.bits(rc.decode_sum(P[1][:1], cb1, cb2, lvb, G.n_bit, rc.ERROR, v=v)), rc.bits(v))
    # two images: code K - 1 - c of the second names -cb1[c]
    G, P, cb1, cb2 = rc.decode_case(rc.RAGGED, 16, 256, 1, 1, 6, two_images=True)
    assert np.array_equal(rc.bits(cb2[255 - 9]), rc.bits(-cb1[9]))


def test_group_layout_leaves_gaps_round_every_section():
    """Sections 16-byte aligned, at least 16 bytes of nobody's between two of them and at both ends; OUT_GAP floats round every
    tensor's span of out; a part's tables are rebased."""
    G = rc.Group(rc.RAGGED, 8, 64, 2, 8)
    m = G.mask()
    edges = np.flatnonzero(np.diff(m.astype(np.int8)))
    starts, ends = edges[0::2] + 1, edges[1::2] + 1
    assert len(starts) == 6 * G.nseg and (starts % 16 == 0).all() and starts[0] >= 16
    assert (starts[1:] - ends[:-1] >= 16).all() and G.ub - ends[-1] >= 16
    om = G.out_mask()
    assert om.sum() == sum(G.Ms) * 8 and not om[:G.OUT_GAP].any() and not om[-G.OUT_GAP:].any()
    t1, t2, ts, nseg, ntiles = G.tables(lo=2, hi=6)
    assert nseg == 4 and ts[0] == 0 and t1[0, 2] == 0 and ts.size == ntiles == sum((M + 63) // 64 for M in G.Ms[2:6])
    assert np.array_equal(t1[:, 6], np.asarray(G.out_off[2:6])) and np.array_equal(t1[:, 3:6], G.layout[0, 2:6, 3:6])
    assert np.array_equal(t1[:, 1:3], t2[:, 1:3]) and not np.array_equal(t1[:, 3:6], t2[:, 3:6])
