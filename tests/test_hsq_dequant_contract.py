"""What the inputs of tests/test_gpu_hsq_dequant.py claim, checked without a GPU (tests/hsq_dequant_contract.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hsq_dequant_contract as hc  # noqa: E402
import rq_contract as rc  # noqa: E402

F = np.float32
TINY = F(2.0 ** -126)      # the smallest normal float32


@pytest.mark.parametrize("n_bit", [5, 6, 8])
def test_division_by_the_scale_is_the_multiplication_by_its_inverse(n_bit):
    """(float(l) * range) / 2**n_bit == (float(l) * range) * 2**-n_bit bit for bit, over every level and every range the GPU tests
    use (halved lb of payload 1 included): the identity level_to_norm rests on, subnormal quotients included."""
    l = np.arange((1 << n_bit) + 1, dtype=np.float32)
    for lb, ub in hc.REGIMES.values():
        for lo in (lb, F(lb * F(0.5))):
            with np.errstate(all="ignore"):
                rng = F(ub) - F(lo)
                a = (l * rng) / F(2 ** n_bit)
                b = (l * rng) * F(2.0 ** -n_bit)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_which_products_are_subnormal():
    """"tiny": every product level * range above level 0 is subnormal up to level 15, and its scaled value always (with these
    ranges the scaled values stay on the 2**-149 grid: the division and the multiplication both return them exactly).  "sub": lb is
    subnormal.  "ordinary": nothing is."""
    for n_bit in (6, 8):
        l = np.arange(1, 1 << n_bit, dtype=np.float32)
        lb, ub = hc.REGIMES["tiny"]
        p = l * (ub - lb)
        assert (p[:15] < TINY).all() and (p > 0).all()
        q = p * F(2.0 ** -n_bit)
        assert (q < TINY).all()
        lb, ub = hc.REGIMES["sub"]
        assert 0 < lb < TINY and ((l * (ub - lb)) * F(2.0 ** -n_bit) < TINY).any()
        lb, ub = hc.REGIMES["ordinary"]
        assert ((l * (ub - lb)) * F(2.0 ** -n_bit) >= TINY).all()
    lb, ub = hc.REGIMES["flat"]
    assert lb == ub


@pytest.mark.parametrize("n_bit", [6, 8])
def test_every_level_occurs_in_the_decode_launches(n_bit):
    every = set(range(1 << n_bit))
    plain = []
    for regime in hc.REGIMES:
        st = hc.level_start(regime)
        seen = [np.concatenate([np.concatenate(row) for row in hc.levels_of_launch(n_bit, R, st)]) for R in (1, 3)]
        assert set(np.concatenate(seen).tolist()) == every      # the two launches of a case
        if n_bit == 6:
            assert set(seen[0].tolist()) == every and set(seen[1].tolist()) == every
        plain.append(seen[0])
    assert set(np.concatenate(plain).tolist()) == every          # the plain launches of the four ranges


@pytest.mark.parametrize("n_bit,rounding", [(6, False), (5, True)])
@pytest.mark.parametrize("regime", sorted(hc.REGIMES))
def test_every_level_occurs_in_the_level_launch(n_bit, rounding, regime):
    """The first tensor's projections land on every level (rounding off), the ends of the range are its first and last
    projections, and the packed form holds what went in."""
    lb, ub = hc.REGIMES[regime]
    u = hc.projections(hc.MS[0], lb, ub, n_bit, seed=3)
    assert u[0] == ub and u[-1] == lb and u.min() == lb and u.max() == ub
    l = hc.quantise(u, lb, ub, n_bit)
    if regime == "flat":
        assert not l.any()
    elif hc.MS[0] > 2 << n_bit:
        assert set(l.tolist()) == set(range(1 << n_bit))
    else:
        assert l.min() == 0 and l.max() == (1 << n_bit) - 1
    r = np.random.RandomState(1).rand(len(u)).astype(np.float32)
    lr = hc.quantise(u, lb, ub, n_bit, r)
    assert ((lr - l) >= 0).all() and ((lr - l) <= 1).all() and lr.max() <= hc.top_level(n_bit, True)
    p = hc.pack6(l)
    assert len(p) == 3 * ((len(l) + 3) // 4)
    w = p[0::3].astype(np.uint32) | (p[1::3].astype(np.uint32) << 8) | (p[2::3].astype(np.uint32) << 16)
    back = np.stack([(w >> (6 * k)) & 63 for k in range(4)], axis=1).reshape(-1)
    assert np.array_equal(back[:len(l)], l) and not back[len(l):].any()
