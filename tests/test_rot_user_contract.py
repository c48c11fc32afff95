"""SIGNS, PER STREAM (include/gq_drive.h, include/gq_eden.h) on the CPU: tests/rot_user_contract.py's seeds and words against plain
big-integer arithmetic and the stepped words, the orders of operations DECODE-MEAN, PER STREAM fixes (each mutation changes bits on the
chosen inputs), and what per-user rotations are FOR -- the error of the mean of R users who compress the SAME gradient: the error of
one user under the shared rotation, falling as 1 / sqrt(R) when every user rotates by a stream of their own.  No GPU."""
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mx_contract as mx  # noqa: E402
import drive_contract as dc  # noqa: E402
import eden_contract as ec  # noqa: E402
import rot_step_contract as rs  # noqa: E402
import rot_user_contract as ru  # noqa: E402

M64 = rs.M64


def test_stream_zero_is_the_stepped_rotation():
    rng = random.Random(7)
    for _ in range(1000):
        s, t = rng.getrandbits(64), rng.getrandbits(64)
        assert ru.words_of(s, t, 0) == rs.step_words(s, t)
    for s in (0, 1, M64):
        assert ru.seed_of(s, 0) == s and ru.words_of(s, 0, 0) == rs.step_words(s, 0)


def _seed_of_big(seed, sigma):
    """The header's rule in unbounded integers, reduced only where the header says mod 2^64."""
    if sigma == 0:
        return seed
    z = (seed + sigma * 0xD6E8FEB86659FD93) % 2 ** 64
    z = ((z ^ (z // 2 ** 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z // 2 ** 27)) * 0x94D049BB133111EB) % 2 ** 64
    return z ^ (z // 2 ** 31)


def test_seed_of_against_big_integers():
    rng = random.Random(11)
    cases = [(s, k) for s in (0, 1, 2, M64, 0x9E3779B97F4A7C15) for k in (0, 1, 2, 7, 2 ** 31 - 1)]
    cases += [(rng.getrandbits(64), rng.randrange(2 ** 31)) for _ in range(1000)]
    for s, k in cases:
        assert ru.seed_of(s, k) == _seed_of_big(s, k), (s, k)
        assert 0 <= ru.seed_of(s, k) <= M64
    # one value written out by hand: seed 1, stream 1
    z = (1 + 0xD6E8FEB86659FD93) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    assert ru.seed_of(1, 1) == z ^ (z >> 31) != 1
    # a stream's words are the stepped words of ITS seed at every step
    assert ru.words_of(5, 3, 9) == rs.step_words(ru.seed_of(5, 9), 3)


@pytest.mark.parametrize("seed", [0, 1, M64])
def test_4096_consecutive_streams_have_4096_distinct_quadruples(seed):
    quads = [ru.words_of(seed, 0, k) for k in range(4096)]
    assert len(set(quads)) == 4096
    assert len(set(w for q in quads for w in q)) == 4 * 4096      # (and no word comes twice)
    assert len(set(ru.words_of(seed, 3, k) for k in range(4096))) == 4096


# ---- the orders DECODE-MEAN, PER STREAM fixes -----------------------------------------------------------------------------------------
def _sections(kind, n, R, seed, step, first=0):
    """R users' sections of R DIFFERENT Gaussian gradients, user r under stream first + r."""
    return [ru.compress(kind, dc.gaussian(n, 40 + r), dc.UNBIASED, seed, step, first + r)[0] for r in range(R)]


@pytest.mark.parametrize("kind", ru.KINDS)
def test_each_mutation_changes_bits(kind):
    n, seed, step, R = 700, 3, 2, 3
    secs = _sections(kind, n, R, seed, step)
    want = ru.decode_mean(kind, secs, n, seed, step)
    for wrong in (ru.decode_mean_rotated_sum, ru.decode_mean_reversed, ru.decode_mean_reciprocal):
        got = wrong(kind, secs, n, seed, step)
        assert not np.array_equal(mx.bits_of(got), mx.bits_of(want)), wrong.__name__
    # and the restatement is what it says: D_r by hand, under stream r's words
    Ds = []
    for r, s in enumerate(secs):
        signs = rs.step_words(ru.seed_of(seed, r), step)
        one = dc.decode_mean([s], n, signs, plain=True) if kind == "drive" else ec.decode_mean([s], n, ru.bits_of_kind(kind), signs, plain=True)
        Ds.append(one)
    acc = np.zeros(n, np.float32)
    for D in Ds:
        acc = (acc + D).astype(np.float32)
    assert np.array_equal(mx.bits_of((acc / np.float32(R)).astype(np.float32)), mx.bits_of(want))
    assert np.array_equal(mx.bits_of(ru.decode_mean(kind, secs[:1], n, seed, step, plain=True)), mx.bits_of(Ds[0]))


@pytest.mark.parametrize("kind", ru.KINDS)
def test_one_payload_under_stream_zero_is_the_stepped_decode(kind):
    n, seed, step = 600, 9, 4
    sec, D = ru.compress(kind, dc.student(n, 5), dc.UNBIASED, seed, step, 0)[:2]
    stepped = ru.compress_under(kind, dc.student(n, 5), dc.UNBIASED, rs.step_words(seed, step))
    assert np.array_equal(sec, stepped[0]) and np.array_equal(mx.bits_of(D), mx.bits_of(stepped[1]))
    assert np.array_equal(mx.bits_of(ru.decode_mean(kind, [sec], n, seed, step, plain=True)), mx.bits_of(D))
    # first_stream shifts the streams: payload r under first + r
    secs = _sections(kind, n, 2, seed, step, first=5)
    a = ru.decode_mean(kind, secs, n, seed, step, first_stream=5)
    b = ru.decode_mean(kind, secs, n, seed, step, first_stream=0)
    assert not np.array_equal(mx.bits_of(a), mx.bits_of(b))


# ---- the error table -----------------------------------------------------------------------------------------------------------------
# R users compress the SAME gradient (the limit of data-parallel training with strongly correlated gradients) at rotation seed 1,
# step 0; the gradient is tests/test_rot_step_contract.py's (4,096 Gaussian elements, seed 11).  As there, the mean of the R decodes
# is taken in float64: a float32 decode has 24 significant bits and R <= 64, so the sum of R equal decodes is exact and "the shared
# rotation gains nothing" can be asserted as an equality.
N, G_SEED, SIGN_SEED = 4096, 11, 1
RS = [1, 4, 16, 64]
_cache = {}


def _errors(kind, mode, own):
    key = (kind, mode, own)
    if key not in _cache:
        g = dc.gaussian(N, G_SEED)
        acc, errs = np.zeros(N, np.float64), {}
        for r in range(max(RS)):
            D = ru.compress(kind, g, dc.MODES[mode], SIGN_SEED, 0, r if own else 0)[1]
            acc += D.astype(np.float64)
            if r + 1 in RS:
                errs[r + 1] = float(np.linalg.norm(acc / (r + 1) - g.astype(np.float64)) / np.linalg.norm(g.astype(np.float64)))
        _cache[key] = errs
    return _cache[key]


@pytest.mark.parametrize("kind", ru.KINDS)
def test_shared_rotation_the_mean_of_r_users_is_one_users_error(kind):
    errs = _errors(kind, "unbiased", False)
    print(kind, "shared, unbiased:", " ".join("R=%d %.4f" % (R, errs[R]) for R in RS))
    for R in (4, 16, 64):
        assert errs[R] == errs[1], (kind, R)


@pytest.mark.parametrize("kind", ru.KINDS)
def test_own_rotations_the_error_falls_as_one_over_sqrt_r(kind):
    """The law for independent unbiased decodes: e_R * sqrt(R) / e_1 in [0.9, 1.1] in every cell (the band
    tests/test_rot_step_contract.py asserts for the same law over steps)."""
    errs = _errors(kind, "unbiased", True)
    ratios = {R: errs[R] * np.sqrt(R) / errs[1] for R in RS}
    print(kind, "own, unbiased:", " ".join("R=%d e=%.4f ratio=%.3f" % (R, errs[R], ratios[R]) for R in RS))
    assert errs[1] == _errors(kind, "unbiased", False)[1]      # (user 0 rotates by stream 0 in both)
    for R in (4, 16, 64):
        assert 0.9 <= ratios[R] <= 1.1, (kind, R, errs[R], ratios[R])


# the floor of tests/test_rot_step_contract.py: the mse scale shrinks, the mean of many decodes tends to (1 - beta) g with beta the
# distortion of the 2^b-level Lloyd-Max quantiser of N(0, 1), and no number of users takes the error below beta
LLOYD_MAX_DISTORTION = {"drive": 1.0 - 2.0 / np.pi, "eden2": 0.1175, "eden3": 0.03454, "eden4": 0.009497}


@pytest.mark.parametrize("kind", ru.KINDS)
def test_own_rotations_mse_the_error_falls_but_not_below_the_quantisers_distortion(kind):
    errs = _errors(kind, "mse", True)
    beta = LLOYD_MAX_DISTORTION[kind]
    print(kind, "own, mse:", " ".join("R=%d %.4f" % (R, errs[R]) for R in RS), "beta %.4f" % beta)
    for R in (4, 16, 64):
        assert errs[R] < errs[1], (kind, R, errs)
        assert errs[R] >= 0.9 * beta, (kind, R, errs)
