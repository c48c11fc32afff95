"""SIGNS, STEPPED (include/gq_drive.h, include/gq_eden.h) on the CPU: tests/rot_step_contract.py's words against the host side's
(MXCompressor.sign_words, DriveCompressor.rotation_words), the consequences the headers state, and what stepping is FOR -- the error
of the mean of T decodes of one gradient: constant under the fixed rotation, falling as 1 / sqrt(T) in step mode with the unbiased
scale, flat with the mse scale.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import drive_contract as dc  # noqa: E402
import eden_contract as ec  # noqa: E402
import rot_step_contract as rs  # noqa: E402

from gq_amd.compressors import DriveCompressor, EdenCompressor, MXCompressor  # noqa: E402

M64, GAMMA = rs.M64, rs.GAMMA
SEEDS = [0, 1, 2, M64]


@pytest.mark.parametrize("seed", SEEDS)
def test_step_zero_is_the_fixed_words(seed):
    assert rs.step_words(seed, 0) == MXCompressor.sign_words(seed)
    assert DriveCompressor.rotation_words(seed, 0) == EdenCompressor.rotation_words(seed, 0) == MXCompressor.sign_words(seed)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("t", [1, 2, 5, 1000, 2 ** 40 + 3, 2 ** 62 - 1])
def test_step_t_is_step_zero_of_a_moved_seed(seed, t):
    want = MXCompressor.sign_words((seed + 4 * t * GAMMA) & M64)
    assert rs.step_words(seed, t) == want
    assert DriveCompressor.rotation_words(seed, t) == want


@pytest.mark.parametrize("seed", SEEDS)
def test_the_words_repeat_after_two_to_the_62_steps(seed):
    assert rs.step_words(seed, 2 ** 62) == rs.step_words(seed, 0)
    assert rs.step_words(seed, 2 ** 62 + 7) == rs.step_words(seed, 7)
    assert rs.step_words(seed, 2 ** 61) != rs.step_words(seed, 0)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_largest_step_wraps_as_the_formula_says(seed):
    # 4 * (2^64 - 1) = -4 mod 2^64: word k is output k - 4 of the stream, i.e. the step before step 0
    t = M64
    want = []
    for k in range(4):
        z = (seed + (k + 1 - 4) * GAMMA) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        want.append(z ^ (z >> 31))
    assert rs.step_words(seed, t) == tuple(want) == DriveCompressor.rotation_words(seed, t)
    assert rs.step_words(seed, t) == rs.step_words(seed, 2 ** 62 - 1)
    # word 3 of the step before step 0 hashes z = seed
    z = seed
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    assert rs.step_words(seed, t)[3] == z ^ (z >> 31)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_words_of_64_consecutive_steps_differ(seed):
    sets = [rs.step_words(seed, t) for t in range(64)]
    assert len(set(sets)) == 64
    assert len(set(w for s in sets for w in s)) == 256      # (and no word comes twice)


# ---- the error table -----------------------------------------------------------------------------------------------------------------
N, G_SEED, SIGN_SEED = 4096, 11, 1
TS = [1, 4, 16, 64, 256]
COMPRESSORS = ["drive", "eden2", "eden3", "eden4"]
_cache = {}


def _decode(name, g, mode, signs):
    if name == "drive":
        return dc.compress(g, dc.MODES[mode], signs)[1]
    return ec.compress(g, int(name[-1]), ec.MODES[mode], signs)[1]


def _errors(name, mode, stepped):
    """e_T = |mean of the first T decodes - g| / |g| for T in TS, and the means.  The mean is taken in float64: a float32 decode
    has 24 significant bits and T <= 256, so the sums of the fixed rotation's T equal decodes are exact and their mean is the
    decode itself."""
    key = (name, mode, stepped)
    if key not in _cache:
        g = dc.gaussian(N, G_SEED)
        acc, errs, means = np.zeros(N, np.float64), {}, {}
        for t in range(max(TS)):
            signs = rs.step_words(SIGN_SEED, t) if stepped else rs.step_words(SIGN_SEED, 0)
            acc += _decode(name, g, mode, signs).astype(np.float64)
            if t + 1 in TS:
                means[t + 1] = acc / (t + 1)
                errs[t + 1] = float(np.linalg.norm(means[t + 1] - g.astype(np.float64)) / np.linalg.norm(g.astype(np.float64)))
        _cache[key] = (errs, means)
    return _cache[key]


@pytest.mark.parametrize("name", COMPRESSORS)
def test_fixed_rotation_the_mean_decode_never_changes(name):
    errs, means = _errors(name, "unbiased", False)
    print(name, "fixed, unbiased:", " ".join("T=%d %.4f" % (T, errs[T]) for T in TS))
    for T in TS:
        assert np.array_equal(means[T].astype(np.float32).view(np.uint32), means[1].astype(np.float32).view(np.uint32)), T
        assert np.array_equal(means[T], means[1]), T
        assert errs[T] == errs[1]


@pytest.mark.parametrize("name", COMPRESSORS)
def test_step_mode_unbiased_the_error_falls_as_one_over_sqrt_t(name):
    """The law for independent unbiased decodes: e_T * sqrt(T) / e_1 in [0.9, 1.1] at every T."""
    errs, _ = _errors(name, "unbiased", True)
    ratios = {T: errs[T] * np.sqrt(T) / errs[1] for T in TS}
    print(name, "step, unbiased:", " ".join("T=%d e=%.4f ratio=%.3f" % (T, errs[T], ratios[T]) for T in TS))
    for T in TS:
        assert 0.9 <= ratios[T] <= 1.1, (name, T, errs[T], ratios[T])


def test_step_mode_mse_drive_stays_above_half_of_one_decode():
    errs, _ = _errors("drive", "mse", True)
    print("drive step, mse:", " ".join("T=%d %.4f" % (T, errs[T]) for T in TS))
    assert errs[256] > 0.5 * errs[1], errs


# The mse scale shrinks: <decode, g> = S * P = P^2 / C2 against |g|^2 = Q per block, so the mean of many decodes tends to (1 - beta) g
# with beta = 1 - P^2 / (Q C2), which for Gaussian coordinates is the distortion of the 2^b-level Lloyd-Max quantiser of N(0, 1)
# (Max 1960: 1 - 2 / pi = 0.3634 at one bit, 0.1175, 0.03454, 0.009497 at 2, 3, 4 bits).  No number of rounds takes the error below
# beta; one decode's error is about sqrt(beta).  (At 2 ... 4 bits beta is below half of sqrt(beta), so "above half of e_1" is
# DRIVE's statement only: eden2's e_256 = 0.118 against e_1 = 0.344.)
LLOYD_MAX_DISTORTION = {"drive": 1.0 - 2.0 / np.pi, "eden2": 0.1175, "eden3": 0.03454, "eden4": 0.009497}


@pytest.mark.parametrize("name", COMPRESSORS)
def test_step_mode_mse_the_error_flattens_at_the_quantisers_distortion(name):
    errs, _ = _errors(name, "mse", True)
    beta = LLOYD_MAX_DISTORTION[name]
    print(name, "step, mse:", " ".join("T=%d %.4f" % (T, errs[T]) for T in TS), "beta %.4f" % beta)
    assert errs[256] >= 0.9 * beta, (name, errs)
