"""SIGNS, PER STREAM and DECODE-MEAN, PER STREAM of include/gq_drive.h and include/gq_eden.h restated on top of
tests/rot_step_contract.py (the words), tests/drive_contract.py and tests/eden_contract.py (everything under given words): the seed of
a stream in Python integers, the four words of (seed, step, stream), a compress under a stream and the decode-mean of R payloads,
every one through its own inverse transform, added in the gradient's domain in the header's order
(tests/test_rot_user_contract.py checks this restatement on the CPU, tests/test_gpu_zz_rot_user_contract.py holds the kernels to it).
kind: "drive", "eden2", "eden3" or "eden4"."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mxr_contract as mxr  # noqa: E402
import drive_contract as dc  # noqa: E402
import eden_contract as ec  # noqa: E402
import rot_step_contract as rs  # noqa: E402

f32 = np.float32
M64 = rs.M64
STREAM_MUL = 0xD6E8FEB86659FD93
KINDS = ["drive", "eden2", "eden3", "eden4"]


def fin(z):
    """splitmix64's finaliser: the two multiplications and the three xor-shifts, mod 2^64."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def seed_of(seed, sigma):
    """seed_0 = seed; seed_sigma = fin(seed + sigma * STREAM_MUL) for sigma >= 1."""
    assert sigma >= 0
    if sigma == 0:
        return seed & M64
    return fin((seed + sigma * STREAM_MUL) & M64)


def words_of(seed, step, sigma):
    """The STEPPED words of (seed_sigma, step)."""
    return rs.step_words(seed_of(seed, sigma), step)


def bits_of_kind(kind):
    return 1 if kind == "drive" else int(kind[-1])


def section_bytes(kind, n):
    return dc.section_bytes(n) if kind == "drive" else ec.section_bytes(n, bits_of_kind(kind))


def compress_under(kind, g, mode, signs, err=None, ef_scale=None):
    """drive_contract.compress / eden_contract.compress under given words -> their tuples (section, D, w, err, x', S, ...)."""
    if kind == "drive":
        return dc.compress(g, mode, signs, err, ef_scale)
    return ec.compress(g, bits_of_kind(kind), mode, signs, err, ef_scale)


def compress(kind, g, mode, seed, step, sigma, err=None, ef_scale=None):
    """One tensor under stream sigma at (seed, step)."""
    return compress_under(kind, g, mode, words_of(seed, step, sigma), err, ef_scale)


def values(kind, sec, n):
    """y [nb, 256]: the decoded values of one section."""
    if kind == "drive":
        return dc.values(*dc.unpack(sec, n))
    b = bits_of_kind(kind)
    return ec.values(*ec.unpack(sec, n, b), ec.TABLES[b])


def scales_of(kind, sec, n):
    return dc.unpack(sec, n)[1] if kind == "drive" else ec.unpack(sec, n, bits_of_kind(kind))[1]


def decodes(kind, sections, n, seed, step, first_stream=0):
    """D_r [n]: payload r through the inverse transform under stream first_stream + r."""
    return [mxr.inverse_blocks(values(kind, s, n), words_of(seed, step, first_stream + r)).reshape(-1)[:n] for r, s in enumerate(sections)]


def decode_mean(kind, sections, n, seed, step, first_stream=0, plain=False):
    """m = (+0 + D_0 + ... + D_{R-1}) / (float)R: payloads ascending, one f32 addition each, a true division; plain: D_0 as it is."""
    Ds = decodes(kind, sections, n, seed, step, first_stream)
    if plain:
        assert len(Ds) == 1
        return Ds[0]
    acc = np.zeros(n, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for D in Ds:
            acc = (acc + D).astype(f32)
        return (acc / f32(len(Ds))).astype(f32)


# ---- what the kernels must NOT compute -----------------------------------------------------------------------------------------------
def decode_mean_rotated_sum(kind, sections, n, seed, step, first_stream=0):
    """The shared launch's shortcut: the mean in the rotated domain, then ONE inverse transform (under the first stream's words)."""
    signs = words_of(seed, step, first_stream)
    if kind == "drive":
        return dc.decode_mean(sections, n, signs)
    return ec.decode_mean(sections, n, bits_of_kind(kind), signs)


def decode_mean_reversed(kind, sections, n, seed, step, first_stream=0):
    """The payloads added in descending order (every payload still under its own stream)."""
    Ds = decodes(kind, sections, n, seed, step, first_stream)
    acc = np.zeros(n, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for D in reversed(Ds):
            acc = (acc + D).astype(f32)
        return (acc / f32(len(Ds))).astype(f32)


def decode_mean_reciprocal(kind, sections, n, seed, step, first_stream=0):
    """A multiplication by the rounded 1 / R in the place of the division."""
    Ds = decodes(kind, sections, n, seed, step, first_stream)
    acc = np.zeros(n, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for D in Ds:
            acc = (acc + D).astype(f32)
        return (acc * (f32(1.0) / f32(len(Ds)))).astype(f32)
