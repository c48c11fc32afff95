"""libgq_sketch.so on the MI355X against the numpy restatement of include/gq_sketch.h (tests/sketch_contract.py), bit for bit: the wire,
the dense output and the error tables, at the smallest shapes at which the launches can go wrong.
(zz: the file runs behind the other GPU tests, like the test_gpu_z_* files.)"""
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import sketch_contract as sc  # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
SEED = 9


def codec_for(n, rows, C=32, cr=64, ef=False):
    from gq_amd.codecs import default_codec_factory
    from gq_amd.compressors import CountSketchCompressor
    c = CountSketchCompressor(n, (n,), Namespace(cr=cr, sketch_rows=rows, sketch_cr=C, sketch_seed=SEED, sketch_ef=ef))
    return default_codec_factory(c, n, (n,))


def group_for(codecs, device="cuda"):
    from gq_amd.codecs import BatchedSketch
    offs, off = [], 0
    for cd in codecs:
        offs.append(off)
        off += cd.nbytes
    return BatchedSketch(codecs, offs, list(range(len(codecs))), torch.device(device, 0), 1, off), offs, off


def special(n, seed):
    """Gaussian with -0, subnormals and large magnitudes sprinkled in."""
    rs = np.random.RandomState(seed)
    w = rs.standard_normal(n).astype(f32)
    z = rs.rand(n)
    w[z < 0.05] = f32(-0.0)
    w[(z >= 0.05) & (z < 0.08)] = np.array(1e-41, f32)
    w[(z >= 0.08) & (z < 0.09)] = f32(-3e30)
    return w


def shapes(rows):
    first = 4096 * 2 * rows
    # (the first sketched size; a last item of one element; --sketch-cr 2 with two windows and a partial last item; 41 items in two or
    # three windows: lists longer than 8 entries, so two levels of sums -- with --sketch-cr 2 itself a window holds 2 r items on average)
    return [(first, 32), (first + 1, 32), (4096 * 4 * rows - 100, 2), (4096 * 40 + 123, 24 // rows)]


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


@pytest.mark.parametrize("rows", [1, 3, 5])
def test_one_tensor_wire_and_decode(rows):
    from gq_amd.codecs import DenseCodec
    assert type(codec_for(1000, rows)) is DenseCodec and type(codec_for(4096 * (2 * rows - 1), rows)) is DenseCodec
    for n, C in shapes(rows):
        cd = codec_for(n, rows, C)
        assert C != 2 or cd.nwin == 2
        if n > 4096 * 40:
            assert cd.nwin >= 2 and max(len(l) for row in sc.lists(SEED, rows, cd.items, cd.nwin) for l in row) > 8
        w = special(n, n % 1000)
        for shift in (0, 1):      # (1: a misaligned view, no 16-byte loads)
            t = torch.from_numpy(np.concatenate([np.zeros(shift, f32), w])).cuda()[shift:]
            wire = torch.full((cd.nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
            out = torch.full((n,), float("nan"), device="cuda")
            cd.encode_decode_into(t, wire, 0, 0, out)
            want = sc.section(w, SEED, rows, C)
            assert np.array_equal(wire.cpu().numpy(), want), (n, shift)
            dec, _ = sc.decode_mean([sc.tables(want)], n, cd.k, SEED)
            assert np.array_equal(bits(out.cpu().numpy()), bits(dec)), (n, shift)
    zeros = torch.from_numpy(np.full(shapes(rows)[1][0], -0.0, f32)).cuda()
    cd = codec_for(zeros.numel(), rows)
    wire = torch.full((cd.nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    cd.encode_into(zeros, wire, 0, 0)
    assert not wire.cpu().numpy()[16:].any()      # (-0 everywhere: every cell is +0)


@pytest.mark.parametrize("rows,ef", [(1, False), (3, False), (3, True), (5, True)])
def test_batch_of_three_tensors_payloads_and_error_tables(rows, ef):
    """Three tensors of mixed layouts in one batch, R = 1 and R = 3 hand-built payloads, garbage in every scratch buffer, and with the
    error accumulation three decodes in a row, E compared each time."""
    ns = [n for n, _ in shapes(rows)[:2]] + [4096 * 30 + 5]
    cds = [codec_for(n, rows, 4, ef=ef) for n in ns]
    for cd in cds:
        cd.E = torch.zeros(cd.cells, device="cuda") if ef else None
    grp, offs, total = group_for(cds)
    for name in ("part", "table", "est", "state", "counts"):
        t = grp._tables[name]
        t.view(torch.int32).fill_(0x7fc12345 if t.dtype == torch.float32 else 0x12345)
    E = [np.zeros(cd.cells, f32) if ef else None for cd in cds]
    for step, R in enumerate((1, 3, 3)):
        users = [[special(n, 17 * step + 5 * u + i) for i, n in enumerate(ns)] for u in range(R)]
        wire = torch.full((R, total), 0xCD, dtype=torch.uint8, device="cuda")
        for u in range(R):
            assert grp.encode([torch.from_numpy(w).cuda() for w in users[u]], wire[u], 0, 0)
        secs = [[sc.section(users[u][i], SEED, rows, 4) for i in range(3)] for u in range(R)]
        assert np.array_equal(wire.cpu().numpy(), np.stack([np.concatenate(s) for s in secs]))
        views = grp.decode_mean(wire, R)
        for i, (n, cd) in enumerate(zip(ns, cds)):
            want, E[i] = sc.decode_mean([sc.tables(secs[u][i]) for u in range(R)], n, cd.k, SEED, E[i])
            assert np.array_equal(bits(views[i].cpu().numpy()), bits(want)), (step, i)
            if ef:
                assert np.array_equal(bits(cd.E.cpu().numpy()), bits(E[i])), (step, i)
