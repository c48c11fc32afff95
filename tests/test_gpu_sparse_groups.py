"""Top-k, sign and Maurey on the MI355X: a multi-tensor group against one-tensor codecs on the same inputs.  Both sides are this
code base's own bit-exact paths, so every comparison is torch.equal on the bits.  Sizes: one item, one item plus one element
(of the 4096-element chunk; 16385 is that for the sign wire's 16384-element item) and several items with a ragged end; one
identity-compressed tensor rides in the group's compress; top-k gets a fourth tensor with k = 0 whose empty section ends the wire."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1001, 4097, 16385]
DENSE = 10


class _K(object):
    def __init__(self, k):
        self.k = k


def _make(kind):
    """(group class, a function that makes the codecs afresh, draws per tensor or None)."""
    from gq_amd import codecs as C
    if kind == "topk":
        sizes, ks = SIZES + [100], [62, 256, 1024, 0]
        return C.BatchedTopK, sizes, lambda: [C.TopKCodec(_K(k), n, (n,)) for n, k in zip(sizes, ks)], None
    if kind == "sign":
        return C.BatchedSign, SIZES, lambda: [C.SignCodec(None, n, (n,)) for n in SIZES], None
    ks = [27, 124, 600]
    return C.BatchedMaurey, SIZES, lambda: [C.MaureyCodec(_K(k), n, (n,)) for n, k in zip(SIZES, ks)], ks


def _bits(t):
    return t.contiguous().view(-1).view(torch.int32)


@pytest.mark.parametrize("kind", ["topk", "sign", "maurey"])
def test_group_equals_one_tensor_codecs(kind):
    from gq_amd.codecs import _up
    dev = torch.device("cuda:0")
    Group, sizes, make_codecs, ks = _make(kind)
    rs = np.random.RandomState(7)
    payloads = [[torch.from_numpy((rs.standard_normal(n) * 1e-2).astype(np.float32)).to(dev) for n in sizes] for _ in range(2)]
    small = torch.from_numpy(rs.standard_normal(DENSE).astype(np.float32)).to(dev)
    us = [torch.from_numpy(rs.rand(k).astype(np.float32)).to(dev) for k in ks] if ks else None
    codecs = make_codecs()
    # the wire: the non-empty sections, the dense tensor, then (top-k) the empty section of the k = 0 tensor at the very end
    offs, off = [], 0
    for cd in codecs:
        if cd.nbytes:
            offs.append(off)
            off = _up(off + cd.nbytes)
    dense_off = off
    user_bytes = _up(off + 4 * DENSE)
    offs += [user_bytes] * (len(codecs) - len(offs))
    idxs = list(range(len(codecs)))
    group = Group(codecs, offs, idxs, dev, 1, user_bytes, dense=[(dense_off, DENSE)])
    draws = (torch.cat(us), {i: int(s) for i, s in enumerate(np.cumsum([0] + ks[:-1]))}) if ks else None
    extra = [{"r": u} for u in us] if ks else [{} for _ in codecs]

    # ---- the wire bytes and the compress launches' dense output
    singles = make_codecs()
    gathered = torch.zeros((2, user_bytes), dtype=torch.uint8, device=dev)
    gathered1 = torch.zeros((2, user_bytes), dtype=torch.uint8, device=dev)
    for row, ts in enumerate(payloads):
        out = torch.full((group.out_floats,), 7.0, dtype=torch.float32, device=dev)
        assert group.encode([t.clone() for t in ts], gathered[row], 0, 0, draws=draws, dense=[small], out=out)
        for cd, t, o, oo, kw in zip(singles, ts, offs, group.out_off, extra):
            dec = torch.full((cd.numel,), 7.0, dtype=torch.float32, device=dev)
            cd.encode_decode_into(t.clone(), gathered1[row], o, 0, dec, **kw)
            assert torch.equal(_bits(out[oo:oo + cd.numel]), _bits(dec)), "dense output of the %d-element tensor" % cd.numel
        gathered1[row, dense_off:dense_off + 4 * DENSE].view(torch.float32).copy_(small)
    assert torch.equal(gathered, gathered1), "wire bytes"

    # ---- the R = 2 decode-mean: whole, as two parts, and per tensor
    whole = [v.clone() for v in group.decode_mean(gathered, 2)]
    group.decode_mean(gathered, 2, part=(0, 2, True))
    parts = [v.clone() for v in group.decode_mean(gathered, 2, part=(2, len(codecs), False))]
    for cd, o, a, b in zip(singles, offs, whole, parts):
        one = cd.decode_mean(gathered, o, 2)
        assert a.shape == one.shape and torch.equal(_bits(a), _bits(one)), "decode-mean of the %d-element tensor" % cd.numel
        assert torch.equal(_bits(b), _bits(one)), "decode-mean in two parts, the %d-element tensor" % cd.numel

    # ---- error feedback with no `out` handed in: the gradients, the residuals and the wire
    errs = [torch.from_numpy((rs.standard_normal(n) * 1e-2).astype(np.float32)).to(dev) for n in sizes]
    ts_g, errs_g = [t.clone() for t in payloads[0]], [e.clone() for e in errs]
    wire_g = torch.zeros(user_bytes, dtype=torch.uint8, device=dev)
    wire_1 = torch.zeros(user_bytes, dtype=torch.uint8, device=dev)
    assert group.encode(ts_g, wire_g, 0, 0, errs=errs_g, ef_scale=0.75, draws=draws, dense=[small])
    for i, (cd, t, e, o) in enumerate(zip(singles, payloads[0], errs, offs)):
        t1, e1 = t.clone(), e.clone()
        one_draws = (us[i], {0: 0}) if ks else None
        assert cd._batched1(dev).encode([t1], cd._at(wire_1, o), 0, 0, errs=[e1], ef_scale=0.75, draws=one_draws)
        assert torch.equal(_bits(ts_g[i]), _bits(t1)), "gradient after error feedback, the %d-element tensor" % cd.numel
        assert torch.equal(_bits(errs_g[i]), _bits(e1)), "residual of the %d-element tensor" % cd.numel
    wire_1[dense_off:dense_off + 4 * DENSE].view(torch.float32).copy_(small)
    assert torch.equal(wire_g, wire_1), "wire bytes under error feedback"
