"""What an item-table group's encode decides on the host, without a GPU: whether it refuses, which draws it picks, whether `out`
becomes the group's own error-feedback buffer, and the exact arguments it hands to its batch's compress / record.  The groups are
built by their own constructors over a recording library (item_host_stubs); _choose_header and _launch are stand-ins that note
what they were given.  Two shapes per class: one tensor of one element (one item) and tensors of 1 and 4,097 elements (a second
item: the smallest shapes at which the table walk differs)."""
import itertools
from argparse import Namespace

import pytest
import torch

import item_host_stubs as stubs
from gq_amd import codecs as C
from gq_amd import compressors as K
from gq_amd import native

SHAPES = ([1], [1, 4097])
SALT, FRESH = 0x11, 0x5EED
CPU = torch.device("cpu")


def _args(**kw):
    base = dict(c_dim=16, k_bit=8, n_bit=6, no_cuda=False, random=0, ef=False, two_phase=False, scale="exp", num_users=2, mode="ps", cr=1)
    base.update(kw)
    return Namespace(**base)


def _flat(cls, comp, **kw):
    return lambda n, **a: cls(comp(n, (n,), _args(**dict(kw, **a))), n, (n,))


# kind -> (group class, codec of n elements, error feedback through the dense decode, wire must be 16-byte aligned, compress's form)
KINDS = {
    "topk": (C.BatchedTopK, _flat(C.TopKCodec, K.TopKSparsificationCompressor), True, False, "plain"),
    "stc": (C.BatchedSTC, _flat(C.STCCodec, K.SparseTernaryCompressor), True, False, "plain"),
    "sign": (C.BatchedSign, _flat(C.SignCodec, K.SignSGDCompressor), False, False, "plain"),
    "thr": (C.BatchedThr, _flat(C.ThrCodec, K.ThresholdSparsificationCompressor), True, False, "thr"),
    "maurey": (C.BatchedMaurey, _flat(C.MaureyCodec, K.MaureySparsification), True, False, "drawn"),
    "mx": (C.BatchedMX, _flat(C.MXCodec, K.MXCompressor, mx_format="fp4", random=1), False, True, "drawn"),
    "mx-nearest": (C.BatchedMX, _flat(C.MXCodec, K.MXCompressor, mx_format="fp8"), False, True, "drawn"),
    "mxr": (C.BatchedMXR, _flat(C.MXRCodec, K.MXCompressor, mx_format="fp4", random=1, mx_rotate="hadamard", mx_rotate_seed=1), False, True,
            "drawn"),
    "drive": (C.BatchedDrive, _flat(C.DriveCodec, K.DriveCompressor), False, True, "rotated"),
    "drive-step": (C.BatchedDrive, _flat(C.DriveCodec, K.DriveCompressor, drive_rotation="step"), False, True, "rotated"),
    "drive-own": (C.BatchedDrive, _flat(C.DriveCodec, K.DriveCompressor, drive_user_rotation="own"), False, True, "rotated"),
    "eden": (C.BatchedEden, _flat(C.EdenCodec, K.EdenCompressor), False, True, "rotated"),
    "eden-own": (C.BatchedEden, _flat(C.EdenCodec, K.EdenCompressor, eden_user_rotation="own", eden_rotation="step"), False, True, "rotated"),
}


class Trace(object):
    """What the stand-ins saw, in order: ("header", errs, align) / ("counter_seed", slot, reserved) / "next_seed" /
    ("launch", name of the batch's method, its arguments, graph_header, defer_reset)."""

    def __init__(self, monkeypatch):
        self.events = ev = []

        def choose_header(group, tensors, slot, align, errs, dense, graph_header, table_current):
            ev.append(("header", errs, align))
            return True

        def launch(group, graph_header, defer_reset, launches, *args):
            assert launches.__self__ is group._batch
            ev.append(("launch", launches.__name__, args, graph_header, defer_reset))

        real_counter_seed = C._BatchedBase._counter_seed

        def counter_seed(group, slot, reserved=False):
            ev.append(("counter_seed", slot, reserved))
            return real_counter_seed(group, slot, reserved)

        def next_seed():
            ev.append("next_seed")
            return FRESH

        def upload(group, tensors, slot, align, errs=None, dense=None):
            ev.append(("upload", errs))
            return True

        monkeypatch.setattr(C._BatchedBase, "_choose_header", choose_header)
        monkeypatch.setattr(C._BatchedBase, "_launch", launch)
        monkeypatch.setattr(C._BatchedBase, "_counter_seed", counter_seed)
        monkeypatch.setattr(C._BatchedBase, "_upload", upload)
        monkeypatch.setattr(C, "_next_seed", next_seed)

    def take(self):
        ev = list(self.events)
        del self.events[:]
        return ev


@pytest.fixture
def trace(monkeypatch):
    stubs.install_groups(monkeypatch)
    return Trace(monkeypatch)


def _group(cls, cds):
    offsets = list(itertools.accumulate([0] + [cd.nbytes for cd in cds[:-1]]))
    g = cls(cds, offsets, list(range(len(cds))), CPU, 2, sum(cd.nbytes for cd in cds))
    tensors = [torch.zeros(cd.numel, dtype=g.dtype) for cd in cds]
    errs = [torch.zeros(cd.numel, dtype=torch.float32) for cd in cds]
    return g, tensors, errs


def _wire(misaligned=False):
    buf = torch.zeros(65536 + 32, dtype=torch.uint8)
    first = (-buf.data_ptr()) % 16 + (1 if misaligned else 0)
    return buf[first:]


def _given(g, cds):
    """A draw plan with the tensors' draws out of the group's order, and the draws in the group's order."""
    counts = [cd.draw_count() for cd in cds]
    r_all = torch.arange(sum(counts) + 3, dtype=torch.float32)
    offsets, at = {}, 3
    for i in reversed(range(len(cds))):
        offsets[i] = at
        at += counts[i]
    return (r_all, offsets), torch.cat([r_all[offsets[i]:offsets[i] + counts[i]] for i in range(len(cds))])


@pytest.mark.parametrize("sizes", SHAPES, ids=["one", "two"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_encode_decisions(trace, kind, sizes):
    cls, codec, dense_ef, aligned, form = KINDS[kind]
    cds = [codec(n) for n in sizes]
    g, tensors, errs = _group(cls, cds)
    assert cls.eligible(cds[0]) and type(g) is cls
    wire, out_given = _wire(), torch.zeros(g.out_floats, dtype=g.dtype)
    pairs = torch.zeros((3, 2), dtype=torch.int64)
    drawn = form == "drawn"
    random = drawn and g.random
    plans = [dict()]
    if drawn:
        plan, in_order = _given(g, cds)
        partial = (plan[0], {0: plan[1][0]}) if len(cds) > 1 else None
        plans = [dict(), dict(draws=plan), dict(seed=77), dict(draws=plan, seed=77), dict(pairs=True), dict(pairs=True, slot=2),
                 dict(pairs=True, slot=0, rng_slot=2), dict(pairs=True, seed=77), dict(pairs=True, draws=plan)]
        if partial is not None:
            plans.append(dict(draws=partial))
    elif form == "rotated":
        plans = [dict(), dict(slot=0, rng_slot=2), dict(stream_base=4), dict(rotation=torch.zeros((1, 2), dtype=torch.int64))]
    for plan, with_errs, with_out in itertools.product(plans, (False, True), (False, True)):
        plan = dict(plan)
        g.rng_pairs = pairs if plan.pop("pairs", False) else None
        slot, rng_slot = plan.pop("slot", 1), plan.pop("rng_slot", None)
        g.stream_base = plan.pop("stream_base", 0)
        if form == "rotated":
            g.rotation = plan.pop("rotation", None)
        e, out = (errs if with_errs else None), (out_given if with_out else None)
        ok = g.encode(tensors, wire, slot, SALT, e, 0.5, rng_slot=rng_slot, out=out, graph_header=None, defer_reset=None, **plan)
        ev = trace.take()
        assert ok is True
        ef = 0.5 if with_errs else None
        want_events = [("header", e, g.align)]
        if drawn:
            want_events.append(("counter_seed", slot, False) if rng_slot is None else ("counter_seed", rng_slot, True))
        # the draws: given / pinned seed / counter pair / fresh seed -- and none where the rounding is to nearest
        lead = ()
        if drawn:
            draws, seed = plan.get("draws"), plan.get("seed")
            given = random and draws is not None and all(i in draws[1] for i in range(len(cds)))
            pair_at = None
            if g.rng_pairs is not None and (rng_slot is not None or slot < 2):
                pair_at = pairs.data_ptr() + 16 * (slot if rng_slot is None else rng_slot)
            if not random:
                lead = (native.RANDOM_OFF, 0, None)
            elif given:
                lead = (native.RANDOM_GIVEN, 0, "given")
            elif seed is not None:
                lead = (native.RANDOM_DEVICE, 77, None)
            elif pair_at is not None:
                lead = (native.RANDOM_DEVICE_COUNTER, pair_at, None)
            else:
                lead = (native.RANDOM_DEVICE, FRESH ^ SALT, None)
                want_events.append("next_seed")
        assert ev[:-1] == want_events
        tag, name, args, graph_header, defer_reset = ev[-1]
        assert (tag, name, graph_header, defer_reset) == ("launch", "compress", None, None)
        assert args[0] is wire
        # out: the caller's, or -- where error feedback needs the dense decode and nobody asked for it -- the group's own buffer
        got_out = args[4] if drawn else args[1]
        if with_out:
            assert got_out is out_given
        elif with_errs and dense_ef:
            assert got_out is g._ef_out and got_out is g._ef_buffer(CPU) and got_out.numel() == g.out_floats and got_out.dtype == torch.float32
        else:
            assert got_out is None
        if form == "plain":
            assert args[2:] == (ef,) and len(args) == 3
        elif form == "thr":
            assert args[2:] == (ef, g.eta) and len(args) == 4 and g.eta == cds[0].eta
        elif drawn:
            mode, sd, r = args[1:4]
            assert (mode, sd) == lead[:2] and args[5] == ef and len(args) == 6
            if lead[2] == "given":
                assert r.dtype == torch.float32 and torch.equal(r, in_order)
            else:
                assert r is None
        else:
            assert args[2] == ef
            if g.own:
                pair, stream = args[3:]
                assert len(args) == 5 and stream == (0 if rng_slot is not None else g.stream_base + slot)
                assert pair is g.rotation and pair.dtype == torch.int64 and tuple(pair.shape) == (1, 2)
            else:
                assert args[3:] == (g.rotation,) and (g.rotation is None or plan == {})
    # a wire that is not 16-byte aligned: refused in front of the header where the launches need it, taken otherwise
    ok = g.encode(tensors, _wire(misaligned=True), 1, SALT, errs, 0.5)
    ev = trace.take()
    if aligned:
        assert ok is False and ev == []
    else:
        assert ok is True and ev[0][0] == "header" and ev[-1][0] == "launch"


@pytest.mark.parametrize("sizes", SHAPES, ids=["one", "two"])
@pytest.mark.parametrize("kind", ["maurey", "mx", "mxr"])
def test_reference_draws_are_required(trace, kind, sizes):
    cls, codec, _, _, _ = KINDS[kind]
    cds = [codec(n, gq_rng="reference") for n in sizes]
    g, tensors, errs = _group(cls, cds)
    assert g.reference_draws and not g.counter
    plan, in_order = _given(g, cds)
    wire = _wire()
    refusals = [None, (plan[0], {})] + ([(plan[0], {1: plan[1][1]})] if len(cds) > 1 else [])
    for draws in refusals:
        assert g.encode(tensors, wire, 1, SALT, errs, 0.5, draws=draws, seed=77) is False
        assert trace.take() == []      # refused in front of the header, no seed taken
    assert g.encode(tensors, wire, 1, SALT, None, None, draws=plan) is True
    ev = trace.take()
    assert [x[0] for x in ev] == ["header", "counter_seed", "launch"]
    assert ev[-1][2][1:3] == (native.RANDOM_GIVEN, 0) and torch.equal(ev[-1][2][3], in_order)


def test_keyed_draws_take_no_pair(trace):
    cds = [KINDS["maurey"][1](1, gq_rng="keyed")]
    g, tensors, _ = _group(C.BatchedMaurey, cds)
    g.rng_pairs = torch.zeros((3, 2), dtype=torch.int64)
    assert not g.counter and g.encode(tensors, _wire(), 1, SALT) is True
    ev = trace.take()
    assert ev[1:3] == [("counter_seed", 1, False), "next_seed"] and ev[-1][2][1:4] == (native.RANDOM_DEVICE, FRESH ^ SALT, None)


@pytest.mark.parametrize("sizes", SHAPES, ids=["one", "two"])
def test_dgc_state(trace, monkeypatch, sizes):
    cds = [KINDS["topk"][1](n) for n in sizes]
    g, tensors, _ = _group(C.BatchedDGC, cds)
    wire, out_given = _wire(), torch.zeros(g.out_floats)
    us, vs = [torch.zeros(n) for n in sizes], [torch.zeros(n) for n in sizes]
    # no state: plain top-k, whatever ef_scale says
    for out in (None, out_given):
        assert g.encode(tensors, wire, 1, SALT, None, 0.9, out=out) is True
        assert trace.take() == [("header", None, g.align), ("launch", "compress", (wire, out, None), None, None)]
    # a record: the header without error buffers, the user's table in the descriptor, the dense decode always
    tables = []
    for out in (None, out_given, None):
        assert g.encode(tensors, wire, 1, SALT, (us, vs), 0.9, out=out) is True
        (_, errs, _), (_, name, args, _, _) = trace.take()
        assert errs is None and name == "record" and args[0] is wire and args[2] == 0.9 and type(args[2]) is float
        assert args[1] is (out_given if out is not None else g._ef_out) and args[1] is not None
        tables.append(g._batch.keep_state)
    tab = tables[0].view(len(sizes), 8)
    assert tables[1] is tables[0] and tables[2] is tables[0] and tables[0].dtype == torch.int64      # built once, never moved
    assert tab[:, 6].tolist() == [u.data_ptr() for u in us] and tab[:, 7].tolist() == [v.data_ptr() for v in vs]
    assert tab[:, 0].tolist() == [g._scratch.data_ptr() + 4 * o for o in g.out_off] and tab[:, 1].tolist() == sizes
    # state buffers that cannot be addressed: refused in front of the header
    strided = [torch.zeros(2 * n)[::2] for n in sizes]      # (a lone element is contiguous whatever its stride)
    for bad in ((us[:-1], vs[:-1]), ([u.double() for u in us], vs), (us, [torch.zeros(n + 1) for n in sizes]),
                (strided, vs))[:4 if len(sizes) > 1 else 3]:
        assert g.encode(tensors, wire, 1, SALT, bad, 0.9) is False
        assert trace.take() == []
    # upload (in front of an address-free graph's replay) declines a table it has not built
    assert g.upload(tensors, 1, (us, vs)) is True and trace.take() == [("upload", None)]
    assert g.upload(tensors, 1, None) is True and trace.take() == [("upload", None)]
    others = [torch.zeros(n) for n in sizes]
    assert g.upload(tensors, 1, (others, vs)) is False and trace.take() == []
    # under stream capture: a known table serves, a new one is an error that names the class
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert g.encode(tensors, wire, 1, SALT, (us, vs), 0.9) is True and g._batch.keep_state is tables[0]
    trace.take()
    with pytest.raises(RuntimeError, match="BatchedDGC: a state table is built by an eager record, not under stream capture"):
        g.encode(tensors, wire, 1, SALT, (others, vs), 0.9)
    assert trace.take() == []


@pytest.mark.parametrize("sizes", SHAPES, ids=["one", "two"])
def test_psgd_state(trace, monkeypatch, sizes):
    comp = lambda n: K.PowerSGDCompressor(n, (1, n), _args(psgd_rank=1, psgd_seed=3))
    cds = [C.PowerSGDCodec(comp(n), n, (1, n), param_index=i) for i, n in enumerate(sizes)]
    g, tensors, errs = _group(C.BatchedPowerSGD, cds)
    wire, out_given = _wire(), torch.zeros(g.out_floats)
    qs = [torch.zeros(cd.m * cd.rank) for cd in cds]
    with pytest.raises(ValueError, match="BatchedPowerSGD.encode: a record needs its user's warm starts"):
        g.encode(tensors, wire, 1, SALT, None, 0.5)
    assert trace.take() == []
    tables = []
    for ebufs, out in itertools.product((None, errs), (None, out_given)):
        assert g.encode(tensors, wire, 1, SALT, (ebufs, qs, 5), 0.5, out=out) is True
        # error feedback does not go through the dense decode: out stays what the caller gave
        assert trace.take() == [("header", ebufs, g.align), ("launch", "compress", (wire, out, 0.5 if ebufs is not None else None), None, None)]
        tables.append(g._batch.keep_state)
    assert all(t is tables[0] for t in tables) and tables[0].view(len(sizes), 2).tolist() == [[q.data_ptr(), 5] for q in qs]
    assert g.encode(tensors, wire, 1, SALT, (None, qs, 6), 0.5) is True and g._batch.keep_state is not tables[0]      # (the key holds the user)
    trace.take()
    strided = [torch.zeros(2 * q.numel())[::2] for q in qs]      # (a lone element is contiguous whatever its stride)
    for bad in ((None, qs[:-1], 5), (None, qs, native.PSGD_MAX_USERS), (None, qs, -1), (None, [q.double() for q in qs], 5),
                (None, [torch.zeros(q.numel() + 1) for q in qs], 5), (errs, strided, 5))[:6 if len(sizes) > 1 else 5]:
        assert g.encode(tensors, wire, 1, SALT, bad, 0.5) is False
        assert trace.take() == []
    assert g.upload(tensors, 1, (errs, qs, 5)) is True and trace.take() == [("upload", errs)]
    assert g.upload(tensors, 1, (None, qs, 7)) is False and g.upload(tensors, 1, None) is False and trace.take() == []
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert g.encode(tensors, wire, 1, SALT, (None, qs, 5), 0.5) is True and g._batch.keep_state is tables[0]
    trace.take()
    with pytest.raises(RuntimeError, match="BatchedPowerSGD: a state table is built by an eager record, not under stream capture"):
        g.encode(tensors, wire, 1, SALT, (None, qs, 8), 0.5)
    assert trace.take() == []


def test_graph_arguments_reach_the_launch(trace):
    g, tensors, errs = _group(C.BatchedSign, [KINDS["sign"][1](1)])
    header, defer = torch.zeros(8, dtype=torch.int64), []
    assert g.encode(tensors, _wire(), 0, SALT, errs, 0.25, graph_header=header, defer_reset=defer) is True
    (_, e, _), (_, name, args, graph_header, defer_reset) = trace.take()
    assert e is errs and name == "compress" and args[1:] == (None, 0.25) and graph_header is header and defer_reset is defer


def test_decode_keywords(trace):
    """decode_into hands the batch the plain, the stepped or the per-stream form, as the group's rotation and `own` say."""
    seen = []
    for kind, rotation in (("sign", None), ("drive", None), ("drive-step", torch.zeros((1, 2), dtype=torch.int64)), ("drive-own", None)):
        g, _, _ = _group(KINDS[kind][0], [KINDS[kind][1](1)])
        g.rotation = rotation if kind != "sign" else g.rotation
        g._batch.decode = lambda gathered, R, out, plain=False, **kw: seen.append(kw)
        g.decode_into(torch.zeros((1, 64), dtype=torch.uint8), 1, torch.zeros(4), plain=True)
        kw = seen.pop()
        if kind == "drive-own":
            assert kw == {"rotation": g.rotation, "first_stream": 0} and g.rotation is not None
        elif rotation is not None:
            assert list(kw) == ["rotation"] and kw["rotation"] is rotation
        else:
            assert kw == {}


WIRE_CODECS = ["stc", "sign", "thr", "maurey", "mx", "mx-nearest", "mxr", "drive", "eden"]


@pytest.mark.parametrize("kind", WIRE_CODECS)
def test_a_wire_of_one_element_is_never_empty(kind):
    cd = KINDS[kind][1](1)
    assert cd._wire_bytes() == cd.nbytes >= 16


def test_a_wire_of_the_smallest_low_rank_matrix_is_never_empty():
    for rank in (1, 2, 4):
        cd = C.PowerSGDCodec(K.PowerSGDCompressor(rank * rank, (rank, rank), _args(psgd_rank=rank, psgd_seed=0)), rank * rank, (rank, rank))
        assert cd._wire_bytes() == cd.nbytes >= 16


def test_top_k_alone_may_have_an_empty_section():
    """8 k bytes, and k may be 0: the one codec whose launches are handed a valid address that no section fills."""
    cd = KINDS["topk"][1](1)
    assert cd.nbytes == 8 and cd._wire_bytes() == 16
