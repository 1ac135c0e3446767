"""A launch's rows, host side (no GPU): csrc/launch_rows.h walking the three
layouts in a stand-alone program under the sanitizers, and launch_rows.py --
the sinks' call forms, shard cache and ``take`` against a recording fake, and
the dispatcher ``deliver``."""
import numpy as np
import pytest
import torch

import launch_rows
from arrival import ArrivalSink
from cross import CrossSink
from density import DensitySink
from engine import deliver
from flux import FluxSink
from summary import SummarySink
from support import hostprog
from track import TrackSink

# the six sinks: a channel per ray (None stays None), or a column per ray (None: idx itself)
CHANNEL_SINKS = {"density": DensitySink, "arrival": ArrivalSink, "flux": FluxSink}
COLUMN_SINKS = {"summary": SummarySink, "track": TrackSink, "cross": CrossSink}
SINKS = {**CHANNEL_SINKS, **COLUMN_SINKS}

NRAY, I0, I1, NOUT = 16, 3, 10, 8          # 7 rows: one batch of 4 and a remainder of 3
NROWS = I1 - I0
# below, at and above the launch; rows read: 0 0 1 3 4 5 7 7 | 7 7 5 4 1 0 0 3
TAIL_FROM = np.array([1, 3, 4, 6, 7, 8, 10, 12, 12, 10, 8, 7, 4, 3, 1, 6], np.int32)
NO_BLOCK = (3, 4, 7, 10, 13)               # a third of the rays; 3, 4 and 10 with tail_from inside the launch
GARBAGE = -777.0                           # buffer rows a ray's tail replaces: never to be read


def layouts():
    """``{name: (logical, tf, program input)}``: the logical rows ``[16, 7, 8]``
    of each layout, each ray's first tail row, and the arrays as the program
    reads them.  Row buffers end with the last row some ray reads."""
    live = 1000.0 * np.arange(NRAY)[:, None, None] + 10.0 * np.arange(I0, I1)[None, :, None] + np.arange(NOUT)
    tail = 1000.0 * np.arange(NRAY)[:, None] + 500.0 + np.arange(NOUT)
    row = np.arange(I0, I1)[None, :, None]
    out = {"dense": (live, np.full(NRAY, I1), [f"0 {NRAY} {I0} {I1} {live.size}", _fmt(live)])}
    tf = np.clip(TAIL_FROM, I0, I1)
    # tails: ray 15, the last of the buffer, reads 3 rows and the buffer ends there
    buf = np.where(row < tf[:, None, None], live, GARBAGE).reshape(-1)[:(15 * NROWS + 3) * NOUT]
    out["tails"] = (np.where(row < tf[:, None, None], live, tail[:, None, :]), tf,
                    [f"1 {NRAY} {I0} {I1} {buf.size}", _fmt(TAIL_FROM), _fmt(buf), _fmt(tail)])
    # row blocks: the rays with one, in a permuted order that ends with ray 15
    have = [j for j in range(NRAY) if j not in NO_BLOCK]
    order = [have[k] for k in np.random.default_rng(4).permutation(len(have) - 1)] + [15]
    slot = np.full(NRAY, -1, np.int32)
    slot[order] = np.arange(len(order))
    tfs = np.where(slot < 0, I0, tf)
    blocks = np.where(row < tfs[:, None, None], live, GARBAGE)[order].reshape(-1)[:(len(order) * NROWS - 4) * NOUT]
    out["slots"] = (np.where(row < tfs[:, None, None], live, tail[:, None, :]), tfs,
                    [f"2 {NRAY} {I0} {I1} {blocks.size}", _fmt(TAIL_FROM), _fmt(slot), _fmt(blocks), _fmt(tail)])
    return out


def _fmt(a):
    return " ".join(repr(v) for v in np.asarray(a).reshape(-1).tolist())


@pytest.mark.parametrize("name", ["dense", "tails", "slots"])
def test_walk_host_program_under_sanitizers(tmp_path, name):
    """csrc/launch_rows.h (what both kernels call) at BATCH 4 in a stand-alone
    program built with ASan + UBSan + float-cast-overflow and run directly:
    every ray's rows come in order -- the rows read, then one tail of the right
    length -- and equal the logical rows built here."""
    exe = hostprog.build("launch_rows", tmp_path)
    logical, tf, lines = layouts()[name]
    nread = tf - I0
    assert name == "dense" or sorted(set(nread.tolist())) == [0, 1, 3, 4, 5, 7]
    out = hostprog.run(exe, lines)
    want = []
    for j in range(NRAY):
        want += [("R", j, i, logical[j, i - I0, 0], logical[j, i - I0, 7]) for i in range(I0, int(tf[j]))]
        if tf[j] < I1:
            want.append(("T", j, int(tf[j]), I1 - int(tf[j]), logical[j, -1, 0], logical[j, -1, 7]))
    got = [(w[0],) + tuple(int(x) for x in w[1:-2]) + (float(w[-2]), float(w[-1]))
           for w in (ln.split() for ln in out)]
    assert got == want
    # the same as rows: the walk reproduces the logical rows, and nothing else
    rows = np.full((NRAY, NROWS, 2), np.nan)
    for g in got:
        if g[0] == "R":
            rows[g[1], g[2] - I0] = g[3:]
        else:
            rows[g[1], g[2] - I0:g[2] - I0 + g[3]] = g[4:]
    assert np.array_equal(rows, logical[:, :, [0, 7]])
    assert GARBAGE not in rows


# ------------------------------------------------------------ launch_rows.py
class FakeTarget:
    """Stands in for a DensityMap / RaySummary: records every add_rows call."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def _chan(self, chan, n):
        return torch.as_tensor(chan).to(torch.int32)

    def _ray(self, ray, n):
        return torch.as_tensor(ray).to(torch.int64)

    def add_rows(self, i0, i1, view, tails=None, slots=None, per_ray=None):
        self.calls.append((i0, i1, view, tails, slots, per_ray))


def _same_call(got, i0, i1, view, tails, slots, per_ray):
    assert got[:2] == (i0, i1) and got[2] is view and got[3] is tails and got[4] is slots
    if per_ray is None:
        assert got[5] is None
    else:
        assert got[5].dtype == per_ray.dtype and torch.equal(got[5], per_ray)


@pytest.mark.parametrize("kind", list(SINKS))
@pytest.mark.parametrize("with_attr", [False, True])
def test_every_call_form_reaches_add_rows(kind, with_attr):
    t = FakeTarget()
    attr = [5, 6, 7, 8, 9, 10] if with_attr else None
    sink = SINKS[kind](t, attr)
    dt = torch.int32 if kind in CHANNEL_SINKS else torch.int64
    whole = None if attr is None else torch.tensor(attr, dtype=dt)
    assert sink.takes_tails and sink.takes_slots
    assert (sink.chan if kind in CHANNEL_SINKS else sink.ray) is sink.per_ray
    assert (sink.summary if kind == "summary" else sink.map) is t
    view, tails, slots = "view", "tails", "slots"        # (passed through untouched)
    forms = [((), {}, None, None), ((tails,), {}, tails, None), ((tails, slots), {}, tails, slots),
             ((), dict(tails=tails), tails, None), ((), dict(tails=tails, slots=slots), tails, slots),
             ((None, None), {}, None, None)]
    for rest, kw, want_t, want_s in forms:
        sink(1, 5, view, *rest, **kw)
        _same_call(t.calls[-1], 1, 5, view, want_t, want_s, whole)
    # the sharded form: idx as a tensor and as a NumPy array
    for idx in (torch.tensor([4, 0, 2]), np.array([1, 5])):
        cols = torch.as_tensor(idx).to(torch.int64)
        if kind in CHANNEL_SINKS:
            sub = None if whole is None else whole[cols]
        else:
            sub = cols if whole is None else whole[cols]
        for rest, kw, want_t, want_s in forms:
            sink(1, 5, view, idx, *rest, **kw)
            _same_call(t.calls[-1], 1, 5, view, want_t, want_s, sub)


@pytest.mark.parametrize("kind", list(SINKS))
def test_shard_cache_is_keyed_by_the_idx_object(kind):
    t = FakeTarget()
    sink = SINKS[kind](t, [5, 6, 7, 8])
    idx = torch.tensor([2, 0])
    sink(1, 5, "v", idx)
    sink(6, 9, "v", idx, "tails")
    assert t.calls[0][5] is t.calls[1][5] and sink._sub[0] is idx        # reused
    assert t.calls[0][5].tolist() == [7, 5] and t.calls[0][5].is_contiguous()
    same_values = idx.clone()
    sink(1, 5, "v", same_values)
    assert t.calls[2][5] is not t.calls[1][5] and sink._sub[0] is same_values   # rebuilt for a new object
    assert t.calls[2][5].tolist() == [7, 5]
    sink(1, 5, "v")                                                        # the plain form: every ray
    assert t.calls[3][5] is sink.per_ray and sink._sub[0] is same_values


def test_take_composes():
    t = FakeTarget()
    d = DensitySink(t, [5, 6, 7, 8, 9]).take([4, 1, 0]).take(torch.tensor([2, 0]))
    assert isinstance(d, DensitySink) and d.map is t and d.chan.tolist() == [5, 9] and d._sub == (None, None)
    assert DensitySink(t).take([1, 0]).chan is None                       # density: None stays None
    s = SummarySink(t).take([4, 1, 0])                                    # summary: None means idx itself
    assert isinstance(s, SummarySink) and s.ray.dtype == torch.int64 and s.ray.tolist() == [4, 1, 0]
    assert s.take([2, 2]).ray.tolist() == [0, 0]
    assert SummarySink(t, [5, 6, 7]).take(np.array([2, 0])).ray.tolist() == [7, 5]
    whole = SummarySink(t, [5, 6, 7])
    part = whole.take([1])
    part(1, 5, "v", torch.tensor([0]))
    assert whole._sub == (None, None) and whole.ray.tolist() == [5, 6, 7]  # take leaves the sink it came from
    for kind, cls in SINKS.items():                                       # each of the six keeps its class
        took = cls(t, [5, 6, 7, 8, 9]).take([4, 1, 0]).take(torch.tensor([2, 0]))
        assert type(took) is cls and took.target is t and took.per_ray.tolist() == [5, 9] and took._sub == (None, None)
        assert not any(issubclass(cls, other) for other in SINKS.values() if other is not cls)   # distinct classes
        none = cls(t).take([1, 0]).per_ray
        assert none is None if kind in CHANNEL_SINKS else none.tolist() == [1, 0]


class FakeEngine:
    def __init__(self):
        self.expanded = []

    def expand(self, view, tails, i0, i1):
        self.expanded.append((view, tails, i0, i1))


class FakeSlots:
    def __init__(self):
        self.calls = []

    def dense(self, view, tails, i0, i1, out=None):
        self.calls.append((view, tails, i0, i1, out))
        return ("dense", len(self.calls))


def _recorder(**attrs):
    calls = []

    def sink(*a, **k):
        calls.append((a, k))
    for k, v in attrs.items():
        setattr(sink, k, v)
    return sink, calls


@pytest.mark.parametrize("idx", [None, "idx"])
def test_deliver_gives_each_sink_the_layout_it_takes(idx):
    ids = () if idx is None else (idx,)
    kw = {} if idx is None else dict(idx=idx)
    assert deliver is launch_rows.deliver
    # a plain sink: tails expanded into the view ...
    eng, (plain, calls) = FakeEngine(), _recorder()
    deliver(eng, plain, 1, 5, "view", "tails", **kw)
    assert eng.expanded == [("view", "tails", 1, 5)] and calls == [((1, 5, "view") + ids, {})]
    # ... row blocks made dense, the buffer kept for the next launch
    slots, scratch = FakeSlots(), {}
    deliver(eng, plain, 1, 5, "blocks", "tails", slots, scratch=scratch, **kw)
    deliver(eng, plain, 5, 9, "blocks", "tails", slots, scratch=scratch, **kw)
    assert slots.calls == [("blocks", "tails", 1, 5, None), ("blocks", "tails", 5, 9, ("dense", 1))]
    assert calls[1:] == [((1, 5, ("dense", 1)) + ids, {}), ((5, 9, ("dense", 2)) + ids, {})]
    assert len(eng.expanded) == 1                       # (dense rows have no tails left to expand)
    # dense rows from the launch itself go as they are
    deliver(eng, plain, 1, 5, "view", None, **kw)
    assert calls[-1] == ((1, 5, "view") + ids, {}) and len(eng.expanded) == 1
    # a sink that takes tails only
    eng, slots, (ts, calls) = FakeEngine(), FakeSlots(), _recorder(takes_tails=True)
    deliver(eng, ts, 1, 5, "view", "tails", **kw)
    deliver(eng, ts, 1, 5, "blocks", "tails", slots, **kw)
    assert calls == [((1, 5, "view") + ids + ("tails",), {}), ((1, 5, ("dense", 1)) + ids, {})]
    assert eng.expanded == [] and len(slots.calls) == 1
    # a sink that takes both
    eng, slots, (full, calls) = FakeEngine(), FakeSlots(), _recorder(takes_tails=True, takes_slots=True)
    deliver(eng, full, 1, 5, "blocks", "tails", slots, **kw)
    deliver(eng, full, 1, 5, "view", "tails", **kw)
    deliver(eng, full, 1, 5, "view", None, **kw)
    assert calls == [((1, 5, "blocks") + ids + ("tails", slots), {}), ((1, 5, "view") + ids + ("tails",), {}),
                     ((1, 5, "view") + ids, {})]
    assert eng.expanded == [] and slots.calls == []


def test_row_args_checks_shapes_before_any_pointer():
    class T:
        def __init__(self, n):
            self.frm = self.slot = torch.zeros(n, dtype=torch.int32)

    view = torch.zeros((3, 4, 8), dtype=torch.float64)
    with pytest.raises(ValueError, match="row slots need tails"):
        launch_rows.row_args(1, 5, view, None, T(3))
    with pytest.raises(ValueError, match="rows must be"):
        launch_rows.row_args(1, 6, view)
    with pytest.raises(ValueError, match="rows must be"):
        launch_rows.row_args(1, 5, view[..., :7])
    with pytest.raises(ValueError, match="tails of 2 rays for 3 rays"):
        launch_rows.row_args(1, 5, view, T(2))
    with pytest.raises(ValueError, match="tails of 3 rays for 5 rays"):
        launch_rows.row_args(1, 5, view, T(3), T(5))
    rows = launch_rows.one_row({0: [1.0, 2.0, 3.0], 3: np.array([[4.0], [5.0], [6.0]])}, "cpu")
    assert rows.shape == (3, 1, 8) and rows.dtype == torch.float64
    assert rows[:, 0, 0].tolist() == [1.0, 2.0, 3.0] and rows[:, 0, 3].tolist() == [4.0, 5.0, 6.0]
    assert rows[:, 0, [1, 2, 4, 5, 6, 7]].abs().sum() == 0
