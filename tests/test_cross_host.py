"""Gate-crossing maps, host side (no GPU): the definition
``cross.reference_cross`` on written-out segments and on the reference's own C1
history, the spec, the shared per-segment code csrc/cross_lines.h in a
stand-alone program under the sanitizers (crafted launches in all three row
layouts), and the argument checks of ``rwrt_ray_cross``."""
import ctypes
import math

import numpy as np
import pytest

import _hip as H
import cross as X
from cross import CrossSpec, Gate, reference_cross
from density import with_channels
from support import hostprog
from support.abi import refused
from support.cases_cross import (C1_GATES, GATES8, VARIANTS, assert_c1, assert_crafted_is_rich, assert_cross, c1_spec,
                                 crafted_spec, reference_and_abs)
from support.cases_track import NRAY, c1_rows, crafted_history, launches_of, rows_of
from support.rows import LAYOUTS, layout_text

TWO_PI = 2 * math.pi
INF, NAN = math.inf, math.nan


def one(rows, spec, chan=None):
    """reference_cross and the list of its crossings."""
    return reference_cross(rows, chan, spec), [x for x in X.crossings(rows, chan, spec)]


# ------------------------------------------------- written-out segments
def test_latitude_gate_segments():
    """Northward and southward with dyadic t, both ends on one side, a start
    exactly on the gate (t == -0.0, tc == i - 1) and an end exactly on it
    (which counts as north of it)."""
    spec = CrossSpec(Gate.lat(0.0), 8, weight="ug")
    rows = rows_of([(1.0, -0.25), (2.0, 0.75), (1.0, -0.25)])            # north at t = 1/4, south at t = 3/4
    rows[0, :, 5] = [2.0, 6.0, 2.0]
    r, xs = one(rows, spec)
    assert [(x[1], x[5], x[6], x[7], x[8]) for x in xs] == [(0, 1, 0.25, 0.25, 3.0), (1, 1, 0.75, 1.75, 3.0)]
    assert r["cnt"].shape == (1, 1, 2, 1, 8) and r["cnt"].sum() == 2 and r["cnt"][0, 0, :, 0, 1].tolist() == [1, 1]
    assert r["tsum"][0, 0, :, 0, 1].tolist() == [0.25, 1.75] and r["wsum"][0, 0, :, 0, 1].tolist() == [3.0, 3.0]
    assert r["ncross"][0, :, 0].tolist() == [1, 1] and r["tfirst"][0, :, 0].tolist() == [0.25, 1.75]
    assert r["dropped"] == 0
    # both ends on one side, either side
    r, xs = one(rows_of([(1.0, 0.25), (2.0, 0.75), (1.0, 1e-300), (0.0, 0.5)]), spec)
    assert xs == [] and r["cnt"].sum() == 0 and r["ncross"].sum() == 0 and np.isnan(r["tfirst"]).all()
    assert one(rows_of([(1.0, -0.25), (2.0, -0.75), (1.0, -1e-300)]), spec)[1] == []
    # a start exactly on the gate (it is north of it), going south: t == -0.0 and tc == i - 1
    r, xs = one(rows_of([(1.0, 0.5), (1.0, 0.0), (1.0, -0.5)]), spec)
    assert len(xs) == 1 and xs[0][1] == 1 and xs[0][6] == 0.0 and math.copysign(1.0, xs[0][6]) == -1.0
    assert xs[0][7] == 1.0 and r["tfirst"][0, 1, 0] == 1.0
    # an end exactly on the gate: crossed northward at t == 1.0, and not again on the way on
    r, xs = one(rows_of([(1.0, -0.5), (1.0, 0.0), (1.0, 0.5)]), spec)
    assert [(x[1], x[6], x[7]) for x in xs] == [(0, 1.0, 1.0)]
    # the longitude at the crossing is wrapped: lon_c = -0.5 falls into the last bin, 13 into bin 0
    assert [x[5] for x in one(rows_of([(-0.5, -1.0), (-0.5, 1.0)]), spec)[1]] == [7]
    assert [x[5] for x in one(rows_of([(13.0, -1.0), (13.0, 1.0)]), spec)[1]] == [0]
    # lon = 1e300 is a finite longitude: the crossing is in a bin
    r, xs = one(rows_of([(1.0, -0.25), (1e300, 0.75)]), spec)
    assert len(xs) == 1 and 0 <= xs[0][5] < 8 and r["cnt"].sum() == 1


def test_meridian_gate_segments():
    """Eastward at pos + 2 pi and westward at pos, a start exactly on the
    meridian moving west, |m1 - m0| == 2 and lon = 1e300 (both dropped), and a
    crossing outside lat_range (per ray only)."""
    spec = CrossSpec(Gate.lon(90.0), 6, lat_range=(-30.0, 60.0), weight="ug")
    pos = math.pi / 2
    assert spec.gates[0].pos == pos
    r, xs = one(rows_of([(pos + TWO_PI - 0.25, 0.1), (pos + TWO_PI + 0.75, 0.5)]), spec)
    assert len(xs) == 1 and xs[0][1] == 0 and abs(xs[0][6] - 0.25) < 4e-15 and abs(xs[0][7] - 0.25) < 4e-15
    lat_c = 0.1 + xs[0][6] * (0.5 - 0.1)
    assert xs[0][5] == math.floor((lat_c - spec.lat0) * spec.inv_dlat) == 2 and r["cnt"][0, 0, 0, 0, 2] == 1
    r, xs = one(rows_of([(0.5, 0.0), (-0.5, 0.0)]), CrossSpec(Gate.lon(0.0), 6))   # westward at lon 0 itself
    assert [(x[1], x[5], x[6], x[7]) for x in xs] == [(1, 3, 0.5, 0.5)]
    assert [(x[1], x[6]) for x in one(rows_of([(pos + 0.5, 0.0), (pos - 0.5, 0.0)]), spec)[1]] == [(1, 0.5)]
    # a start exactly on a meridian (east of it), moving west: t == -0.0
    r, xs = one(rows_of([(1.0, 0.0), (0.0, 0.0), (-0.5, 0.0)]), CrossSpec(Gate.lon(0.0), 6))
    assert len(xs) == 1 and xs[0][1] == 1 and xs[0][6] == 0.0 and math.copysign(1.0, xs[0][6]) == -1.0
    assert xs[0][7] == 1.0
    # two circles in one segment, and lon = 1e300 on both sides: dropped, nothing else
    r, xs = one(rows_of([(pos + 0.5, 0.0), (pos + 0.5 + 2 * TWO_PI, 0.0)]), spec)
    assert xs == [None] and r["dropped"] == 1 and r["cnt"].sum() == 0 and r["ncross"].sum() == 0
    r, xs = one(rows_of([(0.5, 0.0), (1e300, 0.0), (0.5, 0.0)]), spec)
    assert xs == [None, None] and r["dropped"] == 2 and r["ncross"].sum() == 0 and np.isnan(r["tfirst"]).all()
    # outside lat_range: counted per ray, not in the map
    r, xs = one(rows_of([(pos - 0.5, 1.2), (pos + 0.5, 1.2)]), spec)
    assert len(xs) == 1 and xs[0][5] == -1 and r["cnt"].sum() == 0 and r["tsum"].sum() == 0.0
    assert r["ncross"][0, :, 0].tolist() == [1, 0] and r["tfirst"][0, 0, 0] == 0.5 and r["dropped"] == 0
    r, xs = one(rows_of([(pos - 0.5, -0.6), (pos + 0.5, -0.6)]), spec)
    assert xs[0][5] == -1 and r["cnt"].sum() == 0 and r["ncross"].sum() == 1


def test_invalid_rows_channels_and_windows():
    """NaN in the need column makes both neighbouring segments vanish; a ray
    with a channel outside [0, nchan) is not walked; windows of 2 rows."""
    spec = CrossSpec((Gate.lat(0.0), Gate.lon(0.0)), 4, window_rows=2, nt=6, nchan=2)
    pts = [(0.5, -0.5), (0.5, 0.5), (0.5, -0.5), (-0.5, -0.5), (0.5, -0.5), (0.5, 0.5)]
    rows = np.concatenate([rows_of(pts)] * 3)
    r, xs = one(rows, spec, [0, 1, 1])
    assert r["cnt"].shape == (3, 2, 2, 2, 4)
    assert r["cnt"][:, 0].sum(axis=(2, 3)).tolist() == [[3, 3], [0, 0], [3, 0]]     # gate 0, 3 rays: N, S | - | N
    assert r["cnt"][:, 1].sum(axis=(2, 3)).tolist() == [[0, 0], [3, 3], [0, 0]]     # gate 1: west then east, window 1
    assert r["cnt"][..., 0, :].sum() * 2 == r["cnt"][..., 1, :].sum()
    assert r["ncross"][0].tolist() == [[2, 2, 2], [1, 1, 1]] and r["tfirst"][0, 0].tolist() == [0.5, 0.5, 0.5]
    hole = rows.copy()
    hole[:, 1, 4] = NAN                                 # the amplitude of row 1: segments 1 and 2 are not considered
    r, xs = one(hole, spec, [0, 1, 1])
    assert r["ncross"][0].tolist() == [[1, 1, 1], [0, 0, 0]] and r["tfirst"][0, 0].tolist() == [4.5, 4.5, 4.5]
    assert one(hole, with_channels(CrossSpec(spec.gates, 4, need=None), 2), [0, 1, 1])[0]["ncross"][0, 0, 0] == 2
    r, xs = one(rows, spec, [0, 2, -1])
    assert r["ncross"][:, :, 1:].sum() == 0 and np.isnan(r["tfirst"][:, :, 1:]).all() and r["ncross"][0, 0, 0] == 2
    assert r["cnt"][..., 1, :].sum() == 0 and r["cnt"].sum() == 5 and len(xs) == 5
    with pytest.raises(ValueError):
        reference_cross(np.concatenate([rows, rows], axis=1), None, spec)          # 12 rows, 3 windows of 2
    with pytest.raises(ValueError):
        reference_cross(np.zeros((3, 4)), None, spec)
    with pytest.raises(ValueError):
        reference_cross(rows, [0, 1], spec)


# ---------------------------------------------------------------- the spec
def test_spec():
    assert ctypes.sizeof(H.CrossGateC) == 32 and ctypes.sizeof(H.CrossMapC) == 288 and X.MAXGATE == 8
    assert Gate.lat(30) == Gate(0, 30.0) and Gate.lon(-90) == Gate(1, 270.0) and Gate.lon(360).deg == 0.0
    assert Gate.lat(90).pos == math.pi / 2 and Gate.lon(180).pos == math.pi
    s = CrossSpec(Gate.lat(30), 360)
    assert s.gates == (Gate.lat(30),) and s.shape == (1, 1, 2, 1, 360) and (s.ncol, s.wcol, s.nwin) == (4, -1, 1)
    assert s.axis(0) == (0.0, 360 / TWO_PI)
    u = CrossSpec([Gate.lat(-20), Gate.lon(120)], 36, lat_range=(-60, 60), nchan=3, need=None, weight="ug",
                  window_rows=120, nt=1081)
    assert u.nwin == 9 and u.shape == (9, 2, 2, 3, 36) and (u.ncol, u.wcol) == (-1, 5)
    assert CrossSpec(Gate.lat(0), 4, window_rows=120, nt=1082).nwin == 10
    assert u.axis(1) == (-math.pi / 3, 36 / (math.pi / 3 - -math.pi / 3))
    c = u.c_struct()
    assert (c.ngate, c.nbin, c.nchan, c.need, c.wcol, c.window_rows, c.nwin, c.reserved) == (2, 36, 3, -1, 5, 120, 9, 0)
    assert (c.gate[0].kind, c.gate[0].pos, c.gate[0].org, c.gate[0].inv_d) == (0, math.pi * (-20 / 180), 0.0,
                                                                               36 / TWO_PI)
    assert (c.gate[1].kind, c.gate[1].pos, c.gate[1].org, c.gate[1].inv_d) == (1, math.pi * (120 / 180), u.lat0,
                                                                               u.inv_dlat)
    assert with_channels(u, 7).nchan == 7 and with_channels(u, 7).gates == u.gates
    with pytest.raises(Exception):
        u.nbin = 3                                       # frozen
    g = Gate.lat(0)
    for bad in (dict(gates=()), dict(gates=(g,) * 9), dict(gates=(0.0,)), dict(nbin=0), dict(nchan=0),
                dict(lat_range=(10.0, 10.0)), dict(need="lon"), dict(weight="speed"), dict(window_rows=-1),
                dict(window_rows=2.5, nt=9), dict(window_rows=4), dict(window_rows=4, nt=1),
                dict(nbin=2 ** 20, nchan=2 ** 10)):
        with pytest.raises(ValueError):
            CrossSpec(**{**dict(gates=(g,), nbin=7), **bad})
    for bad in ((0, 91.0), (0, NAN), (1, INF), (1, 360.0), (1, -1.0), (2, 0.0)):
        with pytest.raises(ValueError):
            Gate(*bad)


def test_reference_cross_c1_history():
    rows = c1_rows()
    r = reference_cross(rows, np.arange(3), c1_spec(nchan=3))
    assert_c1(r)
    xs = list(X.crossings(rows, np.arange(3), c1_spec(nchan=3)))
    assert len(xs) == 132 + 134 + 18 and None not in xs
    assert all(0.0 <= x[6] <= 1.0 for x in xs if x[0] < 2)            # (-0.0 among them)
    assert all(x[5] >= 0 for x in xs)
    # one channel and no windows: the same crossings
    flat = reference_cross(rows, None, CrossSpec(C1_GATES, 36, weight="amp"))
    assert np.array_equal(flat["cnt"][0, :, :, 0], r["cnt"].sum(axis=(0, 3)))
    assert np.array_equal(flat["ncross"], r["ncross"]) and np.array_equal(flat["tfirst"], r["tfirst"], equal_nan=True)
    assert flat["wsum"][0, 0].sum() > 0 and r["wsum"] is None


# ------------------------------------------- csrc/cross_lines.h on the host
host_program = hostprog.fixture("cross_lines")


def run_host_program(exe, spec, launches, nray=NRAY):
    c = spec.c_struct()
    lines = [f"{c.ngate} {c.nbin} {c.nchan} {c.need} {c.wcol} {c.window_rows} {c.nwin}"]
    for g in range(c.ngate):
        q = c.gate[g]
        lines.append(f"{q.kind} " + " ".join(float(x).hex() for x in (q.pos, q.org, q.inv_d)))
    lines.append(str(len(launches)))
    for L, layout in launches:
        lines += layout_text(L, layout)
    out = hostprog.run(exe, lines)
    floats = lambda s: np.array([float.fromhex(x) if "nan" not in x else NAN for x in s.split()])   # noqa: E731
    cnt = np.array(out[0].split(), np.int64).reshape(spec.shape)
    tsum, wsum = floats(out[1]).reshape(spec.shape), floats(out[2]).reshape(spec.shape)
    per_ray = (spec.ngate, 2, nray)
    return {"cnt": cnt, "tsum": tsum, "wsum": wsum if spec.wcol >= 0 else None, "dropped": int(out[3].split()[1]),
            "ncross": np.array(out[4].split(), np.int32).reshape(per_ray), "tfirst": floats(out[5]).reshape(per_ray)}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_lines_host_program_under_sanitizers(host_program, name):
    """csrc/cross_lines.h (what the kernel calls) in a stand-alone program built
    with ASan + UBSan and run directly: row 0, then a launch [1, 8) with
    tail_from below, at, inside, at the end of and above it and rays without a
    row block, in all three row layouts: cnt, ncross and dropped equal
    reference_cross, tfirst bit for bit, tsum and wsum agree to the bound."""
    spec = crafted_spec(name, 8)
    h = crafted_history(8, seed=3)
    assert {-1, 1, 8, 11} <= set(h["tf"].tolist()) and {-1, 3} <= set(h["chan"].tolist())
    want, a = reference_and_abs(h["rows"], h["chan"], spec)
    if spec.ngate == 8:
        assert_crafted_is_rich(h["rows"], h["chan"], spec)
        assert spec.nwin == 3 or spec.window_rows == 0
    assert want["ncross"].sum() > 5
    off = ~((h["chan"] >= 0) & (h["chan"] < 3))
    assert off.any() and want["ncross"][:, :, off].sum() == 0
    for layout in LAYOUTS:
        got = run_host_program(host_program, spec, launches_of(h, [(1, 8)], layout))
        print(f"{name} {layout}: {want['ncross'].sum()} crossings, {want['cnt'].sum()} in the map, "
              f"{want['dropped']} dropped")
        assert_cross(got, want, a, (name, layout))


@pytest.mark.parametrize("layout", ["dense", "tails", "slots"])
def test_lines_host_program_launches_combine(host_program, layout):
    """Launches [1, 4) and [4, 8) with the carried row give what one launch
    [1, 8) gives; two more, [8, 9) and [9, 30), go on from there."""
    name = "8-gates-weight-windows"
    h = crafted_history(30, seed=4, tf=np.where(np.arange(NRAY) % 3 == 0, 1, 30))   # rays without a block: all tail
    first = dict(h, rows=h["rows"][:, :8])
    spec8 = crafted_spec(name, 8)
    want, a = reference_and_abs(first["rows"], h["chan"], spec8)
    assert want["ncross"].sum() > 50
    one_, two = (run_host_program(host_program, spec8, launches_of(first, b, layout))
                 for b in ([(1, 8)], [(1, 4), (4, 8)]))
    assert_cross(one_, want, a, layout)
    assert_cross(two, want, a, layout + " in two launches")
    spec30 = crafted_spec(name, 30)
    assert spec30.nwin == 10
    got = run_host_program(host_program, spec30, launches_of(h, [(1, 4), (4, 8), (8, 9), (9, 30)], layout))
    want, a = reference_and_abs(h["rows"], h["chan"], spec30)
    assert_cross(got, want, a, layout + " four launches")
    assert want["cnt"][3:].sum() > 0


# ----------------------------------------------------------- C entry point
def _call(lib, m, nray=16, i0=1, i1=5, rows=64, slot=None, tfrom=None, trow=None, ray=None, ncols=16, chan=None,
          prev=64, cnt=64, tsum=64, wsum=None, dropped=64, ncross=64, tfirst=64):
    """rwrt_ray_cross with fake (never dereferenced) device pointers."""
    return lib.rwrt_ray_cross(None if m is None else ctypes.byref(m), nray, i0, i1, rows, slot, tfrom, trow, ray,
                              ncols, chan, prev, cnt, tsum, wsum, dropped, ncross, tfirst, None)


def test_cross_argument_errors_without_a_gpu():
    """Every check happens before any HIP call and names the argument."""
    lib = H.load()
    assert "rwrt_ray_cross" in H.ABI_SYMBOLS
    assert "abi 5" in H.version()                      # an additive member: the version stays
    spec = CrossSpec((Gate.lat(30.0), Gate.lon(180.0)), 7, nchan=2, lat_range=(-60.0, 60.0), window_rows=2, nt=9)
    good = spec.c_struct()

    def m(gate=None, **kw):
        c = spec.c_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        for g, fields in (gate or {}).items():
            for k, v in fields.items():
                setattr(c.gate[g], k, v)
        return c

    cases = [
        (dict(m=None), b"map"),
        (dict(m=m(ngate=0)), b"ngate"), (dict(m=m(ngate=9)), b"ngate"), (dict(m=m(ngate=-1)), b"ngate"),
        (dict(m=m(nbin=0)), b"nbin"), (dict(m=m(nchan=-1)), b"nchan"),
        (dict(m=m(nbin=1 << 20, nchan=1 << 10)), b"2^31"), (dict(m=m(nwin=1 << 30, window_rows=1)), b"2^31"),
        (dict(m=m(nbin=(1 << 31) - 1, nchan=(1 << 31) - 1)), b"2^31"),
        (dict(m=m(gate={0: dict(kind=2)})), b"kind"), (dict(m=m(gate={1: dict(kind=-1)})), b"kind"),
        (dict(m=m(gate={0: dict(pos=NAN)})), b"pos"), (dict(m=m(gate={1: dict(pos=INF)})), b"pos"),
        (dict(m=m(gate={1: dict(org=NAN)})), b"org"), (dict(m=m(gate={1: dict(org=-INF)})), b"org"),
        (dict(m=m(gate={0: dict(inv_d=0.0)})), b"inv_d"), (dict(m=m(gate={1: dict(inv_d=-1.0)})), b"inv_d"),
        (dict(m=m(gate={1: dict(inv_d=INF)})), b"inv_d"), (dict(m=m(gate={0: dict(inv_d=NAN)})), b"inv_d"),
        (dict(m=m(gate={0: dict(org=0.5)})), b"org"),                      # a latitude circle bins over longitude
        (dict(m=m(gate={1: dict(pos=-0.1)})), b"pos"), (dict(m=m(gate={1: dict(pos=TWO_PI)})), b"pos"),
        (dict(m=m(need=0)), b"need"), (dict(m=m(need=1)), b"need"), (dict(m=m(need=7)), b"need"),
        (dict(m=m(need=-2)), b"need"),
        (dict(m=m(wcol=0), wsum=64), b"wcol"), (dict(m=m(wcol=7), wsum=64), b"wcol"), (dict(m=m(wcol=-2)), b"wcol"),
        (dict(m=m(window_rows=-1)), b"window_rows"), (dict(m=m(nwin=0)), b"nwin"),
        (dict(m=m(window_rows=0)), b"nwin"),                                # no windows and nwin = 4
        (dict(m=good, i0=5, i1=10), b"window_rows"),                        # row 9 is past 4 windows of 2 rows
        (dict(m=good, i0=5, i1=5), b"it_begin"), (dict(m=good, i0=6, i1=5), b"it_begin"),
        (dict(m=good, i0=-1, i1=3), b"it_begin"),
        (dict(m=good, slot=64), b"d_row_slot"),
        (dict(m=good, tfrom=64), b"d_tail_row"), (dict(m=good, trow=64), b"d_tail_from"),
        (dict(m=good, rows=None), b"d_rows"),
        (dict(m=good, nray=-1), b"nray"), (dict(m=good, nray=1 << 31), b"nray"),
        (dict(m=good, rows=72), b"16-byte"), (dict(m=good, tfrom=64, trow=72), b"16-byte"),
        (dict(m=good, ncols=15), b"nacc_cols"), (dict(m=good, ncols=-1, ray=64), b"nacc_cols"),
        (dict(m=good, ncols=1 << 31, ray=64), b"nacc_cols"),
        (dict(m=good, prev=None), b"d_prev"), (dict(m=good, cnt=None), b"d_cnt"), (dict(m=good, tsum=None), b"d_tsum"),
        (dict(m=good, dropped=None), b"d_dropped"),
        (dict(m=good, wsum=64), b"d_wsum"), (dict(m=m(wcol=5)), b"d_wsum"),
        (dict(m=good, ncross=None), b"d_ncross"), (dict(m=good, tfirst=None), b"d_tfirst"),
    ]
    for kw, word in cases:
        refused(lib, _call, kw, word, b"rwrt_ray_cross: ")
    # the output pointers are checked with no rays too
    assert _call(lib, good, nray=0, rows=None, cnt=None) == H.RWRT_ERR_ARG
    # no rays: a no-op (no device is touched; there is none on the build host)
    assert _call(lib, good, nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, good, nray=0, rows=None, ncols=0) == H.RWRT_OK
    assert _call(lib, good, nray=0, rows=None, ncross=None, tfirst=None) == H.RWRT_OK        # maps only
    assert _call(lib, good, nray=0, rows=None, i0=8, i1=9) == H.RWRT_OK                      # the last row of window 3
    assert _call(lib, m(wcol=5), nray=0, rows=None, wsum=64) == H.RWRT_OK
    assert _call(lib, m(need=-1, window_rows=0, nwin=1), nray=0, rows=None, i0=100, i1=200) == H.RWRT_OK
    big = CrossSpec(GATES8, 360, nchan=12, weight="amp", window_rows=120, nt=1081).c_struct()
    assert _call(lib, big, nray=0, rows=None, wsum=64) == H.RWRT_OK
