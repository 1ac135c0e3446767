"""Residence-time maps along ray segments, host side (no GPU): the definition
``track.reference_track`` on written-out segments and on the reference's own C1
history, its conservation of the row interval, the shared walk
csrc/track_cells.h in a stand-alone program under the sanitizers (crafted
launches in all three row layouts), and the argument checks of
``rwrt_ray_track``."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import _hip as H
import track as T
from support import hostprog
from support.abi import refused
from support.cases_track import (C1_TRACK, NRAY, VARIANTS, abs_sums, assert_track, c1_rows, crafted_history,
                                 launches_of, rows_of)
from support.rows import LAYOUTS, layout_text
from track import TrackSpec, reference_track, segment_cells

TWO_PI = 2 * math.pi
INF, NAN = math.inf, math.nan


# ------------------------------------------------------------ the walk itself
SMALL_CASES = [
    ((0, 0, 3, 3), [(0, 0, "1/3"), (1, 0, 0), (1, 1, "1/3"), (2, 1, 0), (2, 2, "1/3"), (3, 2, 0), (3, 3, 0)]),
    ((3, 3, 0, 0), [(3, 3, 0), (2, 3, 0), (2, 2, "1/3"), (1, 2, 0), (1, 1, "1/3"), (0, 1, 0), (0, 0, "1/3")]),
    ((0.5, 2, 4.5, 2), [(0, 2, "1/8"), (1, 2, "1/4"), (2, 2, "1/4"), (3, 2, "1/4"), (4, 2, "1/8")]),
    ((5, 1.5, 3, 1.5), [(5, 1, 0), (4, 1, "1/2"), (3, 1, "1/2")]),
    ((3.5, 1.5, 5, 1.5), [(3, 1, "1/3"), (4, 1, "2/3"), (5, 1, 0)]),
    ((-0.5, 0.5, 0.5, -0.5), [(-1, 0, "1/2"), (0, 0, 0), (0, -1, "1/2")]),
]


@pytest.mark.parametrize("case", SMALL_CASES, ids=[str(c[0]) for c in SMALL_CASES])
def test_segment_cells_small_cases(case):
    """The six written-out segments of the definition: the cells in order and
    their weights (thirds to one rounding of a quotient and a difference, the
    dyadic ones exactly)."""
    (X0, Y0, X1, Y1), want = case
    got = segment_cells(float(X0), float(Y0), float(X1), float(Y1), 100)
    assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in want]
    for (_, _, w), (_, _, f) in zip(got, want):
        f = Fraction(f)
        if f.denominator in (1, 2, 4, 8):
            assert w == float(f)
        else:
            assert abs(w - float(f)) <= 2.0 ** -52
    assert abs(sum(w for _, _, w in got) - 1.0) <= len(got) * 2.0 ** -52
    assert all(0.0 <= w <= 1.0 for _, _, w in got)


def test_segment_cells_inside_one_cell_and_drops():
    assert segment_cells(1.5, 1.5, 1.5, 1.5, 1) == [(1, 1, 1.0)]
    assert segment_cells(1.25, 1.75, 1.75, 1.25, 1) == [(1, 1, 1.0)]
    assert segment_cells(0.5, 0.5, 1.5, 0.5, 1) is None and len(segment_cells(0.5, 0.5, 1.5, 0.5, 2)) == 2
    assert segment_cells(0.5, 0.5, 3.5, 2.5, 5) is None and len(segment_cells(0.5, 0.5, 3.5, 2.5, 6)) == 6
    assert segment_cells(1e300, 0.5, 0.5, 0.5, 10 ** 9) is None and segment_cells(0.5, 0.5, 0.5, -INF, 9) is None
    assert segment_cells(2.0 ** 30 + 1.5, 0.5, 2.0 ** 30 + 1.5, 0.5, 9) is None
    assert segment_cells(2.0 ** 30 + 0.5, 0.5, 2.0 ** 30 + 0.5, 0.5, 9) == [(2 ** 30, 0, 1.0)]
    assert segment_cells(-2.0 ** 30, 0.5, -2.0 ** 30, 0.5, 9) == [(-2 ** 30, 0, 1.0)]
    assert segment_cells(-2.0 ** 30 - 0.5, 0.5, 0.5, 0.5, 2 ** 31) is None


def test_segment_cells_random_weights():
    """Random and half-integer segments: the weights lie in [0, 1], sum to 1
    within ncells 2^-52, and the walk ends in the cell of the end point."""
    rng = np.random.default_rng(0)
    for _ in range(20000):
        a = rng.uniform(-8, 8, 4)
        if rng.random() < 0.3:
            a = np.round(a * 2) / 2
        c = segment_cells(*map(float, a), 100)
        ws = [w for _, _, w in c]
        assert min(ws) >= 0.0 and max(ws) <= 1.0 and abs(sum(ws) - 1.0) <= len(ws) * 2.0 ** -52
        assert c[0][:2] == (math.floor(a[0]), math.floor(a[1])) and c[-1][:2] == (math.floor(a[2]), math.floor(a[3]))
        assert all(abs(p[0] - q[0]) + abs(p[1] - q[1]) == 1 for p, q in zip(c, c[1:]))


# ---------------------------------------------------------------- the spec
def test_spec():
    s = TrackSpec(1440, 720)
    assert (s.lon0, s.inv_dlon, s.mode, s.ncol, s.wcol, s.cells) == (0.0, 1440 / TWO_PI, 0, 4, -1, 2160)
    assert (s.lat0, s.inv_dlat) == (-math.pi / 2, 720 / math.pi) and s.shape == (1, 720, 1440) and s.circles is None
    u = TrackSpec(4320, 720, lon_range=(-360, 720), nchan=3, need=None, weight="ug", max_cells=50)
    assert u.lon0 == -2 * math.pi and u.lon1 == 4 * math.pi and u.inv_dlon == 4320 / (u.lon1 - u.lon0)
    assert (u.mode, u.ncol, u.wcol, u.cells, u.circles) == (2, -1, 5, 50, 3)
    c = u.c_struct()
    assert (c.nx, c.ny, c.nchan, c.mode, c.need, c.wcol, c.max_cells, c.reserved, c.lon0, c.inv_dlon, c.lat0,
            c.inv_dlat) == (4320, 720, 3, 2, -1, 5, 50, 0, u.lon0, u.inv_dlon, u.lat0, u.inv_dlat)
    assert ctypes.sizeof(H.TrackMapC) == 64
    for bad in (dict(nx=0), dict(ny=-1), dict(nchan=0), dict(nx=65536, ny=32768), dict(lat_range=(10.0, 10.0)),
                dict(lon_range=(10.0, 10.0)), dict(lon_range=(20.0, 10.0)), dict(lon_range=(0.0, INF)),
                dict(lon_range=(NAN, 10.0)), dict(need="lon"), dict(weight="speed"), dict(max_cells=0),
                dict(max_cells=2.5), dict(max_cells=2 ** 31)):
        with pytest.raises(ValueError):
            TrackSpec(**{**dict(nx=7, ny=5), **bad})
    with pytest.raises(ValueError):
        reference_track(np.zeros((3, 4)), None, s)
    with pytest.raises(ValueError):
        reference_track(np.zeros((3, 4, 8)), [0, 1], s)


@pytest.mark.parametrize("shape", sorted(C1_TRACK))
def test_reference_track_c1_history(shape):
    """The reference's own 90-day C1 history: two live rays of 1080 segments
    each (root 0 is a dead slot: NaN amplitude) deposit 2160 row intervals at
    every resolution; the number of cells is the literal of the definition."""
    rows = c1_rows()
    nseg, ndrop, ncell, total = C1_TRACK[shape]
    spec = TrackSpec(*shape)
    r = reference_track(rows, None, spec)
    ok = T.valid_rows(rows, spec)
    assert int((ok[:, 1:] & ok[:, :-1]).sum()) == nseg
    assert r["dropped"] == ndrop and r["cnt"].sum() == ncell and r["wsum"] is None
    assert abs(r["time"].sum() - total) <= ncell * 2.0 ** -52 * 2 and abs(r["time"].sum() - total) < 1e-9
    by_root = reference_track(rows, np.arange(3), TrackSpec(*shape, nchan=3, weight="amp"))
    assert by_root["cnt"].sum(axis=(1, 2))[0] == 0 and by_root["cnt"].sum() == ncell
    assert np.array_equal(by_root["cnt"].sum(axis=0), r["cnt"][0])
    assert np.all(np.abs(by_root["time"].sum(axis=(1, 2))[1:] - 1080.0) < 1e-9)
    # need = None lets the dead slot in: it rests at its source, 1080 segments of weight 1 in one cell
    loose = reference_track(rows, np.arange(3), TrackSpec(*shape, nchan=3, need=None))
    assert loose["cnt"][0].sum() == 1080 and loose["time"][0].max() == 1080.0 and np.count_nonzero(loose["cnt"][0]) == 1


# ------------------------------------------------------ hand-made segments
def grid_to_rad(spec, X, Y):
    return X / spec.inv_dlon + spec.lon0, Y / spec.inv_dlat + spec.lat0


def scalar_track(rows, chan, spec):
    """The definition of the issue, written independently of
    ``track.deposits``: segment by segment with ``segment_cells``."""
    cnt = np.zeros(spec.shape, np.int64)
    time = np.zeros(spec.shape)
    wsum = np.zeros(spec.shape)
    dropped = considered = 0
    for j in range(rows.shape[0]):
        c = 0 if chan is None else int(chan[j])
        if not 0 <= c < spec.nchan:
            continue
        for i in range(1, rows.shape[1]):
            a, b = rows[j, i - 1], rows[j, i]
            cols = [0, 1] + [q for q in (spec.ncol, spec.wcol) if q >= 0]
            if not all(math.isfinite(a[q]) and math.isfinite(b[q]) for q in cols):
                continue
            considered += 1
            with np.errstate(all="ignore"):
                P = [float((r[0] - spec.lon0) * spec.inv_dlon) for r in (a, b)]
                Q = [float((r[1] - spec.lat0) * spec.inv_dlat) for r in (a, b)]
            seg = segment_cells(P[0], Q[0], P[1], Q[1], spec.cells)
            if seg is None:
                dropped += 1
                continue
            vm = 0.5 * (a[spec.wcol] + b[spec.wcol]) if spec.wcol >= 0 else 0.0
            for ix, iy, w in seg:
                if not 0 <= iy < spec.ny or (spec.unwrapped and not 0 <= ix < spec.nx):
                    continue
                cnt[c, iy, ix % spec.nx] += 1
                time[c, iy, ix % spec.nx] += w
                wsum[c, iy, ix % spec.nx] += w * vm
    return {"cnt": cnt, "time": time, "wsum": wsum if spec.wcol >= 0 else None, "dropped": dropped}, considered


def assert_same(got, want, what=""):
    assert np.array_equal(got["cnt"], want["cnt"]) and got["dropped"] == want["dropped"], what
    assert np.array_equal(got["time"], want["time"]), what
    assert (got["wsum"] is None) == (want["wsum"] is None), what
    if want["wsum"] is not None:
        assert np.array_equal(got["wsum"], want["wsum"]), what


def test_hand_made_segments():
    """Westward and southward, on a grid line, through a node, starting on a
    node, across longitude 0 both ways, out of the latitude range and back, out
    of an unwrapped window, a NaN hole, a dead-slot row with and without
    ``need``, ``lon = 1e300`` and a jump above ``max_cells``."""
    spec = TrackSpec(8, 4, weight="ug")                # dlon = 45 degrees, dlat = 45 degrees
    dx, dy = 1.0 / spec.inv_dlon, 1.0 / spec.inv_dlat
    lat = lambda Y: spec.lat0 + Y * dy                # noqa: E731
    # westward and southward: (5.5, 2.5) -> (3.5, 1.5) crosses x = 5, y = 2 and x = 4
    r = reference_track(rows_of([(5.5 * dx, lat(2.5)), (3.5 * dx, lat(1.5))]), None, spec)
    assert r["cnt"].sum() == 4 and r["dropped"] == 0 and abs(r["time"].sum() - 1.0) < 1e-15
    assert r["cnt"][0, 2, 5] == 1 and r["cnt"][0, 1, 3] == 1 and abs(r["wsum"].sum() - 2.0) < 1e-14
    # on a grid line (Y = 2 exactly, binned into row 2), eastward: columns 0..4
    r = reference_track(rows_of([(0.5 * dx, lat(2.0)), (4.5 * dx, lat(2.0))]), None, spec)
    assert r["cnt"][0, 2].tolist() == [1, 1, 1, 1, 1, 0, 0, 0] and r["cnt"].sum() == 5
    assert np.allclose(r["time"][0, 2, :5], [0.125, 0.25, 0.25, 0.25, 0.125], rtol=0, atol=2e-16)
    # starting on a node and going through nodes: the diagonal
    r = reference_track(rows_of([(0.0, lat(0.0)), (3.0 * dx, lat(3.0))]), None, spec)
    assert r["cnt"].sum() == 7 and r["cnt"][0, 0, 0] == 1 and r["cnt"][0, 3, 3] == 1 and r["cnt"][0, 0, 1] == 1
    assert abs(r["time"].sum() - 1.0) <= 7 * 2.0 ** -52 and r["time"][0, 0, 1] == 0.0
    # across longitude 0, westward then eastward: column -1 is column nx - 1
    east = reference_track(rows_of([(-0.5 * dx, lat(1.5)), (0.5 * dx, lat(1.5))]), None, spec)
    west = reference_track(rows_of([(0.5 * dx, lat(1.5)), (-0.5 * dx, lat(1.5))]), None, spec)
    for r in (east, west):
        assert r["cnt"][0, 1].tolist() == [1, 0, 0, 0, 0, 0, 0, 1] and r["time"][0, 1, 0] == 0.5 == r["time"][0, 1, 7]
    far = reference_track(rows_of([(-8.5 * dx, lat(1.5)), (-9.5 * dx, lat(1.5))]), None, spec)   # one circle west
    assert far["cnt"][0, 1].tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    # out of the latitude range and back: the cells above row ny - 1 are not deposited, the time there is lost
    r = reference_track(rows_of([(1.5 * dx, lat(3.5)), (1.5 * dx, lat(4.5)), (1.5 * dx, lat(3.5))]), None, spec)
    assert r["cnt"].sum() == 2 and r["cnt"][0, 3, 1] == 2 and abs(r["time"].sum() - 1.0) < 1e-15
    # out of an unwrapped window: what a wrapped map folds back is dropped there
    win = TrackSpec(8, 4, lon_range=(0.0, 360.0), weight="ug")
    r = reference_track(rows_of([(6.5 * dx, lat(1.5)), (9.5 * dx, lat(1.5))]), None, win)
    assert r["cnt"][0, 1].tolist() == [0, 0, 0, 0, 0, 0, 1, 1] and abs(r["time"].sum() - 0.5) < 1e-15
    r = reference_track(rows_of([(6.5 * dx, lat(1.5)), (9.5 * dx, lat(1.5))]), None, spec)
    assert r["cnt"][0, 1].tolist() == [1, 1, 0, 0, 0, 0, 1, 1] and abs(r["time"].sum() - 1.0) < 1e-15
    # a NaN hole: the segments on both sides vanish
    pts = [(0.5 * dx, lat(0.5)), (1.5 * dx, lat(0.5)), (NAN, lat(0.5)), (3.5 * dx, lat(0.5)), (4.5 * dx, lat(0.5))]
    r = reference_track(rows_of(pts), None, spec)
    assert r["cnt"][0, 0].tolist() == [1, 1, 0, 1, 1, 0, 0, 0] and abs(r["time"].sum() - 2.0) < 1e-15
    # a dead-slot row (NaN amplitude) with need = 'amp' and with need = None; a NaN weight is a hole too
    rows = rows_of(pts[:2] + [(2.5 * dx, lat(0.5))] + pts[3:])
    rows[0, 2, 4] = NAN
    assert reference_track(rows, None, spec)["cnt"].sum() == 4
    loose = reference_track(rows, None, TrackSpec(8, 4, need=None, weight="ug"))
    assert loose["cnt"][0, 0].tolist() == [1, 2, 2, 2, 1, 0, 0, 0] and abs(loose["time"].sum() - 4.0) < 1e-15
    rows[0, 2, 4], rows[0, 2, 5] = 1.0, INF
    assert reference_track(rows, None, spec)["cnt"].sum() == 4
    assert reference_track(rows, None, TrackSpec(8, 4))["cnt"].sum() == 8
    # lon = 1e300 (finite: a valid row) and a jump above max_cells: dropped, nothing deposited
    r = reference_track(rows_of([(0.5 * dx, lat(0.5)), (1e300, lat(0.5)), (0.5 * dx, lat(0.5))]), None, spec)
    assert r["dropped"] == 2 and r["cnt"].sum() == 0 and r["time"].sum() == 0.0 and r["wsum"].sum() == 0.0
    jump = rows_of([(0.5 * dx, lat(0.5)), (12.5 * dx, lat(0.5)), (13.5 * dx, lat(1.5))])      # 13 cells > 12
    r = reference_track(jump, None, spec)
    assert r["dropped"] == 1 and r["cnt"].sum() == 3
    assert reference_track(jump, None, TrackSpec(8, 4, max_cells=13))["dropped"] == 0
    assert reference_track(jump, None, TrackSpec(8, 4, max_cells=2))["dropped"] == 2
    # a ray with a channel outside [0, nchan) contributes nothing, not even a drop
    off = reference_track(jump, [1], spec)
    assert off["cnt"].sum() == 0 and off["dropped"] == 0


def test_conservation_on_a_whole_globe_map():
    """Whole-globe wrapped maps lose nothing: ``time.sum()`` is the number of
    considered, non-dropped segments within cells 2^-52 and ``cnt.sum()`` the
    number of deposited cells -- at every resolution, for the same rays."""
    h = crafted_history(40, seed=12, nray=24, tf=np.full(24, 40))
    rows = h["rows"]
    rows[..., 1] = np.clip(rows[..., 1], -1.55, 1.55)            # (inf stays a hole; nothing leaves +-90 degrees)
    rows[:, :, 1][np.isinf(h["rows"][..., 1])] = INF
    seen = set()
    for nx, ny in ((7, 5), (64, 32), (360, 180)):
        spec = TrackSpec(nx, ny, nchan=3, weight="ug")
        r = reference_track(rows, h["chan"], spec)
        scalar, considered = scalar_track(rows, h["chan"], spec)
        assert_same(r, scalar, (nx, ny))
        kept = considered - r["dropped"]
        cells = sum(1 for d in T.deposits(rows, h["chan"], spec) if d is not None)
        assert kept > 300 and r["cnt"].sum() == cells and cells >= kept
        assert abs(r["time"].sum() - kept) <= cells * 2.0 ** -52
        seen.add((considered, cells))
    assert len({c for c, _ in seen}) == 1 and len({n for _, n in seen}) == 3


# ------------------------------------------- csrc/track_cells.h on the host
host_program = hostprog.fixture("track_cells")


def run_host_program(exe, spec, launches):
    c = spec.c_struct()
    lines = [f"{c.nx} {c.ny} {c.nchan} {c.mode} {c.need} {c.wcol} {c.max_cells} " + " ".join(
        float(x).hex() for x in (c.lon0, c.inv_dlon, c.lat0, c.inv_dlat)), str(len(launches))]
    for L, layout in launches:
        lines += layout_text(L, layout)
    out = hostprog.run(exe, lines)
    cnt = np.array(out[0].split(), np.int64).reshape(spec.shape)
    time, wsum = (np.array([float.fromhex(x) for x in out[q].split()]).reshape(spec.shape) for q in (1, 2))
    dropped, flushes = int(out[3].split()[1]), int(out[4].split()[1])
    return {"cnt": cnt, "time": time, "wsum": wsum if spec.wcol >= 0 else None, "dropped": dropped}, flushes


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_walk_host_program_under_sanitizers(host_program, name):
    """csrc/track_cells.h (what the kernel calls) in a stand-alone program built
    with ASan + UBSan and run directly: row 0, then a launch [1, 8) with
    tail_from below, at, inside, at the end of and above it and rays without a
    row block, in all three row layouts: cnt and dropped equal
    reference_track, time and wsum agree to the bound."""
    spec = TrackSpec(7, 5, nchan=3, **VARIANTS[name])
    h = crafted_history(8, seed=3)
    assert {-1, 1, 8, 11} <= set(h["tf"].tolist()) and {-1, 3} <= set(h["chan"].tolist())
    want = reference_track(h["rows"], h["chan"], spec)
    scalar, considered = scalar_track(h["rows"], h["chan"], spec)
    assert_same(want, scalar, name)
    a = abs_sums(h["rows"], h["chan"], spec)
    assert want["cnt"].sum() > 50 and np.count_nonzero(want["cnt"]) > 15 and 0 < want["dropped"] < considered
    for layout in LAYOUTS:
        got, flushes = run_host_program(host_program, spec, launches_of(h, [(1, 8)], layout))
        print(f"{name} {layout}: {want['cnt'].sum()} cells, {flushes} flushes, {want['dropped']} dropped")
        assert_track(got, want, a, (name, layout))
        assert 0 < flushes <= want["cnt"].sum()


@pytest.mark.parametrize("layout", ["dense", "tails", "slots"])
def test_walk_host_program_launches_combine(host_program, layout):
    """Launches [1, 4) and [4, 8) with the carried row give what one launch
    [1, 8) gives; two more, [8, 9) and [9, 30), go on from there."""
    spec = TrackSpec(7, 5, nchan=3, weight="ug")
    h = crafted_history(30, seed=4, tf=np.where(np.arange(NRAY) % 3 == 0, 1, 30))   # rays without a block: all tail
    first = dict(h, rows=h["rows"][:, :8])
    want = reference_track(first["rows"], h["chan"], spec)
    a = abs_sums(first["rows"], h["chan"], spec)
    assert want["cnt"].sum() > 100
    one, f1 = run_host_program(host_program, spec, launches_of(first, [(1, 8)], layout))
    two, f2 = run_host_program(host_program, spec, launches_of(first, [(1, 4), (4, 8)], layout))
    assert_track(one, want, a, layout)
    assert_track(two, want, a, layout + " in two launches")
    assert f1 <= f2 <= f1 + NRAY                                        # (a launch's end flushes the run)
    got, _ = run_host_program(host_program, spec, launches_of(h, [(1, 4), (4, 8), (8, 9), (9, 30)], layout))
    assert_track(got, reference_track(h["rows"], h["chan"], spec), abs_sums(h["rows"], h["chan"], spec),
                 layout + " four launches")


def test_walk_host_program_a_ray_at_rest_flushes_once(host_program):
    """Rays at rest for 999 rows, all tail or all read: one flush per
    deposited ray -- not one per row -- of 999 visits and a time of 999.0; a
    ray resting at lon = 1e300 drops its 999 segments."""
    spec = TrackSpec(7, 5, nchan=3, weight="ug")
    h = crafted_history(1000, seed=8, tf=np.full(NRAY, 1))
    h["tail"][10, 0] = 1e300
    h["rows"] = np.repeat(h["tail"][:, None], 1000, axis=1)
    want = reference_track(h["rows"], h["chan"], spec)
    a = abs_sums(h["rows"], h["chan"], spec)
    live = int(want["cnt"].sum()) // 999
    assert want["cnt"].sum() == live * 999 and 10 < live < NRAY and np.all(want["cnt"] % 999 == 0)
    assert want["dropped"] == (999 if 0 <= h["chan"][10] < 3 else 0)
    assert np.array_equal(want["time"], want["cnt"].astype(np.float64))
    for layout in ("tails", "slots", "dense"):
        hh = h if layout != "dense" else dict(h, tf=np.full(NRAY, 1000))
        got, flushes = run_host_program(host_program, spec, launches_of(hh, [(1, 1000)], layout))
        assert_track(got, want, a, layout)
        assert flushes == live, layout


# ----------------------------------------------------------- C entry point
def _call(lib, m, nray=16, i0=1, i1=5, rows=64, slot=None, tfrom=None, trow=None, ray=None, ncols=16, chan=None,
          prev=64, cnt=64, time=64, wsum=None, dropped=64):
    """rwrt_ray_track with fake (never dereferenced) device pointers."""
    return lib.rwrt_ray_track(None if m is None else ctypes.byref(m), nray, i0, i1, rows, slot, tfrom, trow, ray,
                              ncols, chan, prev, cnt, time, wsum, dropped, None)


def test_track_argument_errors_without_a_gpu():
    """Every check happens before any HIP call and names the argument."""
    lib = H.load()
    assert ctypes.sizeof(H.TrackMapC) == 64
    assert "abi 5" in H.version()                      # an additive member: the version stays
    spec = TrackSpec(7, 5, nchan=2, lon_range=(-360.0, 720.0))
    good = spec.c_struct()

    def m(**kw):
        c = spec.c_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    cases = [
        (dict(m=None), b"map"),
        (dict(m=m(nx=0)), b"nx"), (dict(m=m(ny=-1)), b"ny"), (dict(m=m(nchan=0)), b"nchan"),
        (dict(m=m(nx=65536, ny=32768, nchan=1)), b"2^31"), (dict(m=m(nx=1 << 20, ny=1 << 10, nchan=2)), b"2^31"),
        (dict(m=m(mode=1)), b"mode"), (dict(m=m(mode=3)), b"mode"), (dict(m=m(mode=4)), b"mode"),
        (dict(m=m(mode=-1)), b"mode"),
        (dict(m=m(max_cells=0)), b"max_cells"), (dict(m=m(max_cells=-5)), b"max_cells"),
        (dict(m=m(need=0)), b"need"), (dict(m=m(need=1)), b"need"), (dict(m=m(need=7)), b"need"),
        (dict(m=m(need=-2)), b"need"),
        (dict(m=m(wcol=0), wsum=64), b"wcol"), (dict(m=m(wcol=1), wsum=64), b"wcol"),
        (dict(m=m(wcol=7), wsum=64), b"wcol"), (dict(m=m(wcol=-2)), b"wcol"),
        (dict(m=m(inv_dlon=0.0)), b"inv_dlon"), (dict(m=m(inv_dlon=-1.0)), b"inv_dlon"),
        (dict(m=m(inv_dlon=INF)), b"inv_dlon"), (dict(m=m(inv_dlon=NAN)), b"inv_dlon"),
        (dict(m=m(inv_dlat=0.0)), b"inv_dlat"), (dict(m=m(inv_dlat=NAN)), b"inv_dlat"),
        (dict(m=m(inv_dlat=INF)), b"inv_dlat"), (dict(m=m(lat0=NAN)), b"lat0"), (dict(m=m(lat0=-INF)), b"lat0"),
        (dict(m=m(lon0=NAN)), b"lon0"), (dict(m=m(lon0=INF)), b"lon0"),
        (dict(m=m(mode=0)), b"lon0"),                                       # wrapped with lon0 = -2 pi
        (dict(m=good, i0=5, i1=5), b"it_begin"), (dict(m=good, i0=6, i1=5), b"it_begin"),
        (dict(m=good, i0=-1, i1=3), b"it_begin"),
        (dict(m=good, slot=64), b"d_row_slot"),
        (dict(m=good, tfrom=64), b"d_tail_row"), (dict(m=good, trow=64), b"d_tail_from"),
        (dict(m=good, rows=None), b"d_rows"),
        (dict(m=good, nray=-1), b"nray"), (dict(m=good, nray=1 << 31), b"nray"),
        (dict(m=good, rows=72), b"16-byte"), (dict(m=good, tfrom=64, trow=72), b"16-byte"),
        (dict(m=good, ncols=15), b"nacc_cols"), (dict(m=good, ncols=-1, ray=64), b"nacc_cols"),
        (dict(m=good, ncols=1 << 31, ray=64), b"nacc_cols"),
        (dict(m=good, prev=None), b"d_prev"), (dict(m=good, cnt=None), b"d_cnt"), (dict(m=good, time=None), b"d_time"),
        (dict(m=good, dropped=None), b"d_dropped"),
        (dict(m=good, wsum=64), b"d_wsum"), (dict(m=m(wcol=5)), b"d_wsum"),
    ]
    for kw, word in cases:
        refused(lib, _call, kw, word, b"rwrt_ray_track: ")
    # the output pointers are checked with no rays too
    assert _call(lib, good, nray=0, rows=None, cnt=None) == H.RWRT_ERR_ARG
    # no rays: a no-op (no device is touched; there is none on the build host)
    assert _call(lib, good, nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, good, nray=0, rows=None, ncols=0) == H.RWRT_OK
    assert _call(lib, m(wcol=5), nray=0, rows=None, wsum=64) == H.RWRT_OK
    assert _call(lib, m(need=-1, max_cells=1), nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, m(mode=0, lon0=0.0), nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, TrackSpec(1440, 720, nchan=3, weight="amp").c_struct(), nray=0, rows=None, wsum=64) == H.RWRT_OK
