"""Arrival-time maps, host side (no GPU): the NumPy definition
``arrival.reference_arrival`` against a point-by-point loop and on the
reference's own C1 history, the shared per-ray walk csrc/arrival_rows.h in a
stand-alone program under the sanitizers (crafted launches in all three row
layouts), and the argument checks of ``rwrt_ray_arrival``."""
import ctypes
import math

import numpy as np
import pytest

import _hip as H
from arrival import INT32_MAX, ArrivalSpec, reference_arrival
from conftest import golden
from density import DensitySpec, reference_bins
from support import hostprog
from support.abi import refused
from support.cases_density import corner_points, random_points, scalar_bin
from support.rows import LAYOUTS, layout_text, no_block

INF, NAN = math.inf, math.nan


def scalar_arrival(lon, lat, req, chan, spec, row0=0):
    """The definition of the issue, point by point in Python."""
    first = np.full(spec.shape, -1, np.int32)
    last = np.full(spec.shape, -1, np.int32)
    count = None if spec.window_rows is None else np.zeros(spec.count_shape, np.int64)
    for j in range(lon.shape[0]):
        for r in range(lon.shape[1]):
            b = scalar_bin(float(lon[j, r]), float(lat[j, r]), float(req[j, r]), int(chan[j]), spec.bins)
            if b is None:
                continue
            i = row0 + r
            first[b] = i if first[b] < 0 else min(first[b], i)
            last[b] = max(last[b], i)
            if count is not None:
                count[(i // spec.window_rows,) + b] += 1
    return {"first": first, "last": last, "count": count}


def assert_same(got, want, what=""):
    for k in ("first", "last"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k)
    if want["count"] is None:
        assert got["count"] is None, what
    else:
        assert got["count"].dtype == np.int64 and np.array_equal(got["count"], want["count"]), (what, "count")


def test_spec():
    s = ArrivalSpec(1440, 720, nt=1081, nchan=3, window_rows=12)
    assert s.nwin == 91 and s.count_shape == (91, 3, 720, 1440) and s.require == "amp"
    assert s.bins == DensitySpec(1440, 720, nchan=3, weight="amp")
    c = s.c_struct()
    assert (c.bins.nx, c.bins.ny, c.bins.nchan, c.bins.wcol, c.window_rows, c.nwin) == (1440, 720, 3, 4, 12, 91)
    assert c.bins.inv_dlon == s.bins.inv_dlon and c.bins.lat0 == s.bins.lat0
    n = ArrivalSpec(7, 5, nt=8, require=None)
    assert (n.nwin, n.bins.wcol, n.c_struct().window_rows, n.c_struct().nwin) == (0, -1, 0, 0)
    assert ArrivalSpec(7, 5, nt=8, window_rows=3).nwin == 3 and ArrivalSpec(7, 5, nt=9, window_rows=3).nwin == 3
    assert ArrivalSpec(7, 5, nt=8, window_rows=100).nwin == 1
    for bad in (dict(nx=0), dict(nt=0), dict(window_rows=0), dict(window_rows=-2), dict(require="nacc"),
                dict(nchan=0), dict(lat_range=(10.0, 10.0)),
                dict(nx=1440, ny=720, nt=1081, nchan=2, window_rows=1)):     # 2.2e9 counts
        with pytest.raises(ValueError):
            ArrivalSpec(**{**dict(nx=7, ny=5, nt=8), **bad})
    assert ctypes.sizeof(H.ArrivalMap) == 48


@pytest.mark.parametrize("require", ["amp", None])
@pytest.mark.parametrize("window_rows", [None, 1, 3])
def test_reference_arrival_against_the_scalar_definition(require, window_rows):
    pts = corner_points()
    nrow, row0 = 4, 2
    spec = ArrivalSpec(7, 5, nt=row0 + 20, nchan=2, require=require, window_rows=window_rows)
    lon, lat, w = (np.repeat(np.array([p[k] for p in pts])[:, None], nrow, axis=1) for k in range(3))
    chan = np.array([p[3] for p in pts])
    got = reference_arrival(lon, lat, w, chan, spec, row0=row0)
    assert_same(got, scalar_arrival(lon, lat, w, chan, spec, row0), "corner points")
    # written out: the 15 binned points (18 without the requirement) stay nrow rows each
    visited = got["first"] >= 0
    assert np.array_equal(visited, got["last"] >= 0)
    assert set(got["first"][visited].tolist()) == {row0} and set(got["last"][visited].tolist()) == {row0 + nrow - 1}
    if window_rows is not None:
        assert got["count"].sum() == (15 if require else 18) * nrow
    rl, rt, rw, rc = random_points(4000, spec.bins, seed=5)
    lon, lat, w, chan = rl.reshape(200, 20), rt.reshape(200, 20), rw.reshape(200, 20), rc[:200]
    got = reference_arrival(lon, lat, w, chan, spec, row0=row0)
    want = scalar_arrival(lon, lat, w, chan, spec, row0)
    assert_same(got, want, "random")
    assert (want["first"] >= 0).sum() > 30 and (want["last"] > want["first"]).any()
    with pytest.raises(ValueError):
        reference_arrival(lon, lat, w, chan, spec, row0=row0 + 1)      # a row past spec.nt


def c1_points():
    hist = golden("traj_C1.npz")["hist"]              # (7, 1081, 3)
    return hist[0].T, hist[1].T, hist[4].T            # [3, 1081] each


@pytest.mark.parametrize("nx,ny", [(1440, 720), (144, 72), (7, 5)])
def test_reference_arrival_c1_history(nx, ny):
    """The reference's own 90-day C1 history, one channel per root, 12-row
    (one-day) windows: the literals pin the definition to reference data."""
    lon, lat, amp = c1_points()
    chan = np.arange(3)
    for require in ("amp", None):
        spec = ArrivalSpec(nx, ny, nt=1081, nchan=3, require=require, window_rows=12)
        assert spec.nwin == 91
        a = reference_arrival(lon, lat, amp, chan, spec)
        first, last, count = a["first"], a["last"], a["count"]
        assert count.sum(axis=(0, 2, 3)).tolist() == ([0, 1081, 1081] if require else [1081, 1081, 1081])
        assert (count.sum(axis=(1, 2, 3)) > 0).all()                       # all 91 windows
        assert count.sum(axis=(1, 2, 3)).tolist() == ([24] * 90 + [2] if require else [36] * 90 + [3])
        dens = reference_bins(lon, lat, amp, chan[:, None], DensitySpec(nx, ny, nchan=3, weight=require))[0]
        assert np.array_equal(count.sum(axis=0), dens)
        visited = first >= 0
        assert np.array_equal(visited, dens > 0) and np.array_equal(visited, last >= 0)
        assert (first[visited] <= last[visited]).all() and (last[~visited] == -1).all()
        nvis = visited.sum(axis=(1, 2)).tolist()
        if (nx, ny) == (1440, 720):
            assert nvis == ([0, 1077, 1075] if require else [1, 1077, 1075])
        if (nx, ny) == (144, 72) and require:
            assert nvis == [0, 671, 707]
        if (nx, ny) == (7, 5) and require:
            assert nvis == [0, 7, 7] and first.max() == 119
        if require is None:
            assert first[0].max() == 0 and last[0].max() == 1080           # the dead root slot never moves
        # without windows: the same bounds, no counts
        b = reference_arrival(lon, lat, amp, chan, ArrivalSpec(nx, ny, nt=1081, nchan=3, require=require))
        assert b["count"] is None and np.array_equal(b["first"], first) and np.array_equal(b["last"], last)


# ------------------------------------------------ csrc/arrival_rows.h on the host
host_program = hostprog.fixture("arrival_rows")
NRAY = 41


def crafted_launch(i0, i1, seed, tf=None):
    """Logical rows ``[NRAY, i1 - i0, 8]`` of a launch ``[i0, i1)`` that all
    three layouts can hold: ray j's rows from ``tf[j]`` on repeat its tail row.
    ``tf`` runs through values below, at, inside, at the end of and above the
    launch; the j % 3 == 0 rays (no row block in the slots layout) have at most
    i0.  Every fourth ray drifts slowly (bin runs across window bounds), the
    others jump from bin to bin; some tails are NaN or have a non-finite
    amplitude."""
    rng = np.random.default_rng(seed)
    nrow = i1 - i0
    rows = rng.uniform(-3.0, 3.0, (NRAY, nrow, 8))
    rows[..., 0] = rng.uniform(-70.0, 70.0, (NRAY, nrow))
    rows[..., 1] = rng.uniform(-1.8, 1.8, (NRAY, nrow))
    slow = np.arange(NRAY) % 4 == 1
    rows[slow, :, 0] = rng.uniform(0.0, 6.0, (slow.sum(), 1)) + 0.05 * np.arange(nrow)
    rows[slow, :, 1] = rng.uniform(-1.0, 1.0, (slow.sum(), 1))
    rows[3, nrow // 2, 4] = NAN                                  # a hole in a run
    rows[7, 0, 0] = INF
    tail = rng.uniform(-3.0, 3.0, (NRAY, 8))
    tail[:, 0] = rng.uniform(-70.0, 70.0, NRAY)
    tail[:, 1] = rng.uniform(-1.8, 1.8, NRAY)
    tail[5::7, 0] = NAN
    tail[6::11, 4] = INF
    if tf is None:
        choice = sorted({i0 - 2, i0, i0 + 1, i0 + 3, i0 + 4, i0 + 5, i1 - 1, i1, i1 + 3})
        j = np.arange(NRAY)
        k = np.cumsum(j % 3 != 0)                                 # (the rays with a block take every value)
        tf = np.where(j % 3 == 0, np.array([i0 - 2, i0])[(j // 3) % 2], np.array(choice)[k % len(choice)])
    tf = np.asarray(tf, np.int32)
    cut = np.clip(tf, i0, i1)
    for j in range(NRAY):
        rows[j, cut[j] - i0:] = tail[j]
    # a slow ray whose tail continues its last bin: the run goes on into the tail
    for j in np.where(slow)[0]:
        if i0 < cut[j] < i1:
            tail[j] = rows[j, cut[j] - i0 - 1]
            rows[j, cut[j] - i0:] = tail[j]
    chan = rng.integers(-1, 4, NRAY).astype(np.int32)            # -1 and nchan = 3 among them
    return dict(i0=i0, i1=i1, rows=rows, tail=tail, tf=tf, chan=chan)


def run_host_program(exe, spec, launches, layout):
    c = spec.c_struct()
    lines = [f"{c.bins.nx} {c.bins.ny} {c.bins.nchan} {c.bins.wcol} {c.bins.inv_dlon.hex()} {c.bins.lat0.hex()} "
             f"{c.bins.inv_dlat.hex()} {c.window_rows} {c.nwin}", str(len(launches))]
    for L in launches:
        lines += layout_text(L, layout)
    out = hostprog.run(exe, lines)
    first = np.array(out[0].split(), np.int64)
    got = {"first": np.where(first == INT32_MAX, -1, first).astype(np.int32).reshape(spec.shape),
           "last": np.array(out[1].split(), np.int32).reshape(spec.shape), "count": None}
    if spec.window_rows is not None:
        got["count"] = np.array(out[2].split(), np.int64).reshape(spec.count_shape)
    emits = [int(x) for x in out[-1].split()[1:]]
    return got, emits


def reference_of(launches, spec):
    """reference_arrival of the launches' logical rows, combined with min, max, add."""
    col = spec.bins.wcol if spec.bins.wcol >= 0 else 4
    parts = [reference_arrival(L["rows"][..., 0], L["rows"][..., 1], L["rows"][..., col], L["chan"], spec,
                               row0=L["i0"]) for L in launches]
    first = np.stack([np.where(p["first"] < 0, INT32_MAX, p["first"]) for p in parts]).min(axis=0)
    return {"first": np.where(first == INT32_MAX, -1, first).astype(np.int32),
            "last": np.stack([p["last"] for p in parts]).max(axis=0),
            "count": None if spec.window_rows is None else sum(p["count"] for p in parts)}


@pytest.mark.parametrize("window_rows", [1, 2, 3, 100, None])
@pytest.mark.parametrize("require", ["amp", None, "k"])
def test_walk_host_program_under_sanitizers(host_program, window_rows, require):
    """csrc/arrival_rows.h (what the kernel calls) in a stand-alone program
    built with ASan + UBSan and run directly: a launch [1, 8) -- it begins
    mid-window for W = 2 and W = 3 -- with tail_from below, at, inside and
    above it and rays without a row block, in all three row layouts, equals
    reference_arrival; W = 1, W larger than the launch and no windows too.  The
    program itself checks every tail's window split against its rows one by
    one."""
    spec = ArrivalSpec(7, 5, nt=8, nchan=3, require=require, window_rows=window_rows)
    L = crafted_launch(1, 8, seed=3)
    assert {-1, 1, 8, 11} <= set(L["tf"].tolist())                      # below, at, at the end, above
    assert {-1, 3} & set(L["chan"].tolist())
    want = reference_of([L], spec)
    assert (want["first"] >= 0).sum() > 20
    if window_rows == 2:
        assert spec.nwin == 4 and (want["count"].sum(axis=(1, 2, 3)) > 0).all()   # a tail from row 1 spans 4 windows
    for layout in LAYOUTS:
        got, _ = run_host_program(host_program, spec, [L], layout)
        assert_same(got, want, layout)


@pytest.mark.parametrize("layout", ["dense", "tails", "slots"])
def test_walk_host_program_launches_combine(host_program, layout):
    """Launches [1, 4) and [4, 8) give what one launch [1, 8) gives; a third
    and a fourth, [8, 9) and [9, 30), go on from there (W = 3: [4, 8) and
    [8, 9) begin mid-window)."""
    spec = ArrivalSpec(7, 5, nt=30, nchan=3, window_rows=3)
    whole = crafted_launch(1, 8, seed=4, tf=np.full(NRAY, 8))           # no tails in the logical rows
    parts = [dict(whole, i0=1, i1=4, rows=whole["rows"][:, :3], tf=np.full(NRAY, 4)),
             dict(whole, i0=4, i1=8, rows=whole["rows"][:, 3:])]
    if layout == "slots":                                               # (rays without a block: all tail)
        for p in [whole] + parts:
            nob = no_block(NRAY)
            p["tf"] = np.where(nob, p["i0"], p["tf"])
            p["rows"] = p["rows"].copy()
            p["rows"][nob] = p["tail"][nob, None]
    one, _ = run_host_program(host_program, spec, [whole], layout)
    two, _ = run_host_program(host_program, spec, parts, layout)
    assert_same(two, one, layout)
    assert_same(one, reference_of([whole], spec), layout)
    more = parts + [crafted_launch(8, 9, seed=6), crafted_launch(9, 30, seed=7)]
    got, _ = run_host_program(host_program, spec, more, layout)
    assert_same(got, reference_of(more, spec), layout)


def test_walk_host_program_frozen_rays_cost_windows_not_rows(host_program):
    """Rays that are all tail over 999 rows: one min, one max and one add per
    window touched per counted ray -- O(windows), not O(rows)."""
    spec = ArrivalSpec(7, 5, nt=1000, nchan=3, window_rows=12)
    L = crafted_launch(1, 1000, seed=8, tf=np.full(NRAY, 1))
    L["rows"] = np.repeat(L["tail"][:, None], 999, axis=1)
    want = reference_of([L], spec)
    col = L["rows"][:, 0, :]
    counted = int((np.isfinite(col[:, 0]) & np.isfinite(col[:, 4]) & (np.abs(col[:, 1]) < math.pi / 2)
                   & (L["chan"] >= 0) & (L["chan"] < 3)).sum())
    assert counted > 10
    for layout in ("tails", "slots"):
        got, emits = run_host_program(host_program, spec, [L], layout)
        assert_same(got, want, layout)
        assert emits == [counted, counted, counted * 84]                 # rows 1..999 touch windows 0..83
    assert want["count"].sum() == counted * 999


# ----------------------------------------------------------- C entry point
def _call(lib, m, nray=16, i0=1, i1=5, rows=64, slot=None, tfrom=None, trow=None, chan=None, first=64, last=64,
          count=64):
    """rwrt_ray_arrival with fake (never dereferenced) device pointers."""
    return lib.rwrt_ray_arrival(None if m is None else ctypes.byref(m), nray, i0, i1, rows, slot, tfrom, trow,
                                chan, first, last, count, None)


def test_arrival_argument_errors_without_a_gpu():
    """Every check happens before any HIP call and names the argument."""
    lib = H.load()
    assert ctypes.sizeof(H.ArrivalMap) == 48
    assert "abi 5" in H.version()                      # an additive member: the version stays
    spec = ArrivalSpec(7, 5, nt=8, nchan=2, window_rows=3)
    good = spec.c_struct()

    def m(window_rows=3, nwin=3, **kw):
        c = spec.c_struct()
        c.window_rows, c.nwin = window_rows, nwin
        for k, v in kw.items():
            setattr(c.bins, k, v)
        return c

    cases = [
        (dict(m=None), b"map"),
        (dict(m=m(nx=0)), b"nx"), (dict(m=m(ny=-1)), b"ny"), (dict(m=m(nchan=0)), b"nchan"),
        (dict(m=m(nx=65536, ny=32768, nchan=1)), b"2^31"), (dict(m=m(nx=1 << 20, ny=1 << 10, nchan=2)), b"2^31"),
        (dict(m=m(wcol=0)), b"wcol"), (dict(m=m(wcol=1)), b"wcol"), (dict(m=m(wcol=7)), b"wcol"),
        (dict(m=m(wcol=-2)), b"wcol"),
        (dict(m=m(inv_dlon=0.0)), b"inv_dlon"), (dict(m=m(inv_dlon=-1.0)), b"inv_dlon"),
        (dict(m=m(inv_dlon=INF)), b"inv_dlon"), (dict(m=m(inv_dlon=NAN)), b"inv_dlon"),
        (dict(m=m(inv_dlat=0.0)), b"inv_dlat"), (dict(m=m(inv_dlat=NAN)), b"inv_dlat"),
        (dict(m=m(inv_dlat=INF)), b"inv_dlat"), (dict(m=m(lat0=NAN)), b"lat0"),
        (dict(m=good, i0=5, i1=5), b"it_begin"), (dict(m=good, i0=6, i1=5), b"it_begin"),
        (dict(m=good, i0=-1, i1=5), b"it_begin"),
        (dict(m=good, slot=64), b"d_row_slot"),
        (dict(m=good, tfrom=64), b"d_tail_row"), (dict(m=good, trow=64), b"d_tail_from"),
        (dict(m=good, rows=None), b"d_rows"),
        (dict(m=good, nray=-1), b"nray"), (dict(m=good, nray=1 << 31), b"nray"),
        (dict(m=good, rows=72), b"16-byte"), (dict(m=good, tfrom=64, trow=72), b"16-byte"),
        (dict(m=good, first=None), b"d_first"), (dict(m=good, last=None), b"d_last"),
        (dict(m=m(window_rows=-1)), b"window_rows"),
        (dict(m=good, count=None), b"d_count"),
        (dict(m=m(nwin=0)), b"nwin"), (dict(m=m(nwin=-1)), b"nwin"),
        (dict(m=m(nwin=1 << 26)), b"2^31"),                       # 2^26 * 70 bins
        (dict(m=m(nwin=30678338)), b"2^31"),                      # 30 678 338 * 70 = 2^31 + 12
        (dict(m=m(window_rows=1 << 30, nwin=1 << 30, nx=1, ny=1, nchan=1), i1=6), None),   # (2^60 rows: fine)
        (dict(m=good, i1=10), b"it_end"),                         # 3 windows of 3 rows end at row 9
        (dict(m=m(window_rows=2, nwin=2), i1=5), b"it_end"),
    ]
    for kw, word in cases:
        if word is None:
            assert _call(lib, nray=0, **kw) == H.RWRT_OK, kw
            continue
        refused(lib, _call, kw, word, b"rwrt_ray_arrival: ")
    # no rays: a no-op (no device is touched; there is none on the build host)
    assert _call(lib, good, nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, good, nray=0, rows=None, i1=9) == H.RWRT_OK                      # the last row of the last window
    assert _call(lib, m(nwin=30678337), nray=0, rows=None) == H.RWRT_OK                # 2^31 - 58 counts
    # no windows: d_count and nwin are not looked at, any it_end goes
    assert _call(lib, m(window_rows=0, nwin=0), nray=0, rows=None, count=None, i1=1 << 30) == H.RWRT_OK
    assert _call(lib, m(window_rows=0, nwin=0, wcol=-1), nray=0, rows=None, count=None) == H.RWRT_OK
