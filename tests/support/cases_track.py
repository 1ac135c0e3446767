"""Crafted histories, spec variants and comparisons of the track tests, which
the cross tests borrow."""
import math

import numpy as np

import track as T
from conftest import golden
from support.rows import layout_device

TWO_PI = 2 * math.pi
INF, NAN = math.inf, math.nan


# ---------------------------------------------------- the reference's C1 history
def c1_rows():
    hist = golden("traj_C1.npz")["hist"]              # (7, 1081, 3): lon lat k l amp ug vg
    rows = np.full((3, 1081, 8), NAN)
    for c in range(7):
        rows[:, :, c] = hist[c].T
    return rows


# (map) -> considered segments, dropped, cell deposits, sum of time: need = 'amp', lat -90..90, max_cells = nx + ny
C1_TRACK = {(1440, 720): (2160, 0, 42669, 2160.0), (360, 180): (2160, 0, 12271, 2160.0),
            (7, 5): (2160, 0, 2282, 2160.0)}


def rows_of(points, amp=1.0, ug=2.0):
    """One ray through ``points`` = [(lon, lat), ...] (radians)."""
    r = np.zeros((1, len(points), 8))
    r[0, :, 0] = [p[0] for p in points]
    r[0, :, 1] = [p[1] for p in points]
    r[0, :, 4], r[0, :, 5] = amp, ug
    return r


# ------------------------------------------------------------- crafted launches
NRAY = 41
VARIANTS = {
    "wrapped": dict(),
    "wrapped-weight": dict(weight="ug"),
    "window": dict(lon_range=(-360.0, 720.0)),
    "window-weight-no-need": dict(lon_range=(-360.0, 720.0), weight="vg", need=None),
    "short-segments": dict(weight="k", max_cells=3),
}


def crafted_history(nt, seed, nray=NRAY, tf=None, i0=1):
    """A logical history ``[nray, nt, 8]`` (row 0 the initial row) whose rows
    ``[i0, nt)`` all three layouts can hold as one launch: ray j's rows from
    ``tf[j]`` on repeat its tail row.  ``tf`` runs through values below, at,
    inside, at the end of and above the launch; the j % 3 == 0 rays (no row
    block in the slots layout) have at most i0.  By j % 4: rays that cross a
    few cells per row in any direction, rays that drift slowly (several rows
    per cell, going on into the tail), rays that jump (many segments above
    ``max_cells``) and rays that move along grid lines and through nodes of a
    7 x 5 map (coordinates that are multiples of half a cell).  Longitudes
    span about three circles either side of 0, latitudes leave +-90 degrees;
    NaN and inf holes in lon, lat, amp and ug, in rows and in tails; lon =
    1e300 in a row and in a tail; channels -1 and 3 among 0..2."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-3.0, 3.0, (nray, nt, 8))
    kind = np.arange(nray) % 4
    lon = rng.uniform(-15.0, 15.0, (nray, 1)) + np.cumsum(rng.uniform(-1.2, 1.2, (nray, nt)), axis=1)
    lat = rng.uniform(-1.2, 1.2, (nray, 1)) + np.cumsum(rng.uniform(-0.5, 0.5, (nray, nt)), axis=1)
    slow = kind == 1
    lon[slow] = rng.uniform(-6.0, 12.0, (slow.sum(), 1)) + 0.05 * np.arange(nt)
    lat[slow] = rng.uniform(-1.0, 1.0, (slow.sum(), 1)) - 0.01 * np.arange(nt)
    jumpy = kind == 2
    lon[jumpy] = rng.uniform(-20.0, 20.0, (jumpy.sum(), nt))
    lat[jumpy] = rng.uniform(-1.8, 1.8, (jumpy.sum(), nt))
    lines = kind == 3
    hx, hy = TWO_PI / 7 / 2, math.pi / 5 / 2                  # half a cell of the 7 x 5 map
    lon[lines] = hx * rng.integers(-20, 21, (lines.sum(), nt))
    lat[lines] = -math.pi / 2 + hy * rng.integers(0, 11, (lines.sum(), nt))
    rows[..., 0], rows[..., 1] = lon, lat
    rows[3, nt // 2, 5] = NAN                                    # holes
    rows[7, i0, 0] = INF
    rows[9, nt // 2, 1] = -INF
    rows[13, i0, 4] = NAN
    rows[17, nt - 1, 4] = INF
    rows[4, min(i0 + 1, nt - 1), 0] = 1e300                      # finite: dropped on both sides
    rows[21, :, 0:2] = rows[21, :1, 0:2]                         # at rest while it is read
    tail = rows[:, -1].copy()
    tail[:, 0] += rng.uniform(-0.8, 0.8, nray)
    tail[5::7, 0] = NAN
    tail[6::11, 4] = INF
    tail[8::13, 5] = NAN
    tail[10, 0] = 1e300
    if tf is None:
        i1 = nt
        choice = sorted({i0 - 2, i0, i0 + 1, i0 + 3, i0 + 4, i0 + 5, i1 - 1, i1, i1 + 3})
        j = np.arange(nray)
        q = np.cumsum(j % 3 != 0)                                 # (the rays with a block take every value)
        tf = np.where(j % 3 == 0, np.array([i0 - 2, i0])[(j // 3) % 2], np.array(choice)[q % len(choice)])
    tf = np.asarray(tf, np.int32)
    cut = np.clip(tf, i0, nt)
    for j in range(nray):
        rows[j, cut[j]:] = tail[j]
    # a slow ray whose tail continues its last cell: the run goes on into the tail
    for j in np.where(slow)[0]:
        if i0 < cut[j] < nt:
            tail[j] = rows[j, cut[j] - 1]
            rows[j, cut[j]:] = tail[j]
    chan = rng.integers(-1, 4, nray).astype(np.int32)            # -1 and nchan = 3 among them
    return dict(rows=rows, tail=tail, tf=tf, chan=chan)


def launch(h, i0, i1):
    """Rows ``[i0, i1)`` of the history as a launch of support/rows.py (the
    tails of a launch that ends before the history's tail starts are above it)."""
    return dict(i0=i0, i1=i1, rows=h["rows"][:, i0:i1], tail=h["tail"], tf=h["tf"], chan=h["chan"])


SENTINEL = {0: 1.0, 1: 0.1}   # lon lat of a row that must never be read: valid, in the map, deposited if it were


def device_layouts(h, i0, i1, seed=1):
    """``name -> (view, tails, slots)`` device objects of rows [i0, i1) of the history."""
    return layout_device(launch(h, i0, i1), SENTINEL, seed)


def launches_of(h, bounds, layout):
    """The history as launches: row 0 as a dense launch [0, 1), then the
    launches ``bounds`` = [(i0, i1), ...] in ``layout``."""
    out = [(dict(i0=0, i1=1, rows=h["rows"][:, :1], tail=h["tail"], tf=np.full(len(h["tf"]), 1), chan=h["chan"]),
            "dense")]
    return out + [(launch(h, i0, i1), layout) for i0, i1 in bounds]


def abs_sums(rows, chan, spec):
    """Per cell the sum of |w| and of |w vm| of its deposits: the sum|v| of the
    rounding bound."""
    a = np.zeros((2,) + spec.shape)
    for d in T.deposits(rows, chan, spec):
        if d is not None:
            c, iy, ix, w, wv = d
            a[0, c, iy, ix] += abs(w)
            a[1, c, iy, ix] += abs(wv)
    return a


def sum_bound(cnt, abs_sum):
    """|got - ref| <= 2 (n + 1) 2^-53 sum|v| per cell: the bound of a sum of n
    terms in any order, twice (both sides are rounded sums), plus one rounding
    for a tail added as a product (tests/test_gpu_density.py)."""
    return 2.0 * (cnt + 1) * 2.0 ** -53 * abs_sum


def assert_track(got, want, a=None, what=""):
    """cnt and dropped exactly; time and wsum exactly (``a`` None) or to the bound."""
    assert got["cnt"].dtype == np.int64 and np.array_equal(got["cnt"], want["cnt"]), (what, "cnt")
    assert int(got["dropped"]) == int(want["dropped"]), (what, "dropped", got["dropped"], want["dropped"])
    for q, name in enumerate(("time", "wsum")):
        if want[name] is None:
            assert got[name] is None, (what, name)
            continue
        assert np.all(np.isfinite(got[name])), (what, name)
        if a is None:
            assert np.array_equal(got[name], want[name]), (what, name)
        else:
            err = np.abs(got[name] - want[name])
            assert np.all(err <= sum_bound(want["cnt"], a[q])), (what, name, float(err.max()))


def reference_and_abs(rows, chan, spec):
    """``reference_track`` and the per-cell sums of |w| and |w vm| (the
    sum|v| of the rounding bound) in one pass over the deposits."""
    cnt = np.zeros(spec.shape, np.int64)
    sums = np.zeros((2,) + spec.shape)
    a = np.zeros((2,) + spec.shape)
    dropped = 0
    for d in T.deposits(rows, chan, spec):
        if d is None:
            dropped += 1
            continue
        c, iy, ix, w, wv = d
        cnt[c, iy, ix] += 1
        sums[0, c, iy, ix] += w
        sums[1, c, iy, ix] += wv
        a[0, c, iy, ix] += abs(w)
        a[1, c, iy, ix] += abs(wv)
    return {"cnt": cnt, "time": sums[0], "wsum": sums[1] if spec.wcol >= 0 else None, "dropped": dropped}, a


def start(m, rows0):
    """Row 0 of a history ``[nray, 8]`` into the map."""
    s = m.spec
    return m.start(rows0[:, 0], rows0[:, 1], None if s.ncol < 0 else rows0[:, s.ncol],
                   None if s.wcol < 0 else rows0[:, s.wcol])
