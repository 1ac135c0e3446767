"""Wave-ray flux maps, host side (no GPU): the NumPy definition
``flux.reference_flux`` against a point-by-point loop and on the reference's
own C1 history, the shared accept rule and per-ray walk csrc/flux_rows.h in a
stand-alone program under the sanitizers (crafted launches in all three row
layouts), and the argument checks of ``rwrt_ray_flux``."""
import ctypes
import math

import numpy as np
import pytest

import _hip as H
import flux as F
from conftest import golden
from density import DensitySpec, reference_bins
from flux import FluxSpec, reference_flux
from support import hostprog
from support.abi import refused
from support.cases_density import corner_points, random_points
from support.cases_flux import (NRAY, VARIANTS, abs_sums, assert_flux, columns, crafted_launch, reference_of,
                                sum_bound)
from support.rows import LAYOUTS, layout_text, no_block

TWO_PI = 2 * math.pi
INF, NAN = math.inf, math.nan


def scalar_point(lon, lat, k, l, ug, vg, c, spec):
    """The accept rule of the issue for one point, in Python floats:
    ``((c, iy, ix), vx, vy, speed)`` or None."""
    if not 0 <= c < spec.nchan:
        return None
    if not all(math.isfinite(x) for x in (lon, lat, ug, vg)):
        return None
    if not (abs(k) <= spec.wn_max and abs(l) <= spec.wn_max):
        return None
    s2 = ug * ug + vg * vg
    if not math.isfinite(s2) or not spec.s2_min <= s2 <= spec.s2_max:
        return None
    if spec.vector == "unit" and not s2 > 0:
        return None
    fy = (lat - spec.lat0) * spec.inv_dlat
    if not math.isfinite(fy) or not 0 <= math.floor(fy) < spec.ny:
        return None
    if spec.lon_range is None:
        lam = (lon % TWO_PI) % TWO_PI
        ix = min(math.floor(lam * spec.inv_dlon), spec.nx - 1)
    else:
        fx = (lon - spec.lon0) * spec.inv_dlon
        if not 0 <= math.floor(fx) < spec.nx:
            return None
        ix = math.floor(fx)
    speed = math.sqrt(s2)
    vx, vy = (ug / speed, vg / speed) if spec.vector == "unit" else (ug, vg)
    return (c, math.floor(fy), ix), vx, vy, speed


def scalar_flux(lon, lat, k, l, ug, vg, chan, spec, row0=0):
    """The definition of the issue, point by point in Python."""
    count = np.zeros(spec.shape, np.int64)
    rowsum = np.zeros(spec.shape, np.int64)
    total = np.zeros(spec.shape + (3,))
    for j in range(lon.shape[0]):
        for r in range(lon.shape[1]):
            p = scalar_point(*(float(a[j, r]) for a in (lon, lat, k, l, ug, vg)), int(chan[j]), spec)
            if p is None:
                continue
            b, vx, vy, speed = p
            count[b] += 1
            rowsum[b] += row0 + r
            total[b + (0,)] += vx
            total[b + (1,)] += vy
            total[b + (2,)] += speed
    return {"count": count, "rowsum": rowsum, "sum": total}


def test_spec():
    s = FluxSpec(1440, 720)
    assert (s.lon0, s.inv_dlon, s.mode) == (0.0, 1440 / (2 * math.pi), 0) and s.inv_dlon == DensitySpec(1440, 720).inv_dlon
    assert (s.lat0, s.inv_dlat) == (DensitySpec(1440, 720).lat0, DensitySpec(1440, 720).inv_dlat)
    assert (s.s2_min, s.s2_max, s.wn_max) == (0.0, INF, INF) and s.shape == (1, 720, 1440) and s.circles is None
    u = FluxSpec(4320, 720, lon_range=(-360, 720), nchan=3, vector="unit", speed_range=(0.5, 80.0), wn_max=40.0)
    assert u.lon0 == -2 * math.pi and u.lon1 == 4 * math.pi and u.inv_dlon == 4320 / (u.lon1 - u.lon0)
    assert (u.mode, u.s2_min, u.s2_max, u.circles) == (3, 0.25, 6400.0, 3)
    c = u.c_struct()
    assert (c.nx, c.ny, c.nchan, c.mode, c.lon0, c.inv_dlon, c.lat0, c.inv_dlat, c.s2_min, c.s2_max, c.wn_max) == \
        (4320, 720, 3, 3, u.lon0, u.inv_dlon, u.lat0, u.inv_dlat, 0.25, 6400.0, 40.0)
    assert FluxSpec(7, 5, lon_range=(0, 360)).mode == 2 and FluxSpec(7, 5, lon_range=(0, 360)).circles == 1
    assert FluxSpec(7, 5, lon_range=(-180, 180)).circles is None and FluxSpec(7, 5, lon_range=(0, 400)).circles is None
    for bad in (dict(nx=0), dict(ny=-1), dict(nchan=0), dict(nx=65536, ny=32768), dict(lat_range=(10.0, 10.0)),
                dict(lon_range=(10.0, 10.0)), dict(lon_range=(20.0, 10.0)), dict(lon_range=(0.0, INF)),
                dict(lon_range=(NAN, 10.0)), dict(vector="amp"), dict(speed_range=(-1.0, 2.0)),
                dict(speed_range=(2.0, 1.0)), dict(speed_range=(NAN, 1.0)), dict(speed_range=(0.0, NAN)),
                dict(wn_max=-1.0), dict(wn_max=NAN)):
        with pytest.raises(ValueError):
            FluxSpec(**{**dict(nx=7, ny=5), **bad})
    assert ctypes.sizeof(H.FluxMapC) == 72
    # fold: whole circles from a multiple of 360, nx divisible by their number
    with pytest.raises(ValueError):
        F.fold_arrays(FluxSpec(7, 5), np.zeros((1, 5, 7, 2)))
    with pytest.raises(ValueError):
        F.fold_arrays(FluxSpec(7, 5, lon_range=(-360, 720)), np.zeros((1, 5, 7, 2)))
    with pytest.raises(ValueError):
        F.fold_arrays(FluxSpec(6, 5, lon_range=(-180, 900)), np.zeros((1, 5, 6, 2)))
    sp, (a,) = F.fold_arrays(FluxSpec(6, 1, lon_range=(-360, 720)), np.arange(12).reshape(1, 1, 6, 2))
    assert sp == FluxSpec(2, 1) and a.tolist() == [[[[0 + 4 + 8, 1 + 5 + 9], [2 + 6 + 10, 3 + 7 + 11]]]]


def corner_rows(nrow, seed=11):
    """The corner points of the density tests as ``[npoint, nrow]`` rays that
    stay where they are: their weight column is ug (NaN, inf and 1e300 among
    them: 1e300 squared is not finite), k, l and vg are drawn."""
    pts = corner_points()
    rng = np.random.default_rng(seed)
    lon, lat, ug = (np.repeat(np.array([p[q] for p in pts])[:, None], nrow, axis=1) for q in range(3))
    chan = np.array([p[3] for p in pts])
    k, l, vg = (rng.uniform(-3.0, 3.0, lon.shape) for _ in range(3))
    return lon, lat, k, l, ug, vg, chan


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_reference_flux_against_the_scalar_definition(name):
    spec = FluxSpec(7, 5, nchan=2, **VARIANTS[name])
    row0 = 2
    lon, lat, k, l, ug, vg, chan = corner_rows(4)
    got = reference_flux(lon, lat, k, l, ug, vg, chan, spec, row0=row0)
    assert_flux(got, scalar_flux(lon, lat, k, l, ug, vg, chan, spec, row0), None, "corner points")
    assert got["count"].sum() > 0 and got["rowsum"].sum() >= row0 * got["count"].sum()
    if name == "wrapped":
        # written out: the 15 points the density map bins with a finite weight, less the two with
        # |ug| = 1e300 (s2 overflows), 4 rows each (rows 2..5: 14 per point)
        assert got["count"].sum() == 13 * 4 and got["rowsum"].sum() == 13 * 14
        assert got["count"][0, 2].tolist() == [16, 4, 0, 4, 0, 0, 4]
    rl, rt, rw, rc = random_points(4000, DensitySpec(7, 5, nchan=2), seed=5)
    rng = np.random.default_rng(6)
    lon, lat, ug, chan = rl.reshape(200, 20), rt.reshape(200, 20), rw.reshape(200, 20), rc[:200]
    k, l, vg = (rng.uniform(-3.0, 3.0, lon.shape) for _ in range(3))
    k[rng.random(lon.shape) < 0.02] = NAN
    vg[rng.random(lon.shape) < 0.02] = INF
    rest = int(np.where((chan >= 0) & (chan < 2))[0][0])
    ug[rest] = vg[rest] = 0.0                                   # a ray at rest: no direction
    got = reference_flux(lon, lat, k, l, ug, vg, chan, spec, row0=row0)
    want = scalar_flux(lon, lat, k, l, ug, vg, chan, spec, row0)
    assert_flux(got, want, None, "random")
    n = int(want["count"].sum())
    assert n > 50 and np.count_nonzero(want["count"]) > 15
    # each filter drops some points and keeps some: against the same spec without it
    loose = reference_flux(lon, lat, k, l, ug, vg, chan, FluxSpec(7, 5, nchan=2), row0=row0)["count"].sum()
    v = VARIANTS[name]
    for key in ("speed_range", "wn_max", "lon_range"):
        if key in v:
            without = {q: w for q, w in v.items() if q != key}
            more = reference_flux(lon, lat, k, l, ug, vg, chan, FluxSpec(7, 5, nchan=2, **without), row0=row0)
            assert 0 < n < more["count"].sum() <= loose, key
    if v.get("vector") == "unit":
        # a unit vector per point: |sum| <= count, and the points at rest are not counted
        assert np.all(np.hypot(want["sum"][..., 0], want["sum"][..., 1]) <= want["count"] * (1 + 1e-15))
        vel = reference_flux(lon, lat, k, l, ug, vg, chan, FluxSpec(7, 5, nchan=2, **{**v, "vector": "velocity"}),
                             row0=row0)
        at_rest = sum(scalar_point(*(float(a[rest, r]) for a in (lon, lat, k, l, ug, vg)), int(chan[rest]),
                                   FluxSpec(7, 5, nchan=2, **{**v, "vector": "velocity"})) is not None
                      for r in range(lon.shape[1]))
        assert ("speed_range" in v) == (at_rest == 0) and vel["count"].sum() - n == at_rest
        assert np.array_equal(vel["sum"][..., 2] > 0, want["sum"][..., 2] > 0)


# ---------------------------------------------------- the reference's C1 history
def c1_columns():
    hist = golden("traj_C1.npz")["hist"]              # (7, 1081, 3): lon lat k l amp ug vg
    return [hist[c].T for c in (0, 1, 2, 3, 5, 6)]    # [3, 1081] each


def test_reference_flux_c1_history_wrapped():
    """The reference's own 90-day C1 history, one channel per root, default
    filters: root 0 is a dead slot (NaN ug), and the map is the density map
    weighted by ug."""
    lon, lat, k, l, ug, vg = c1_columns()
    chan = np.arange(3)
    for nx, ny in ((1440, 720), (144, 72)):
        spec = FluxSpec(nx, ny, nchan=3)
        f = reference_flux(lon, lat, k, l, ug, vg, chan, spec)
        assert f["count"].sum(axis=(1, 2)).tolist() == [0, 1081, 1081]
        assert f["rowsum"].sum(axis=(1, 2)).tolist() == [0, 1080 * 1081 // 2, 1080 * 1081 // 2]
        dspec = DensitySpec(nx, ny, nchan=3, weight="ug")
        count, wsum = reference_bins(lon, lat, ug, chan[:, None], dspec)
        assert np.array_equal(f["count"], count)
        abs_w = reference_bins(lon, lat, np.abs(ug), chan[:, None], dspec)[1]
        assert np.all(np.abs(f["sum"][..., 0] - wsum) <= 2.0 * (count + 1) * 2.0 ** -53 * abs_w)
        assert np.array_equal(f["sum"][..., 0], wsum)          # (the same terms in the same order)
        assert np.all(f["sum"][..., 2] >= np.hypot(f["sum"][..., 0], f["sum"][..., 1]) * (1 - 1e-12))
        unit = reference_flux(lon, lat, k, l, ug, vg, chan, FluxSpec(nx, ny, nchan=3, vector="unit"))
        assert np.array_equal(unit["count"], f["count"]) and np.array_equal(unit["sum"][..., 2], f["sum"][..., 2])


# literals computed from the golden history: the rows of each root with -360 <= lon < 720 degrees (root 0, the
# dead slot, stays at its source), the points the map counts, and those per circle of the window
C1_IN_WINDOW = {"rows_in_window": [1081, 230, 229], "count": [0, 230, 229], "by_circle": [0, 198, 261]}


def test_reference_flux_c1_history_three_circles():
    """The unwrapped window (-360, 720) keeps the rows whose longitude lies in
    it -- the rays of C1 leave it eastward -- and its fold onto [0, 360) is the
    wrapped map of those rows."""
    lon, lat, k, l, ug, vg = c1_columns()
    chan = np.arange(3)
    inside = (lon >= -TWO_PI) & (lon < 2 * TWO_PI)
    assert np.nanmax(lon) * 180 / math.pi > 3600.0 and np.nanmin(lon) >= 0.0
    assert inside.sum(axis=1).tolist() == C1_IN_WINDOW["rows_in_window"]
    for nx, ny in ((4320, 720), (432, 72)):
        spec = FluxSpec(nx, ny, nchan=3, lon_range=(-360.0, 720.0))
        f = reference_flux(lon, lat, k, l, ug, vg, chan, spec)
        assert f["count"].sum(axis=(1, 2)).tolist() == C1_IN_WINDOW["count"]
        assert f["count"].sum(axis=(1, 2)).tolist() == [0] + inside.sum(axis=1).tolist()[1:]
        per = nx // 3
        by_circle = f["count"].reshape(3, ny, 3, per).sum(axis=(0, 1, 3)).tolist()
        assert by_circle == C1_IN_WINDOW["by_circle"]                      # nothing west of 0
        wspec, (count, rowsum, total) = F.fold_arrays(spec, f["count"], f["rowsum"], f["sum"])
        assert wspec == FluxSpec(per, ny, nchan=3)
        keep = np.where(inside, lon, NAN)                                  # the wrapped map restricted to those rows
        w = reference_flux(keep, lat, k, l, ug, vg, chan, wspec)
        assert np.array_equal(count, w["count"]) and np.array_equal(rowsum, w["rowsum"])
        a = abs_sums(keep, lat, k, l, ug, vg, chan, wspec)
        assert np.all(np.abs(total - w["sum"]) <= sum_bound(w["count"], a))


# ------------------------------------------------ csrc/flux_rows.h on the host
host_program = hostprog.fixture("flux_rows")


def run_host_program(exe, spec, launches, layout):
    c = spec.c_struct()
    lines = [f"{c.nx} {c.ny} {c.nchan} {c.mode} " + " ".join(
        float(x).hex() for x in (c.lon0, c.inv_dlon, c.lat0, c.inv_dlat, c.s2_min, c.s2_max, c.wn_max)),
        str(len(launches))]
    for L in launches:
        lines += layout_text(L, layout)
    out = hostprog.run(exe, lines)
    cnt = np.array(out[0].split(), np.int64).reshape(spec.shape + (2,))
    total = np.array([float.fromhex(x) for x in out[1].split()]).reshape(spec.shape + (3,))
    emits = [int(x) for x in out[-1].split()[1:]]
    print(f"{layout}: emits (add_cnt, add_sum) = {emits}")
    return {"count": np.ascontiguousarray(cnt[..., 0]), "rowsum": np.ascontiguousarray(cnt[..., 1]),
            "sum": total}, emits


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_walk_host_program_under_sanitizers(host_program, name):
    """csrc/flux_rows.h (what the kernel calls) in a stand-alone program built
    with ASan + UBSan and run directly: a launch [1, 8) with tail_from below,
    at, inside, at the end of and above it and rays without a row block, in all
    three row layouts: count and rowsum equal reference_flux, the sums agree to
    the bound."""
    spec = FluxSpec(7, 5, nchan=3, **VARIANTS[name])
    L = crafted_launch(1, 8, seed=3)
    assert {-1, 1, 8, 11} <= set(L["tf"].tolist())                      # below, at, at the end, above
    assert {-1, 3} <= set(L["chan"].tolist())
    want, a = reference_of([L], spec)
    total = int(np.isin(L["chan"], (0, 1, 2)).sum()) * 7
    assert 20 < want["count"].sum() < total and np.count_nonzero(want["count"]) > 10, want["count"].sum()
    for layout in LAYOUTS:
        got, emits = run_host_program(host_program, spec, [L], layout)
        assert_flux(got, want, a, (name, layout))
        assert emits[0] == emits[1] <= want["count"].sum()


@pytest.mark.parametrize("layout", ["dense", "tails", "slots"])
def test_walk_host_program_launches_combine(host_program, layout):
    """Launches [1, 4) and [4, 8) give what one launch [1, 8) gives; a third
    and a fourth, [8, 9) and [9, 30), go on from there."""
    spec = FluxSpec(7, 5, nchan=3, lon_range=(-360.0, 720.0))
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
    want, a = reference_of([whole], spec)
    assert want["count"].sum() > 20
    assert_flux(one, want, a, layout)
    assert_flux(two, want, a, layout + " in two launches")
    more = parts + [crafted_launch(8, 9, seed=6), crafted_launch(9, 30, seed=7)]
    got, _ = run_host_program(host_program, spec, more, layout)
    want, a = reference_of(more, spec)
    assert_flux(got, want, a, layout + " four launches")


def test_walk_host_program_frozen_rays_cost_one_emit_pair(host_program):
    """Rays that are all tail over 999 rows: one add_cnt and one add_sum per
    counted ray -- not one per row -- with rowsum = 999 * 1000 / 2 each."""
    spec = FluxSpec(7, 5, nchan=3)
    L = crafted_launch(1, 1000, seed=8, tf=np.full(NRAY, 1))
    L["rows"] = np.repeat(L["tail"][:, None], 999, axis=1)
    want, a = reference_of([L], spec)
    idx = F.accept(*columns(L["tail"]), L["chan"], spec)[0]
    counted = int((idx >= 0).sum())
    assert 10 < counted < NRAY
    assert want["count"].sum() == counted * 999 and want["rowsum"].sum() == counted * (999 * 1000 // 2)
    for layout in ("tails", "slots"):
        got, emits = run_host_program(host_program, spec, [L], layout)
        assert_flux(got, want, a, layout)
        assert emits == [counted, counted]


# ----------------------------------------------------------- C entry point
def _call(lib, m, nray=16, i0=1, i1=5, rows=64, slot=None, tfrom=None, trow=None, chan=None, cnt=64, total=64):
    """rwrt_ray_flux with fake (never dereferenced) device pointers."""
    return lib.rwrt_ray_flux(None if m is None else ctypes.byref(m), nray, i0, i1, rows, slot, tfrom, trow, chan,
                             cnt, total, None)


def test_flux_argument_errors_without_a_gpu():
    """Every check happens before any HIP call and names the argument."""
    lib = H.load()
    assert ctypes.sizeof(H.FluxMapC) == 72
    assert "abi 5" in H.version()                      # an additive member: the version stays
    spec = FluxSpec(7, 5, nchan=2, lon_range=(-360.0, 720.0), speed_range=(0.5, 80.0), wn_max=40.0)
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
        (dict(m=m(mode=4)), b"mode"), (dict(m=m(mode=7)), b"mode"), (dict(m=m(mode=-1)), b"mode"),
        (dict(m=m(inv_dlon=0.0)), b"inv_dlon"), (dict(m=m(inv_dlon=-1.0)), b"inv_dlon"),
        (dict(m=m(inv_dlon=INF)), b"inv_dlon"), (dict(m=m(inv_dlon=NAN)), b"inv_dlon"),
        (dict(m=m(inv_dlat=0.0)), b"inv_dlat"), (dict(m=m(inv_dlat=NAN)), b"inv_dlat"),
        (dict(m=m(inv_dlat=INF)), b"inv_dlat"), (dict(m=m(lat0=NAN)), b"lat0"), (dict(m=m(lat0=-INF)), b"lat0"),
        (dict(m=m(lon0=NAN)), b"lon0"), (dict(m=m(lon0=INF)), b"lon0"),
        (dict(m=m(mode=0)), b"lon0"), (dict(m=m(mode=1)), b"lon0"),          # wrapped with lon0 = -2 pi
        (dict(m=m(s2_min=NAN)), b"s2_min"), (dict(m=m(s2_min=-1.0)), b"s2_min"),
        (dict(m=m(s2_max=NAN)), b"s2_max"), (dict(m=m(s2_max=0.2)), b"s2_max"),
        (dict(m=m(wn_max=NAN)), b"wn_max"), (dict(m=m(wn_max=-1.0)), b"wn_max"),
        (dict(m=good, i0=5, i1=5), b"it_begin"), (dict(m=good, i0=6, i1=5), b"it_begin"),
        (dict(m=good, slot=64), b"d_row_slot"),
        (dict(m=good, tfrom=64), b"d_tail_row"), (dict(m=good, trow=64), b"d_tail_from"),
        (dict(m=good, rows=None), b"d_rows"),
        (dict(m=good, nray=-1), b"nray"), (dict(m=good, nray=1 << 31), b"nray"),
        (dict(m=good, rows=72), b"16-byte"), (dict(m=good, tfrom=64, trow=72), b"16-byte"),
        (dict(m=good, cnt=None), b"d_cnt"), (dict(m=good, total=None), b"d_sum"),
    ]
    for kw, word in cases:
        refused(lib, _call, kw, word, b"rwrt_ray_flux: ")
    # the output pointers are checked with no rays too
    assert _call(lib, good, nray=0, rows=None, cnt=None) == H.RWRT_ERR_ARG
    # no rays: a no-op (no device is touched; there is none on the build host)
    assert _call(lib, good, nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, m(mode=3), nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, m(mode=0, lon0=0.0), nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, m(s2_min=0.0, s2_max=INF, wn_max=INF), nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, m(s2_min=4.0, s2_max=4.0, wn_max=0.0), nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, FluxSpec(1440, 720, nchan=3).c_struct(), nray=0, rows=None) == H.RWRT_OK
