"""The WKB phase along rays and wave-field maps, host side (no GPU): the
definition ``phase.reference_phase`` on written-out segments and on the
reference's own C1 history, the spec, the shared per-row code
csrc/phase_rows.h in a stand-alone program under the sanitizers (crafted
launches in all three row layouts and in chunks), and the argument checks of
``rwrt_ray_phase``."""
import ctypes
import math

import numpy as np
import pytest

import _hip as H
import phase as P
from density import DensitySpec, reference_bins, with_channels
from phase import PhaseSpec, reference_phase
from support import hostprog
from support.abi import refused
from support.cases_phase import (NRAY, VARIANTS, assert_phase, assert_same_run, crafted_history, crafted_spec,
                                 launches_of, run_host_program)
from support.cases_track import c1_rows
from support.rows import LAYOUTS

INF, NAN = math.inf, math.nan
ONE = PhaseSpec(8, 4, weight=None, need=None)     # boxes of 45 degrees


def ray(points, amp=1.0):
    """One ray through ``points`` = [(lon, lat, k, l), ...]."""
    r = np.zeros((1, len(points), 8))
    r[0, :, :4] = points
    r[0, :, 4] = amp
    return r


def box(spec, lon, lat):
    return math.floor((lat - spec.lat0) * spec.inv_dlat), math.floor((lon % (2 * math.pi)) * spec.inv_dlon)


# ------------------------------------------------- written-out segments
def test_zonal_and_meridional_segments():
    """k = 3 along the equator from lon 0 to 1: theta == 3.0 exactly; l = 2
    along a meridian: the trapezoid of l / cos(lat); both at once add up."""
    r = reference_phase(ray([(0.0, 0.0, 3.0, 0.0), (1.0, 0.0, 3.0, 0.0)]), None, ONE)
    assert r["theta"].tolist() == [3.0] and r["nseg"].tolist() == [1] and r["S"].tolist() == [3.0]
    assert r["cnt"].sum() == 2 and r["dropped"] == 0 and r["wabs"] is None
    iy, ix = box(ONE, 0.0, 0.0)
    assert r["cnt"][0, iy, ix] == 1 and r["re"][0, iy, ix] == 1.0 and r["im"][0, iy, ix] == 0.0     # row 0: psi = 0
    iy, ix = box(ONE, 1.0, 0.0)
    assert r["cnt"][0, iy, ix] == 1
    assert r["re"][0, iy, ix] == np.cos(np.array([3.0]))[0] and r["im"][0, iy, ix] == np.sin(np.array([3.0]))[0]
    # a varying k: the mean of the two ends
    assert reference_phase(ray([(0.5, 0.0, 1.0, 0.0), (2.5, 0.0, 2.0, 0.0)]), None, ONE)["theta"].tolist() == [3.0]
    # westward: a negative phase
    assert reference_phase(ray([(1.0, 0.0, 3.0, 0.0), (0.0, 0.0, 3.0, 0.0)]), None, ONE)["theta"].tolist() == [-3.0]
    r = reference_phase(ray([(0.0, 0.0, 0.0, 2.0), (0.0, 0.5, 0.0, 2.0)]), None, ONE)
    a1 = 2.0 / np.cos(np.array([0.5]))[0]
    want = (0.5 * (2.0 + a1)) * 0.5
    assert abs(r["theta"][0] - want) <= 2.0 ** -52 * want and 1.06 < r["theta"][0] < 1.08
    assert r["S"][0] == r["theta"][0]
    both = reference_phase(ray([(0.0, 0.0, 3.0, 2.0), (1.0, 0.5, 3.0, 2.0)]), None, ONE)
    assert both["theta"][0] == 3.0 + r["theta"][0]
    # theta0 is where the sum starts, and row 0 deposits it
    r0 = reference_phase(ray([(0.0, 0.0, 3.0, 0.0), (1.0, 0.0, 3.0, 0.0)]), None, ONE, theta0=[0.5])
    assert r0["theta"].tolist() == [3.5]
    iy, ix = box(ONE, 0.0, 0.0)
    assert r0["re"][0, iy, ix] == np.cos(np.array([0.5]))[0]


def test_holes_poles_channels():
    """A hole between valid rows: theta is carried over it and nseg is not
    incremented; a row at or beyond a pole is a hole; a ray with a channel out
    of range keeps theta0 and deposits nothing."""
    pts = [(0.0, 0.0, 2.0, 0.0), (1.0, 0.0, 2.0, 0.0), (2.0, 0.0, 2.0, 0.0), (3.0, 0.0, 2.0, 0.0)]
    whole = reference_phase(ray(pts), None, ONE)
    assert whole["theta"].tolist() == [6.0] and whole["nseg"].tolist() == [3] and whole["cnt"].sum() == 4
    for col, bad in ((0, NAN), (1, INF), (2, NAN), (3, -INF), (1, P.HALF_PI), (1, -P.HALF_PI), (1, 1.6)):
        r = ray(pts)
        r[0, 1, col] = bad
        got = reference_phase(r, None, ONE)
        assert got["theta"].tolist() == [2.0] and got["nseg"].tolist() == [1] and got["cnt"].sum() == 3, (col, bad)
        assert got["dropped"] == 0
    # just inside the pole: a valid row (cos > 0)
    r = ray(pts)
    r[0, 1, 1] = np.nextafter(P.HALF_PI, 0.0)
    assert reference_phase(r, None, ONE)["nseg"].tolist() == [3]
    # the need and the weight columns
    r = ray(pts)
    r[0, 2, 4] = NAN
    assert reference_phase(r, None, ONE)["nseg"].tolist() == [3]
    for spec in (PhaseSpec(8, 4, weight=None), PhaseSpec(8, 4, need=None)):       # need = amp | weight = amp
        got = reference_phase(r, None, spec)
        assert got["nseg"].tolist() == [1] and got["theta"].tolist() == [2.0] and got["cnt"].sum() == 3
    # channels
    three = np.concatenate([ray(pts)] * 3)
    got = reference_phase(three, [1, 2, -1], with_channels(ONE, 2), theta0=[0.25, 0.5, 0.75])
    assert got["theta"].tolist() == [6.25, 0.5, 0.75] and got["nseg"].tolist() == [3, 0, 0]
    assert got["cnt"][0].sum() == 0 and got["cnt"][1].sum() == 4 and got["S"].tolist() == [6.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        reference_phase(three, [0, 1], ONE)
    with pytest.raises(ValueError):
        reference_phase(np.zeros((3, 4)), None, ONE)
    with pytest.raises(ValueError):
        reference_phase(three, None, ONE, theta0=[0.0])


def test_weights_omega_and_dropped():
    """The weight column weighs the deposit and wabs sums |w|; omega_dt turns
    the phase by the row number; a binned row whose psi is not finite is
    counted in dropped and nowhere else."""
    spec = PhaseSpec(8, 4, weight="ug", need=None)
    r = ray([(0.25, 0.0, 0.0, 0.0), (0.5, 0.0, 0.0, 0.0), (0.75, 0.0, 0.0, 0.0)])
    r[0, :, 5] = [2.0, -3.0, 0.5]
    got = reference_phase(r, None, spec)
    iy, ix = box(spec, 0.25, 0.0)
    assert got["cnt"][0, iy, ix] == 3 and got["re"][0, iy, ix] == -0.5 and got["wabs"][0, iy, ix] == 5.5
    assert got["im"][0, iy, ix] == 0.0 and got["theta"].tolist() == [0.0]
    turned = reference_phase(r, None, PhaseSpec(8, 4, weight="ug", need=None, omega_dt=0.5))
    psi = -0.5 * np.arange(3.0)
    assert abs(turned["re"][0, iy, ix] - (np.array([2.0, -3.0, 0.5]) * np.cos(psi)).sum()) < 1e-15
    assert abs(turned["im"][0, iy, ix] - (np.array([2.0, -3.0, 0.5]) * np.sin(psi)).sum()) < 1e-15
    assert turned["wabs"][0, iy, ix] == 5.5 and turned["theta"].tolist() == [0.0]
    # k0 + k1 overflows: theta and psi are infinite from row 1 on
    big = ray([(0.25, 0.0, 1e308, 0.0), (0.5, 0.0, 1e308, 0.0), (0.75, 0.0, 1e308, 0.0)])
    got = reference_phase(big, None, ONE)
    assert got["dropped"] == 2 and got["cnt"].sum() == 1 and got["re"].sum() == 1.0 and got["nseg"].tolist() == [2]
    assert not np.isfinite(got["theta"][0])
    # outside lat_range: integrated, not deposited, not dropped
    band = PhaseSpec(8, 4, lat_range=(-30.0, 30.0), weight=None, need=None)
    got = reference_phase(ray([(0.0, 0.0, 3.0, 0.0), (1.0, 1.0, 3.0, 0.0)]), None, band)
    assert got["cnt"].sum() == 1 and got["nseg"].tolist() == [1] and got["dropped"] == 0


def test_reference_phase_c1_history():
    """The reference's own C1 history: cnt is the ray-density count of the
    same rows on the same grid; the phases are tens of radians."""
    rows = c1_rows()
    spec = PhaseSpec(36, 18, nchan=3)
    got = reference_phase(rows, np.arange(3), spec)
    count, wsum = reference_bins(rows[..., 0], rows[..., 1], rows[..., 4], np.arange(3)[:, None],
                                 DensitySpec(36, 18, nchan=3, weight="amp"))
    assert np.array_equal(got["cnt"], count) and count.sum() > 2000
    assert np.allclose(got["wabs"], np.abs(wsum), rtol=1e-12) and got["dropped"] == 0
    print("C1: theta", got["theta"].tolist(), "S", got["S"].tolist(), "nseg", got["nseg"].tolist())
    assert np.isfinite(got["theta"]).all() and np.abs(got["theta"]).max() > 10.0
    assert (got["S"] * (1 + 1e-12) >= np.abs(got["theta"])).all()
    theta, nseg, S, ok = P.phase_along(rows, np.arange(3), spec)
    assert np.array_equal(theta[:, -1], got["theta"]) and np.array_equal(nseg, ok[:, 1:].sum(axis=1))
    amp = np.hypot(got["re"], got["im"])
    assert np.all(amp <= got["wabs"] * (1 + 1e-12))


# ---------------------------------------------------------------- the spec
def test_spec():
    assert ctypes.sizeof(H.PhaseMapC) == 56
    s = PhaseSpec(36, 18)
    assert (s.nchan, s.lat_range, s.need, s.weight, s.omega_dt) == (1, (-90, 90), "amp", "amp", 0.0)
    assert s.shape == (1, 18, 36) and (s.ncol, s.wcol) == (4, 4) and s.lon_range is None
    u = PhaseSpec(1440, 720, nchan=3, lat_range=(-60, 60), need=None, weight="ug", omega_dt=-0.25)
    c = u.c_struct()
    assert (c.nx, c.ny, c.nchan, c.need, c.wcol, c.reserved) == (1440, 720, 3, -1, 5, 0)
    assert (c.lat0, c.inv_dlat, c.inv_dlon, c.omega_dt) == (-math.pi / 3, 720 / (math.pi / 3 - -math.pi / 3),
                                                            1440 / (2 * math.pi), -0.25)
    d = DensitySpec(1440, 720, nchan=3, lat_range=(-60, 60), weight="ug").c_struct()
    assert (c.lat0, c.inv_dlat, c.inv_dlon) == (d.lat0, d.inv_dlat, d.inv_dlon)          # the density map's grid
    assert with_channels(u, 7).nchan == 7 and with_channels(u, 7).omega_dt == -0.25
    with pytest.raises(Exception):
        u.nx = 3                                         # frozen
    for bad in (dict(nx=0), dict(ny=-1), dict(nchan=0), dict(nx=2 ** 16, ny=2 ** 15), dict(lat_range=(10.0, 10.0)),
                dict(need="lon"), dict(weight="speed"), dict(omega_dt=NAN), dict(omega_dt=INF)):
        with pytest.raises(ValueError):
            PhaseSpec(**{**dict(nx=7, ny=5), **bad})


# ------------------------------------------- csrc/phase_rows.h on the host
host_program = hostprog.fixture("phase_rows")


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_rows_host_program_under_sanitizers(host_program, name):
    """csrc/phase_rows.h (what the kernel calls) in a stand-alone program built
    with ASan + UBSan and run directly: row 0, then a launch [1, 24) with
    tail_from below, at, inside, at the end of and above it and rays without a
    row block, in all three row layouts: cnt, nseg and dropped equal
    reference_phase, theta, re, im and wabs agree to the bars."""
    spec = crafted_spec(name)
    h = crafted_history(24, seed=3)
    assert {-1, 1, 23, 24, 27} <= set(h["tf"].tolist()) and {-1, 3} <= set(h["chan"].tolist())
    theta0 = np.linspace(-1.0, 1.0, NRAY)
    want = reference_phase(h["rows"], h["chan"], spec, theta0)
    off = ~((h["chan"] >= 0) & (h["chan"] < 3))
    assert off.any() and np.array_equal(want["theta"][off], theta0[off]) and want["nseg"][off].sum() == 0
    assert want["nseg"].sum() > 200 and want["cnt"].sum() > 200 and np.count_nonzero(want["cnt"]) > 20
    for layout in LAYOUTS:
        got = run_host_program(host_program, spec, launches_of(h, [(1, 24)], layout), theta0=theta0)
        assert_phase(got, want, (name, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["7x5-amp", "36x18-unweighted-omega"])
def test_rows_host_program_launches_combine(host_program, name, layout):
    """The launches [1, 9), [9, 10) and [10, 24) with the carried row give
    what one launch [1, 24) gives: theta, nseg, the carried rows and cnt the
    same values, the sums within the bound."""
    spec = crafted_spec(name)
    h = crafted_history(24, seed=4)
    want = reference_phase(h["rows"], h["chan"], spec)
    one, three = (run_host_program(host_program, spec, launches_of(h, b, layout))
                  for b in ([(1, 24)], [(1, 9), (9, 10), (10, 24)]))
    assert_phase(one, want, (name, layout))
    assert_phase(three, want, (name, layout, "in three launches"))
    assert_same_run(one, three, want, (name, layout))
    # the carried row is the last row where that is valid
    last = h["rows"][:, -1]
    live = P.phase_valid(h["rows"], spec)[:, -1] & (h["chan"] >= 0) & (h["chan"] < 3)
    assert live.sum() > 5 and np.array_equal(one["carry"][:3, live], last[live, :3].T)
    assert np.isnan(one["carry"][0, ~live]).all()


def test_rows_host_program_drops_a_tail(host_program):
    """A tail whose psi is not finite: every row of it is dropped; a finite
    tail of n rows is n deposits and n - 1 more segments."""
    spec = PhaseSpec(8, 4, weight="amp")
    rows = np.zeros((2, 6, 8))
    rows[:, :, 0] = 0.25 * np.arange(6)
    rows[:, :, 4] = 1.5
    rows[0, :, 2] = 1e308
    rows[1, :, 2] = 2.0
    rows[:, 3:] = rows[:, 3:4]
    h = dict(rows=rows, tail=rows[:, 3].copy(), tf=np.array([3, 3], np.int32), chan=np.zeros(2, np.int32))
    want = reference_phase(rows, None, spec)
    assert want["dropped"] == 5 and want["cnt"].sum() == 7 and want["nseg"].tolist() == [5, 5]
    assert want["theta"][1] == 1.5
    for layout in ("dense", "tails"):
        got = run_host_program(host_program, spec, launches_of(h, [(1, 6)], layout), nray=2)
        assert_phase(got, want, layout)


# ----------------------------------------------------------- C entry point
def _call(lib, m, nray=16, i0=1, i1=5, rows=64, slot=None, tfrom=None, trow=None, ray=None, ncols=16, chan=None,
          carry=64, theta=64, nseg=64, cnt=64, re=64, im=64, wabs=64, dropped=64):
    """rwrt_ray_phase with fake (never dereferenced) device pointers."""
    return lib.rwrt_ray_phase(None if m is None else ctypes.byref(m), nray, i0, i1, rows, slot, tfrom, trow, ray,
                              ncols, chan, carry, theta, nseg, cnt, re, im, wabs, dropped, None)


def test_phase_argument_errors_without_a_gpu():
    """Every check happens before any HIP call and names the argument."""
    lib = H.load()
    assert "rwrt_ray_phase" in H.ABI_SYMBOLS
    assert "abi 5" in H.version()                      # an additive member: the version stays
    spec = PhaseSpec(7, 5, nchan=2, lat_range=(-60.0, 60.0))
    good = spec.c_struct()

    def m(**kw):
        c = spec.c_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    cases = [
        (dict(m=None), b"map"),
        (dict(m=m(nx=0)), b"nx"), (dict(m=m(ny=-1)), b"ny"), (dict(m=m(nchan=0)), b"nchan"),
        (dict(m=m(nx=1 << 16, ny=1 << 15)), b"2^31"), (dict(m=m(nx=1 << 15, ny=1 << 10, nchan=1 << 6)), b"2^31"),
        (dict(m=m(need=0)), b"need"), (dict(m=m(need=1)), b"need"), (dict(m=m(need=7)), b"need"),
        (dict(m=m(need=-2)), b"need"),
        (dict(m=m(wcol=0)), b"wcol"), (dict(m=m(wcol=7)), b"wcol"), (dict(m=m(wcol=-2)), b"wcol"),
        (dict(m=m(inv_dlon=0.0)), b"inv_dlon"), (dict(m=m(inv_dlon=NAN)), b"inv_dlon"),
        (dict(m=m(inv_dlon=INF)), b"inv_dlon"), (dict(m=m(inv_dlat=-1.0)), b"inv_dlat"),
        (dict(m=m(inv_dlat=INF)), b"inv_dlat"), (dict(m=m(lat0=NAN)), b"lat0"), (dict(m=m(lat0=-INF)), b"lat0"),
        (dict(m=m(omega_dt=NAN)), b"omega_dt"), (dict(m=m(omega_dt=INF)), b"omega_dt"),
        (dict(m=good, i0=5, i1=5), b"it_begin"), (dict(m=good, i0=6, i1=5), b"it_begin"),
        (dict(m=good, i0=-1, i1=3), b"it_begin"),
        (dict(m=good, slot=64), b"d_row_slot"),
        (dict(m=good, tfrom=64), b"d_tail_row"), (dict(m=good, trow=64), b"d_tail_from"),
        (dict(m=good, rows=None), b"d_rows"),
        (dict(m=good, nray=-1), b"nray"), (dict(m=good, nray=1 << 31), b"nray"),
        (dict(m=good, rows=72), b"16-byte"), (dict(m=good, tfrom=64, trow=72), b"16-byte"),
        (dict(m=good, ncols=15), b"nacc_cols"), (dict(m=good, ncols=-1, ray=64), b"nacc_cols"),
        (dict(m=good, ncols=1 << 31, ray=64), b"nacc_cols"),
        (dict(m=good, carry=None), b"d_carry"), (dict(m=good, theta=None), b"d_theta"),
        (dict(m=good, nseg=None), b"d_nseg"), (dict(m=good, cnt=None), b"d_cnt"), (dict(m=good, re=None), b"d_re"),
        (dict(m=good, im=None), b"d_im"), (dict(m=good, dropped=None), b"d_dropped"),
        (dict(m=good, wabs=None), b"d_wabs"), (dict(m=m(wcol=-1)), b"d_wabs"),
    ]
    for kw, word in cases:
        refused(lib, _call, kw, word, b"rwrt_ray_phase: ")
    # the output pointers are checked with no rays too
    assert _call(lib, good, nray=0, rows=None, cnt=None) == H.RWRT_ERR_ARG
    # no rays: a no-op (no device is touched; there is none on the build host)
    assert _call(lib, good, nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, good, nray=0, rows=None, ncols=0) == H.RWRT_OK
    assert _call(lib, good, nray=0, rows=None, i0=0, i1=1) == H.RWRT_OK
    assert _call(lib, m(wcol=-1), nray=0, rows=None, wabs=None) == H.RWRT_OK
    assert _call(lib, m(need=-1, omega_dt=-0.5), nray=0, rows=None, i0=100, i1=200) == H.RWRT_OK
    big = PhaseSpec(1440, 720, nchan=12).c_struct()
    assert _call(lib, big, nray=0, rows=None) == H.RWRT_OK
