"""Caustic-aware wave-field maps, host side (no GPU): the definition
``wave.reference_wave`` as a composition of ``tube.reference_tube`` and
``phase.reference_phase``, the spec, the shared per-row code csrc/wave_rows.h
in a stand-alone program under the sanitizers (the crafted history of the tube
tests, four seeds, three grids, all three row layouts, three splits), the
argument checks of ``rwrt_ray_wave`` and what ``WR.ray_wave`` refuses before
any work."""
import ctypes
import math

import numpy as np
import pytest

import _hip as H
from phase import reference_phase
from support import hostprog
from support.abi import refused
from support.cases_track import sum_bound
from support.cases_wave import (NT_CRAFTED, SEEDS, SPECS, SPLITS, assert_same_run, assert_wave, crafted_history,
                                crafted_nbr, crafted_spec, deposits, launches_of, run_host_program)
from support.rows import LAYOUTS
from tube import lattice_neighbours, reference_tube
from wave import HALF_PI, WaveSpec, reference_wave

INF, NAN = math.inf, math.nan
PI = math.pi
CASES = [(name, seed) for name in sorted(SPECS) for seed in SEEDS]


# ------------------------------------------- the crafted history is rich enough
@pytest.mark.parametrize("name,seed", CASES)
def test_crafted_history_is_rich_enough(name, seed):
    """Asserted from the two composed definitions alone, so that no comparison
    below passes vacuously: deposits behind one and behind two caustics, rows
    with jac == 0, rows that are tube-open and not phase-valid, and a smallest
    |D| that d_floor = 0.01 clips (cos varies by under 5 % over the lattice,
    so |jac / jac_0| is within 5 % of |D|)."""
    spec = crafted_spec(name)
    h = crafted_history(NT_CRAFTED, seed)
    d = deposits(h["rows"], crafted_nbr(), h["chan"], spec)
    live = ~d["zero"]
    st = dict(deposits=int(live.sum()), mu1=int((d["mu"][live] >= 1).sum()), mu2=int((d["mu"][live] >= 2).sum()),
              zero=int(d["zero"].sum()), open_not_valid=d["open_not_valid"], dmin=float(d["absd"][live].min()))
    print(name, seed, st)
    assert st["mu1"] >= 159 and st["mu2"] >= 2
    assert 1 <= st["zero"] <= 2
    if spec.need is None:
        assert st["open_not_valid"] == 3
    assert 0.0029 <= st["dmin"] <= 0.0060
    want = reference_wave(h["rows"], crafted_nbr(), h["chan"], crafted_spec(name, d_floor=0.01))
    plain = reference_wave(h["rows"], crafted_nbr(), h["chan"], spec)
    assert want["clipped"] >= 1 and plain["clipped"] == 0
    assert want["cnt"].sum() == plain["cnt"].sum() - want["clipped"] and want["dropped"] == plain["dropped"]
    assert plain["dropped"] == st["zero"] and plain["cnt"].sum() == st["deposits"]


# ------------------------------------------------ invariants of the composition
@pytest.mark.parametrize("name", sorted(SPECS))
def test_per_ray_arrays_are_the_sibling_definitions(name):
    """theta and nseg equal reference_phase's, mu, first, nrow, close_row and
    dlast equal reference_tube's: the same values, bit for bit."""
    spec = crafted_spec(name, omega_dt=0.375)
    h = crafted_history(NT_CRAFTED, 3)
    theta0 = np.linspace(-1.0, 1.0, h["rows"].shape[0])
    got = reference_wave(h["rows"], crafted_nbr(), h["chan"], spec, theta0)
    ph = reference_phase(h["rows"], h["chan"], spec.phase_spec(), theta0)
    tu = reference_tube(h["rows"], crafted_nbr(), h["chan"], spec.tube_spec())
    for k in ("theta", "S"):
        assert got[k].tobytes() == ph[k].tobytes(), k
    assert got["nseg"].dtype == np.int32 and np.array_equal(got["nseg"], ph["nseg"])
    for k in ("mu", "first", "nrow", "close_row", "code"):
        assert got[k].dtype == tu[k].dtype and np.array_equal(got[k], tu[k]), k
    assert got["dlast"].tobytes() == tu["dlast"].tobytes()
    # every deposit is a tube point and a phase point
    assert np.all(got["cnt"] <= tu["cnt"]) and np.all(got["cnt"] <= ph["cnt"])
    assert got["cnt"].dtype == np.int64 and got["cnt"].shape == spec.shape


def _lattice_history(nt, scale_x, scale_y, seed=11, nn=3):
    """A ``nn x nn`` lattice, one wavenumber, carried by a diagonal linear map
    ``(scale_x[i], scale_y[i])``; k, l random, amp positive."""
    rng = np.random.default_rng(seed)
    iy, ix = (a.reshape(-1) for a in np.meshgrid(np.arange(nn), np.arange(nn), indexing="ij"))
    rows = rng.uniform(-3.0, 3.0, (nn * nn, nt, 8))
    for i in range(nt):
        rows[:, i, 0] = 1.0 + 0.01 * i + 0.0625 * scale_x[i] * (ix - 1)
        rows[:, i, 1] = 0.2 + 0.004 * i + 0.03125 * scale_y[i] * (iy - 1)
    rows[..., 4] = rng.uniform(0.5, 2.0, (nn * nn, nt))
    return rows, lattice_neighbours(nn, nn, 1, nlead=1)


def test_before_any_caustic_and_without_spreading_it_is_the_phase_map():
    """spread=False on a history whose rows are all open and all before any
    caustic: mu == 0 everywhere, so the maps are reference_phase's on those
    rows (the sums taken in another order)."""
    nt = 9
    rows, nbr = _lattice_history(nt, 1.0 + 0.05 * np.arange(nt), 1.0 - 0.03 * np.arange(nt))
    for kw in (dict(), dict(omega_dt=0.25), dict(weight=None, need=None)):
        spec = WaveSpec(**{**dict(nx=36, ny=18, weight="amp", spread=False), **kw})
        got = reference_wave(rows, nbr, None, spec)
        ph = reference_phase(rows, None, spec.phase_spec())
        assert got["mu"].tolist() == [0] * 9 and got["nrow"].tolist() == [nt] * 9 and got["dropped"] == 0
        assert np.array_equal(got["cnt"], ph["cnt"]) and got["cnt"].sum() == 9 * nt
        a = got["wabs"]
        for k in ("re", "im"):
            assert np.all(np.abs(got[k] - ph[k]) <= sum_bound(got["cnt"], a)), k
        if spec.wcol >= 0:
            assert np.all(np.abs(got["wabs"] - ph["wabs"]) <= sum_bound(got["cnt"], a))
        else:
            assert ph["wabs"] is None and np.array_equal(got["wabs"], got["cnt"].astype(np.float64))
    # with spreading the weights differ: |D| != 1 behind row 0
    wide = reference_wave(rows, nbr, None, WaveSpec(36, 18, weight="amp"))
    assert not np.array_equal(wide["wabs"], got["wabs"]) and np.array_equal(wide["cnt"], got["cnt"])


def test_flipping_one_rays_maslov_parity_changes_re():
    """A hand-made case: a 2 x 2 lattice of which two rays deposit (the other
    two, in no channel, only span the stencils).  Moving the northern
    neighbour of ray 0 across it from row 2 on reflects that ray's tube: its mu
    goes from 0 to 1, ray 1's stays, and ray 0's deposits from row 2 on turn
    from w cos(psi) into w cos(psi - pi/2) -- the Maslov term is not vacuous."""
    nt = 5
    rng = np.random.default_rng(7)
    rows = rng.uniform(-1.0, 1.0, (4, nt, 8))
    x, y = np.array([0.0, 0.05, 0.0, 0.05]), np.array([0.0, 0.0, 0.04, 0.04])
    for i in range(nt):
        rows[:, i, 0] = 1.0 + 0.02 * i + x
        rows[:, i, 1] = 0.3 + 0.01 * i + y
    rows[..., 4] = 1.5
    nbr = lattice_neighbours(2, 2, 1, nlead=1)
    chan = np.array([0, 0, -1, -1])
    spec = WaveSpec(36, 18, weight="amp", spread=False, need=None)
    flipped = rows.copy()
    flipped[2, 2:, 1] -= 0.08                      # ray 2, ray 0's N neighbour, now lies south of it
    a, b = reference_wave(rows, nbr, chan, spec), reference_wave(flipped, nbr, chan, spec)
    assert a["mu"].tolist() == [0, 0, 0, 0] and b["mu"].tolist() == [1, 0, 0, 0] and b["first"][0] == 2
    assert a["nrow"].tolist() == [nt, nt, 0, 0] and b["nrow"].tolist() == [nt, nt, 0, 0]
    assert np.array_equal(a["cnt"], b["cnt"]) and a["cnt"].sum() == 2 * nt
    assert a["theta"].tobytes() == b["theta"].tobytes()          # ray 0 and ray 1 did not move
    assert not np.array_equal(a["re"], b["re"])
    # by hand: ray 0's rows 2.. lose w cos(theta) and gain w cos(theta - pi/2)
    from phase import phase_along
    theta = phase_along(rows, chan, spec.phase_spec())[0][0]
    lost = sum(1.5 * math.cos(theta[i]) for i in range(2, nt))
    gain = sum(1.5 * math.cos(theta[i] - HALF_PI) for i in range(2, nt))
    assert abs((b["re"].sum() - a["re"].sum()) - (gain - lost)) <= 1e-13 * 1.5 * 2 * nt
    assert abs(gain - lost) > 0.1


# ---------------------------------------------------------------- the spec
def test_spec():
    assert ctypes.sizeof(H.WaveMapC) == 72
    s = WaveSpec(36, 18)
    assert (s.nchan, s.lat_range, s.need, s.weight, s.spread, s.max_sep, s.omega_dt, s.d_floor) == \
        (1, (-90, 90), "amp", None, True, 0.5, 0.0, 0.0)
    assert s.shape == (1, 18, 36) and (s.ncol, s.wcol) == (4, -1)
    u = WaveSpec(1440, 720, nchan=3, lat_range=(-60, 60), need=None, weight="ug", spread=False, max_sep=INF,
                 omega_dt=-0.25, d_floor=0.125)
    c = u.c_struct()
    assert (c.nx, c.ny, c.nchan, c.need, c.wcol, c.spread) == (1440, 720, 3, -1, 5, 0)
    assert (c.lat0, c.inv_dlat, c.inv_dlon) == (-PI / 3, 720 / (PI / 3 - -PI / 3), 1440 / (2 * PI))
    assert (c.max_sep, c.omega_dt, c.d_floor) == (INF, -0.25, 0.125)
    t, p = u.tube_spec(), u.phase_spec()
    assert (t.nx, t.ny, t.nchan, t.need, t.max_sep, t.lat_range) == (1440, 720, 3, None, INF, (-60, 60))
    assert (p.nx, p.ny, p.nchan, p.need, p.weight, p.omega_dt, p.lat_range) == (1440, 720, 3, None, "ug", -0.25, (-60, 60))
    from raymap import with_channels
    assert with_channels(u, 7).nchan == 7 and with_channels(u, 7).d_floor == 0.125
    with pytest.raises(Exception):
        u.nx = 3                                         # frozen
    for bad in (dict(nx=0), dict(ny=-1), dict(nchan=0), dict(nx=2 ** 16, ny=2 ** 15), dict(lat_range=(10.0, 10.0)),
                dict(need="lon"), dict(weight="lat"), dict(max_sep=0.0), dict(max_sep=-1.0), dict(max_sep=NAN),
                dict(omega_dt=INF), dict(omega_dt=NAN), dict(d_floor=-0.5), dict(d_floor=INF), dict(d_floor=NAN),
                dict(spread=2)):
        with pytest.raises(ValueError):
            WaveSpec(**{**dict(nx=7, ny=5), **bad})


# -------------------------------------------- csrc/wave_rows.h on the host
host_program = hostprog.fixture("wave_rows")


@pytest.mark.parametrize("name,seed", CASES)
def test_rows_host_program_under_sanitizers(host_program, name, seed):
    """csrc/wave_rows.h (what the kernel calls) in a stand-alone program built
    with ASan + UBSan and run directly: row 0, then the launch [1, 24) in all
    three row layouts and in three splits.  Integers, clipped and dropped equal
    reference_wave, the floats within the bars of assert_wave; every split and
    layout gives the same per-ray state bit for bit."""
    spec = crafted_spec(name)
    h = crafted_history(NT_CRAFTED, seed)
    nbr = crafted_nbr()
    want = reference_wave(h["rows"], nbr, h["chan"], spec)
    first = None
    for layout in LAYOUTS:
        for split, bounds in SPLITS.items():
            got = run_host_program(host_program, spec, nbr, launches_of(h, bounds, layout))
            assert got["bad"] == 0
            assert_wave(got, want, (name, seed, layout, split))
            first = first or got
            assert_same_run(first, got, want, (name, seed, layout, split))


@pytest.mark.parametrize("name", sorted(SPECS))
def test_rows_host_program_d_floor_omega_and_no_spreading(host_program, name):
    """d_floor = 0.01 clips at least one row; omega_dt != 0 deposits a
    constant tail row by row; spread=False; theta0; a launch from row 0."""
    h = crafted_history(NT_CRAFTED, 2)
    nbr = crafted_nbr()
    theta0 = np.linspace(-2.0, 2.0, h["rows"].shape[0])
    for kw in (dict(d_floor=0.01), dict(omega_dt=0.375), dict(spread=False, weight=None, omega_dt=-0.5, d_floor=0.01)):
        spec = crafted_spec(name, **kw)
        want = reference_wave(h["rows"], nbr, h["chan"], spec, theta0)
        if spec.d_floor:
            assert want["clipped"] >= 1
        first = None
        for layout, split in (("slots", "three"), ("tails", "five"), ("dense", "one")):
            got = run_host_program(host_program, spec, nbr, launches_of(h, SPLITS[split], layout), theta0=theta0)
            assert_wave(got, want, (name, kw, layout, split))
            first = first or got
            assert_same_run(first, got, want, (name, kw, layout, split))
    whole = [(dict(i0=0, i1=NT_CRAFTED, rows=h["rows"], tail=h["tail"], tf=np.full(len(h["tf"]), NT_CRAFTED),
                   chan=h["chan"]), "dense")]
    got = run_host_program(host_program, spec, nbr, whole, theta0=theta0)
    assert_wave(got, want, (name, "one launch from row 0"))
    assert_same_run(first, got, want, (name, "one launch from row 0"))


def test_rows_host_program_bad_neighbours(host_program):
    """A neighbour index out of range is not followed: the error flag is set,
    the index counts as no neighbour."""
    spec = crafted_spec("7x5")
    h = crafted_history(NT_CRAFTED, 1)
    nbr = crafted_nbr()
    bad = nbr.copy()
    bad[1, 14] = nbr.shape[1]
    bad[2, 15] = -2
    got = run_host_program(host_program, spec, bad, launches_of(h, [(1, 24)], "slots"))
    assert got["bad"] == 1
    fixed = bad.copy()
    fixed[1, 14] = fixed[2, 15] = -1
    assert_wave(got, reference_wave(h["rows"], fixed, h["chan"], spec), "out of range as none")


# ----------------------------------------------------------- C entry point
def _call(lib, m, nray=16, i0=1, i1=5, rows=64, slot=None, tfrom=None, trow=None, chan=None, nbr=64, si=64, sf=64,
          cnt=64, re=64, im=64, wabs=64, dropped=64, clipped=64, err=64):
    """rwrt_ray_wave with fake (never dereferenced) device pointers."""
    return H.entry("rwrt_ray_wave")(None if m is None else ctypes.byref(m), nray, i0, i1, rows, slot, tfrom, trow,
                                    chan, nbr, si, sf, cnt, re, im, wabs, dropped, clipped, err, None)


def test_wave_argument_errors_without_a_gpu():
    """Every check happens before any HIP call (there is no device on the
    build host to ask for) and names the argument."""
    lib = H.load()
    assert "rwrt_ray_wave" in H.ABI_SYMBOLS and hasattr(lib, "rwrt_ray_wave")
    assert "rwrt_ray_wave" in H.LATER_SIGNATURES and lib.rwrt_ray_wave.argtypes is None
    assert "abi 5" in H.version()                      # an additive member: the version stays
    spec = WaveSpec(7, 5, nchan=2, lat_range=(-60.0, 60.0), weight="amp")
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
        (dict(m=m(spread=2)), b"spread"), (dict(m=m(spread=-1)), b"spread"),
        (dict(m=m(inv_dlon=0.0)), b"inv_dlon"), (dict(m=m(inv_dlon=NAN)), b"inv_dlon"),
        (dict(m=m(inv_dlon=INF)), b"inv_dlon"), (dict(m=m(inv_dlat=-1.0)), b"inv_dlat"),
        (dict(m=m(inv_dlat=INF)), b"inv_dlat"), (dict(m=m(lat0=NAN)), b"lat0"), (dict(m=m(lat0=-INF)), b"lat0"),
        (dict(m=m(max_sep=0.0)), b"max_sep"), (dict(m=m(max_sep=-0.5)), b"max_sep"), (dict(m=m(max_sep=NAN)), b"max_sep"),
        (dict(m=m(omega_dt=NAN)), b"omega_dt"), (dict(m=m(omega_dt=INF)), b"omega_dt"),
        (dict(m=m(d_floor=-1e-3)), b"d_floor"), (dict(m=m(d_floor=NAN)), b"d_floor"), (dict(m=m(d_floor=INF)), b"d_floor"),
        (dict(m=good, i0=5, i1=5), b"it_begin"), (dict(m=good, i0=6, i1=5), b"it_begin"),
        (dict(m=good, i0=-1, i1=3), b"it_begin"),
        (dict(m=good, slot=64), b"d_row_slot"),
        (dict(m=good, tfrom=64), b"d_tail_row"), (dict(m=good, trow=64), b"d_tail_from"),
        (dict(m=good, rows=None), b"d_rows"),
        (dict(m=good, nray=-1), b"nray"), (dict(m=good, nray=1 << 31), b"nray"),
        (dict(m=good, rows=72), b"16-byte"), (dict(m=good, tfrom=64, trow=72), b"16-byte"),
        (dict(m=good, nbr=None), b"d_nbr"), (dict(m=good, si=None), b"d_state_i"), (dict(m=good, sf=None), b"d_state_f"),
        (dict(m=good, cnt=None), b"d_cnt"), (dict(m=good, re=None), b"d_re"), (dict(m=good, im=None), b"d_im"),
        (dict(m=good, wabs=None), b"d_wabs"), (dict(m=good, dropped=None), b"d_dropped"),
        (dict(m=good, clipped=None), b"d_clipped"), (dict(m=good, err=None), b"d_err"),
    ]
    for kw, word in cases:
        refused(lib, _call, kw, word, b"rwrt_ray_wave: ")
    # the output pointers are checked with no rays too
    assert _call(lib, good, nray=0, rows=None, clipped=None) == H.RWRT_ERR_ARG
    # no rays: a no-op (no device is touched; there is none on the build host)
    assert _call(lib, good, nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, good, nray=0, rows=None, i0=0, i1=1) == H.RWRT_OK
    assert _call(lib, m(need=-1, wcol=-1, max_sep=INF, d_floor=0.0, spread=0), nray=0, rows=None, i0=100, i1=200) == H.RWRT_OK
    assert _call(lib, WaveSpec(1440, 720, nchan=12).c_struct(), nray=0, rows=None) == H.RWRT_OK


# ------------------------------------------------------------ WR.ray_wave
def test_ray_wave_refusals_before_any_work():
    """A process group, and sources without a lattice and without nbr, are
    refused before ray_initial (which would need the basic state): row 0 of
    the history stays untouched."""
    from wr import WR
    w = WR(2, 6, 7200.0, 86400.0, 0.0, nx=144, ny=73)
    w.set_zwn([2.0, 4.0])
    spec = WaveSpec(36, 18)
    w.set_source_array([10.0, 12.0, 14.0, 10.0, 12.0, 14.0], [20.0, 20.0, 20.0, 22.0, 22.0, 22.0])
    with pytest.raises(ValueError, match="nbr"):
        w.ray_wave(spec)
    w.set_source_matrix(10.0, 20.0, 2.0, 2.0, 3, 2)
    with pytest.raises(NotImplementedError, match="neighbours"):
        w.ray_wave(spec, group=object())
    with pytest.raises(ValueError):
        w.ray_wave(spec, nbr=np.zeros((4, 5), np.int32))
    with pytest.raises(ValueError):
        w.ray_wave(spec, by="source")
    assert np.isnan(w.rlon).all()
