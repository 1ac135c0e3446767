"""Caustic-aware wave-field maps on the GPU (``rwrt_ray_wave``, wave.py):
``cnt``, ``nseg``, ``mu``, ``first``, ``nrow``, ``close_row``, ``dropped`` and
``clipped`` equal the definition ``wave.reference_wave`` exactly, ``theta``,
``dlast``, ``re``, ``im`` and ``wabs`` agree within the bars of
``support.cases_wave.assert_wave`` (phase's and tube's own bars, composed) --
on the crafted history of the tube tests in every row layout and split, on the
two lattices of real rays through ``WR.ray_wave`` (forward, backward,
``by='zwn'``, ``mode='numpy'``), next to a ``PhaseSink`` and a ``TubeSink`` in
one ``Tee`` (whose per-ray arrays it must give bit for bit) and through
``EnsembleWR.reduce`` over a member stack.

Fixture of the real rays: lattice (A) on the non-zonal state and (B) on the
zonal one (tests/support/cases_tube.py: 252 slots, 121 rows of 2 h); each
history, reference and map is computed once per module."""
import numpy as np
import pytest
import torch

import _hip as H
from phase import PhaseMap, PhaseSink
from summary import Tee
from support import cases_phase, cases_tube
from support.cases import bs_of
from support.cases_tube import NT, TSTEP, lattice_cfg, lattice_nbr
from support.cases_wave import (NRAY, NT_CRAFTED, SEEDS, SPECS, SPLITS, assert_same_run, assert_wave,
                                crafted_history, crafted_nbr, crafted_spec, deposits, device_layouts,
                                numpy_with_state, start, sum_bound)
from support.rows import LAYOUTS
from tube import TubeMap, TubeSink, lattice_neighbours
from wave import WaveMap, WaveSink, WaveSpec, reference_wave

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPEC = WaveSpec(36, 18, weight="amp")
_REAL = {}


def _wr(name, backward=False, kind=None):
    from wr import WR
    own, c = lattice_cfg(name)
    bs = bs_of(kind or own)
    w = WR(c.nzwn, c.nsource, TSTEP, (NT - 1) * TSTEP, 0.0, nx=bs.nlon, ny=bs.nlat, backward=backward)
    w.bs = bs
    w.set_zwn(c.zwn)
    w.set_source_matrix(c.SW_lon, c.SW_lat, c.dlon, c.dlat, c.nnx, c.nny)
    return w


def real(name, backward=False, kind=None, spec=SPEC):
    """``ray_run``'s history ``[252, 121, 8]`` of the lattice, its reference
    and the map of ``WR.ray_wave`` -- computed once."""
    kind = kind or lattice_cfg(name)[0]
    key = (name, backward, kind, spec)
    if key not in _REAL:
        hkey = (name, backward, kind)
        with np.errstate(all="ignore"):
            if hkey not in _REAL:
                hist = _wr(name, backward, kind)._history_rows("rk45", "numpy", None)
                hist.setflags(write=False)
                _REAL[hkey] = hist
            hist = _REAL[hkey]
            want = reference_wave(hist, lattice_nbr(name), None, spec)
            w = _wr(name, backward, kind)
            m = w.ray_wave(spec)
        assert np.isnan(w.rlon[1:]).all() and not np.isnan(w.rlon[0]).any()
        for a in (v for v in want.values() if isinstance(v, np.ndarray)):
            a.setflags(write=False)
        _REAL[key] = dict(hist=hist, want=want, map=m, got=m.numpy())
    return _REAL[key]


# ------------------------------------------------------ crafted history
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", sorted(SPECS))
def test_crafted_rows_every_layout_and_split(name, seed):
    """The crafted history of the host tests (40 rays: a partial wave; jac ==
    0, deposits behind one and two caustics, rows that are tube-open and not
    phase-valid, one-sided stencils, tails of differing tail_from among a
    stencil's rays, sentinel rows where nothing may be read) in every layout
    and in three splits, against the reference and against one another."""
    spec = crafted_spec(name)
    h = crafted_history(NT_CRAFTED, seed)
    nbr = crafted_nbr()
    want = reference_wave(h["rows"], nbr, h["chan"], spec)
    assert want["mu"].sum() >= 10 and want["dropped"] >= 1 and want["cnt"].sum() >= 159
    first = None
    for layout in LAYOUTS:
        for split, bounds in SPLITS.items():
            m = start(WaveMap(spec, NRAY, nbr, DEV, h["chan"]), h["rows"][:, 0])
            for i0, i1 in bounds:
                m.add_rows(i0, i1, *device_layouts(h, i0, i1)[layout])
            got = numpy_with_state(m)
            assert_wave(got, want, (name, seed, layout, split))
            first = first or got
            assert_same_run(first, got, want, (name, seed, layout, split))


@pytest.mark.parametrize("name", sorted(SPECS))
def test_crafted_rows_d_floor_omega_theta0_and_restart(name):
    """d_floor = 0.01 clips at least one row; omega_dt != 0 deposits a constant
    tail row by row; spread=False; theta0; one dense launch from row 0 fixes
    the stencils itself; restart() starts over."""
    h = crafted_history(NT_CRAFTED, 2)
    nbr = crafted_nbr()
    theta0 = np.linspace(-2.0, 2.0, NRAY)
    for kw in (dict(d_floor=0.01), dict(omega_dt=0.375), dict(spread=False, weight=None, omega_dt=-0.5, d_floor=0.01)):
        spec = crafted_spec(name, **kw)
        want = reference_wave(h["rows"], nbr, h["chan"], spec, theta0)
        if spec.d_floor:
            assert want["clipped"] >= 1
        first = None
        for layout, split in (("slots", "three"), ("tails", "five"), ("dense", "one")):
            m = start(WaveMap(spec, NRAY, nbr, DEV, h["chan"], theta0), h["rows"][:, 0])
            for i0, i1 in SPLITS[split]:
                m.add_rows(i0, i1, *device_layouts(h, i0, i1)[layout])
            got = numpy_with_state(m)
            assert_wave(got, want, (name, kw, layout, split))
            first = first or got
            assert_same_run(first, got, want, (name, kw, layout, split))
    m = WaveMap(spec, NRAY, nbr, DEV, h["chan"], theta0)
    m.add_rows(0, NT_CRAFTED, torch.as_tensor(h["rows"], device=DEV))
    assert_same_run(first, numpy_with_state(m), want, "from row 0")
    kept = m.numpy()["cnt"]
    assert m.restart() is m and int(m.nrow.sum()) == 0 and int(m.nseg.sum()) == 0
    assert torch.equal(m.theta, m.theta0) and torch.isnan(m.prev[:4]).all() and torch.isnan(m.prev[5:]).all()
    m.add_rows(1, 5, torch.as_tensor(h["rows"][:, 1:5], device=DEV))          # no row 0 since: every tube is closed
    assert np.array_equal(m.numpy()["cnt"], kept) and int(m.nrow.sum()) == 0
    assert int(m.nseg.sum()) > 0                                              # ... and the phase goes on


# ------------------------------------------------------ parity on real rays
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("name", ["A", "B"])
def test_ray_wave_equals_the_reference_on_the_history(name, backward):
    """WR.ray_wave against reference_wave of the same run's history; from the
    reference alone: at least 20 deposits behind a caustic."""
    f = real(name, backward)
    d = deposits(f["hist"], lattice_nbr(name), None, SPEC)
    behind = int((d["mu"][~d["zero"]] >= 1).sum())
    print(name, backward, dict(deposits=int(f["want"]["cnt"].sum()), behind_a_caustic=behind,
                               caustics=int(f["want"]["mu"].sum()), dropped=f["want"]["dropped"]))
    assert behind >= 20 and f["want"]["mu"].sum() >= 20
    assert_wave(f["got"], f["want"], (name, backward))
    c = lattice_cfg(name)[1]
    assert f["got"]["mu"].reshape(3, c.nsource, c.nzwn).shape == (3, 42, 2)
    if backward:
        assert not np.array_equal(f["want"]["cnt"], real(name)["want"]["cnt"])
        assert np.array_equal(f["want"]["code"], real(name)["want"]["code"])      # (row 0 is the same row)


def test_by_zwn_and_mode_numpy():
    """by='zwn' splits the same deposits into one map per wavenumber; the
    per-ray arrays do not change; mode='numpy' is the reference on the
    delivered history."""
    f = real("A")
    with np.errstate(all="ignore"):
        m = _wr("A").ray_wave(SPEC, by="zwn")
        host = _wr("A").ray_wave(SPEC, mode="numpy")
    got = m.numpy()
    assert m.spec.nchan == 2 and np.array_equal(got["cnt"].sum(axis=0), f["want"]["cnt"][0])
    assert got["cnt"][1].sum() > 100
    for k in ("mu", "first", "nrow", "close_row", "nseg"):
        assert np.array_equal(got[k], f["got"][k]), k
    for k in ("theta", "dlast"):
        assert got[k].tobytes() == f["got"][k].tobytes(), k
    chan = np.tile(np.arange(2), 3 * 42).astype(np.int32)
    assert_wave(got, reference_wave(f["hist"], lattice_nbr("A"), chan, m.spec), "by zwn")
    for k in ("cnt", "re", "im", "wabs", "theta", "nseg", "mu", "nrow", "dlast"):
        assert np.array_equal(host[k], f["want"][k], equal_nan=True), k
    assert host["dropped"] == f["want"]["dropped"] and host["clipped"] == 0


# -------------------------------------------- against the sibling products
def test_one_tee_with_the_phase_and_the_tube_product():
    """One integration into Tee(PhaseSink, TubeSink, WaveSink), omega_dt != 0,
    in launches of 37 rows: theta and nseg are PhaseMap's, mu, first, nrow,
    close_row and dlast are TubeMap's, bit for bit; the wave map is the
    reference's, and it is not the phase map."""
    name = "A"
    f = real(name)
    spec = WaveSpec(36, 18, weight="amp", omega_dt=0.375)
    w = _wr(name)
    eng = w.bs.engine()
    rows0 = eng.initial_rows(w.source_lon, w.source_lat, w.zwn, w.freq)            # [7, 3, ns, nz]
    r0 = rows0.reshape(7, -1).cpu().numpy()
    y0 = rows0[:5].reshape(5, -1).contiguous()
    nray, nbr = r0.shape[1], lattice_nbr(name)
    pm = cases_phase.start(PhaseMap(spec.phase_spec(), nray, eng.device), r0.T)
    tm = cases_tube.start(TubeMap(spec.tube_spec(), nray, nbr, eng.device), r0.T)
    wm = start(WaveMap(spec, nray, nbr, eng.device), r0.T)
    with np.errstate(all="ignore"):
        eng.integrate(y0.clone(), NT, TSTEP, ttotal=(NT - 1) * TSTEP, chunk=37,
                      sink=Tee(PhaseSink(pm), TubeSink(tm), WaveSink(wm)))
        want = reference_wave(f["hist"], nbr, None, spec)
    got, ph, tu = wm.numpy(), pm.numpy(), tm.numpy()
    assert_wave(got, want, "tee")
    assert got["theta"].tobytes() == ph["theta"].tobytes() and np.array_equal(got["nseg"], ph["nseg"])
    assert wm.prev[:4].cpu().numpy().tobytes() == pm.prev.cpu().numpy().tobytes()      # the carried rows too
    for k in ("mu", "first", "nrow", "close_row"):
        assert np.array_equal(got[k], tu[k]), k
    assert got["dlast"].tobytes() == tu["dlast"].tobytes()
    assert got["mu"].sum() >= 20 and got["nseg"].sum() > 1000
    # the same rays as WR.ray_wave's: only psi turns with the row
    assert got["theta"].tobytes() == f["got"]["theta"].tobytes() and np.array_equal(got["cnt"], f["got"]["cnt"])
    assert np.all(got["cnt"] <= ph["cnt"]) and np.all(got["cnt"] <= tu["cnt"]) and got["cnt"].sum() < ph["cnt"].sum()
    assert not np.allclose(got["re"], ph["re"])


# ------------------------------------------------- refusals, fields, output
def test_what_a_wave_map_refuses():
    spec = crafted_spec("7x5")
    h = crafted_history(NT_CRAFTED, 3)
    nbr = crafted_nbr()
    for bad in (nbr[:, :-1], nbr.astype(np.float64), np.where(nbr == 0, NRAY, nbr), np.where(nbr == 0, -2, nbr)):
        with pytest.raises(ValueError):
            WaveMap(spec, NRAY, bad, DEV)
    with pytest.raises(ValueError):
        WaveMap(spec, NRAY, nbr, DEV, theta0=np.zeros(3))
    m = WaveMap(spec, NRAY, nbr, DEV, h["chan"])
    with pytest.raises(ValueError, match="k and l"):
        m.start(h["rows"][:, 0, 0], h["rows"][:, 0, 1], h["rows"][:, 0, 4], h["rows"][:, 0, 4])
    start(m, h["rows"][:, 0])
    rows = torch.as_tensor(h["rows"], device=DEV)
    with pytest.raises(ValueError):
        m.add_rows(1, 3, rows[:5, 1:3].contiguous())                          # 5 rays for 40 columns
    with pytest.raises(NotImplementedError):
        m.add_rows(1, 3, rows[:5, 1:3].contiguous(), ray=torch.arange(5, device=DEV))
    with pytest.raises(NotImplementedError):
        WaveSink(m).take(np.arange(5))
    with pytest.raises(NotImplementedError):
        m.allreduce(None)
    # an index that went bad on the device is not followed: the error word says so
    m.nbr[1, 4] = NRAY + 7
    m.add_rows(0, 1, rows[:, :1].contiguous())
    m.add_rows(1, 3, rows[:, 1:3].contiguous())
    with pytest.raises(H.RwrtError, match="neighbour"):
        m.numpy()


def test_derived_fields_and_output(tmp_path):
    import ncio
    f = real("A")
    m, got = f["map"], f["got"]
    cnt, hit = got["cnt"], got["cnt"] > 0
    amp = np.hypot(got["re"], got["im"])
    for name, want in (("field", got["re"]), ("amplitude", amp), ("mean_phase", np.arctan2(got["im"], got["re"])),
                       ("coherence", amp / np.where(hit, got["wabs"], 1.0))):
        a = getattr(m, name)().cpu().numpy()
        assert np.array_equal(np.isnan(a), ~hit), name
        assert np.allclose(a[hit], want[hit], rtol=1e-13, atol=1e-300), name
    coh = m.coherence().cpu().numpy()[hit]
    assert np.all(coh <= 1.0 + 1e-12)
    # (a quotient of the device's: it may be a product with 1 / 2 pi, one more rounding)
    assert np.allclose(m.cycles().cpu().numpy(), got["theta"] / (2.0 * np.pi), rtol=4e-16, atol=0.0)
    for name in ("wave.nc", "wave.npz"):
        path = str(tmp_path / name)
        m.output(path)
        d = ncio.read(path)
        assert d["cnt"].shape == (1, 18, 36) and np.array_equal(d["cnt"], cnt)
        assert d["cnt"].dtype.kind == ("i" if name.endswith(".npz") else "f")
        for k in ("re", "im", "wabs", "theta", "dlast"):
            assert np.array_equal(d[k], got[k], equal_nan=True), k
        for k in ("nseg", "mu", "first", "nrow", "close_row"):
            assert np.array_equal(d[k], got[k]), k
        assert d["dropped"].tolist() == [float(got["dropped"])] and d["clipped"].tolist() == [0.0]
        assert d["lon_edges"].shape == (37,)


# --------------------------------------------------------- member stacks
def test_ensemble_reduce_by_member():
    """EnsembleWR.reduce with a WaveMap over a 2-member stack and the
    neighbours of nlead = 3 * 2, by='member': channel m and the rays of member
    m are WR.ray_wave on member m alone -- the integers and the per-ray floats
    exactly, the sums within the bound of a sum taken in any order."""
    import synthetic as S
    from ensemble import EnsembleWR
    from levels import Levels
    from raymap import with_channels
    kinds = ("nonzonal", "zonal")
    bgs = [S.background(k) for k in kinds]
    lv = Levels(bgs[0]["lat"], bgs[0]["lon"], 2)
    lv.set_levels(np.stack([b["u"] for b in bgs]), np.stack([b["v"] for b in bgs]))
    c = lattice_cfg("A")[1]
    ew = EnsembleWR(lv, c.nzwn, c.nsource, TSTEP, (NT - 1) * TSTEP)
    ew.set_zwn(c.zwn)
    ew.set_source_matrix(c.SW_lon, c.SW_lat, c.dlon, c.dlat, c.nnx, c.nny)
    nbr = lattice_neighbours(c.nnx, c.nny, c.nzwn, nlead=3 * ew.nmember)

    def make(device, chan, nray):
        m = WaveMap(with_channels(SPEC, ew.nmember), nray, nbr, device, chan)
        m.start(ew.rlon[0], ew.rlat[0], ew.ramp[0], ew.ramp[0], k=ew.rzwn[0], l=ew.rmwn[0])
        return m, WaveSink(m)

    with np.errstate(all="ignore"):
        got = ew.reduce(make, by="member").numpy()
    assert got["cnt"].shape == (2, 18, 36) and got["mu"].shape == (2 * 252,)
    for mem, kind in enumerate(kinds):
        f = real("A", kind=kind)
        alone, want = f["got"], f["want"]
        sel = slice(mem * 252, (mem + 1) * 252)
        assert np.array_equal(got["cnt"][mem], alone["cnt"][0])
        for k in ("mu", "first", "nrow", "close_row", "nseg"):
            assert np.array_equal(got[k][sel], alone[k]), (kind, k)
        for k in ("theta", "dlast"):
            assert got[k][sel].tobytes() == alone[k].tobytes(), (kind, k)
        bound = sum_bound(want["cnt"][0], want["wabs"][0])
        for k in ("re", "im", "wabs"):
            assert np.all(np.abs(got[k][mem] - alone[k][0]) <= bound), (kind, k)
        assert want["mu"].sum() >= 20
    assert got["dropped"] == sum(real("A", kind=k)["got"]["dropped"] for k in kinds)
