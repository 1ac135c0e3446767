"""Ray-tube maps on the GPU (``rwrt_ray_tube``, tube.py): ``cnt``, ``ncaus``,
``mu``, ``first``, ``nrow``, ``close_row`` and ``dropped`` equal the
definition ``tube.reference_tube`` exactly, ``dmin``, ``dlast``, ``f0`` and
``flast`` agree within 1e-12 relative and ``slog`` per box within the bound of
``support.cases_tube.assert_tube`` -- on the two lattices of real rays through
``WR.ray_tube`` (forward, backward, ``max_sep`` 0.5 and inf, ``by='zwn'``),
however the run is split into launches, in every row layout on crafted rows,
and through ``EnsembleWR.reduce`` over a member stack.

Fixture of the real rays: lattice (A) on the non-zonal state and (B) on the
zonal one (tests/support/cases_tube.py: 252 slots, 121 rows of 2 h); each
history, reference and map is computed once per module."""
import math

import numpy as np
import pytest
import torch

import _hip as H
from support.cases import bs_of
from support.cases_tube import (NRAY, NT, TSTEP, assert_same_run, assert_tube, crafted_history,
                                crafted_nbr, crafted_spec, device_layouts, lattice_cfg, lattice_nbr, start)
from support.rows import LAYOUTS
from tube import TubeMap, TubeSink, TubeSpec, lattice_neighbours, reference_tube, tube_valid

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPEC = TubeSpec(36, 18)
WIDE = TubeSpec(36, 18, max_sep=math.inf)
NT_CRAFTED = 24
SPLITS = {"one": [(1, 24)], "three": [(1, 9), (9, 10), (10, 24)], "five": [(1, 4), (4, 8), (8, 9), (9, 17), (17, 24)]}
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
    and the map of ``WR.ray_tube`` -- computed once."""
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
            want = reference_tube(hist, lattice_nbr(name), None, spec)
            w = _wr(name, backward, kind)
            m = w.ray_tube(spec)
        assert np.isnan(w.rlon[1:]).all() and not np.isnan(w.rlon[0]).any()
        for a in (v for v in want.values() if isinstance(v, np.ndarray)):
            a.setflags(write=False)
        _REAL[key] = dict(hist=hist, want=want, map=m, got=m.numpy())
    return _REAL[key]


def _stats(name, f):
    hist, want = f["hist"], f["want"]
    nbr = lattice_nbr(name)
    both = (nbr[0] >= 0) & (nbr[1] >= 0)
    raw = hist[nbr[1].clip(0), :, 0] - hist[nbr[0].clip(0), :, 0]
    ok = tube_valid(hist, SPEC)
    pair_ok = ok & ok[nbr[0].clip(0)] & ok[nbr[1].clip(0)]
    st = dict(tubes=int((want["nrow"] > 0).sum()), closing=int((want["close_row"] > 0).sum()),
              caustics=int(want["mu"].sum()), rays_with=int((want["mu"] > 0).sum()),
              one_sided=int(((want["code"] > 1).any(axis=0) & (want["nrow"] > 0)).sum()),
              wrapped=int((np.abs(raw[both][pair_ok[both]]) > math.pi).sum()),
              deposits=int(want["cnt"].sum()), dropped=int(want["dropped"]))
    print(name, st)
    return st


# ------------------------------------------------------ parity on real rays
def test_lattice_a_is_rich_enough():
    """Asserted from the reference alone, so that no comparison below passes
    vacuously: caustics, tubes closing in mid-run, one-sided stencils, wrapped
    differences, and a tube that max_sep = 0.5 closes before inf does."""
    f, g = real("A"), real("A", spec=WIDE)
    st = _stats("A", f)
    assert st["caustics"] >= 20 and st["closing"] >= 10 and st["one_sided"] >= 1 and st["wrapped"] >= 1
    a, b = f["want"]["close_row"], g["want"]["close_row"]
    earlier = (a > 0) & ((b < 0) | (b > a))
    print("closed earlier by max_sep = 0.5:", int(earlier.sum()), "of", int((a > 0).sum()))
    assert earlier.sum() >= 1
    assert _stats("B", real("B"))["caustics"] >= 20


@pytest.mark.parametrize("name", ["A", "B"])
def test_ray_tube_equals_the_reference_on_the_history(name):
    """WR.ray_tube against reference_tube of the same run's history."""
    f = real(name)
    assert_tube(f["got"], f["want"], name)
    c = lattice_cfg(name)[1]
    assert f["got"]["mu"].reshape(3, c.nsource, c.nzwn).shape == (3, 42, 2)
    # an open row is a ray point of the density map too
    from density import DensitySpec
    with np.errstate(all="ignore"):
        dens = _wr(name).ray_density(DensitySpec(36, 18, weight="amp")).count.cpu().numpy()
    assert np.all(f["got"]["cnt"] <= dens) and f["got"]["cnt"].sum() == f["want"]["nrow"].sum() - f["want"]["dropped"]


def test_max_sep_inf_against_half_a_radian():
    f, g = real("A"), real("A", spec=WIDE)
    assert_tube(g["got"], g["want"], "A, max_sep inf")
    assert g["got"]["nrow"].sum() > f["got"]["nrow"].sum()
    assert np.all(g["got"]["nrow"] >= f["got"]["nrow"])
    # the rows both keep open are the same rows: up to the first caustic they agree
    same = f["got"]["close_row"] == g["got"]["close_row"]
    assert same.sum() >= 20 and np.array_equal(f["got"]["mu"][same], g["got"]["mu"][same])
    assert f["got"]["dlast"][same].tobytes() == g["got"]["dlast"][same].tobytes()


def test_by_zwn_and_mode_numpy():
    """by='zwn' splits the same deposits into one map per wavenumber; the
    per-ray arrays do not change; mode='numpy' is the reference on the
    delivered history."""
    f = real("A")
    with np.errstate(all="ignore"):
        m = _wr("A").ray_tube(SPEC, by="zwn")
        host = _wr("A").ray_tube(SPEC, mode="numpy")
    got = m.numpy()
    assert m.spec.nchan == 2 and np.array_equal(got["cnt"].sum(axis=0), f["want"]["cnt"][0])
    assert np.array_equal(got["ncaus"].sum(axis=0), f["want"]["ncaus"][0]) and got["cnt"][1].sum() > 100
    for k in ("mu", "first", "nrow", "close_row"):
        assert np.array_equal(got[k], f["got"][k]), k
    for k in ("dmin", "dlast", "f0", "flast"):
        assert got[k].tobytes() == f["got"][k].tobytes(), k
    chan = np.tile(np.arange(2), 3 * 42).astype(np.int32)
    assert_tube(got, reference_tube(f["hist"], lattice_nbr("A"), chan, m.spec), "by zwn")
    for k in ("cnt", "ncaus", "slog", "mu", "nrow", "dlast"):
        assert np.array_equal(host[k], f["want"][k], equal_nan=True), k
    # an explicit nbr is the lattice's
    with np.errstate(all="ignore"):
        w, c = _wr("A"), lattice_cfg("A")[1]
        iy, ix = np.divmod(np.arange(c.nsource), c.nnx)
        w.set_source_array((c.SW_lon + ix * c.dlon) % 360.0, c.SW_lat + iy * c.dlat)      # (the same bits)
        assert np.array_equal(w.source_lon, _wr("A").source_lon) and np.array_equal(w.source_lat, _wr("A").source_lat)
        with pytest.raises(ValueError):
            w.ray_tube(SPEC)
        given = w.ray_tube(SPEC, nbr=lattice_nbr("A")).numpy()
    assert np.array_equal(given["cnt"], f["got"]["cnt"]) and np.array_equal(given["mu"], f["got"]["mu"])


def test_backward_ray_tube():
    """WR(backward=True).ray_tube against the reference on that history; the
    backward rays are not the forward ones."""
    f, fwd = real("A", backward=True), real("A")
    assert_tube(f["got"], f["want"], "A backward")
    assert f["want"]["nrow"].sum() > 1000 and not np.array_equal(f["want"]["cnt"], fwd["want"]["cnt"])
    assert np.array_equal(f["want"]["code"], fwd["want"]["code"])          # (row 0 is the same row)


# ------------------------------------------- one run, however it is split
def _engine_run(name, spec, **kw):
    w = _wr(name)
    eng = w.bs.engine()
    rows0 = eng.initial_rows(w.source_lon, w.source_lat, w.zwn, w.freq)            # [7, 3, ns, nz]
    r0 = rows0.reshape(7, -1).cpu().numpy()
    y0 = rows0[:5].reshape(5, -1).contiguous()
    sink_kw = {k: kw.pop(k) for k in ("takes_tails", "takes_slots") if k in kw}
    m = start(TubeMap(spec, r0.shape[1], lattice_nbr(name), eng.device), r0.T)
    sink = TubeSink(m)
    for k, v in sink_kw.items():
        setattr(sink, k, v)
    with np.errstate(all="ignore"):
        res = eng.integrate(y0.clone(), NT, TSTEP, ttotal=(NT - 1) * TSTEP, sink=sink, **kw)
    return m.numpy(), res.bounds


RUNS = {
    "one launch": (dict(), 1),
    "five launches of 24 rows": (dict(chunk=24), 5),
    "dense rows": (dict(chunk=40, takes_tails=False, takes_slots=False), 3),
    "tails": (dict(chunk=40, takes_slots=False), 3),
    "priority order after a short first launch": (dict(first_chunk=5), 2),
}


def test_one_run_however_it_is_split():
    """The same rays in one launch, in five launches of 24 rows, delivered
    dense, with tails and as row blocks, and ordered by the cost a short first
    launch has measured: the integers equal, the per-ray floats bit for bit."""
    f = real("A")
    first = None
    for what, (kw, nlaunch) in RUNS.items():
        got, bounds = _engine_run("A", SPEC, **kw)
        assert len(bounds) == nlaunch and bounds[0][0] == 1 and bounds[-1][1] == NT, (what, bounds)
        assert_tube(got, f["want"], what)
        first = first or got
        assert_same_run(first, got, f["want"], what)
    assert_same_run(first, f["got"], f["want"], "WR.ray_tube")


@pytest.mark.parametrize("name", ["7x5", "36x18-inf-no-need", "36x18-band-tight"])
def test_crafted_rows_every_layout_and_split(name):
    """The crafted history of the host tests (40 rays: a partial wave; jac ==
    0, NaN need, one-sided stencils, neighbours that are -1, tails of
    differing tail_from among a stencil's rays, sentinel rows where nothing
    may be read) in every layout and in three splits."""
    spec = crafted_spec(name)
    h = crafted_history(NT_CRAFTED, seed=3)
    nbr = crafted_nbr()
    want = reference_tube(h["rows"], nbr, h["chan"], spec)
    assert want["mu"].sum() >= 10 and (want["close_row"] > 0).sum() >= 5 and (nbr < 0).any()
    if name == "7x5":
        assert want["dropped"] >= 1
    first = None
    for layout in LAYOUTS:
        for split, bounds in SPLITS.items():
            m = start(TubeMap(spec, NRAY, nbr, DEV, h["chan"]), h["rows"][:, 0])
            for i0, i1 in bounds:
                m.add_rows(i0, i1, *device_layouts(h, i0, i1)[layout])
            got = m.numpy()
            assert_tube(got, want, (name, layout, split))
            first = first or got
            assert_same_run(first, got, want, (name, layout, split))
    # one dense launch from row 0 fixes the stencils itself; restart() starts over
    m = TubeMap(spec, NRAY, nbr, DEV, h["chan"])
    m.add_rows(0, NT_CRAFTED, torch.as_tensor(h["rows"], device=DEV))
    assert_same_run(first, m.numpy(), want, "from row 0")
    kept = m.numpy()["cnt"]
    assert m.restart() is m and int(m.nrow.sum()) == 0 and torch.isnan(m.prev).all()
    m.add_rows(1, 5, torch.as_tensor(h["rows"][:, 1:5], device=DEV))          # no row 0 since: every tube is closed
    assert np.array_equal(m.numpy()["cnt"], kept) and int(m.nrow.sum()) == 0


def test_what_a_tube_map_refuses():
    spec = crafted_spec("7x5")
    h = crafted_history(NT_CRAFTED, seed=3)
    nbr = crafted_nbr()
    for bad in (nbr[:, :-1], nbr.astype(np.float64), np.where(nbr == 0, NRAY, nbr), np.where(nbr == 0, -2, nbr)):
        with pytest.raises(ValueError):
            TubeMap(spec, NRAY, bad, DEV)
    m = start(TubeMap(spec, NRAY, nbr, DEV, h["chan"]), h["rows"][:, 0])
    rows = torch.as_tensor(h["rows"], device=DEV)
    with pytest.raises(ValueError):
        m.add_rows(1, 3, rows[:5, 1:3].contiguous())                          # 5 rays for 40 columns
    with pytest.raises(NotImplementedError):
        m.add_rows(1, 3, rows[:5, 1:3].contiguous(), ray=torch.arange(5, device=DEV))
    with pytest.raises(NotImplementedError):
        TubeSink(m).take(np.arange(5))
    with pytest.raises(NotImplementedError):
        m.allreduce(None)
    # an index that went bad on the device is not followed: the error word says so
    m.nbr[1, 4] = NRAY + 7
    m.add_rows(0, 1, rows[:, :1].contiguous())
    m.add_rows(1, 3, rows[:, 1:3].contiguous())
    with pytest.raises(H.RwrtError, match="neighbour"):
        m.numpy()


# ------------------------------------------------- derived fields, output
def test_derived_fields_and_output(tmp_path):
    import ncio
    f = real("A")
    m, got = f["map"], f["got"]
    cnt, hit = got["cnt"], got["cnt"] > 0
    safe = np.where(hit, cnt, 1)
    for name, want in (("mean_log_spreading", got["slog"] / safe),
                       ("geometric_amplitude", np.exp(-got["slog"] / (2.0 * safe))),
                       ("caustic_density", got["ncaus"] / safe)):
        a = getattr(m, name)().cpu().numpy()
        assert np.array_equal(np.isnan(a), ~hit), name
        assert np.allclose(a[hit], want[hit], rtol=1e-13, atol=0.0), name
    lam = m.ftle(TSTEP).cpu().numpy()
    two = got["nrow"] >= 2
    assert np.array_equal(np.isnan(lam), ~two) and two.sum() >= 50
    j = int(np.argmax(got["nrow"]))
    F0 = np.array([[got["f0"][0, j], got["f0"][2, j]], [got["f0"][1, j], got["f0"][3, j]]])
    F1 = np.array([[got["flast"][0, j], got["flast"][2, j]], [got["flast"][1, j], got["flast"][3, j]]])
    sig = np.linalg.svd(F1 @ np.linalg.inv(F0), compute_uv=False)[0]
    assert abs(lam[j] - math.log(sig) / ((got["nrow"][j] - 1) * TSTEP)) <= 1e-9 * abs(lam[j]) + 1e-18
    for name in ("tube.nc", "tube.npz"):
        path = str(tmp_path / name)
        m.output(path)
        d = ncio.read(path)
        assert d["cnt"].shape == (1, 18, 36) and np.array_equal(d["cnt"], cnt) and np.array_equal(d["ncaus"], got["ncaus"])
        assert d["cnt"].dtype.kind == ("i" if name.endswith(".npz") else "f")
        for k in ("slog", "dmin", "dlast", "f0", "flast"):
            assert np.array_equal(d[k], got[k], equal_nan=True), k
        for k in ("mu", "first", "nrow", "close_row"):
            assert np.array_equal(d[k], got[k]), k
        assert d["dropped"].tolist() == [float(got["dropped"])] and d["lon_edges"].shape == (37,)


# --------------------------------------------------------- member stacks
def test_ensemble_reduce_by_member():
    """EnsembleWR.reduce with a TubeMap over a 2-member stack and the
    neighbours of nlead = 3 * 2, by='member': channel m and the rays of member
    m are WR.ray_tube on member m alone -- the integers and the per-ray floats
    exactly, slog within the bound."""
    import synthetic as S
    from ensemble import EnsembleWR
    from levels import Levels
    from raymap import with_channels
    from support.cases_track import sum_bound
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
        m = TubeMap(with_channels(SPEC, ew.nmember), nray, nbr, device, chan)
        m.start(ew.rlon[0], ew.rlat[0], ew.ramp[0])
        return m, TubeSink(m)

    with np.errstate(all="ignore"):
        got = ew.reduce(make, by="member").numpy()
    assert got["cnt"].shape == (2, 18, 36) and got["mu"].shape == (2 * 252,)
    for mem, kind in enumerate(kinds):
        f = real("A", kind=kind)
        alone, want = f["got"], f["want"]
        sel = slice(mem * 252, (mem + 1) * 252)
        assert np.array_equal(got["cnt"][mem], alone["cnt"][0]) and np.array_equal(got["ncaus"][mem], alone["ncaus"][0])
        for k in ("mu", "first", "nrow", "close_row"):
            assert np.array_equal(got[k][sel], alone[k]), (kind, k)
        for k in ("dmin", "dlast"):
            assert got[k][sel].tobytes() == alone[k].tobytes(), (kind, k)
        for k in ("f0", "flast"):
            assert got[k][:, sel].tobytes() == alone[k].tobytes(), (kind, k)
        assert np.all(np.abs(got["slog"][mem] - alone["slog"][0]) <= sum_bound(want["cnt"][0], want["sabs"][0]))
        assert want["mu"].sum() >= 20
    assert got["dropped"] == sum(real("A", kind=k)["got"]["dropped"] for k in kinds)
