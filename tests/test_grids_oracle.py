"""The CPU oracle and the host ``BS`` equal the reference off the 144 x 73 grid.

``tests/golden/grid_<name>.npz`` hold the reference's own records on five
grids (``support/cases_grids.py``; made by ``tests/golden/make_grid_golden.py``):
1 degree, 10 degrees, 33 x 127, the non-cyclic 73 x 144 and 0.25 degrees.  This
file pins ``oracle/rwrt_oracle.py`` and ``bs.BS.ready`` to them bit for bit
before ``tests/test_gpu_grids.py`` compares the kernels with the same records,
and asserts that the records still contain the events they were chosen for
(seam crossings, rejected attempts, dying rays, the clamped cells).
"""
import hashlib

import numpy as np
import pytest

import rwrt_oracle as O
from support import cases_grids as CG
from support.bits import bitwise

GRIDS = list(CG.STATIC)


def sha(F):
    return hashlib.sha256(np.ascontiguousarray(F, dtype=np.float64).tobytes()).hexdigest()


def sample(F):
    return F[::-(-F.shape[0] // 8), ::-(-F.shape[1] // 8), :]


@pytest.mark.parametrize("name", GRIDS)
def test_events_in_the_committed_records(name):
    """What the fixtures were chosen for is still in them: enough live rays,
    dying rays, rejected attempts, live seam crossings; on ``nc`` rows in the
    clamped last column; on ``g1`` and ``q`` the clamped seam cell at
    ``nextafter(2 pi, 0)``; the clamped top row exactly where the latitude axis
    reaches it (2.5 degrees, ``g10``, ``g127``, ``q``; not ``g1``)."""
    g = CG.golden(name)
    e = CG.check_events(name, g)
    assert g["hist"].shape[2] == CG.NRAY and g["track"].shape == (2, CG.NT, CG.NRAY)
    assert g["rows"][0] == 0 and g["rows"][-1] == CG.NT - 1 and g["rk4_rows"][-1] == CG.NT - 1
    assert bitwise(g["hist"][:2], g["track"][:, g["rows"]])
    assert e["top_reaches"] == (name != "g1")


@pytest.mark.refhost
@pytest.mark.parametrize("name", GRIDS)
def test_oracle_fields_bitwise(name):
    g = CG.golden(name)
    bg = CG.background(name)
    assert tuple(g["shape"]) == bg.fields.shape
    assert bitwise(bg.lat, g["lat"]) and bitwise(bg.lon, g["lon"])
    assert bitwise(sample(bg.fields), g["sample"])
    assert sha(bg.fields) == str(g["sha256"])


@pytest.mark.refhost
@pytest.mark.parametrize("name", GRIDS)
def test_host_bs_ready_fields_bitwise(name):
    """The package's host ``BS.load_arrays`` + ``ready(xcyclic=)``: the same hash
    (``q`` included: 721 x 1440 takes about a second)."""
    from bs import BS
    g = CG.golden(name)
    st = CG.state(name)
    bs = BS(len(st["lon"]), len(st["lat"]))
    bs.load_arrays(**st)
    bs.ready(xcyclic=CG.xcyclic(name))
    assert tuple(g["shape"]) == bs.fields.shape
    assert bitwise(bs.lat, g["lat"]) and bitwise(bs.lon, g["lon"])
    assert sha(bs.fields) == str(g["sha256"])


@pytest.mark.refhost
@pytest.mark.parametrize("name", GRIDS)
def test_mercator_point_bitwise(name):
    g = CG.golden(name)
    with np.errstate(all="ignore"):
        out = O.mercator_point(CG.background(name), g["merc_lon"].copy(), g["merc_lat"].copy())
    assert bitwise(out[:12], g["merc_out"])


@pytest.mark.refhost
@pytest.mark.parametrize("name", GRIDS)
def test_rhs_bitwise(name):
    g = CG.golden(name)
    with np.errstate(all="ignore"):
        d, bad = O.rhs(CG.background(name), g["rhs_y"].copy())
    assert np.array_equal(bad, g["rhs_bad"])
    assert bitwise(d, g["rhs_dydt"])


@pytest.mark.refhost
@pytest.mark.parametrize("name", GRIDS)
def test_single_step_bitwise(name):
    g = CG.golden(name)
    bg = CG.background(name)
    y, h = g["step_y"], g["step_h"]
    with np.errstate(all="ignore"):
        yn, K = O.dp54_attempt(lambda t, y: O.rhs(bg, y)[0], np.zeros(len(h)), y, g["step_f"], h)
        en = O.error_norm(K, h, y, yn, 1e-6, 1e-6)
    assert bitwise(K, g["step_K"])
    assert bitwise(yn, g["step_y_new"])
    assert bitwise(en, np.nan_to_num(g["step_err"], nan=0.0))


_RUN = {}


def oracle_rows(name):
    if name not in _RUN:
        slon, slat = CG.sources()
        with np.errstate(all="ignore"):
            rows = np.array(O.ray_initial(CG.background(name), slon, slat, CG.ZWN, CG.FREQ)).reshape(7, -1)
        _RUN[name] = rows
    return _RUN[name]


@pytest.mark.refhost
@pytest.mark.parametrize("name", GRIDS)
def test_initial_rows_bitwise(name):
    assert bitwise(oracle_rows(name), CG.golden(name)["row0"])


@pytest.mark.refhost
@pytest.mark.parametrize("name", GRIDS)
def test_rk45_history_bitwise(name):
    g = CG.golden(name)
    row0 = oracle_rows(name)
    with np.errstate(all="ignore"):
        hist, nacc, nrej, st = O.ray_run(CG.background(name), row0[:5].copy(), CG.NT, CG.TSTEP,
                                         ttotal=(CG.NT - 1) * CG.TSTEP, row0=row0)
    assert st == 0
    assert bitwise(hist[:2], g["track"])
    assert bitwise(hist[:, g["rows"]], g["hist"])
    assert np.array_equal(nacc, g["nacc"])
    assert int(nacc.sum() + nrej.sum()) == int(g["attempts"])


@pytest.mark.refhost
@pytest.mark.parametrize("name", GRIDS)
def test_rk4_history_bitwise(name):
    g = CG.golden(name)
    row0 = oracle_rows(name)
    with np.errstate(all="ignore"):
        hist, st = O.ray_run_rk4(CG.background(name), row0[:5].copy(), CG.NT, CG.TSTEP, row0=row0)
    assert bitwise(hist[:, g["rk4_rows"]], g["rk4"])
