"""The static ray kernels off the 144 x 73 grid, bit for bit.

Five grids (``support/cases_grids.py``): 1 degree (the clamped seam cell, a
top row that is not clamped), 10 degrees (almost no cell changes), 33 x 127
(``W*H`` a multiple of the 64-point image tile, odd ``nlon``), the non-cyclic
73 x 144 (the clamped last column) and 0.25 degrees (16 234 image tiles, about
four cell changes per row).  288 ray slots from sources on both sides of the
0/360 seam, 41 rows of 2 h.

Against the reference's own records (``tests/golden/grid_<name>.npz``, pinned
to the oracle by tests/test_grids_oracle.py): the element kernels, one DP5(4)
attempt, the initial rows, the RK45 and RK4 histories in one launch and in
chunks, and the ``WR`` drop-in.  Against the plain run of the same grid, which
equals the records by those tests: the latency mode, the drain-time hand-off
and the member stack.  Against the oracle computed here: backward tracing,
``rwrt_bs_ready``, and the time-varying kernels on the 7 x 12 and 19 x 36 grids
(the block cache where ``H`` is below its 8 x 8).

Every comparison is of bit patterns (``support.bits.bitwise``) or of integers.
"""
import numpy as np
import pytest
import torch

import rwrt_oracle as O
from support import cases_grids as CG
from support.bits import bitwise

pytestmark = pytest.mark.gpu

GRIDS = list(CG.STATIC)
KW = dict(ttotal=(CG.NT - 1) * CG.TSTEP)
HOT = O.TimeVaryingBackground.HOT

_BS, _ENG, _PLAIN = {}, {}, {}


def host_bs(name):
    if name not in _BS:
        from bs import BS
        st = CG.state(name)
        bs = BS(len(st["lon"]), len(st["lat"]))
        bs.load_arrays(**st)
        bs.ready(xcyclic=CG.xcyclic(name))
        _BS[name] = bs
    return _BS[name]


def levels_of(name, kinds=("nonzonal",), fp32=False):
    from levels import Levels
    sts = [CG.state(name, k) for k in kinds]
    lv = Levels(sts[0]["lat"], sts[0]["lon"], len(kinds), fp32=fp32)
    for j, s in enumerate(sts):
        lv.set_level(j, s["u"], s["v"])
    return lv


def engine(name):
    """The static engine of a grid, built once: through the host ``BS`` (its
    ``ready(xcyclic=)`` included), ``q`` through one fp64 level of ``Levels``
    (``rwrt_bs_ready``)."""
    if name not in _ENG:
        from engine import RayEngine
        _ENG[name] = RayEngine.from_levels(levels_of(name)) if name == "q" else RayEngine.from_bs(host_bs(name))
    return _ENG[name]


class Collect:
    """A dense collecting sink: rows 1..nt-1 as ``[nray, nt-1, 8]``."""

    def __init__(self, nray, device, nt=CG.NT):
        self.rows = torch.full((nray, nt - 1, 8), -7.0, dtype=torch.float64, device=device)

    def __call__(self, i0, i1, rows):
        self.rows[:, i0 - 1:i1 - 1] = rows


def result(res, rows):
    return dict(rows=rows.cpu().numpy().copy(), nacc=res.nacc.cpu().numpy().copy(),
                nrej=res.nrej.cpu().numpy().copy(), nanrow=res.nanrow.cpu().numpy().copy())


def same(got, want, what):
    assert bitwise(got["rows"], want["rows"]), f"{what}: rows differ"
    for k in ("nacc", "nrej", "nanrow"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs"


def y0_of(g):
    return torch.as_tensor(np.ascontiguousarray(g["row0"][:5]))


def run(eng, y0, nt=CG.NT, rk4=False, **kw):
    c = Collect(y0.shape[1], eng.device, nt)
    if rk4:
        res = eng.integrate_rk4(y0.clone(), nt, CG.TSTEP, sink=c, **kw)
    else:
        res = eng.integrate(y0.clone(), nt, CG.TSTEP, ttotal=(nt - 1) * CG.TSTEP, sink=c, **kw)
    return result(res, c.rows)


def history(g, r):
    """``hist[7, NT, nray]``: the records' row 0 and the rows of a run."""
    return np.concatenate([g["row0"][:, None], np.transpose(r["rows"][:, :, :7], (2, 1, 0))], axis=1)


def plain(name):
    """The plain one-launch RK45 run of a grid (computed once, read-only)."""
    if name not in _PLAIN:
        r = run(engine(name), y0_of(CG.golden(name)))
        for v in r.values():
            v.setflags(write=False)
        _PLAIN[name] = r
    return _PLAIN[name]


# ------------------------------------------------------------- against the records
@pytest.mark.parametrize("name", GRIDS)
def test_t0_mercator_point(name):
    g = CG.golden(name)
    out = engine(name).mercator_point(g["merc_lon"], g["merc_lat"]).cpu().numpy()
    assert bitwise(out, g["merc_out"])


@pytest.mark.parametrize("name", GRIDS)
def test_t0_rhs(name):
    g = CG.golden(name)
    assert bitwise(engine(name).rhs(g["rhs_y"]).cpu().numpy(), g["rhs_dydt"])


@pytest.mark.parametrize("name", GRIDS)
def test_t1_single_attempt(name):
    g = CG.golden(name)
    K, yn, err = engine(name).attempt(g["step_y"], g["step_f"], g["step_h"])
    assert bitwise(K.cpu().numpy(), g["step_K"])
    assert bitwise(yn.cpu().numpy(), g["step_y_new"])
    assert bitwise(err.cpu().numpy(), g["step_err"])


@pytest.mark.parametrize("name", GRIDS)
def test_initial_rows(name):
    """``rwrt_ray_initial``: the reference's row 0, the order of the roots included."""
    g = CG.golden(name)
    slon, slat = CG.sources()
    rows = engine(name).initial_rows(slon, slat, CG.ZWN, CG.FREQ).cpu().numpy()
    assert bitwise(rows.reshape(7, -1), g["row0"])


@pytest.mark.parametrize("name", GRIDS)
def test_rk45_one_launch(name):
    g = CG.golden(name)
    r = plain(name)
    h = history(g, r)
    assert bitwise(h[:2], g["track"])
    assert bitwise(h[:, g["rows"]], g["hist"])
    assert np.array_equal(r["nacc"], g["nacc"])
    assert int(r["nacc"].sum() + r["nrej"].sum()) == int(g["attempts"])


@pytest.mark.parametrize("name", GRIDS)
def test_rk45_chunks_of_7(name):
    g = CG.golden(name)
    r = run(engine(name), y0_of(g), chunk=7)
    h = history(g, r)
    assert bitwise(h[:2], g["track"])
    assert bitwise(h[:, g["rows"]], g["hist"])
    assert np.array_equal(r["nacc"], g["nacc"])
    same(r, plain(name), "chunk=7")


@pytest.mark.parametrize("chunk", [None, 13], ids=["one_launch", "chunks_of_13"])
@pytest.mark.parametrize("name", GRIDS)
def test_rk4(name, chunk):
    g = CG.golden(name)
    r = run(engine(name), y0_of(g), rk4=True, chunk=chunk)
    assert bitwise(history(g, r)[:, g["rk4_rows"]], g["rk4"])


@pytest.mark.refhost
@pytest.mark.parametrize("inte_method", ["rk45", ""], ids=["rk45", "rk4"])
@pytest.mark.parametrize("name", ["g1", "g127"])
def test_wr_dropin(name, inte_method):
    """``WR(..., nx=nlon, ny=nlat).ray_run(mode='hip')``: the history arrays
    (host initial rows, chunked delivery) equal the reference's."""
    from wr import WR
    g = CG.golden(name)
    bs = host_bs(name)
    s = CG.SEEDS
    w = WR(len(CG.ZWN), s["nnx"] * s["nny"], CG.TSTEP, (CG.NT - 1) * CG.TSTEP, CG.FREQ, nx=bs.nlon, ny=bs.nlat)
    w.bs = bs
    w.set_zwn(CG.ZWN)
    w.set_source_matrix(s["SW_lon"], s["SW_lat"], s["dlon"], s["dlat"], s["nnx"], s["nny"])
    with np.errstate(all="ignore"):
        w.ray_run(mode="hip", inte_method=inte_method)
    h = np.array([w.rlon, w.rlat, w.rzwn, w.rmwn, w.ramp, w.rug, w.rvg]).reshape(7, CG.NT, -1)
    if inte_method == "rk45":
        assert bitwise(h[:2], g["track"])
        assert bitwise(h[:, g["rows"]], g["hist"])
    else:
        assert bitwise(h[:, g["rk4_rows"]], g["rk4"])


# ------------------------------------------------- against the plain run of the grid
@pytest.mark.parametrize("name", GRIDS)
def test_latency_mode(name):
    """Every live ray in latency mode at 16 and at 1 ray per wave, and a ragged
    97 at 4 per wave, over three launches: the plain run's bits."""
    eng, g = engine(name), CG.golden(name)
    cap = eng.team_capacity()
    for team in (cap, (cap, 1), (97, 4)):
        r = run(eng, y0_of(g), chunk=14, first_chunk=[5], team=team)
        assert all(l["n_heavy"] > 0 for l in eng.launch_log), (team, eng.launch_log)
        same(r, plain(name), f"team={team}")


@pytest.mark.parametrize("name", GRIDS)
def test_drain_handoff(name):
    eng, g = engine(name), CG.golden(name)
    try:
        eng.handoff = 0
        want = run(eng, y0_of(g))
        assert sum(eng.handoffs()) == 0
        same(want, plain(name), "handoff 0")
        for n in (16, 4, 1):
            eng.handoff = n
            r = run(eng, y0_of(g))
            moved = eng.handoffs()
            assert sum(moved) > 0, (n, moved)
            same(r, want, f"handoff {n}")
    finally:
        eng.handoff = 16


@pytest.mark.refhost
@pytest.mark.parametrize("name", ["g1", "nc", "q"])
def test_backward(name):
    """``integrate(backward=True)`` equals the oracle's forward integration of
    the negated RHS (``support.backward.oracle_backward``)."""
    from support.backward import first_nan_row, oracle_backward
    g = CG.golden(name)
    r0 = g["row0"]
    with np.errstate(all="ignore"):
        hist, nacc, nrej, status = oracle_backward(CG.background(name), r0[:5], CG.NT, CG.TSTEP, row0=r0, **KW)
    assert status == 0
    live0 = ~np.isnan(r0[3])
    assert (~np.isnan(hist[0, -1]) & live0).sum() >= 50          # rays that reach the last row
    r = run(engine(name), y0_of(g), backward=True)
    assert bitwise(history(g, r), hist)
    assert np.array_equal(r["nacc"], nacc) and np.array_equal(r["nrej"], nrej)
    assert np.array_equal(r["nanrow"], first_nan_row(hist[0], CG.NT))
    fwd = plain(name)["rows"]
    assert (fwd[live0, 5, :2] != r["rows"][live0, 5, :2]).any(axis=1).all()   # not the forward run


MEMBERS = {"g127": ("nonzonal", "zonal", "superrotation"), "g10": ("nonzonal", "zonal", "superrotation"),
           "g1": ("nonzonal", "zonal", "superrotation"), "q": ("nonzonal", "zonal")}


@pytest.mark.parametrize("name", list(MEMBERS))
def test_member_stack(name):
    """The 288 slots dealt round-robin over the members of a stack on the
    grid's axes: each ray's rows and counters are the static engine's on its
    member alone; member 0 is the grid's own state, so its rays' rows are the
    reference's too.  (``q``: two members, 200 MB of images, within
    ``stack_fits``.)"""
    from engine import RayEngine
    g = CG.golden(name)
    kinds = MEMBERS[name]
    nm = len(kinds)
    lv = levels_of(name, kinds)
    es = RayEngine.from_levels(lv, members=True)
    slon, slat = CG.sources()
    member = np.arange(CG.NRAY) % nm
    y0 = torch.empty((5, CG.NRAY), dtype=torch.float64, device=es.device)
    want = dict(rows=np.empty((CG.NRAY, CG.NT - 1, 8)), nacc=np.empty(CG.NRAY, np.int64),
                nrej=np.empty(CG.NRAY, np.int64), nanrow=np.empty(CG.NRAY, np.int32))
    for m in range(nm):
        e = RayEngine.from_packed(lv.packed[m], lv.lon, lv.lat)
        ym = e.initial_rows(slon, slat, CG.ZWN, CG.FREQ)[:5].reshape(5, -1).contiguous()
        sel = member == m
        idx = torch.as_tensor(np.nonzero(sel)[0], device=es.device)
        assert int((~torch.isnan(ym[3, idx])).sum()) >= 30, kinds[m]
        y0[:, idx] = ym[:, idx]
        rm = run(e, ym)
        if m == 0:
            same(rm, plain(name), "member 0 alone")
        for k in want:
            want[k][sel] = rm[k][sel]
    c = Collect(CG.NRAY, es.device)
    res = es.integrate(y0.clone(), CG.NT, CG.TSTEP, sink=c, member=torch.as_tensor(member), **KW)
    got = result(res, c.rows)
    same(got, want, "stack")
    own = member == 0
    assert bitwise(np.transpose(got["rows"][own, :, :2], (2, 1, 0)), g["track"][:, 1:, own])


@pytest.mark.refhost
@pytest.mark.parametrize("name", GRIDS)
def test_bs_ready(name):
    """``rwrt_bs_ready`` on the grid's axes: the packed hot fields equal the
    oracle's, fp64 and fp32 storage.  ``Levels`` has no non-cyclic form (it
    always appends the cyclic column), so on ``nc`` the first ``nlon`` columns
    are compared -- the non-cyclic state is exactly those."""
    ref = CG.background(name).fields[..., HOT]
    for fp32 in (False, True):
        lv = levels_of(name, fp32=fp32)
        dev = lv.packed[0].cpu().numpy()
        want = ref.astype(np.float32) if fp32 else ref
        assert dev.shape[0] == len(lv.lon) + 1
        if CG.xcyclic(name):
            assert bitwise(dev[..., :11], want), fp32
        else:
            assert bitwise(dev[:-1, :, :11], want), fp32
            assert bitwise(dev[-1, :, :11], want[0]), fp32
        assert not dev[..., 11].any()


# ------------------------------------------- time-varying kernels on small grids
TV_HELD = [(32, 0), (64, 0), (32, (64, 1))]       # as tests/test_gpu_ref90.py
_TV = {}


def tv_case(name, fp32):
    """``(levels, y0, oracle history, oracle nacc)`` of a small time-varying grid."""
    if (name, fp32) not in _TV:
        from levels import Levels
        bl = CG.tv_levels(name)
        lv = Levels(bl[0]["lat"], bl[0]["lon"], CG.TV_NLEV, t0=0.0, dt=6 * 3600.0, fp32=fp32)
        for j, b in enumerate(bl):
            lv.set_level(j, b["u"], b["v"])
        obs = [O.Background(**b) for b in bl]
        ob = O.TimeVaryingBackground(obs, 0.0, 6 * 3600.0, fp32=fp32)
        slon, slat = CG.sources()
        with np.errstate(all="ignore"):
            row0 = np.array(O.ray_initial(obs[0], slon, slat, CG.ZWN, CG.FREQ)).reshape(7, -1)
            hist, nacc, _, status = O.ray_run(ob, row0[:5].copy(), CG.TV_NT, CG.TSTEP, row0=row0)
        assert status == 0
        assert (~np.isnan(row0[3])).sum() >= 150 and (~np.isnan(hist[3, -1])).sum() >= 100
        _TV[(name, fp32)] = (lv, row0, hist, nacc)
    return _TV[(name, fp32)]


@pytest.mark.refhost
@pytest.mark.parametrize("lanes,team", TV_HELD, ids=["pair32", "lanes64", "latency_waves"])
@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", list(CG.TV_SMALL))
def test_time_varying_small_grids(name, fp32, lanes, team):
    """Five levels on 7 x 12 (``H`` below the latency waves' 8 x 8 block) and on
    19 x 36, 13 rows: the initial rows and every row equal the oracle's
    ``TimeVaryingBackground`` run, lane pairs, 64 lanes and latency waves."""
    from engine import RayEngine
    lv, row0, hist, nacc = tv_case(name, fp32)
    eng = RayEngine.from_levels(lv)
    assert eng.bg is not None
    eng.tv_lanes = lanes
    slon, slat = CG.sources()
    assert bitwise(eng.initial_rows(slon, slat, CG.ZWN, CG.FREQ).cpu().numpy().reshape(7, -1), row0)
    kw = dict(order_policy="cell", first_chunk=[6], team=team) if team else {}
    r = run(eng, torch.as_tensor(row0[:5].copy()), nt=CG.TV_NT, **kw)
    if team:
        assert any(l["n_heavy"] for l in eng.launch_log), eng.launch_log
    assert bitwise(np.transpose(r["rows"][:, :, :7], (2, 1, 0)), hist[:, 1:])
    assert np.array_equal(r["nacc"], nacc)
