"""Backward ray tracing on the GPU (RWRT_PARAMS_BACKWARD, RayEngine.integrate(backward=True),
WR(backward=True)) against its definition: the oracle's interval loop on the
negated RHS (tests/support/backward.py ``oracle_backward``), run here with the
kernels' own sin / cos / tan / pow (``O.device_math``), so that the comparison
does not depend on this host's libm.  Row ``i`` is the state at ``-t_eval[i]``.

Fixture: the zonal and the non-zonal state at 2.5 degrees, 4 x 4 sources x 4
wavenumbers x 3 roots = 192 slots, 181 rows of 2 h.  The oracle runs, the
forward runs and the one-launch backward runs are computed once per module.
"""
import numpy as np
import pytest
import torch

import rwrt_oracle as O
from support.backward import KINDS, NT, TSTEP, background, cfg, first_nan_row, oracle_backward
from support.bits import bitwise
from support.cases import bs_of, tv_engine

pytestmark = pytest.mark.gpu

KW = dict(ttotal=(NT - 1) * TSTEP)
NAMES = ("rlon", "rlat", "rzwn", "rmwn", "ramp", "rug", "rvg")


def _wr(kind, backward, bs=None):
    from wr import WR
    c = cfg()
    bs = bs or bs_of(kind)
    w = WR(c.nzwn, c.nsource, TSTEP, (NT - 1) * TSTEP, 0.0, nx=bs.nlon, ny=bs.nlat, backward=backward)
    w.bs = bs
    w.set_zwn(c.zwn)
    w.set_source_matrix(c.SW_lon, c.SW_lat, c.dlon, c.dlat, c.nnx, c.nny)
    return w


class Collect:
    """A dense collecting sink: rows 1..nt-1 as ``[nray, nt-1, 8]``."""

    def __init__(self, nray, device, nt=NT):
        self.rows = torch.full((nray, nt - 1, 8), -7.0, dtype=torch.float64, device=device)

    def __call__(self, i0, i1, rows):
        self.rows[:, i0 - 1:i1 - 1] = rows


class CollectBlocks(Collect):
    """A sink that takes a launch's row blocks (the live rays' rows and the
    tails) and makes them dense itself."""
    takes_slots = True

    def __call__(self, i0, i1, view, tails, slots):
        self.blocks = view.shape[0]
        self.rows[:, i0 - 1:i1 - 1] = slots.dense(view, tails, i0, i1)


def _result(res, rows):
    st = res.state["state"].cpu().numpy()
    return dict(rows=rows.cpu().numpy().copy(), nacc=res.nacc.cpu().numpy().copy(), nrej=res.nrej.cpu().numpy().copy(),
                nanrow=res.nanrow.cpu().numpy().copy(), y=st[:5].copy(), h_abs=st[11].copy())


def _same(got, want, what, keys=("rows", "nacc", "nrej", "nanrow", "y", "h_abs")):
    for k in keys:
        assert bitwise(got[k], want[k]), f"{what}: {k} differs"


def _run(eng, y0, backward=True, sink=None, **kw):
    c = sink or Collect(y0.shape[1], eng.device)
    res = eng.integrate(y0.clone(), NT, TSTEP, sink=c, backward=backward, **KW, **kw)
    assert res.backward is backward
    return res, c


@pytest.fixture(scope="module")
def fx():
    out = {}
    for kind in KINDS:
        w = _wr(kind, True)
        eng = w.bs.engine()
        rows0 = eng.initial_rows(w.source_lon, w.source_lat, w.zwn, w.freq)        # [7, 3, ns, nz]
        r0 = rows0.reshape(7, -1).cpu().numpy()
        y0 = rows0[:5].reshape(5, -1).contiguous()
        nray = y0.shape[1]
        assert nray == 192
        keep = {}
        with np.errstate(all="ignore"), O.device_math():
            hist, nacc, nrej, status = oracle_backward(background(kind), r0[:5], NT, TSTEP, row0=r0, keep=keep, **KW)
        assert status == 0 and len(keep["nacc_rows"]) == NT - 1
        rows = np.empty((nray, NT - 1, 8))
        rows[:, :, :7] = np.transpose(hist[:, 1:], (2, 1, 0))
        rows[:, :, 7] = np.array(keep["nacc_rows"], dtype=np.float64).T
        want = dict(rows=rows, nacc=nacc, nrej=nrej, nanrow=first_nan_row(hist[0], NT), h_abs=keep["solver"].h_abs,
                    hist=hist)
        fres, fc = _run(eng, y0, backward=False)
        res, c = _run(eng, y0)
        assert len(res.bounds) == 1
        fwd, one = _result(fres, fc.rows), _result(res, c.rows)
        # what the comparisons need to see (else they could pass vacuously)
        live0 = ~np.isnan(r0[:5].mean(axis=0))
        assert live0.sum() >= 30 and (~live0).sum() >= 1, (kind, int(live0.sum()))
        froze = want["nanrow"][live0]
        if kind == "nonzonal":
            assert ((froze > 1) & (froze < NT)).sum() >= 3, sorted(froze[froze < NT].tolist())
        differs = (fwd["rows"][live0, 9, :5] != one["rows"][live0, 9, :5]).any(axis=1)
        assert differs.all(), f"{kind}: {int((~differs).sum())} live rays have the forward run's row 10"
        out[kind] = dict(w=w, eng=eng, y0=y0, r0=r0, want=want, one=one, fwd=fwd, live0=live0, min_step=res.params[2])
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_one_launch_equals_the_oracle_bit_for_bit(fx, kind):
    """All eight row columns (the nacc column: the oracle's counters after every
    interval), nacc, nrej, nanrow and the state's h_abs row, NaN positions
    included.  (h_abs: the oracle stores max(h_abs, min_step) for a column it
    does not step, rkf45.py:383-387 applied at the step's start; the state
    row keeps the unclamped value and clamps when it next steps -- compared
    after that clamp, which changes nothing above min_step.)"""
    f = fx[kind]
    got, want = f["one"], f["want"]
    for c, name in enumerate(("lon", "lat", "k", "l", "amp", "ug", "vg", "nacc")):
        assert bitwise(got["rows"][:, :, c], want["rows"][:, :, c]), name
    assert np.array_equal(got["nacc"], want["nacc"]) and np.array_equal(got["nrej"], want["nrej"])
    assert np.array_equal(got["nanrow"], want["nanrow"])
    h = got["h_abs"]
    with np.errstate(invalid="ignore"):
        h = np.where(h < f["min_step"], f["min_step"], h)
    assert bitwise(h, want["h_abs"])
    assert np.array_equal(np.isnan(got["h_abs"]), ~f["live0"])
    # ug, vg of a row: the true group velocity at the point, not the negated one
    live_end = f["live0"] & ~np.isnan(want["hist"][0, -1])      # (a dead slot keeps its source's lon, lat)
    assert live_end.sum() >= 1
    M = O.mercator_point(background(kind), want["hist"][0, -1, live_end], want["hist"][1, -1, live_end])
    ug, _ = O.ugvg_extent(M[0], M[1], M[6], M[7], want["hist"][2, -1, live_end], want["hist"][3, -1, live_end])
    assert np.allclose(got["rows"][live_end, -1, 5], ug, rtol=1e-12)


LAYOUTS = ("chunks37", "own_buffer", "row_blocks", "no_tails", "priority12")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_schedules_and_row_layouts_give_the_same_bits(fx, layout, kind):
    """Five launches of 37 rows (the carried state resumes; rays freeze on both
    sides of the boundaries); the caller's dense ``out``; a sink that takes row
    blocks (slots + tails); every row written by the launch itself; and the
    priority order after a 12-row leading launch: rows, counters, nanrow and
    the state's y and h_abs rows after the last launch equal the one-launch run."""
    f = fx[kind]
    eng, y0 = f["eng"], f["y0"]
    n = y0.shape[1]
    if layout == "own_buffer":
        out = torch.full((n, NT - 1, 8), -7.0, dtype=torch.float64, device=eng.device)
        res = eng.integrate(y0.clone(), NT, TSTEP, out=out, backward=True, **KW)
        got = _result(res, out)
    elif layout == "row_blocks":
        c = CollectBlocks(n, eng.device)
        res, _ = _run(eng, y0, sink=c, chunk=37)
        assert c.blocks <= f["live0"].sum() < n          # (row blocks for the live rays only)
        got = _result(res, c.rows)
    elif layout == "no_tails":
        tails = eng.use_tails
        try:
            eng.use_tails = False
            res, c = _run(eng, y0, chunk=37)
        finally:
            eng.use_tails = tails
        got = _result(res, c.rows)
    elif layout == "priority12":
        res, c = _run(eng, y0, order_policy="priority", first_chunk=12)
        assert [b - a for a, b in res.bounds] == [12, 168]
        got = _result(res, c.rows)
    else:
        res, c = _run(eng, y0, chunk=37)
        assert len(res.bounds) == 5
        got = _result(res, c.rows)
    _same(got, f["one"], f"{layout}/{kind}")
    assert res.failed is False and res.backward is True


@pytest.mark.parametrize("kind", KINDS)
def test_handoff_and_latency_mode_are_schedule_only(fx, kind):
    """Both are supported backward.  The drain-time hand-off at 0 and at 16
    (rays are handed off at 16, none at 0) and the latency mode (team=8 after
    a 12-row leading launch; 8 rays run in the quad layout) give the bits of
    the one-launch run."""
    f = fx[kind]
    eng, y0 = f["eng"], f["y0"]
    keep = eng.handoff
    try:
        eng.handoff = 0
        res, c = _run(eng, y0)
        assert sum(eng.handoffs()) == 0
        _same(_result(res, c.rows), f["one"], f"handoff 0/{kind}")
        eng.handoff = 16
        res, c = _run(eng, y0)
        assert sum(eng.handoffs()) > 0, eng.handoffs()
        _same(_result(res, c.rows), f["one"], f"handoff 16/{kind}")
        res, c = _run(eng, y0, first_chunk=12, team=8)
        assert [l["n_heavy"] for l in eng.launch_log] == [8, 8], eng.launch_log
        _same(_result(res, c.rows), f["one"], f"team 8/{kind}")
    finally:
        eng.handoff = keep


@pytest.mark.parametrize("kind", KINDS)
def test_a_forward_run_after_a_backward_one_is_unchanged(fx, kind):
    """Isolation: the same engine and context, a forward integrate after the
    backward calls equals the one taken before them."""
    f = fx[kind]
    res, c = _run(f["eng"], f["y0"], backward=False)
    _same(_result(res, c.rows), f["fwd"], f"forward/{kind}")


def test_wr_backward_history_is_the_oracles(fx):
    f = fx["nonzonal"]
    w = _wr("nonzonal", True, bs=f["w"].bs)
    with np.errstate(all="ignore"):
        res = w.ray_run(mode="hip", inte_method="rk45")
    assert res.backward is True and w.last_run is res
    hist = f["want"]["hist"]
    got = np.array([getattr(w, n) for n in NAMES]).reshape(7, NT, -1)
    assert bitwise(got[:, 0], f["r0"])                               # row 0: the initial rows
    assert bitwise(got, hist)
    brk = res.break_row
    assert brk is None or np.isnan(got[:, brk:]).all()
    assert np.array_equal(res.nacc.cpu().numpy(), f["want"]["nacc"])
    # the forward WR on the same sources differs
    assert not bitwise(got[0, 10], f["fwd"]["rows"][:, 9, 0])


def test_products_of_backward_rays(fx):
    """One product of each sink family on the backward history: the points of
    ``ray_density`` (a receptor's footprint) and the segments of ``ray_cross``."""
    from cross import CrossSpec, Gate, reference_cross
    from density import DensitySpec, reference_bins
    f = fx["nonzonal"]
    hist = f["want"]["hist"]
    rows = np.full((hist.shape[2], NT, 8), np.nan)
    rows[:, :, :7] = np.transpose(hist, (2, 1, 0))
    dspec = DensitySpec(72, 36)
    w = _wr("nonzonal", True, bs=f["w"].bs)
    with np.errstate(all="ignore"):
        dmap = w.ray_density(dspec)
        want, _ = reference_bins(rows[..., 0].T, rows[..., 1].T, None, None, dspec)
    assert want.sum() > 1000
    assert np.array_equal(dmap.count.cpu().numpy(), want)
    xspec = CrossSpec((Gate.lat(30.0),), 36)
    with np.errstate(all="ignore"):
        got = w.ray_cross(xspec).numpy()
        ref = reference_cross(rows, None, xspec)
    assert int(ref["ncross"].sum()) > 5
    assert np.array_equal(got["cnt"], ref["cnt"]) and np.array_equal(got["ncross"], ref["ncross"])
    assert got["dropped"] == ref["dropped"]


def test_what_backward_refuses_is_refused_before_any_launch(fx):
    from engine import RayEngine
    from levels import Levels
    import synthetic as S
    f = fx["zonal"]
    eng, y0 = f["eng"], f["y0"]

    def sink(*a):
        raise AssertionError("a launch was made")

    with pytest.raises(NotImplementedError, match="RK4"):
        eng.integrate_rk4(y0.clone(), NT, TSTEP, sink=sink, backward=True)
    with pytest.raises(NotImplementedError, match="stop_row"):
        eng.integrate(y0.clone(), NT, TSTEP, sink=sink, backward=True, stop_row=5, **KW)
    with pytest.raises(NotImplementedError, match="group"):
        eng.integrate(y0.clone(), NT, TSTEP, sink=sink, backward=True, group=object(), **KW)
    with pytest.raises(NotImplementedError, match="checkpoint"):
        eng.resume({}, NT, TSTEP, backward=True)
    res, _ = _run(eng, y0, chunk=90)
    with pytest.raises(NotImplementedError, match="checkpoint"):
        RayEngine.checkpoint(res)
    tv = tv_engine(False)
    with pytest.raises(NotImplementedError, match="time-varying"):
        tv.integrate(y0.clone(), NT, TSTEP, sink=sink, backward=True, **KW)
    bgs = [S.background(k) for k in KINDS]
    lv = Levels(bgs[0]["lat"], bgs[0]["lon"], 2)
    lv.set_levels(np.stack([b["u"] for b in bgs]), np.stack([b["v"] for b in bgs]))
    es = RayEngine.from_levels(lv, members=True)
    with pytest.raises(NotImplementedError, match="member"):
        es.integrate(y0.clone(), NT, TSTEP, sink=sink, backward=True, member=np.zeros(y0.shape[1], np.int64), **KW)
    # and the C entry refuses what the engine would not send: a time-varying init with the flag
    p = RayEngine.params(NT, TSTEP, backward=True)
    with pytest.raises(NotImplementedError):
        tv.init(y0.clone(), p)


def test_device_round_trip_on_the_zonal_state(fx):
    """Forward rows 0..20, then 20 rows backward from row 20's state: all 40
    live rays return within 1e-4 rad (the oracle's round trip measures 2.3e-5
    and 1.6e-5; rtol = 1e-6 over 20 intervals, times four)."""
    f = fx["zonal"]
    eng, live = f["eng"], f["live0"]
    assert live.sum() == 40
    end = torch.as_tensor(f["fwd"]["rows"][:, 19, :5].T.copy(), device=eng.device).contiguous()
    assert not torch.isnan(end[:, torch.as_tensor(live)]).any()
    c = Collect(end.shape[1], eng.device, 21)
    res = eng.integrate(end, 21, TSTEP, sink=c, backward=True, ttotal=20 * TSTEP)
    back = c.rows[:, 19].cpu().numpy()
    assert not np.isnan(back[live, :2]).any(), "a live ray did not return"
    dlon = np.abs(back[live, 0] - f["r0"][0, live]).max()
    dlat = np.abs(back[live, 1] - f["r0"][1, live]).max()
    print(f"device round trip, 20 rows: max |dlon| {dlon:.3g} rad, max |dlat| {dlat:.3g} rad")
    assert dlon <= 1e-4 and dlat <= 1e-4, (dlon, dlat)
    assert res.backward is True
