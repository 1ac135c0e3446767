"""Release stacks on the GPU (rwrt_rk45_*_rel, RayEngine.integrate(release=),
release.ReleaseWR): a ray's rows, counters and state are bit for bit what the
time-varying engine of the same build gives for that ray alone on the same
levels with ``t0 = levels.t0 - release`` -- whatever the other rays, the queue
order, the row layout, the chunking or ``tv_lanes``.

Levels: the five 2.5-degree levels of the time-varying family, 6 h apart,
fp64 (``support.cases.tv(False)``); 4 x 4 sources x 4 wavenumbers x 3 roots =
192 slots per release; 37 rows of 2 h (72 h: every release runs past the last
level); four releases -- a level time twice, a time between two levels, and
one that reaches the clamp within two rows -- 768 rays.  The references (a
time-varying engine per release on a shallow copy of the levels with its own
``t0``) are computed once and shared."""
import copy

import numpy as np
import pytest
import torch

import synthetic as S
from support.cases import DT, tv

pytestmark = pytest.mark.gpu

NT, TSTEP = 37, 7200.0
RELEASES = (0.0, DT, 1.5 * DT, 3 * DT + 1234.5)
NREL = len(RELEASES)
LANES = (32, 64)
KEYS = ("rows", "nacc", "nrej", "nanrow", "y", "h_abs")
KW = dict(ttotal=(NT - 1) * TSTEP)


def _cfg():
    return S.config("C2", SW_lon=90, SW_lat=-10, dlon=25, dlat=25, nnx=4, nny=4, zwn=[1, 3, 5, 7])


class Collect:
    """A dense collecting sink: rows 1..nt-1 as ``[nray, nt-1, 8]``."""

    def __init__(self, nray, device, nt=NT):
        self.rows = torch.full((nray, nt - 1, 8), -7.0, dtype=torch.float64, device=device)

    def __call__(self, i0, i1, rows):
        self.rows[:, i0 - 1:i1 - 1] = rows


def _result(res, rows):
    st = res.state["state"].cpu().numpy()
    return dict(rows=rows.cpu().numpy(), nacc=res.nacc.cpu().numpy(), nrej=res.nrej.cpu().numpy(),
                nanrow=res.nanrow.cpu().numpy(), y=st[:5].T.copy(), h_abs=st[11].copy())


def _same(got, want, what):
    for k in KEYS:
        if k in got:
            assert np.array_equal(got[k], want[k], equal_nan=True), f"{what}: {k} differs"


def _live_rows(rows):
    """Which rays are live at a stored row ``rows[nray, 8]``: the solver's own
    test, a finite mean of lon lat k l amp (a dead root slot keeps its source's
    lon and lat; its l is NaN)."""
    return ~np.isnan(rows[:, :5].sum(1))


def _lanes(eng, lanes):
    eng.tv_lanes = lanes
    return eng


@pytest.fixture(scope="module")
def fx():
    from engine import RayEngine
    from release import ReleaseWR
    eng = tv(False)[0]
    lv = eng.levels
    assert lv.nlev == 5 and lv.dt == DT and lv.t0 == 0.0 and not lv.fp32
    cfg = _cfg()
    rw = ReleaseWR(lv, RELEASES, cfg.nzwn, cfg.nsource, TSTEP, (NT - 1) * TSTEP)
    rw.set_zwn(cfg.zwn)
    rw.set_source_matrix(cfg.SW_lon, cfg.SW_lat, cfg.dlon, cfg.dlat, cfg.nnx, cfg.nny)
    nslot = 3 * rw.nsource * rw.nzwn
    assert nslot == 192 and rw.nray == 768
    er = RayEngine.from_levels(lv)          # the release engine (its own context and tv_lanes)
    src, zc = er.sources(rw.source_lon, rw.source_lat), er.zwn_tensor(rw.zwn, rw.freq)
    refs, rows0, y0, ref = [], [], [], {}
    for r in RELEASES:
        lr = copy.copy(lv)                  # (shallow: the packed tensors are shared)
        lr.t0 = lv.t0 - r
        e = RayEngine.from_levels(lr)
        assert e.bg.t0 == -r and e.bg.d_levels == er.bg.d_levels
        refs.append(e)
        r0, info = er.initial_rows_dev(src, zc, packed=lv.state_at(r).contiguous())
        assert int(info.item()) == 0
        rows0.append(r0)
        y0.append(r0[:5].reshape(5, nslot).contiguous())
    for lanes in LANES:
        ref[lanes] = []
        for e, y in zip(refs, y0):
            c = Collect(nslot, e.device)
            res = _lanes(e, lanes).integrate(y.clone(), NT, TSTEP, sink=c, **KW)
            ref[lanes].append(_result(res, c.rows))
    # the reference engine's own rows do not depend on tv_lanes (a schedule setting)
    for a, b in zip(ref[32], ref[64]):
        _same(a, b, "tv_lanes 32 against 64")
    # what the comparisons below need to see (else they could pass vacuously)
    live6 = []
    for i, (r, y) in enumerate(zip(ref[64], y0)):
        live0 = ~torch.isnan(y.sum(0)).cpu().numpy()
        assert live0.sum() >= 30 and (~live0).sum() >= 1, (RELEASES[i], int(live0.sum()))
        froze = r["nanrow"][live0]
        assert ((froze >= 1) & (froze < NT)).sum() >= 1, (RELEASES[i], sorted(froze.tolist()))
        live6.append(_live_rows(r["rows"][:, 5]))          # (row 6 is rows[:, 5])
    for i in range(NREL):
        for j in range(i + 1, NREL):
            both = live6[i] & live6[j]
            a, b = ref[64][i]["rows"][both, 5, :2], ref[64][j]["rows"][both, 5, :2]
            assert ((a != b).any(1)).sum() >= 30, (RELEASES[i], RELEASES[j], int(both.sum()))
    return dict(lv=lv, rw=rw, er=er, plain=eng, refs=refs, rows0=rows0, y0=y0, ref=ref, nslot=nslot)


def _dealing(fx, how):
    """``(y0[5, 768], rel[768], slot[768])``: ray q is slot ``slot[q]`` of
    release ``rel[q]``.  'major': release after release; 'robin': ray q in
    release q % 4 -- neighbouring queue entries share a source and differ in
    release."""
    n = fx["nslot"]
    if how == "major":
        rel, slot = np.repeat(np.arange(NREL), n), np.tile(np.arange(n), NREL)
    else:
        rel, slot = np.tile(np.arange(NREL), n), np.repeat(np.arange(n), NREL)
    y0 = torch.stack([fx["y0"][i][:, j] for i, j in zip(rel, slot)], dim=1).contiguous()
    return y0, rel, slot


def _expected(fx, lanes, rel, slot, ref=None):
    ref = ref or fx["ref"][lanes]
    return {k: np.stack([ref[i][k][j] for i, j in zip(rel, slot)]) for k in KEYS if k in ref[0]}


def _times(rel):
    return np.asarray(RELEASES)[rel]


def test_initial_rows_and_init_equal_the_references(fx):
    from release import reference_state_at
    lv, er = fx["lv"], fx["er"]
    host = lv.packed.cpu().numpy()
    for r in RELEASES + (0.25 * DT, -3.0, 4 * DT, 9 * DT):
        got = lv.state_at(r).cpu().numpy()
        assert np.array_equal(got, reference_state_at(host, r, DT, lv.t0)), r
    assert lv.state_at(0.0).data_ptr() == lv.packed[0].data_ptr()
    assert lv.state_at(DT).data_ptr() == lv.packed[1].data_ptr()
    assert lv.state_at(99 * DT).data_ptr() == lv.packed[4].data_ptr()
    rw = fx["rw"]
    src, zc = er.sources(rw.source_lon, rw.source_lat), er.zwn_tensor(rw.zwn, rw.freq)
    for i, lev in ((0, 0), (1, 1)):
        want, _ = er.initial_rows_dev(src, zc, packed=lv.packed[lev])
        assert np.array_equal(fx["rows0"][i].cpu().numpy(), want.cpu().numpy(), equal_nan=True), RELEASES[i]
    p = er.params(NT, TSTEP)
    for how in ("major", "robin"):
        y0, rel, slot = _dealing(fx, how)
        st = er.init(y0.clone(), p, release=_times(rel))
        assert st["t0"].dtype == torch.float64 and np.array_equal(st["t0"].cpu().numpy(), lv.t0 - _times(rel))
        state, live = st["state"].cpu().numpy(), st["live"].cpu().numpy()
        total = np.zeros(2, np.int64)
        for i, e in enumerate(fx["refs"]):
            sm = e.init(fx["y0"][i].clone(), p)
            total += sm["summary"].cpu().numpy()
            sel = rel == i
            assert np.array_equal(state[:, sel], sm["state"].cpu().numpy()[:, slot[sel]], equal_nan=True), (how, i)
            assert np.array_equal(live[sel], sm["live"].cpu().numpy()[slot[sel]])
        assert np.array_equal(st["summary"].cpu().numpy(), total)
        assert (st["count"] == 0).all() and (st["nanrow"] == NT).all()
        # take() carries the level origin
        idx = torch.arange(5, 40, 3, device=er.device)
        assert np.array_equal(er.take(st, idx)["t0"].cpu().numpy(), (lv.t0 - _times(rel))[5:40:3])


LAYOUTS = ("one_launch", "chunks_uneven", "own_buffer", "density_slots", "no_tails", "priority")


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("how", ("major", "robin"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_rows_counters_and_state_equal_the_time_varying_engine(fx, layout, how, lanes):
    """Rows [nray, 36, 8], nacc, nrej, nanrow and the final y, h_abs: one launch;
    five launches of uneven length; the caller's own dense buffer; a sink that
    takes row blocks (DensitySink); every row written by the launch itself;
    and a priority order after a short leading launch."""
    from density import DensityMap, DensitySink, DensitySpec
    from engine import RayEngine
    er = _lanes(fx["er"], lanes)
    y0, rel, slot = _dealing(fx, how)
    want = _expected(fx, lanes, rel, slot)
    kw = dict(release=_times(rel), **KW)
    n = y0.shape[1]
    uneven = [3, 11, 2, 13]      # then the 7 rows left: five launches
    if layout == "density_slots":
        spec = DensitySpec(72, 36, nchan=NREL)
        dmap = DensityMap(spec, er.device)
        res = er.integrate(y0.clone(), NT, TSTEP, chunk=13, sink=DensitySink(dmap, rel.astype(np.int32)), **kw)
        got = _result(res, torch.zeros(0))
        del got["rows"]
        assert er.rows_bytes < n * 13 * 64   # (row blocks for the live rays only)
        for i, e in enumerate(fx["refs"]):
            one = DensityMap(DensitySpec(72, 36), e.device)
            _lanes(e, lanes).integrate(fx["y0"][i].clone(), NT, TSTEP, sink=DensitySink(one), **KW)
            assert np.array_equal(dmap.count[i].cpu().numpy(), one.count[0].cpu().numpy()), RELEASES[i]
    elif layout == "own_buffer":
        out = torch.full((n, NT - 1, 8), -7.0, dtype=torch.float64, device=er.device)
        res = er.integrate(y0.clone(), NT, TSTEP, out=out, **kw)
        got = _result(res, out)
    elif layout == "priority":
        c = Collect(n, er.device)
        res = er.integrate(y0.clone(), NT, TSTEP, sink=c, order_policy="priority", first_chunk=[5], **kw)
        assert [b - a for a, b in res.bounds] == [5, 31]
        got = _result(res, c.rows)
    else:
        c = Collect(n, er.device)
        tails = RayEngine.use_tails
        try:
            if layout == "no_tails":
                er.use_tails = False
            if layout == "chunks_uneven":
                res = er.integrate(y0.clone(), NT, TSTEP, sink=c, first_chunk=uneven, **kw)
                assert [b - a for a, b in res.bounds] == uneven + [7]
            else:
                res = er.integrate(y0.clone(), NT, TSTEP, sink=c, **kw)
                assert len(res.bounds) == 1
        finally:
            er.use_tails = tails
        got = _result(res, c.rows)
    _same(got, want, f"{layout}/{how}/{lanes}")
    assert res.failed is False and res.break_row is None


@pytest.mark.parametrize("lanes", LANES)
def test_a_lane_that_pulls_a_second_ray(fx, lanes):
    """More live rays than the launch's work-queue grid holds at once, one row
    per launch, releases dealt round-robin: some lanes take a second live ray
    within a launch, and it usually has another release than their first.  The
    premise is read from the launches themselves (``Context.last_grid``: the
    blocks that pulled from the queue x the rays a block holds) and asserted
    for every launch.  A build that sets the lane's t0 once per lane fails
    here.  Every copy of a ray must equal the time-varying engine's ray."""
    import _hip as H
    er = _lanes(fx["er"], lanes)
    nt = 5
    y0, rel, slot = _dealing(fx, "robin")
    ref = []
    for e, y in zip(fx["refs"], fx["y0"]):
        out = torch.empty((y.shape[1], nt - 1, 8), dtype=torch.float64, device=e.device)
        res = _lanes(e, lanes).integrate(y.clone(), nt, TSTEP, ttotal=(nt - 1) * TSTEP, out=out)
        ref.append(_result(res, out))
    want = _expected(fx, lanes, rel, slot, ref)
    # rays live at the start of launch i (row i + 1): live at row i (row 0: the initial rows)
    live_at = [int((~torch.isnan(y0.sum(0))).sum().item())] + \
              [int(_live_rows(want["rows"][:, i]).sum()) for i in range(nt - 2)]
    ncu = torch.cuda.get_device_properties(er.device).multi_processor_count
    rep = (ncu * 256) // min(live_at) + 16     # (at most 256 rays per block, one block per CU: checked below)
    n = y0.shape[1] * rep
    out = torch.empty((n, nt - 1, 8), dtype=torch.float64, device=er.device)
    grids = []

    def sink(i0, i1, rows):
        out[:, i0 - 1:i1 - 1] = rows
        grids.append(er.ctx.last_grid())

    res = er.integrate(y0.repeat(1, rep), nt, TSTEP, ttotal=(nt - 1) * TSTEP, release=np.tile(_times(rel), rep),
                       sink=sink, chunk=1)
    assert len(grids) == nt - 1
    second = []
    for (blocks, per), live in zip(grids, live_at):
        assert per == 4 * lanes and blocks >= 1, (blocks, per)
        second.append(live * rep - blocks * per)      # live rays that are some lane's second (or later) at least
    print(f"second-ray premise: {H.version()!r} from {H.LIB_PATH}; tv_lanes {lanes}, {ncu} CUs, grids {grids}, "
          f"live rays per launch {[v * rep for v in live_at]}, second pulls at least {second}")
    assert min(second) >= 1000, (grids, live_at, rep)
    got = _result(res, out)
    for k in KEYS:
        g = got[k].reshape((rep,) + want[k].shape)
        bad = [r for r in range(rep) if not np.array_equal(g[r], want[k], equal_nan=True)]
        print(f"second-ray result: {k}: {len(bad)} of {rep} copies differ")
        assert not bad, f"{k}: {len(bad)} of {rep} copies differ from the time-varying engine (first: copy {bad[0]})"


@pytest.mark.parametrize("lanes", LANES)
def test_all_releases_zero_and_the_path_before(fx, lanes):
    """Every ray with r = 0 equals the plain time-varying integrate without
    ``release`` bit for bit; and a plain integrate after the release calls
    equals the one before them."""
    er = _lanes(fx["er"], lanes)
    y = fx["y0"][0]
    n = y.shape[1]
    c0 = Collect(n, er.device)
    before = _result(er.integrate(y.clone(), NT, TSTEP, sink=c0, chunk=13, **KW), c0.rows)
    _same(before, fx["ref"][lanes][0], "the plain path against the reference at r = 0")
    c1 = Collect(n, er.device)
    res = er.integrate(y.clone(), NT, TSTEP, sink=c1, chunk=13, release=np.zeros(n), **KW)
    assert "t0" in res.state
    _same(_result(res, c1.rows), before, "all releases 0")
    c2 = Collect(n, er.device)
    res = er.integrate(y.clone(), NT, TSTEP, sink=c2, chunk=13, **KW)
    assert "t0" not in res.state
    _same(_result(res, c2.rows), before, "the plain path after the release calls")


def test_products_by_release_equal_the_per_release_products(fx):
    from density import DensityMap, DensitySink, DensitySpec
    from summary import RaySummary, SummarySink
    rw, nslot = fx["rw"], fx["nslot"]
    regions = [(60.0, 200.0, 0.0, 60.0), (300.0, 40.0, -60.0, 10.0)]
    counts, sums = [], []
    for i, e in enumerate(fx["refs"]):
        r0 = fx["rows0"][i]
        one = DensityMap(DensitySpec(72, 36), e.device)
        one.add_points(r0[0], r0[1])
        e.integrate(fx["y0"][i].clone(), NT, TSTEP, sink=DensitySink(one), **KW)
        counts.append(one.count[0].cpu().numpy())
        rs = RaySummary(nslot, regions, e.device)
        rs.start(r0[0], r0[1], r0[3], r0[4])
        e.integrate(fx["y0"][i].clone(), NT, TSTEP, sink=SummarySink(rs), **KW)
        sums.append(rs.numpy())
    dmap = rw.ray_density(DensitySpec(72, 36), by="release")
    got = dmap.count.cpu().numpy()
    assert got.shape == (NREL, 36, 72)
    for i in range(NREL):
        assert np.array_equal(got[i], counts[i]), RELEASES[i]
    assert rw.ray_density(DensitySpec(72, 36), by=None).count.cpu().numpy().sum() == sum(c.sum() for c in counts)
    rs = rw.ray_summary(regions=regions).numpy()
    for name, a in rs.items():
        lead = a.shape[:-4]
        assert a.shape[-4:] == rw.slot_shape, name
        for i in range(NREL):
            want = sums[i][name].reshape(lead + rw.slot_shape[1:])
            assert np.array_equal(a[..., i, :, :, :], want, equal_nan=True), (name, RELEASES[i])
    with pytest.raises(ValueError, match="release"):
        rw.ray_density(DensitySpec(72, 36), by="member")


def test_releasewr_ray_run_equals_the_references(fx, tmp_path):
    from ensemble import member_outcomes
    rw, nslot = fx["rw"], fx["nslot"]
    res = rw.ray_run()
    cfg = _cfg()
    assert rw.rlon.shape == (NT, NREL, 3, cfg.nsource, cfg.nzwn)
    assert len(res.break_row) == NREL and len(res.failed) == NREL
    ref = fx["ref"][rw.engine().tv_lanes]
    for i in range(NREL):
        r0 = fx["rows0"][i].cpu().numpy().reshape(7, nslot)
        for v, name in enumerate(("rlon", "rlat", "rzwn", "rmwn", "ramp", "rug", "rvg")):
            h = getattr(rw, name)[:, i].reshape(NT, nslot)
            assert np.array_equal(h[0], r0[v], equal_nan=True), (RELEASES[i], name, "row 0")
            assert np.array_equal(h[1:], ref[i]["rows"][:, :, v].T, equal_nan=True), (RELEASES[i], name)
        sel = slice(i * nslot, (i + 1) * nslot)
        assert np.array_equal(res.nacc[sel].cpu().numpy(), ref[i]["nacc"])
        assert np.array_equal(res.nanrow[sel].cpu().numpy(), ref[i]["nanrow"])
    live = np.concatenate([~np.isnan(y.sum(0).cpu().numpy()) for y in fx["y0"]])
    failed, brk = member_outcomes(np.repeat(np.arange(NREL), nslot), live, np.ones(NREL * nslot),
                                  np.concatenate([r["nanrow"] for r in ref]), NREL, NT)
    assert res.failed == failed == [False] * NREL and res.break_row == brk
    from scipy.io import netcdf_file
    path = str(tmp_path / "rays.nc")
    rw.output(path)
    with netcdf_file(path, "r", mmap=False) as f:
        assert f.dimensions["release"] == NREL and f.dimensions["time"] == NT
        assert np.array_equal(f.variables["release_time"][:], np.asarray(RELEASES))
        assert f.variables["release_time"].dimensions == ("release",) and f.variables["release_time"].units == b"s"
        assert np.array_equal(f.variables["release_index"][:], np.arange(NREL))
        v = f.variables["rmwn"]
        assert v.dimensions == ("time", "release", "root", "source", "zwn")
        assert np.array_equal(v[:], rw.rmwn, equal_nan=True)


def test_what_release_stacks_refuse_is_refused_before_any_launch(fx):
    from engine import RayEngine
    from levels import Levels
    er = fx["er"]
    y0, rel, _ = _dealing(fx, "major")
    r = _times(rel)
    n = y0.shape[1]

    def sink(*a):
        raise AssertionError("a launch was made")

    def refused(exc, match, eng=er, y=y0, **kw):
        kw = dict(KW, sink=sink, **kw)
        with pytest.raises(exc, match=match):
            eng.integrate(y.clone(), NT, TSTEP, **kw)

    refused(ValueError, "entries", release=r[:-1])
    bad = r.copy()
    bad[17] = float("nan")
    refused(ValueError, "finite", release=bad)
    bad[17] = float("inf")
    refused(ValueError, "finite", release=torch.as_tensor(bad))
    refused(ValueError, "latency", release=r, team=4)
    refused(ValueError, "latency", release=r, team="auto")
    refused(NotImplementedError, "group", release=r, group=object())
    refused(NotImplementedError, "checkpoint", release=r, stop_row=5)
    refused(NotImplementedError, "backward", release=r, backward=True)
    with pytest.raises(NotImplementedError, match="RK4"):
        er.integrate_rk4(y0.clone(), NT, TSTEP, release=r)
    # an engine that is not time-varying; a member stack; fp32 levels
    static = RayEngine.from_packed(fx["lv"].packed[0], fx["lv"].lon, fx["lv"].lat)
    refused(ValueError, "time-varying", eng=static, release=r)
    stack = RayEngine.from_levels(fx["lv"], members=True)
    refused(NotImplementedError, "member", eng=stack, release=r, member=np.zeros(n, np.int64))
    b = S.background_level(0)
    l32 = Levels(b["lat"], b["lon"], 2, fp32=True)
    for j in range(2):
        l32.set_level(j, b["u"], b["v"])
    refused(NotImplementedError, "fp64", eng=RayEngine.from_levels(l32), release=r)
    with pytest.raises(NotImplementedError, match="fp64"):
        l32.state_at(0.0)
    # a state of a release init: no latency mode in run(), no checkpoint; the state untouched
    p = er.params(NT, TSTEP)
    st = er.init(y0.clone(), p, release=r)
    keep = {k: st[k].clone() for k in ("state", "count", "nanrow", "t0")}
    tb = torch.as_tensor(np.arange(NT) * TSTEP, device=er.device)
    out = torch.full((n, 4, 8), -7.0, dtype=torch.float64, device=er.device)
    with pytest.raises(ValueError, match="latency"):
        er.run(st, p, tb, 1, 5, out, order=er.live_first_order_of(st), n_heavy=4)
    with pytest.raises(NotImplementedError, match="checkpoint"):
        er.advance(st, p, tb, 1, stop_row=5, sink=sink)
    for k, v in keep.items():
        assert torch.equal(st[k].view(torch.int64) if v.dtype == torch.float64 else st[k],
                           v.view(torch.int64) if v.dtype == torch.float64 else v), k
    assert (out == -7.0).all()

    class Res:
        state, next_row, backward = st, 5, False

    with pytest.raises(NotImplementedError, match="release"):
        RayEngine.checkpoint(Res)
