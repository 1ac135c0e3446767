"""Member stacks on the GPU (rwrt_rk45_*_stack, RayEngine.from_levels(members=True),
ensemble.EnsembleWR): a ray's rows, counters and state are bit for bit what the
static engine of the same build (``RayEngine.from_packed(levels.packed[m], ..)``)
gives for that ray on its member alone -- whatever the other rays, the queue
order, the row layout or the chunking.

Members: the zonal state, the non-zonal state and level 8 of the time-varying
family, 2.5 degrees; 4 x 4 sources x 4 wavenumbers x 3 roots = 192 slots per
member, 576 rays (no multiple of 64 x 3: every wave ends in a drain); 181 rows
of 2 h.  The static runs are computed once and shared."""
import numpy as np
import pytest
import torch

import synthetic as S

pytestmark = pytest.mark.gpu

NT, TSTEP = 181, 7200.0
KINDS = ("zonal", "nonzonal", "level8")


def _bg(kind):
    return S.background_level(8) if kind == "level8" else S.background(kind)


def _cfg():
    return S.config("C2", SW_lon=90, SW_lat=-10, dlon=25, dlat=25, nnx=4, nny=4, zwn=[1, 3, 5, 7])


def _levels(kinds):
    from levels import Levels
    bgs = [_bg(k) for k in kinds]
    lv = Levels(bgs[0]["lat"], bgs[0]["lon"], len(kinds))
    lv.set_levels(np.stack([b["u"] for b in bgs]), np.stack([b["v"] for b in bgs]))
    return lv


def _ensemble(lv):
    from ensemble import EnsembleWR
    cfg = _cfg()
    ew = EnsembleWR(lv, cfg.nzwn, cfg.nsource, TSTEP, (NT - 1) * TSTEP)
    ew.set_zwn(cfg.zwn)
    ew.set_source_matrix(cfg.SW_lon, cfg.SW_lat, cfg.dlon, cfg.dlat, cfg.nnx, cfg.nny)
    return ew


class Collect:
    """A dense collecting sink: rows 1..nt-1 as ``[nray, nt-1, 8]``."""

    def __init__(self, nray, device):
        self.rows = torch.full((nray, NT - 1, 8), -7.0, dtype=torch.float64, device=device)

    def __call__(self, i0, i1, rows):
        self.rows[:, i0 - 1:i1 - 1] = rows


def _result(res, rows):
    return dict(rows=rows.cpu().numpy(), nacc=res.nacc.cpu().numpy(), nrej=res.nrej.cpu().numpy(),
                nanrow=res.nanrow.cpu().numpy())


def _same(got, want, what):
    for k in ("rows", "nacc", "nrej", "nanrow"):
        if k in got:
            assert np.array_equal(got[k], want[k], equal_nan=True), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def fx():
    from engine import RayEngine
    lv = _levels(KINDS)
    ew = _ensemble(lv)
    nslot = 3 * ew.nsource * ew.nzwn
    assert nslot == 192
    es = RayEngine.from_levels(lv, members=True)
    statics = [RayEngine.from_packed(lv.packed[m], lv.lon, lv.lat) for m in range(len(KINDS))]
    rows0 = [e.initial_rows(ew.source_lon, ew.source_lat, ew.zwn, ew.freq) for e in statics]   # [7, 3, ns, nz]
    y0 = [r[:5].reshape(5, nslot).contiguous() for r in rows0]
    ref = []
    for e, y in zip(statics, y0):
        c = Collect(nslot, e.device)
        res = e.integrate(y.clone(), NT, TSTEP, ttotal=(NT - 1) * TSTEP, sink=c)
        ref.append(_result(res, c.rows))
    # what the comparisons below need to see (else they could pass vacuously)
    for m, (r, y) in enumerate(zip(ref, y0)):
        live0 = ~torch.isnan(y.sum(0)).cpu().numpy()
        assert live0.sum() >= 30 and (~live0).sum() >= 1, (KINDS[m], int(live0.sum()))
        assert (~np.isnan(r["rows"][:, -1, 0])).sum() >= 1, KINDS[m]
        froze = r["nanrow"][live0]
        if m > 0:
            assert ((froze >= 1) & (froze < 90)).sum() >= 3 and ((froze >= 90) & (froze < NT)).sum() >= 3, \
                (KINDS[m], sorted(froze[froze < NT].tolist()))
    return dict(lv=lv, ew=ew, es=es, statics=statics, rows0=rows0, y0=y0, ref=ref, nslot=nslot)


def _dealing(fx, how):
    """``(y0[5, 576], member[576], slot[576])``: ray r is slot ``slot[r]`` of
    member ``member[r]``.  'major': member after member; 'robin': ray r in
    member r % 3 -- neighbouring queue entries share a source and differ in
    member."""
    n, nm = fx["nslot"], len(KINDS)
    if how == "major":
        member, slot = np.repeat(np.arange(nm), n), np.tile(np.arange(n), nm)
    else:
        member, slot = np.tile(np.arange(nm), n), np.repeat(np.arange(n), nm)
    y0 = torch.stack([fx["y0"][m][:, j] for m, j in zip(member, slot)], dim=1).contiguous()
    return y0, member, slot


def _expected(fx, member, slot):
    ref = fx["ref"]
    return {k: np.stack([ref[m][k][j] for m, j in zip(member, slot)]) for k in ("rows", "nacc", "nrej", "nanrow")}


def test_initial_rows_and_init_equal_the_members(fx):
    es, ew = fx["es"], fx["ew"]
    got = es.initial_rows(ew.source_lon, ew.source_lat, ew.zwn, ew.freq)
    assert tuple(got.shape) == (3, 7, 3, ew.nsource, ew.nzwn)
    for m in range(3):
        assert np.array_equal(got[m].cpu().numpy(), fx["rows0"][m].cpu().numpy(), equal_nan=True), KINDS[m]
    p = es.params(NT, TSTEP)
    for how in ("major", "robin"):
        y0, member, slot = _dealing(fx, how)
        st = es.init(y0.clone(), p, member)
        assert st["member"].dtype == torch.int32 and np.array_equal(st["member"].cpu().numpy(), member)
        state, live = st["state"].cpu().numpy(), st["live"].cpu().numpy()
        total = np.zeros(2, np.int64)
        for m, e in enumerate(fx["statics"]):
            sm = e.init(fx["y0"][m].clone(), p)
            total += sm["summary"].cpu().numpy()
            sel = member == m
            assert np.array_equal(state[:, sel], sm["state"].cpu().numpy()[:, slot[sel]], equal_nan=True), (how, KINDS[m])
            assert np.array_equal(live[sel], sm["live"].cpu().numpy()[slot[sel]])
        assert np.array_equal(st["summary"].cpu().numpy(), total)
        assert (st["count"] == 0).all() and (st["nanrow"] == NT).all()
        # take() carries the member
        idx = torch.arange(5, 40, 3, device=es.device)
        assert np.array_equal(es.take(st, idx)["member"].cpu().numpy(), member[5:40:3])


LAYOUTS = ("one_launch", "chunks37", "own_buffer", "density_slots", "no_tails")


@pytest.mark.parametrize("how", ("major", "robin"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_rows_and_counters_equal_the_static_engine(fx, layout, how):
    """Rows [nray, 180, 8], nacc, nrej, nanrow: one launch; five launches of
    37 rows (rays freeze on both sides of the boundaries: the frozen-flag and
    tail paths); the caller's own dense buffer; a sink that takes row blocks
    (DensitySink); and with every row written by the launch itself."""
    from density import DensityMap, DensitySink, DensitySpec
    from engine import RayEngine
    es = fx["es"]
    y0, member, slot = _dealing(fx, how)
    want = _expected(fx, member, slot)
    kw = dict(ttotal=(NT - 1) * TSTEP, member=member)
    n = y0.shape[1]
    if layout == "density_slots":
        spec = DensitySpec(72, 36, nchan=3)
        dmap = DensityMap(spec, es.device)
        res = es.integrate(y0.clone(), NT, TSTEP, chunk=37, sink=DensitySink(dmap, member.astype(np.int32)), **kw)
        got = _result(res, torch.zeros(0))
        del got["rows"]
        assert es.rows_bytes < n * 37 * 64   # (row blocks for the live rays only)
        for m, e in enumerate(fx["statics"]):
            one = DensityMap(DensitySpec(72, 36), e.device)
            e.integrate(fx["y0"][m].clone(), NT, TSTEP, ttotal=(NT - 1) * TSTEP, sink=DensitySink(one))
            assert np.array_equal(dmap.count[m].cpu().numpy(), one.count[0].cpu().numpy()), KINDS[m]
    elif layout == "own_buffer":
        out = torch.full((n, NT - 1, 8), -7.0, dtype=torch.float64, device=es.device)
        res = es.integrate(y0.clone(), NT, TSTEP, out=out, **kw)
        got = _result(res, out)
    else:
        c = Collect(n, es.device)
        tails = RayEngine.use_tails
        try:
            if layout == "no_tails":
                es.use_tails = False
            res = es.integrate(y0.clone(), NT, TSTEP, chunk=None if layout == "one_launch" else 37, sink=c, **kw)
            assert len(res.bounds) == (1 if layout == "one_launch" else 5)
        finally:
            es.use_tails = tails
        got = _result(res, c.rows)
    _same(got, want, f"{layout}/{how}")
    assert res.failed is False and res.break_row is None


def test_priority_order_with_a_leading_chunk_gives_the_same_bits(fx):
    es = fx["es"]
    y0, member, slot = _dealing(fx, "robin")
    c = Collect(y0.shape[1], es.device)
    res = es.integrate(y0.clone(), NT, TSTEP, ttotal=(NT - 1) * TSTEP, member=member, sink=c,
                       order_policy="priority", first_chunk=[12])
    assert [b - a for a, b in res.bounds] == [12, 168]
    _same(_result(res, c.rows), _expected(fx, member, slot), "priority")


def test_four_copies_of_one_state_round_robin(fx):
    """Rays dealt round-robin over four copies of the non-zonal state equal the
    static engine on those rays (the stack path changes nothing but the
    member offset)."""
    from engine import RayEngine
    lv = _levels(("nonzonal",) * 4)
    es = RayEngine.from_levels(lv, members=True)
    y0 = fx["y0"][1]
    member = np.arange(y0.shape[1]) % 4
    c = Collect(y0.shape[1], es.device)
    res = es.integrate(y0.clone(), NT, TSTEP, ttotal=(NT - 1) * TSTEP, member=torch.as_tensor(member), sink=c, chunk=37)
    _same(_result(res, c.rows), fx["ref"][1], "four copies")


def test_more_live_rays_than_lanes_one_row_per_launch(fx):
    """The stale-cell trap needs a lane that pulls a second ray within one
    launch: more live rays than the persistent grid has lanes (256 CUs x 256).
    The round-robin dealing repeated 480 times (276 480 rays, ~85 000 live),
    13 rows, one row per launch: a lane's second ray often starts in the cell
    its first one still held, in another member.  Every copy of a ray must
    equal the static engine's ray."""
    es = fx["es"]
    nt, rep = 13, 480
    y0, member, slot = _dealing(fx, "robin")
    ref = []
    for e, y in zip(fx["statics"], fx["y0"]):
        out = torch.empty((y.shape[1], nt - 1, 8), dtype=torch.float64, device=e.device)
        res = e.integrate(y.clone(), nt, TSTEP, ttotal=(nt - 1) * TSTEP, out=out)
        ref.append(_result(res, out))
    want = {k: np.stack([ref[m][k][j] for m, j in zip(member, slot)]) for k in ("rows", "nacc", "nrej", "nanrow")}
    live = int((~np.isnan(want["rows"][:, 0, 0])).sum()) * rep
    lanes = torch.cuda.get_device_properties(es.device).multi_processor_count * 256
    assert live > lanes, (live, lanes)
    n = y0.shape[1] * rep
    out = torch.empty((n, nt - 1, 8), dtype=torch.float64, device=es.device)

    def sink(i0, i1, rows):
        out[:, i0 - 1:i1 - 1] = rows

    res = es.integrate(y0.repeat(1, rep), nt, TSTEP, ttotal=(nt - 1) * TSTEP, member=np.tile(member, rep),
                       sink=sink, chunk=1)
    got = _result(res, out)
    for k in ("rows", "nacc", "nrej", "nanrow"):
        g = got[k].reshape((rep,) + want[k].shape)
        bad = [r for r in range(rep) if not np.array_equal(g[r], want[k], equal_nan=True)]
        assert not bad, f"{k}: {len(bad)} of {rep} copies differ from the static engine (first: copy {bad[0]})"


def test_products_by_member_equal_the_per_member_products(fx):
    from cross import CrossMap, CrossSink, CrossSpec, Gate
    from density import DensityMap, DensitySink, DensitySpec
    from summary import RaySummary, SummarySink
    ew, nslot = fx["ew"], fx["nslot"]
    kw = dict(ttotal=(NT - 1) * TSTEP)
    regions = [(60.0, 200.0, 0.0, 60.0), (300.0, 40.0, -60.0, 10.0)]
    gates = (Gate.lat(25.0), Gate.lon(180.0))
    # the per-member products, from the static engines
    counts, sums, crosses = [], [], []
    for m, e in enumerate(fx["statics"]):
        r0 = fx["rows0"][m]
        one = DensityMap(DensitySpec(72, 36), e.device)
        one.add_points(r0[0], r0[1])
        e.integrate(fx["y0"][m].clone(), NT, TSTEP, sink=DensitySink(one), **kw)
        counts.append(one.count[0].cpu().numpy())
        rs = RaySummary(nslot, regions, e.device)
        rs.start(r0[0], r0[1], r0[3], r0[4])
        e.integrate(fx["y0"][m].clone(), NT, TSTEP, sink=SummarySink(rs), **kw)
        sums.append(rs.numpy())
        cm = CrossMap(CrossSpec(gates, 36), nslot, e.device)
        cm.start(r0[0], r0[1], r0[4])
        e.integrate(fx["y0"][m].clone(), NT, TSTEP, sink=CrossSink(cm), **kw)
        crosses.append(cm.numpy())
    assert sum(int(c["ncross"].sum()) for c in crosses) > 20
    # one map per member
    dmap = ew.ray_density(DensitySpec(72, 36), by="member")
    got = dmap.count.cpu().numpy()
    assert got.shape == (3, 36, 72)
    for m in range(3):
        assert np.array_equal(got[m], counts[m]), KINDS[m]
    # the summaries: fields (nmember, 3, nsource, nzwn)
    rs = ew.ray_summary(regions=regions).numpy()
    for name, a in rs.items():
        lead = a.shape[:-4]
        assert a.shape[-4:] == ew.slot_shape, name
        for m in range(3):
            want = sums[m][name].reshape(lead + ew.slot_shape[1:])
            assert np.array_equal(a[..., m, :, :, :], want, equal_nan=True), (name, KINDS[m])

    # a gate-crossing map through reduce
    def make(device, chan, nray):
        cm = CrossMap(CrossSpec(gates, 36, nchan=3), nray, device, chan)
        cm.start(ew.rlon[0], ew.rlat[0], ew.ramp[0])
        return cm, CrossSink(cm)

    cm = ew.reduce(make).numpy()
    for m in range(3):
        sel = slice(m * nslot, (m + 1) * nslot)
        assert np.array_equal(cm["cnt"][:, :, :, m], crosses[m]["cnt"][:, :, :, 0]), KINDS[m]
        assert np.array_equal(cm["ncross"][:, :, sel], crosses[m]["ncross"])
        assert np.array_equal(cm["tfirst"][:, :, sel], crosses[m]["tfirst"], equal_nan=True)


def test_ensemble_ray_run_equals_a_wr_per_member(fx, tmp_path):
    from bs import BS
    from wr import WR
    ew, cfg = fx["ew"], _cfg()
    res = ew.ray_run()
    assert ew.rlon.shape == (NT, 3, 3, cfg.nsource, cfg.nzwn)
    assert len(res.break_row) == 3 and len(res.failed) == 3
    for m, kind in enumerate(KINDS):
        bg = _bg(kind)
        bs = BS(len(bg["lon"]), len(bg["lat"]))
        bs.load_arrays(**bg)
        bs.ready(xcyclic=True)
        w = WR(cfg.nzwn, cfg.nsource, TSTEP, (NT - 1) * TSTEP, 0.0, nx=bs.nlon, ny=bs.nlat)
        w.bs = bs
        w.set_zwn(cfg.zwn)
        w.set_source_matrix(cfg.SW_lon, cfg.SW_lat, cfg.dlon, cfg.dlat, cfg.nnx, cfg.nny)
        w.ray_run(mode="hip", inte_method="rk45")
        for name in ("rlon", "rlat", "rzwn", "rmwn", "ramp", "rug", "rvg"):
            assert np.array_equal(getattr(ew, name)[:, m], getattr(w, name), equal_nan=True), (kind, name)
        assert res.break_row[m] == w.last_run.break_row and res.failed[m] == w.last_run.failed
        sel = slice(m * fx["nslot"], (m + 1) * fx["nslot"])
        assert np.array_equal(res.nacc[sel].cpu().numpy(), w.last_run.nacc.cpu().numpy())
    ew.output(str(tmp_path / "rays.npz"))


def test_what_stacks_refuse_is_refused_before_any_launch(fx):
    from engine import RayEngine
    from levels import Levels
    es = fx["es"]
    y0, member, _ = _dealing(fx, "major")
    kw = dict(ttotal=(NT - 1) * TSTEP)

    def sink(*a):
        raise AssertionError("a launch was made")

    with pytest.raises(ValueError, match="team"):
        es.integrate(y0.clone(), NT, TSTEP, member=member, team=4, sink=sink, **kw)
    bad = member.copy()
    bad[17] = 3
    with pytest.raises(ValueError, match="member"):
        es.integrate(y0.clone(), NT, TSTEP, member=bad, sink=sink, **kw)
    bad[17] = -1
    with pytest.raises(ValueError, match="member"):
        es.integrate(y0.clone(), NT, TSTEP, member=bad, sink=sink, **kw)
    with pytest.raises(ValueError, match="member"):
        es.integrate(y0.clone(), NT, TSTEP, sink=sink, **kw)          # no member at all
    with pytest.raises(ValueError, match="entries"):
        es.integrate(y0.clone(), NT, TSTEP, member=member[:-1], sink=sink, **kw)
    with pytest.raises(NotImplementedError):
        es.integrate(y0.clone(), NT, TSTEP, member=member, group=object(), sink=sink, **kw)
    with pytest.raises(NotImplementedError):
        es.integrate_rk4(y0.clone(), NT, TSTEP)
    with pytest.raises(NotImplementedError):
        es.integrate(y0.clone(), NT, TSTEP, member=member, stop_row=5, sink=sink, **kw)
    with pytest.raises(NotImplementedError):
        es.resume({}, NT, TSTEP)
    b = _bg("zonal")
    with pytest.raises(NotImplementedError, match="fp64"):
        RayEngine.from_levels(Levels(b["lat"], b["lon"], 2, fp32=True), members=True)
    with pytest.raises(ValueError, match="member"):
        fx["statics"][0].init(fx["y0"][0].clone(), es.params(NT, TSTEP), member=member[:192])
