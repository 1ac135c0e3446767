"""Gate-crossing maps on the GPU (``rwrt_ray_cross``, cross.py): ``cnt``,
``ncross`` and ``dropped`` equal the definition ``cross.reference_cross``
exactly, ``tfirst`` bit for bit, and ``tsum`` / ``wsum`` agree within the
rounding bound of a sum taken in any order -- for crafted rows in every row
layout (dense, tails, row blocks), under contention, through
``RayEngine.integrate`` / ``integrate_rk4`` in any chunking and row layout, next
to a ``DensitySink`` in one ``Tee``, across shards, through ``WR.ray_cross`` on
the reference's C1 history, as the selection of a second integration, and on a
time-varying background."""
import math

import numpy as np
import pytest
import torch

import synthetic as S
from cross import CrossMap, CrossSink, CrossSpec, Gate
from density import DensityMap, DensitySink, DensitySpec, reference_bins
from engine import Tails
from summary import Tee
from support.cases import NT_C2, c1_wr, c2_chan, c2_hist, c2_wr, c2_y0, engine, tv_engine
from support.cases_cross import (GATES8, VARIANTS, assert_c1, assert_cross, assert_crafted_is_rich, c1_spec,
                                 crafted_spec, reference_and_abs)
from support.cases_track import assert_track, crafted_history, device_layouts, start
from support.cases_track import reference_and_abs as track_reference_and_abs
from support.dist import one_rank
from track import TrackMap, TrackSink, TrackSpec

pytestmark = pytest.mark.gpu
DEV = "cuda"


def scaled(m, factor):
    """The maps and ncross of ``factor`` identical deliveries (tfirst stays)."""
    return {k: v if v is None or k == "tfirst" else v * factor for k, v in m.items()}


# ------------------------------------------------- crafted rows, entry point
@pytest.mark.parametrize("nray", [41, 130], ids=["41-rays", "130-rays"])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_crafted_rows_every_layout(name, nray):
    """Row 0 and the launch [1, 8) of the host tests (41 rays: a partial wave,
    and 130: three waves, the last partial), every layout, sentinel rows where
    nothing may be read: cnt, ncross and dropped equal reference_cross, tfirst
    bit for bit, tsum and wsum agree to the bound; a second identical
    delivery, the carried rows reset in between, doubles the sums and leaves
    tfirst; launches [1, 4) and [4, 8) give what one launch [1, 8) gives; a
    map without per-ray arrays gives the same maps."""
    spec = crafted_spec(name, 8)
    h = crafted_history(8, seed=3, nray=nray)
    assert {-1, 1, 8, 11} <= set(h["tf"].tolist()) and {-1, 3} <= set(h["chan"].tolist())
    want, a = reference_and_abs(h["rows"], h["chan"], spec)
    if spec.ngate == 8:
        assert_crafted_is_rich(h["rows"], h["chan"], spec)
    assert want["ncross"].sum() > 5
    row0 = h["rows"][:, 0]
    whole, first, second = device_layouts(h, 1, 8), device_layouts(h, 1, 4), device_layouts(h, 4, 8)
    for layout, (view, tails, slots) in whole.items():
        m = start(CrossMap(spec, nray, DEV, h["chan"]), row0)
        got = m.numpy()
        # row 0 crosses nothing
        assert got["cnt"].sum() == 0 and got["ncross"].sum() == 0 and np.isnan(got["tfirst"]).all()
        m.add_rows(1, 8, view, tails, slots)
        assert_cross(m.numpy(), want, a, (name, layout))
        start(m.restart(), row0).add_rows(1, 8, view, tails, slots)
        assert_cross(m.numpy(), scaled(want, 2), 2 * a, (name, layout, "twice"))
        m2 = start(CrossMap(spec, nray, DEV, h["chan"]), row0)
        m2.add_rows(1, 4, *first[layout])
        m2.add_rows(4, 8, *second[layout])
        assert_cross(m2.numpy(), want, a, (name, layout, "in two launches"))
        m3 = start(CrossMap(spec, nray, DEV, h["chan"]), row0)
        m3.ncross = m3.tfirst = None                                          # maps only
        m3.add_rows(1, 8, view, tails, slots)
        got = dict(cnt=m3.cnt.cpu().numpy(), tsum=m3.tsum.cpu().numpy(), dropped=int(m3.dropped.item()),
                   wsum=None if m3.wsum is None else m3.wsum.cpu().numpy())
        assert_cross(got, want, a, (name, layout, "maps only"), per_ray=False)


def test_contention_one_bin():
    """4 160 rays all crossing 0 deg northward in one bin on segment 1 (t = 1/4:
    tc = 0.25 and the weight 3.0 are dyadic, so the sums are exact in any
    order) and then the meridian 0 deg westward in one bin on segment 2 (sums
    to the bound), in one launch; the same with the last rows as a tail."""
    nray = 4160
    rows = np.zeros((nray, 4, 8))
    rows[:, :, 0] = [1.0, 2.0, -0.5, -0.5]
    rows[:, :, 1] = [-0.25, 0.75, 0.75, 0.75]
    rows[:, :, 4] = 1.0
    rows[:, :, 5] = [2.0, 6.0, 1.0, 1.0]
    spec = CrossSpec((Gate.lat(0.0), Gate.lon(0.0)), 360, weight="ug")
    want, a = reference_and_abs(rows, None, spec)
    assert want["cnt"].sum() == 2 * nray and np.count_nonzero(want["cnt"]) == 2
    for tailed in (False, True):
        m = start(CrossMap(spec, nray, DEV), rows[:, 0])
        if tailed:
            tails = Tails(nray, DEV)
            tails.frm.fill_(2)
            tails.row.copy_(torch.as_tensor(rows[:, 2]))
            buf = rows[:, 1:].copy()
            buf[:, 1:, 0], buf[:, 1:, 1] = 1.0, -1.0                    # sentinel rows: they would cross back
            m.add_rows(1, 4, torch.as_tensor(buf, device=DEV), tails)
        else:
            m.add_rows(1, 4, torch.as_tensor(rows[:, 1:], device=DEV))
        got = m.numpy()
        assert_cross(got, want, a, ("contention", tailed))
        ix = math.floor(1.25 * spec.inv_dlon)
        assert got["cnt"][0, 0, 0, 0, ix] == nray and got["tsum"][0, 0, 0, 0, ix] == 0.25 * nray
        assert got["wsum"][0, 0, 0, 0, ix] == 3.0 * nray
        assert got["cnt"][0, 1, 1].sum() == nray and np.count_nonzero(got["cnt"][0, 1, 1]) == 1
        assert (got["ncross"][0, 0] == 1).all() and (got["tfirst"][0, 0] == 0.25).all()


# ------------------------------------------------ C2 through the engine
C2_SPEC = CrossSpec((Gate.lat(25.0), Gate.lon(120.0), Gate.lon(180.0), Gate.lon(270.0)), 36, nchan=4, weight="amp",
                    window_rows=12, nt=NT_C2)
_WANT = {}


def c2_want(method="rk45"):
    """reference_cross of the history the summary tests gathered with a plain
    sink, and its sum|v| -- computed once."""
    if method not in _WANT:
        want, a = reference_and_abs(c2_hist("zonal", method), c2_chan(), C2_SPEC)
        for v in list(want.values()) + [a]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WANT[method] = (want, a)
    return _WANT[method]


def c2_cross(idx=None, rk4=False, tee=False, m=None, **kw):
    eng = engine("zonal")
    row0, y0 = c2_y0("zonal")
    if m is None:
        m = start(CrossMap(C2_SPEC, 3072, eng.device, c2_chan()), row0.T)
    sink = CrossSink(m)
    dm = None
    if tee:
        dm = DensityMap(DensitySpec(144, 72, nchan=4, weight="amp"), eng.device)
        sink = Tee(DensitySink(dm, torch.as_tensor(c2_chan())), sink)
    if idx is not None:
        y0 = y0[:, torch.as_tensor(idx)].contiguous()
        sink = sink.take(idx)
    if rk4:
        eng.integrate_rk4(y0, NT_C2, 7200.0, sink=sink, **kw)
    else:
        eng.integrate(y0, NT_C2, 7200.0, ttotal=(NT_C2 - 1) * 7200.0, sink=sink, **kw)
    return (m, dm) if tee else m


def test_c2_reference_is_not_vacuous():
    """The CPU oracle gives 5487 northward and 5600 southward crossings of 25 N
    on 1024 rays and 743, 1125 and 792 eastward crossings of the meridians,
    none westward; the host libm may move a count by a few, so floors."""
    want, _ = c2_want()
    n = want["ncross"].sum(axis=2)
    print("C2 crossings per gate and direction:", n.tolist(), "rays across 25 N:",
          int((want["ncross"][0].sum(axis=0) > 0).sum()), "dropped:", want["dropped"])
    assert n[0].sum() > 5000 and n[0].min() > 2000 and n[2, 0] > 500
    assert n[1, 0] > 300 and n[3, 0] > 300 and want["cnt"].shape == (10, 4, 2, 4, 36)
    assert (want["cnt"].sum(axis=(1, 2, 3, 4)) > 0).all() and (want["cnt"].sum(axis=(0, 1, 2, 4)) > 0).all()


@pytest.mark.parametrize("path", ["slots", "tails", "dense"])
def test_c2_chunking_and_row_layouts(path):
    """chunk = 120, chunk = 5 and short leading launches with the latency mode,
    on the row-block, the tails and the dense path: all equal reference_cross
    of the delivered history."""
    want, a = c2_want()
    eng = engine("zonal")
    try:
        if path == "tails":
            eng.use_slots = False
        if path == "dense":
            eng.use_tails = False
        for kw in (dict(chunk=120), dict(chunk=5), dict(first_chunk=[6, 24], team=[64, 64, 64])):
            assert_cross(c2_cross(**kw).numpy(), want, a, (path, kw))
    finally:
        for name in ("use_slots", "use_tails"):
            eng.__dict__.pop(name, None)


def test_c2_rk4():
    want, a = c2_want("rk4")
    assert want["ncross"].sum() > 5000
    assert_cross(c2_cross(rk4=True, chunk=7).numpy(), want, a, "rk4")


def test_c2_tee_with_a_density_sink():
    """One integration into Tee(DensitySink, CrossSink): the crossing map as
    alone, the density map unchanged."""
    want, a = c2_want()
    m, dm = c2_cross(tee=True, chunk=40)
    got = m.numpy()
    assert_cross(got, want, a, "tee")
    pts = c2_hist("zonal")[:, 1:]
    dens = reference_bins(pts[..., 0], pts[..., 1], pts[..., 4], c2_chan()[:, None],
                          DensitySpec(144, 72, nchan=4, weight="amp"))[0]
    assert np.array_equal(dm.numpy()[0], dens)
    # the derived fields
    cnt = got["cnt"]
    mean = m.mean_rows().cpu().numpy()
    assert np.array_equal(np.isnan(mean), cnt == 0)
    assert np.array_equal(mean[cnt > 0], (got["tsum"] / np.where(cnt == 0, 1, cnt))[cnt > 0])
    assert np.array_equal(m.mean_days(7200.0).cpu().numpy()[cnt > 0], mean[cnt > 0] * (7200.0 / 86400.0))
    assert np.array_equal(np.isnan(m.mean_weight().cpu().numpy()), cnt == 0)
    assert np.array_equal(m.net().cpu().numpy(), cnt[:, :, 0] - cnt[:, :, 1])
    for d, sel in ((None, want["ncross"][0].sum(axis=0) > 0), ("north", want["ncross"][0, 0] > 0),
                   (1, want["ncross"][0, 1] > 0)):
        assert np.array_equal(m.crossed(0, d).cpu().numpy(), sel)
    assert np.array_equal(m.crossed(2, "east").cpu().numpy(), want["ncross"][2, 0] > 0)
    with pytest.raises(ValueError):
        m.crossed(0, "up")
    assert m.bin_edges(0).tolist() == np.linspace(0.0, 360.0, 37).tolist()
    assert m.bin_edges(1).tolist() == np.linspace(-90.0, 90.0, 37).tolist()


def test_c2_shards_combine():
    """The two halves of shard_indices(world=2), permuted and integrated one
    after the other through take(idx) into one map, and the two emulated ranks
    of run_sharded in reverse order (the sharded sink form), equal the whole
    set's map."""
    import shard
    want, a = c2_want()
    row0, y0 = c2_y0("zonal")
    live = ~np.isnan(row0[:5].mean(axis=0))
    rng = np.random.default_rng(2)
    m = None
    for r in range(2):
        m = c2_cross(idx=rng.permutation(shard.shard_indices(live, r, 2)), m=m, chunk=50)
    assert_cross(m.numpy(), want, a, "take")
    eng = engine("zonal")
    m = start(CrossMap(C2_SPEC, 3072, eng.device, c2_chan()), row0.T)
    for r in (1, 0):
        shard.run_sharded(eng, y0, NT_C2, 7200.0, rank=r, world=2, ttotal=(NT_C2 - 1) * 7200.0,
                          sink=CrossSink(m), gather=False)
    assert_cross(m.numpy(), want, a, "run_sharded")


def test_crossed_selects_the_rays_of_a_second_integration():
    """``crossed(0, 'south')`` as the ``idx`` of a second integration through
    ``TrackSink.take``: only the selected rays run, the selection equals the
    NumPy one and the track map is reference_track of those rays' history."""
    want, _ = c2_want()
    m = c2_cross(chunk=60)
    idx = torch.nonzero(m.crossed(0, "south")).reshape(-1)
    sel = np.nonzero(want["ncross"][0, 1] > 0)[0]
    assert np.array_equal(idx.cpu().numpy(), sel) and 500 < len(sel) < 3072
    eng = engine("zonal")
    row0, y0 = c2_y0("zonal")
    tspec = TrackSpec(72, 36, nchan=4, weight="amp")
    tm = start(TrackMap(tspec, 3072, eng.device, c2_chan()), row0.T)
    res = eng.integrate(y0[:, idx.cpu()].contiguous(), NT_C2, 7200.0, ttotal=(NT_C2 - 1) * 7200.0,
                        sink=TrackSink(tm).take(idx), chunk=60)
    chan = np.where(np.isin(np.arange(3072), sel), c2_chan(), -1)
    twant, ta = track_reference_and_abs(c2_hist("zonal"), chan, tspec)
    assert twant["cnt"].sum() > 10000 and res is not None
    assert_track(tm.numpy(), twant, ta, "selected rays")
    # only the selected rays ran: every other column still carries its row 0 (none, for a dead slot: NaN amplitude)
    rest = np.setdiff1d(np.arange(3072), sel)
    lon0 = np.where(np.isfinite(row0[4]), row0[0], np.nan)
    assert np.array_equal(tm.prev[0].cpu().numpy()[rest], lon0[rest], equal_nan=True)
    assert res.ray_steps > 0 and y0[:, idx.cpu()].shape[1] == len(sel)


# ------------------------------------------------------------ WR.ray_cross (C1)
def test_c1_ray_cross_equals_the_reference_history():
    """C1, 90 days through WR.ray_cross by root, in both modes: the literals of
    the definition on the reference's own golden history."""
    spec = c1_spec()
    wr = c1_wr()
    with np.errstate(all="ignore"):
        m = wr.ray_cross(spec, by="root")
    assert m.spec.nchan == 3
    got = m.numpy()
    assert_c1(got, "hip")
    assert got["ncross"].reshape(3, 2, 3, wr.nsource, wr.nzwn).shape == (3, 2, 3, 1, 1)
    assert np.isnan(wr.rlon[1:]).all() and not np.isnan(wr.rlon[0]).any()
    with np.errstate(all="ignore"):
        host = c1_wr().ray_cross(spec, by="root", mode="numpy")
    assert_c1(host, "numpy")
    assert np.array_equal(host["cnt"], got["cnt"]) and np.array_equal(host["ncross"], got["ncross"])
    with pytest.raises(ValueError):
        c1_wr().ray_cross(spec, by="source")


# ------------------------------------------------- time-varying background
def test_time_varying_background():
    eng = tv_engine(False)
    cfg = S.config("C2")
    deg = math.pi / 180.0
    ix, iy = np.meshgrid(np.arange(cfg.nnx), np.arange(cfg.nny))
    slon = ((cfg.SW_lon % 360.0 + ix.ravel() * cfg.dlon) % 360.0) * deg
    slat = (cfg.SW_lat + iy.ravel() * cfg.dlat) * deg
    init = eng.initial_rows(slon, slat, cfg.zwn, cfg.freq)
    y0 = init[:5].reshape(5, -1).contiguous()
    row0 = init.reshape(init.shape[0], -1).cpu().numpy()
    nt = 13
    got = {}
    eng.integrate(y0.clone(), nt, 7200.0, ttotal=(nt - 1) * 7200.0,
                  sink=lambda a, b, o: got.__setitem__(a, o.cpu().numpy().copy()))
    nray = y0.shape[1]
    hist = np.full((nray, nt, 8), np.nan)
    hist[:, 0, :row0.shape[0]] = row0.T
    hist[:, 1:] = np.concatenate([got[k] for k in sorted(got)], axis=1)
    # gates through the cloud of the rays' points: quantiles of its latitudes and longitudes, in whole degrees
    ok = np.isfinite(hist[..., 4])
    lats = np.unique(np.round(np.quantile(hist[..., 1][ok], [0.25, 0.5, 0.75]) / deg))
    lons = np.unique(np.round(np.quantile(hist[..., 0][ok], [0.2, 0.4, 0.6, 0.8]) / deg))
    spec = CrossSpec([Gate.lat(q) for q in lats] + [Gate.lon(q) for q in lons], 90, weight="amp", window_rows=4, nt=nt)
    want, a = reference_and_abs(hist, None, spec)
    print("time-varying: crossings per gate and direction", want["ncross"].sum(axis=2).tolist())
    assert want["ncross"].sum() > 20
    for kw in (dict(), dict(chunk=5)):
        m = start(CrossMap(spec, nray, eng.device), hist[:, 0])
        eng.integrate(y0.clone(), nt, 7200.0, ttotal=(nt - 1) * 7200.0, sink=CrossSink(m), **kw)
        assert_cross(m.numpy(), want, a, kw)


# ------------------------------------------------------------- allreduce
def _allreduce_body(dist, ops):
    rng = np.random.default_rng(0)
    n = 2000
    spec = CrossSpec((Gate.lat(0.0), Gate.lon(180.0)), 36, weight="ug")
    rows = np.zeros((n, 2, 8))
    rows[..., 0] = rng.uniform(0, 6.28, (n, 1)) + rng.uniform(-0.6, 0.6, (n, 2))
    rows[..., 1] = rng.uniform(-0.3, 0.3, (n, 1)) + rng.uniform(-0.3, 0.3, (n, 2))
    rows[..., 4], rows[..., 5] = 1.0, rng.uniform(-2, 2, (n, 2))
    rows[0, 1, 0] = 1e300
    m = CrossMap(spec, n, "cuda:0")
    m.start(rows[:, 0, 0], rows[:, 0, 1], rows[:, 0, 4], rows[:, 0, 5])
    m.add_rows(1, 2, torch.as_tensor(rows[:, 1:], device="cuda:0"))
    before, prev = m.numpy(), m.prev.clone()
    m.allreduce(dist.group.WORLD)
    after = m.numpy()
    same_prev = bool(torch.equal(prev, m.prev))
    kinds = [str(o) for o in ops]
    # WR.ray_cross with a group, through the N-rank branches on one rank
    # (shard.COLLECTIVE_MIN_WORLD = 1, as tests/test_gpu_multirank.py does)
    import shard
    wspec = CrossSpec((Gate.lat(25.0), Gate.lon(180.0)), 36, weight="amp")
    with np.errstate(all="ignore"):
        alone = c2_wr().ray_cross(wspec, by="zwn").numpy()
        shard.COLLECTIVE_MIN_WORLD = 1
        grouped = c2_wr().ray_cross(wspec, by="zwn", group=dist.group.WORLD).numpy()
    return dist.get_backend(), kinds, same_prev, before, after, alone, grouped, len(ops) - len(kinds)


def test_allreduce_one_rank_group_leaves_the_map_unchanged():
    backend, kinds, same_prev, before, after, alone, grouped, nops_wr = one_rank(_allreduce_body)
    assert backend == "nccl" and same_prev
    # cnt tsum wsum dropped ncross | tfirst
    assert len(kinds) == 6 and sum("SUM" in k for k in kinds) == 5 and "MIN" in kinds[-1]
    assert before["ncross"].sum() > 300 and before["dropped"] == 1 and np.isnan(before["tfirst"]).any()
    assert_cross(after, before, None, "one rank")
    # the grouped drop-in: the same map as the run without a group, all-reduced
    assert alone["cnt"].shape == (1, 2, 2, 4, 36) and alone["ncross"].sum() > 1000
    assert_cross(grouped, dict(alone, tsum=grouped["tsum"], wsum=grouped["wsum"]), None, "grouped")
    for name in ("tsum", "wsum"):
        assert np.allclose(alone[name], grouped[name], rtol=1e-12, atol=1e-9)
    assert nops_wr >= 6


# ------------------------------------------------------------------- output
def test_output_round_trips(tmp_path):
    import ncio
    spec = CrossSpec((Gate.lat(0.0), Gate.lon(90.0)), 6, nchan=2, lat_range=(-60.0, 60.0), weight="ug",
                     window_rows=2, nt=4)
    h = crafted_history(4, seed=5, nray=64, tf=np.full(64, 4))
    chan = (np.arange(64) % 2).astype(np.int32)
    m = start(CrossMap(spec, 64, DEV, chan), h["rows"][:, 0])
    m.add_rows(1, 4, torch.as_tensor(h["rows"][:, 1:], device=DEV))
    want, a = reference_and_abs(h["rows"], chan, spec)
    got = m.numpy()
    assert_cross(got, want, a, "output")
    assert got["cnt"].sum() > 10
    for name in ("map.nc", "map.npz"):
        path = str(tmp_path / name)
        m.output(path)
        d = ncio.read(path)
        assert d["cnt"].shape == (2, 2, 2, 2, 6) and np.array_equal(d["cnt"], got["cnt"])
        assert d["cnt"].dtype.kind == ("i" if name.endswith(".npz") else "f")
        assert np.array_equal(d["tsum"], got["tsum"]) and np.array_equal(d["wsum"], got["wsum"])
        assert d["dropped"].tolist() == [float(got["dropped"])]
        assert d["ncross"].shape == (2, 2, 64) and np.array_equal(d["ncross"], got["ncross"])
        assert np.array_equal(d["tfirst"], got["tfirst"], equal_nan=True)
        assert d["gate_kind"].tolist() == [0.0, 1.0] and d["gate_pos"].tolist() == [0.0, 90.0]
        assert d["bin_edges"].shape == (2, 7)
        assert d["bin_edges"][0].tolist() == [0.0, 60.0, 120.0, 180.0, 240.0, 300.0, 360.0] == m.bin_edges(0).tolist()
        assert d["bin_edges"][1].tolist() == [-60.0, -40.0, -20.0, 0.0, 20.0, 40.0, 60.0] == m.bin_edges(1).tolist()
        assert d["bin_centres"][1].tolist() == [-50.0, -30.0, -10.0, 10.0, 30.0, 50.0]
    assert len(GATES8) == 8
