"""Residence-time maps along ray segments on the GPU (``rwrt_ray_track``,
track.py): ``cnt`` and ``dropped`` equal the definition
``track.reference_track`` exactly and ``time`` / ``wsum`` agree within the
rounding bound of a sum taken in any order -- for crafted rows in every row
layout (dense, tails, row blocks), under contention, through
``RayEngine.integrate`` / ``integrate_rk4`` in any chunking and row layout,
next to a ``DensitySink`` in one ``Tee``, across shards, through
``WR.ray_track`` on the reference's C1 history, and on a time-varying
background."""
import math

import numpy as np
import pytest
import torch

import synthetic as S
import track as T
from density import DensityMap, DensitySink, DensitySpec, reference_bins
from engine import Tails
from summary import Tee
from support.cases import NT_C2, c1_wr, c2_chan, c2_hist, c2_wr, c2_y0, engine, tv_engine
from support.cases_track import (C1_TRACK, VARIANTS, assert_track, c1_rows, crafted_history, device_layouts,
                                 reference_and_abs, start, sum_bound)
from support.dist import one_rank
from track import TrackMap, TrackSink, TrackSpec, reference_track

pytestmark = pytest.mark.gpu
DEV = "cuda"


def scaled(m, factor):
    return {k: None if v is None else v * factor for k, v in m.items()}


# ------------------------------------------------- crafted rows, entry point
@pytest.mark.parametrize("nray", [41, 130], ids=["41-rays", "130-rays"])
@pytest.mark.parametrize("shape", [(7, 5, 3), (64, 32, 1)], ids=["7x5x3", "64x32x1"])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_crafted_rows_every_layout(name, shape, nray):
    """Row 0 and the launch [1, 8) of the host tests (41 rays, and 130: three
    waves, the last partial), every layout: cnt and dropped equal
    reference_track, time and wsum agree to the bound; a second identical
    delivery, the carried rows reset in between, doubles everything; launches
    [1, 4) and [4, 8) give what one launch [1, 8) gives.  The rows with lon =
    1e300 go to the device too: the header's drop rule stops them."""
    nx, ny, nchan = shape
    spec = TrackSpec(nx, ny, nchan=nchan, **VARIANTS[name])
    h = crafted_history(8, seed=3, nray=nray)
    if nchan == 1:                                     # channels 0..2 are the one map; -1 and 3 stay outside
        h["chan"] = np.where((h["chan"] >= 0) & (h["chan"] < 3), 0, h["chan"]).astype(np.int32)
    assert {-1, 1, 8, 11} <= set(h["tf"].tolist()) and {-1, 3} <= set(h["chan"].tolist())
    want, a = reference_and_abs(h["rows"], h["chan"], spec)
    assert want["cnt"].sum() > 50 and want["dropped"] > 0
    row0 = h["rows"][:, 0]
    whole, first, second = device_layouts(h, 1, 8), device_layouts(h, 1, 4), device_layouts(h, 4, 8)
    for layout, (view, tails, slots) in whole.items():
        m = start(TrackMap(spec, nray, DEV, h["chan"]), row0)
        assert m.numpy()["cnt"].sum() == 0                                   # row 0 deposits nothing
        m.add_rows(1, 8, view, tails, slots)
        assert_track(m.numpy(), want, a, (name, layout))
        start(m.restart(), row0).add_rows(1, 8, view, tails, slots)
        assert_track(m.numpy(), scaled(want, 2), 2 * a, (name, layout, "twice"))
        m2 = start(TrackMap(spec, nray, DEV, h["chan"]), row0)
        m2.add_rows(1, 4, *first[layout])
        m2.add_rows(4, 8, *second[layout])
        assert_track(m2.numpy(), want, a, (name, layout, "in two launches"))


def exact_lon(spec, X):
    """A longitude whose grid coordinate is exactly X (searched among the
    neighbours of X / inv_dlon: the product is rounded)."""
    lon = X / spec.inv_dlon + spec.lon0
    for step in (math.inf, -math.inf):
        cand = lon
        for _ in range(256):
            if (cand - spec.lon0) * spec.inv_dlon == X:
                return float(cand)
            cand = np.nextafter(cand, step)
    raise AssertionError(f"no longitude with X = {X}")


def test_contention_three_cells():
    """4 160 rays x 7 segments between X = 0.5 and X = 2.5 of one map row, back
    and forth: the weights are 1/4 1/2 1/4 either way (dyadic), so cnt and time
    -- and wsum with ug = 4 -- are exact in any order, and every other cell is
    untouched."""
    nray, nt = 4160, 8
    for spec in (TrackSpec(1440, 720, weight="ug"), TrackSpec(3, 5, weight="ug"),
                 TrackSpec(1440, 720, lon_range=(0.0, 360.0))):
        lon = [exact_lon(spec, 0.5), exact_lon(spec, 2.5)]
        rows = np.zeros((nray, nt, 8))
        rows[..., 0] = np.array([lon[i % 2] for i in range(nt)])
        rows[..., 1], rows[..., 4], rows[..., 5] = 0.1, 1.0, 4.0
        iy = math.floor((0.1 - spec.lat0) * spec.inv_dlat)
        n = nray * (nt - 1)
        for tailed in (False, True):
            m = start(TrackMap(spec, nray, DEV), rows[:, 0])
            if tailed:        # the last four rows as a tail: one more segment, then three at rest in cell 0 or 2
                tails = Tails(nray, DEV)
                tails.frm.fill_(4)
                tails.row.copy_(torch.as_tensor(rows[:, 4]))
                hist = rows.copy()
                hist[:, 4:] = rows[:, 4:5]
                m.add_rows(1, nt, torch.as_tensor(hist[:, 1:], device=DEV), tails)
                want = reference_track(hist[:1], None, spec)
            else:
                m.add_rows(1, nt, torch.as_tensor(rows[:, 1:], device=DEV))
                want = reference_track(rows[:1], None, spec)
            got = m.numpy()
            assert got["dropped"] == 0 and got["cnt"].sum() == want["cnt"].sum() * nray
            assert np.array_equal(got["cnt"], want["cnt"] * nray)
            assert np.array_equal(got["time"], want["time"] * nray) and got["time"].sum() == float(n)
            assert np.count_nonzero(got["cnt"]) == 3 and np.count_nonzero(got["cnt"][0, iy, :3]) == 3
            if not tailed:
                assert got["cnt"][0, iy, :3].tolist() == [n, n, n]
                assert got["time"][0, iy, :3].tolist() == [0.25 * n, 0.5 * n, 0.25 * n]
            if spec.wcol >= 0:
                assert np.array_equal(got["wsum"], 4.0 * got["time"])


def test_start_derived_fields_fold_and_output(tmp_path):
    """``start`` deposits nothing; ``seconds`` and ``mean_weight`` (NaN exactly
    where time is 0); ``fold`` sums three circles onto one; ``output``
    round-trips."""
    import ncio
    spec = TrackSpec(6, 4, nchan=2, lon_range=(-360.0, 720.0), weight="ug")
    dx = 1.0 / spec.inv_dlon
    lon = np.array([[0.5, 1.5], [0.5 - 2.0, 1.5 - 2.0], [0.5 + 2.0, 1.5 + 2.0], [-0.5, -0.5]]) * dx + spec.lon0 + 2 * dx
    rows = np.zeros((4, 2, 8))
    rows[..., 0] = lon
    rows[..., 1], rows[..., 4] = 0.1, 1.0
    rows[..., 5] = np.array([[2.0, 4.0], [1.0, 1.0], [0.0, 8.0], [5.0, 5.0]])
    chan = np.array([0, 0, 0, 1])
    m = start(TrackMap(spec, 4, DEV, chan), rows[:, 0])
    assert m.numpy()["cnt"].sum() == 0 and not torch.isnan(m.prev).any()
    m.add_rows(1, 2, torch.as_tensor(rows[:, 1:], device=DEV))
    want, a = reference_and_abs(rows, chan, spec)
    got = m.numpy()
    assert_track(got, want, a, "two rows")
    assert want["cnt"].sum() == 7 and want["time"].sum() == 4.0
    sec, mean = m.seconds(7200.0).cpu().numpy(), m.mean_weight().cpu().numpy()
    assert np.array_equal(sec, got["time"] * 7200.0)
    assert np.array_equal(np.isnan(mean), got["time"] == 0)
    assert mean[0, 2, 2] == 3.0 and mean[0, 2, 0] == 1.0 and mean[0, 2, 4] == 4.0 and mean[1, 2, 1] == 5.0
    assert m.lon_edges.tolist() == [-360.0, -180.0, 0.0, 180.0, 360.0, 540.0, 720.0]
    assert m.lat_edges[0] == -90.0 and m.lat_edges[-1] == 90.0 and len(m.lat_edges) == 5
    with pytest.raises(ValueError):
        TrackMap(TrackSpec(6, 4), 4, DEV).mean_weight()
    w = m.fold()
    assert w.spec == TrackSpec(2, 4, nchan=2, weight="ug") and w.lon_edges.tolist() == [0.0, 180.0, 360.0]
    wa = w.numpy()
    assert np.array_equal(wa["cnt"], got["cnt"].reshape(2, 4, 3, 2).sum(axis=2)) and wa["cnt"].sum() == 7
    assert np.array_equal(wa["time"], got["time"].reshape(2, 4, 3, 2).sum(axis=2))
    with pytest.raises(ValueError):
        TrackMap(TrackSpec(7, 4, lon_range=(-360.0, 720.0)), 4, DEV).fold()
    with pytest.raises(ValueError):
        w.fold()
    with pytest.raises(ValueError):
        m.add_rows(1, 2, torch.as_tensor(rows[:3, 1:], device=DEV))          # 3 rays, 4 columns, no ray
    with pytest.raises(ValueError):
        TrackMap(spec, 4, DEV).start(rows[:, 0, 0], rows[:, 0, 1], rows[:, 0, 4])   # the weight is missing
    for name in ("map.nc", "map.npz"):
        path = str(tmp_path / name)
        m.output(path)
        d = ncio.read(path)
        assert d["cnt"].shape == (2, 4, 6) and np.array_equal(d["cnt"], got["cnt"])
        if name.endswith(".npz"):
            assert d["cnt"].dtype.kind == "i"
        assert np.array_equal(d["time"], got["time"]) and np.array_equal(d["wsum"], got["wsum"])
        assert d["dropped"].tolist() == [0.0]
        assert d["lon"].tolist() == [-270.0, -90.0, 90.0, 270.0, 450.0, 630.0] and d["lat"][0] == -67.5
        assert np.array_equal(d["lon_edges"], m.lon_edges)


# ------------------------------------------------ C2 through the engine
C2_SPEC = TrackSpec(144, 72, nchan=4, weight="amp")
C2_WINDOW = TrackSpec(216, 36, nchan=4, lon_range=(-360.0, 720.0), need=None, max_cells=4)
_WANT = {}


def c2_want(method="rk45", spec=C2_SPEC):
    """reference_track of the history the summary tests gathered with a plain
    sink, and its sum|v| -- computed once."""
    key = (method, spec)
    if key not in _WANT:
        _WANT[key] = reference_and_abs(c2_hist("zonal", method), c2_chan(), spec)
    return _WANT[key]


def c2_track(spec=C2_SPEC, idx=None, rk4=False, tee=False, m=None, **kw):
    eng = engine("zonal")
    row0, y0 = c2_y0("zonal")
    if m is None:
        m = start(TrackMap(spec, 3072, eng.device, c2_chan()), row0.T)
    sink = TrackSink(m)
    dm = None
    if tee:
        dm = DensityMap(DensitySpec(spec.nx, spec.ny, nchan=4, weight="amp"), eng.device)
        sink = Tee(DensitySink(dm, torch.as_tensor(c2_chan())), sink)
    if idx is not None:
        y0 = y0[:, torch.as_tensor(idx)].contiguous()
        sink = sink.take(idx)
    if rk4:
        eng.integrate_rk4(y0, NT_C2, 7200.0, sink=sink, **kw)
    else:
        eng.integrate(y0, NT_C2, 7200.0, ttotal=(NT_C2 - 1) * 7200.0, sink=sink, **kw)
    return (m, dm) if tee else m


@pytest.mark.parametrize("path", ["slots", "tails", "dense"])
def test_c2_chunking_and_row_layouts(path):
    """chunk = 120, chunk = 5 and short leading launches with the latency mode,
    on the row-block, the tails and the dense path: all equal reference_track
    of the delivered history (cnt and dropped exactly, time and wsum to the
    bound); a window map with a small max_cells too."""
    want, a = c2_want()
    assert want["cnt"].sum() > 100000 and (want["cnt"].sum(axis=(1, 2)) > 0).all()
    wwant, wa = c2_want(spec=C2_WINDOW)
    assert wwant["cnt"].sum() > 10000
    eng = engine("zonal")
    try:
        if path == "tails":
            eng.use_slots = False
        if path == "dense":
            eng.use_tails = False
        for kw in (dict(chunk=120), dict(chunk=5), dict(first_chunk=[6, 24], team=[64, 64, 64])):
            assert_track(c2_track(**kw).numpy(), want, a, (path, kw))
        assert_track(c2_track(C2_WINDOW, chunk=50).numpy(), wwant, wa, (path, "window"))
    finally:
        for name in ("use_slots", "use_tails"):
            eng.__dict__.pop(name, None)


def test_c2_rk4():
    want, a = c2_want("rk4")
    assert_track(c2_track(rk4=True, chunk=7).numpy(), want, a, "rk4")


def test_c2_tee_with_a_density_sink():
    """One integration into Tee(DensitySink, TrackSink): the track map as
    alone, the density map unchanged."""
    want, a = c2_want()
    m, dm = c2_track(tee=True, chunk=40)
    got = m.numpy()
    assert_track(got, want, a, "tee")
    pts = c2_hist("zonal")[:, 1:]
    dens = reference_bins(pts[..., 0], pts[..., 1], pts[..., 4], c2_chan()[:, None],
                          DensitySpec(C2_SPEC.nx, C2_SPEC.ny, nchan=4, weight="amp"))[0]
    assert np.array_equal(dm.numpy()[0], dens)
    for q, name in enumerate(("time", "wsum")):
        err, b = np.abs(got[name] - want[name]), sum_bound(want["cnt"], a[q])
        print(f"C2 {name}: max err {err.max():.3g}, max err/bound {np.max(err[b > 0] / b[b > 0]):.3g}")
    ok = T.valid_rows(c2_hist("zonal"), C2_SPEC)
    live = (ok[:, 1:] & ok[:, :-1]).sum()
    print(f"C2: {live} segments, {want['cnt'].sum()} cells, {want['dropped']} dropped")


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
        m = c2_track(idx=rng.permutation(shard.shard_indices(live, r, 2)), m=m, chunk=50)
    assert_track(m.numpy(), want, a, "take")
    eng = engine("zonal")
    m = start(TrackMap(C2_SPEC, 3072, eng.device, c2_chan()), row0.T)
    for r in (1, 0):
        shard.run_sharded(eng, y0, NT_C2, 7200.0, rank=r, world=2, ttotal=(NT_C2 - 1) * 7200.0,
                          sink=TrackSink(m), gather=False)
    assert_track(m.numpy(), want, a, "run_sharded")


# ------------------------------------------------------------ WR.ray_track (C1)
def test_c1_ray_track_equals_the_reference_history():
    """C1, 90 days through WR.ray_track by root, in both modes: equal to
    reference_track of the reference's own golden history; the cells are the
    literals of the definition and the time is the 2160 live segments."""
    nseg, ndrop, ncell, total = C1_TRACK[(1440, 720)]
    spec = TrackSpec(1440, 720, weight="ug")
    want, a = reference_and_abs(c1_rows(), np.arange(3), TrackSpec(1440, 720, nchan=3, weight="ug"))
    assert want["cnt"].sum() == ncell and want["cnt"].sum(axis=(1, 2))[0] == 0
    wr = c1_wr()
    with np.errstate(all="ignore"):
        m = wr.ray_track(spec, by="root")
    assert m.spec.nchan == 3
    got = m.numpy()
    assert_track(got, want, a, "hip")
    assert got["cnt"].sum() == ncell and got["dropped"] == ndrop and abs(got["time"].sum() - total) < 1e-9
    assert np.isnan(wr.rlon[1:]).all() and not np.isnan(wr.rlon[0]).any()
    with np.errstate(all="ignore"):
        host = c1_wr().ray_track(spec, by="root", mode="numpy")
    assert_track(host, want, a, "numpy")
    assert host["cnt"].sum() == ncell and abs(host["time"].sum() - total) < 1e-9
    coarse = c1_wr()
    with np.errstate(all="ignore"):
        g = coarse.ray_track(TrackSpec(360, 180), by="root").numpy()
    assert g["cnt"].sum() == C1_TRACK[(360, 180)][2] and abs(g["time"].sum() - total) < 1e-9 and g["wsum"] is None
    with pytest.raises(ValueError):
        c1_wr().ray_track(spec, by="source")


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
    spec = TrackSpec(360, 180, weight="amp")
    want, a = reference_and_abs(hist, None, spec)
    assert want["cnt"].sum() > 1000
    for kw in (dict(), dict(chunk=5)):
        m = start(TrackMap(spec, nray, eng.device), hist[:, 0])
        eng.integrate(y0.clone(), nt, 7200.0, ttotal=(nt - 1) * 7200.0, sink=TrackSink(m), **kw)
        assert_track(m.numpy(), want, a, kw)


# ------------------------------------------------------------- allreduce
def _allreduce_body(dist, ops):
    rng = np.random.default_rng(0)
    n = 2000
    spec = TrackSpec(144, 72, weight="ug")
    rows = np.zeros((n, 2, 8))
    rows[..., 0] = rng.uniform(0, 6.28, (n, 1)) + rng.uniform(-0.3, 0.3, (n, 2))
    rows[..., 1] = rng.uniform(-1.4, 1.4, (n, 1)) + rng.uniform(-0.1, 0.1, (n, 2))
    rows[..., 4], rows[..., 5] = 1.0, rng.uniform(-2, 2, (n, 2))
    rows[0, 1, 0] = 1e300
    m = TrackMap(spec, n, "cuda:0")
    m.start(rows[:, 0, 0], rows[:, 0, 1], rows[:, 0, 4], rows[:, 0, 5])
    m.add_rows(1, 2, torch.as_tensor(rows[:, 1:], device="cuda:0"))
    before, prev = m.numpy(), m.prev.clone()
    m.allreduce(dist.group.WORLD)
    after = m.numpy()
    same_prev = bool(torch.equal(prev, m.prev))
    nops = len(ops)
    all_sum = all(o == dist.ReduceOp.SUM for o in ops)
    # WR.ray_track with a group, through the N-rank branches on one rank
    # (shard.COLLECTIVE_MIN_WORLD = 1, as tests/test_gpu_multirank.py does)
    import shard
    with np.errstate(all="ignore"):
        alone = c2_wr().ray_track(spec, by="zwn").numpy()
        shard.COLLECTIVE_MIN_WORLD = 1
        grouped = c2_wr().ray_track(spec, by="zwn", group=dist.group.WORLD).numpy()
    return dist.get_backend(), nops, all_sum, same_prev, before, after, alone, grouped, len(ops) - nops


def test_allreduce_one_rank_group_leaves_the_map_unchanged():
    backend, nops, all_sum, same_prev, before, after, alone, grouped, nops_wr = one_rank(_allreduce_body)
    assert backend == "nccl" and nops == 4 and all_sum and same_prev          # cnt, time, wsum, dropped
    assert before["cnt"].sum() > 2000 and before["dropped"] == 1
    assert_track(after, before, None, "one rank")
    # the grouped drop-in: the same map as the run without a group, all-reduced
    assert alone["cnt"].shape == (4, 72, 144) and alone["cnt"].sum() > 10000
    assert np.array_equal(alone["cnt"], grouped["cnt"]) and alone["dropped"] == grouped["dropped"]
    for name in ("time", "wsum"):
        assert np.allclose(alone[name], grouped[name], rtol=1e-12, atol=1e-9)
    assert nops_wr >= 4
