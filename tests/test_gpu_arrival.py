"""Arrival-time maps on the GPU (``rwrt_ray_arrival``, arrival.py): ``first``,
``last`` and ``count`` equal the NumPy definition ``arrival.reference_arrival``
exactly -- for crafted rows in every row layout (dense, tails, row blocks),
under contention, through ``RayEngine.integrate`` / ``integrate_rk4`` in any
chunking and row layout, next to a ``DensitySink`` in one ``Tee``, across
shards, through ``WR.ray_arrival`` on the reference's C1 history and on a
time-varying background."""
import math

import numpy as np
import pytest
import torch

import synthetic as S
from arrival import ArrivalMap, ArrivalSink, ArrivalSpec, reference_arrival
from conftest import golden
from density import DensityMap, DensitySink, DensitySpec, bin_index
from engine import Tails
from summary import Tee
from support.cases import NT_C2, c1_wr, c2_chan, c2_ref, c2_wr, engine, tv_engine
from support.cases_density import BOUNDARY_TF, I0, I1, NRAY, corner_points, crafted, launch
from support.dist import one_rank
from support.rows import SENTINEL, layout_device

pytestmark = pytest.mark.gpu
DEV = "cuda"


def assert_same(got, want, what=""):
    for k in ("first", "last"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k)
    if want["count"] is None:
        assert got["count"] is None, what
    else:
        assert got["count"].dtype == np.int64 and np.array_equal(got["count"], want["count"]), (what, "count")


# ------------------------------------------------- crafted rows, entry point
def boundary_tf():
    j = np.arange(NRAY)
    return np.where(j % 3 == 0, np.array(BOUNDARY_TF[:2])[(j // 3) % 2], np.array(BOUNDARY_TF)[j % 8])


@pytest.mark.parametrize("require", ["amp", None])
@pytest.mark.parametrize("nx,ny,nchan,window_rows,boundary", [
    (7, 5, 3, 1, False), (7, 5, 3, 2, False), (7, 5, 3, 3, False), (7, 5, 3, 100, False), (7, 5, 3, None, False),
    (7, 5, 3, 2, True), (7, 5, 3, 3, True), (1440, 720, 1, 2, False)],
    ids=["7x5x3-W1", "7x5x3-W2", "7x5x3-W3", "7x5x3-W100", "7x5x3-none", "7x5x3-W2-tf", "7x5x3-W3-tf",
         "1440x720-W2"])
def test_crafted_rows_every_layout(nx, ny, nchan, window_rows, boundary, require):
    """130 rays x 7 rows from row 1 (mid-window for W = 2 and W = 3), every
    layout: the three outputs equal reference_arrival; a second identical call
    leaves first and last and doubles count; launches [1, 4) and [4, 8) give
    what one launch [1, 8) gives.  ``boundary``: tail_from below, at and above
    the launch and rows read on either side of the kernel's batch of 4."""
    spec = ArrivalSpec(nx, ny, nt=I1, nchan=nchan, require=require, window_rows=window_rows)
    rows, tail, tf = crafted(seed=4, tf=boundary_tf()) if boundary else crafted()
    chan = np.random.default_rng(7).integers(-1, nchan + 1, NRAY).astype(np.int32)
    assert {-1, nchan} <= set(chan.tolist())
    want = reference_arrival(rows[..., 0], rows[..., 1], rows[..., 4], chan, spec, row0=I0)
    nbin = int((bin_index(rows[..., 0], rows[..., 1], rows[..., 4], chan[:, None], spec.bins) >= 0).sum())
    assert 0 < nbin < NRAY * (I1 - I0) and (want["first"] >= 0).sum() > 20
    assert want["first"][want["first"] >= 0].min() == I0 and want["last"].max() == I1 - 1
    dchan = torch.as_tensor(chan, device=DEV)
    for name, (view, tails, slots) in layout_device(launch(rows, tail, tf), SENTINEL).items():
        m = ArrivalMap(spec, DEV)
        m.add_rows(I0, I1, view, tails, slots, dchan)
        got = m.numpy()
        assert_same(got, want, name)
        if window_rows is not None:
            assert int(got["count"].sum()) == nbin, name
        m.add_rows(I0, I1, view, tails, slots, dchan)
        twice = m.numpy()
        assert np.array_equal(twice["first"], want["first"]) and np.array_equal(twice["last"], want["last"]), name
        if window_rows is not None:
            assert np.array_equal(twice["count"], 2 * want["count"]), name
        m2 = ArrivalMap(spec, DEV)
        mid = I0 + 3
        m2.add_rows(I0, mid, view[:, :mid - I0].contiguous(), tails, slots, dchan)
        m2.add_rows(mid, I1, view[:, mid - I0:].contiguous(), tails, slots, dchan)
        assert_same(m2.numpy(), want, name + " in two launches")


def test_contention_one_bin():
    """All 130 x 7 points in one bin, dense and all-tail: first 1, last 7, the
    counts per window exact and every other bin untouched."""
    spec = ArrivalSpec(1440, 720, nt=I1, window_rows=3)
    rows = np.zeros((NRAY, I1 - I0, 8))
    rows[..., 0], rows[..., 1], rows[..., 4] = 1.0, 0.1, 1.0
    b = int(bin_index(1.0, 0.1, 1.0, None, spec.bins))
    for tailed in (False, True):
        m = ArrivalMap(spec, DEV)
        tails = None
        if tailed:
            tails = Tails(NRAY, DEV)
            tails.frm.fill_(I0)
            tails.row.copy_(torch.as_tensor(rows[:, 0]))
        m.add_rows(I0, I1, torch.as_tensor(rows, device=DEV), tails)
        a = m.numpy()
        assert a["first"].reshape(-1)[b] == 1 and a["last"].reshape(-1)[b] == 7
        assert (a["first"] >= 0).sum() == 1 and (a["last"] >= 0).sum() == 1
        # rows 1..7 in windows of 3: rows 1 2 | 3 4 5 | 6 7
        assert a["count"].reshape(3, -1)[:, b].tolist() == [2 * NRAY, 3 * NRAY, 2 * NRAY]
        assert a["count"].sum() == 910 and np.count_nonzero(a["count"]) == 3


def test_add_points_is_row_zero_and_the_helpers(tmp_path):
    import ncio
    spec = ArrivalSpec(7, 5, nt=9, nchan=2, window_rows=4)
    pts = corner_points()
    lon, lat, w, chan = (np.array([p[k] for p in pts]) for k in range(4))
    m = ArrivalMap(spec, DEV)
    m.add_points(lon, lat, w, chan)
    want = reference_arrival(lon[:, None], lat[:, None], w[:, None], chan, spec)
    assert_same(m.numpy(), want, "row 0")
    assert want["count"].sum() == 15 and want["count"][1:].sum() == 0 and want["first"].max() == 0
    # one more point, row 6 (window 1), latitude row 3 (0.7 rad = 40 degrees: centre 36)
    row = torch.zeros((1, 1, 8), dtype=torch.float64, device=DEV)
    row[0, 0, 0], row[0, 0, 1] = 5.0, 0.7
    m.add_rows(6, 7, row)
    a = m.numpy()
    b = np.unravel_index(int(bin_index(5.0, 0.7, 0.0, 0, spec.bins)), spec.shape)
    assert a["first"][b] == 6 and a["last"][b] == 6 and a["count"][(1,) + b] == 1
    days = m.days(7200.0)
    assert days.dtype == np.float64 and days[b] == 0.5 and np.isnan(days[a["first"] < 0]).all()
    assert (days[(a["first"] == 0)] == 0.0).all()
    h = m.hovmoller(36.0, 90.0)                                # centres 36 and 72
    assert h.is_cuda and tuple(h.shape) == (3, 2, 7)
    assert np.array_equal(h.cpu().numpy(), a["count"][:, :, 3:].sum(axis=2))
    assert np.array_equal(m.hovmoller(-90.0, 90.0).cpu().numpy(), a["count"].sum(axis=2))
    assert len(m.lon_edges) == 8 and m.lat_edges[0] == -90.0 and m.lat_edges[-1] == 90.0
    for name in ("map.nc", "map.npz"):
        path = str(tmp_path / name)
        m.output(path)
        d = ncio.read(path)
        assert d["first"].dtype.kind == "i" and np.array_equal(d["first"], a["first"])
        assert np.array_equal(d["last"], a["last"])
        assert d["count"].shape == (3, 2, 5, 7) and np.array_equal(d["count"], a["count"])
        assert d["window_row"].tolist() == [0, 4, 8] and d["lat"][0] == -72.0
    with pytest.raises(ValueError):
        m.add_rows(9, 10, row)                                 # past spec.nt
    with pytest.raises(ValueError):
        ArrivalMap(ArrivalSpec(7, 5, nt=9), DEV).hovmoller(0.0, 10.0)


# ------------------------------------------------ C2 through the engine
C2_SPEC = ArrivalSpec(360, 180, nt=NT_C2, nchan=4, window_rows=12)
_WANT = {}


def c2_want(method="rk45"):
    """reference_arrival of the dense rows the density tests gathered with a
    plain sink (computed once), and their reference density map."""
    if method not in _WANT:
        pts, (count, _) = c2_ref(method)
        _WANT[method] = (reference_arrival(pts[..., 0], pts[..., 1], pts[..., 4], c2_chan(), C2_SPEC, row0=1), count)
    return _WANT[method]


def c2_arrival(spec=C2_SPEC, idx=None, rk4=False, tee=False, **kw):
    g = golden("init_C2_zonal.npz")
    eng = engine("zonal")
    y0 = torch.as_tensor(g["rows"][:5].reshape(5, -1))
    chan = torch.as_tensor(c2_chan())
    if idx is not None:
        y0 = y0[:, torch.as_tensor(idx)].contiguous()
    m = ArrivalMap(spec, eng.device)
    sink = ArrivalSink(m, chan)
    dm = None
    if tee:
        dm = DensityMap(DensitySpec(spec.nx, spec.ny, nchan=4, weight="amp"), eng.device)
        sink = Tee(DensitySink(dm, chan), sink)
    if idx is not None:
        sink = sink.take(idx)
    if rk4:
        eng.integrate_rk4(y0, NT_C2, 7200.0, sink=sink, **kw)
    else:
        eng.integrate(y0, NT_C2, 7200.0, ttotal=(NT_C2 - 1) * 7200.0, sink=sink, **kw)
    return (m, dm) if tee else m


@pytest.mark.parametrize("path", ["slots", "tails", "dense"])
def test_c2_chunking_and_row_layouts(path):
    """chunk = 120, chunk = 5 and short leading launches with the latency mode,
    on the row-block, the tails and the dense path: all equal
    reference_arrival of the dense rows."""
    want, _ = c2_want()
    assert want["count"].sum() > 100000 and (want["count"].sum(axis=(1, 2, 3)) > 0).all()
    assert want["first"].max() > 12 and C2_SPEC.nwin == 11
    eng = engine("zonal")
    try:
        if path == "tails":
            eng.use_slots = False
        if path == "dense":
            eng.use_tails = False
        for kw in (dict(chunk=120), dict(chunk=5), dict(first_chunk=[6, 24], team=[64, 64, 64])):
            assert_same(c2_arrival(**kw).numpy(), want, (path, kw))
    finally:
        for a in ("use_slots", "use_tails"):
            eng.__dict__.pop(a, None)


def test_c2_rk4():
    want, _ = c2_want("rk4")
    for kw in (dict(), dict(chunk=7)):
        assert_same(c2_arrival(rk4=True, **kw).numpy(), want, kw)


def test_c2_tee_with_a_density_sink():
    """One integration into Tee(DensitySink, ArrivalSink): the windows of
    count sum to the density map's counts (weight 'amp': the same points)."""
    want, dens_want = c2_want()
    m, dm = c2_arrival(tee=True, chunk=40)
    a = m.numpy()
    assert_same(a, want, "tee")
    dens = dm.numpy()[0]
    assert np.array_equal(dens, dens_want) and np.array_equal(a["count"].sum(axis=0), dens)


def combine(parts):
    first = np.stack([np.where(p["first"] < 0, np.iinfo(np.int32).max, p["first"]) for p in parts]).min(axis=0)
    return {"first": np.where(first == np.iinfo(np.int32).max, -1, first).astype(np.int32),
            "last": np.stack([p["last"] for p in parts]).max(axis=0), "count": sum(p["count"] for p in parts)}


def test_c2_shards_combine():
    """The two halves of shard_indices(world=2), run into two maps, combine to
    the whole-set map with min, max and sum; so do the two emulated ranks of
    run_sharded into one map (the sharded sink form, chan indexed by the shard)."""
    import shard
    want, _ = c2_want()
    g = golden("init_C2_zonal.npz")
    y0 = g["rows"][:5].reshape(5, -1)
    live = ~np.isnan(y0.mean(axis=0))
    parts = [c2_arrival(idx=shard.shard_indices(live, r, 2), chunk=50).numpy() for r in range(2)]
    assert parts[0]["count"].sum() > 0 and parts[1]["count"].sum() > 0
    assert_same(combine(parts), want, "two maps")
    eng = engine("zonal")
    m = ArrivalMap(C2_SPEC, eng.device)
    for r in range(2):
        shard.run_sharded(eng, torch.as_tensor(y0), NT_C2, 7200.0, rank=r, world=2,
                          ttotal=(NT_C2 - 1) * 7200.0, sink=ArrivalSink(m, c2_chan()), gather=False)
    assert_same(m.numpy(), want, "run_sharded")


# ------------------------------------------------------- WR.ray_arrival (C1)
def test_c1_ray_arrival_equals_the_reference_history():
    """C1, 90 days through WR.ray_arrival by root, 1440 x 720, one-day
    windows: equal to reference_arrival of the reference's own golden history
    (row 0 included); mode='numpy' the same; the history arrays keep row 0."""
    hist = golden("traj_C1.npz")["hist"]              # (7, 1081, 3)
    spec = ArrivalSpec(1440, 720, nt=1081, window_rows=12)
    want = reference_arrival(hist[0].T, hist[1].T, hist[4].T, np.arange(3), ArrivalSpec(
        1440, 720, nt=1081, nchan=3, window_rows=12))
    assert want["count"].sum(axis=(0, 2, 3)).tolist() == [0, 1081, 1081]
    assert (want["first"] >= 0).sum(axis=(1, 2)).tolist() == [0, 1077, 1075]
    wr = c1_wr()
    with np.errstate(all="ignore"):
        m = wr.ray_arrival(spec, by="root")
    assert m.spec.nchan == 3
    assert_same(m.numpy(), want, "hip")
    assert np.isnan(wr.rlon[1:]).all() and not np.isnan(wr.rlon[0]).any()
    with np.errstate(all="ignore"):
        assert_same(c1_wr().ray_arrival(spec, by="root", mode="numpy"), want, "numpy")
        no0 = c1_wr().ray_arrival(spec, by="root", include_initial=False).numpy()
        rk4 = c1_wr().ray_arrival(spec, by="root", inte_method="").numpy()
    visited = no0["first"] >= 0
    assert visited.sum() > 2000 and (no0["first"][visited] >= 1).all() and no0["count"].sum() == 2160
    per_root = rk4["count"].sum(axis=(0, 2, 3))
    assert per_root[0] == 0 and (per_root[1:] > 0).all() and (per_root <= 1081).all()
    with pytest.raises(ValueError):
        c1_wr().ray_arrival(ArrivalSpec(1440, 720, nt=1080))
    with pytest.raises(ValueError):
        c1_wr().ray_arrival(spec, by="source")


# ------------------------------------------------- time-varying background
@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32-storage"])
def test_time_varying_background(fp32):
    eng = tv_engine(fp32)
    cfg = S.config("C2")
    deg = math.pi / 180.0
    ix, iy = np.meshgrid(np.arange(cfg.nnx), np.arange(cfg.nny))
    slon = ((cfg.SW_lon % 360.0 + ix.ravel() * cfg.dlon) % 360.0) * deg
    slat = (cfg.SW_lat + iy.ravel() * cfg.dlat) * deg
    y0 = eng.initial_rows(slon, slat, cfg.zwn, cfg.freq)[:5].reshape(5, -1).contiguous()
    nt = 13
    got = {}
    eng.integrate(y0.clone(), nt, 7200.0, ttotal=(nt - 1) * 7200.0,
                  sink=lambda a, b, o: got.__setitem__(a, o.cpu().numpy().copy()))
    pts = np.concatenate([got[k] for k in sorted(got)], axis=1)
    spec = ArrivalSpec(1440, 720, nt=nt, window_rows=5)
    want = reference_arrival(pts[..., 0], pts[..., 1], pts[..., 4], None, spec, row0=1)
    assert want["count"].sum() > 1000 and want["last"].max() == nt - 1
    for kw in (dict(), dict(chunk=5)):
        m = ArrivalMap(spec, eng.device)
        eng.integrate(y0.clone(), nt, 7200.0, ttotal=(nt - 1) * 7200.0, sink=ArrivalSink(m), **kw)
        assert_same(m.numpy(), want, kw)


# ------------------------------------------------------------- allreduce
def _allreduce_body(dist, ops):
    rng = np.random.default_rng(0)
    m = ArrivalMap(ArrivalSpec(144, 72, nt=9, window_rows=4), "cuda:0")
    m.add_points(rng.uniform(0, 6.28, 5000), rng.uniform(-1.5, 1.5, 5000), rng.uniform(0, 2, 5000))
    before = m.numpy()
    m.allreduce(dist.group.WORLD)
    after = m.numpy()
    nops = len(ops)
    names = [next((n for n in ("MIN", "MAX", "SUM") if o == getattr(dist.ReduceOp, n)), "?") for o in ops]
    # WR.ray_arrival with a group, through the N-rank branches on one rank
    # (shard.COLLECTIVE_MIN_WORLD = 1, as tests/test_gpu_multirank.py does)
    import shard
    spec = ArrivalSpec(144, 72, nt=61, window_rows=12)
    with np.errstate(all="ignore"):
        alone = c2_wr().ray_arrival(spec, by="zwn").numpy()
        shard.COLLECTIVE_MIN_WORLD = 1
        grouped = c2_wr().ray_arrival(spec, by="zwn", group=dist.group.WORLD).numpy()
    return dist.get_backend(), names, before, after, alone, grouped, len(ops) - nops


def test_allreduce_one_rank_group_leaves_the_map_unchanged():
    backend, names, before, after, alone, grouped, nops_wr = one_rank(_allreduce_body)
    assert backend == "nccl" and names == ["MIN", "MAX", "SUM"]
    assert before["count"].sum() == 5000 and before["count"][1:].sum() == 0
    assert_same(after, before, "one rank")
    # the grouped drop-in: the same map as the run without a group, all-reduced
    assert alone["count"].shape == (6, 4, 72, 144) and alone["count"].sum() > 10000
    assert_same(grouped, alone, "grouped")
    assert nops_wr >= 3
