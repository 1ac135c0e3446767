"""Ray-density maps on the GPU (``rwrt_ray_density``, density.py): the counts
equal the NumPy definition ``density.reference_bins`` exactly -- for crafted
rows in every row layout (dense, tails, row blocks), under contention, through
``RayEngine.integrate`` / ``integrate_rk4`` in any chunking and row layout,
through ``WR.ray_density`` on the reference's C1 history, on a time-varying
background and across shards; the weighted sums within the rounding bound of
a sum taken in any order."""
import math

import numpy as np
import pytest
import torch

import synthetic as S
from conftest import golden
from density import DensityMap, DensitySink, DensitySpec, bin_index, reference_bins
from engine import Tails
from support.cases import C2_SPEC, NT_C2, c1_wr, c2_chan, c2_ref, c2_wr, engine, tv_engine
from support.cases_density import BOUNDARY_TF, I0, I1, NRAY, corner_points, crafted, launch
from support.dist import one_rank
from support.rows import SENTINEL, layout_device

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------- crafted rows, entry point
@pytest.mark.parametrize("spec,with_chan", [
    (DensitySpec(7, 5), False), (DensitySpec(7, 5, nchan=3, weight="amp"), True),
    (DensitySpec(1440, 720, weight="amp"), True), (DensitySpec(1440, 720, nchan=3), True)],
    ids=["7x5", "7x5x3-amp", "1440x720-amp", "1440x720x3"])
def test_crafted_rows_every_layout(spec, with_chan):
    every_layout_equals_reference_bins(spec, with_chan, *crafted())


@pytest.mark.parametrize("spec,with_chan", [(DensitySpec(7, 5, nchan=3, weight="amp"), True)], ids=["7x5x3-amp"])
def test_crafted_rows_tail_from_clamp_and_batch_boundary(spec, with_chan):
    """``tail_from`` from BOUNDARY_TF, unclamped, in every layout: 0, 1, 3, 4, 5
    and 7 rows read (the rays without a row block: at most I0)."""
    j = np.arange(NRAY)
    tf = np.where(j % 3 == 0, np.array(BOUNDARY_TF[:2])[(j // 3) % 2], np.array(BOUNDARY_TF)[j % 8])
    assert all(set(tf[j % 3 == r].tolist()) == set(BOUNDARY_TF) for r in (1, 2))
    assert sorted(set((np.clip(tf, I0, I1) - I0).tolist())) == [0, 1, 3, 4, 5, 7]
    every_layout_equals_reference_bins(spec, with_chan, *crafted(seed=4, tf=tf))


def every_layout_equals_reference_bins(spec, with_chan, rows, tail, tf):
    rng = np.random.default_rng(7)
    chan = rng.integers(-1, spec.nchan + 1, NRAY).astype(np.int32) if with_chan else None
    cref = None if chan is None else chan[:, None]
    want, wwant = reference_bins(rows[..., 0], rows[..., 1], rows[..., 4], cref, spec)
    nbin = int((bin_index(rows[..., 0], rows[..., 1], rows[..., 4], cref, spec) >= 0).sum())
    assert 0 < nbin < NRAY * (I1 - I0)
    abs_sum = None
    if spec.wcol >= 0:
        abs_sum = reference_bins(rows[..., 0], rows[..., 1], np.abs(rows[..., 4]), cref, spec)[1]
    for name, (view, tails, slots) in layout_device(launch(rows, tail, tf), SENTINEL).items():
        m = DensityMap(spec, DEV)
        m.add_rows(I0, I1, view, tails, slots, None if chan is None else torch.as_tensor(chan, device=DEV))
        count, wsum = m.numpy()
        assert np.array_equal(count, want), name
        assert int(count.sum()) == nbin, name
        if spec.wcol >= 0:
            bound = 2.0 * (want + 1) * 2.0 ** -53 * abs_sum
            assert np.all(np.abs(wsum - wwant) <= bound), name
        # accumulation: a second call doubles every count
        m.add_rows(I0, I1, view, tails, slots, None if chan is None else torch.as_tensor(chan, device=DEV))
        assert np.array_equal(m.numpy()[0], 2 * want), name


def test_contention_one_bin():
    """All 130 x 7 points in one bin: exactly 910 there and nowhere else; the
    sum of 910 ones is exact in any order."""
    spec = DensitySpec(1440, 720, weight="amp")
    rows = np.zeros((NRAY, I1 - I0, 8))
    rows[..., 0], rows[..., 1], rows[..., 4] = 1.0, 0.1, 1.0
    b = int(bin_index(1.0, 0.1, 1.0, None, spec))
    for tailed in (False, True):
        m = DensityMap(spec, DEV)
        tails = None
        if tailed:    # every ray's rows are its tail: one atomic of 7 per ray
            tails = Tails(NRAY, DEV)
            tails.frm.fill_(I0)
            tails.row.copy_(torch.as_tensor(rows[:, 0]))
        m.add_rows(I0, I1, torch.as_tensor(rows, device=DEV), tails)
        count, wsum = m.numpy()
        assert count.reshape(-1)[b] == 910 and count.sum() == 910
        assert wsum.reshape(-1)[b] == 910.0 and np.count_nonzero(wsum) == 1


def test_add_points_is_row_zero():
    spec = DensitySpec(7, 5, nchan=2, weight="amp")
    pts = corner_points()
    lon, lat, w, chan = (np.array([p[k] for p in pts]) for k in range(4))
    m = DensityMap(spec, DEV)
    m.add_points(lon, lat, w, chan)
    want, wwant = reference_bins(lon, lat, w, chan.astype(np.int64), spec)
    count, wsum = m.numpy()
    assert np.array_equal(count, want) and count.sum() == 15
    assert np.array_equal(wsum, wwant)        # (one point per atomic, at most two per bin: exact)
    assert len(m.lon_edges) == 8 and m.lat_edges[0] == -90.0 and m.lat_edges[-1] == 90.0


# ------------------------------------------------ C2 through the engine
def c2_density(spec=C2_SPEC, idx=None, rk4=False, **kw):
    g = golden("init_C2_zonal.npz")
    eng = engine("zonal")
    y0 = torch.as_tensor(g["rows"][:5].reshape(5, -1))
    chan = torch.as_tensor(c2_chan()) if spec.nchan == 4 else None
    if idx is not None:
        y0 = y0[:, torch.as_tensor(idx)].contiguous()
    m = DensityMap(spec, eng.device)
    sink = DensitySink(m, chan)
    if idx is not None:
        sink = sink.take(idx)
    if rk4:
        eng.integrate_rk4(y0, NT_C2, 7200.0, sink=sink, **kw)
    else:
        eng.integrate(y0, NT_C2, 7200.0, ttotal=(NT_C2 - 1) * 7200.0, sink=sink, **kw)
    return m


@pytest.mark.parametrize("path", ["slots", "tails", "dense"])
def test_c2_chunking_and_row_layouts(path):
    """chunk = 120, chunk = 5 and short leading launches with the latency mode
    give identical counts, on the row-block, the tails and the dense path, all
    equal to reference_bins of the dense rows."""
    _, (want, _) = c2_ref()
    assert want.sum() > 100000
    eng = engine("zonal")
    try:
        if path == "tails":
            eng.use_slots = False
        if path == "dense":
            eng.use_tails = False
        for kw in (dict(chunk=120), dict(chunk=5), dict(first_chunk=[6, 24], team=[64, 64, 64])):
            count = c2_density(**kw).numpy()[0]
            assert np.array_equal(count, want), (path, kw)
            if path == "slots":
                assert eng.rows_bytes < 3072 * min(kw.get("chunk", 120), 120) * 64   # (row blocks were used)
    finally:
        for a in ("use_slots", "use_tails"):
            eng.__dict__.pop(a, None)


def test_c2_rk4():
    _, (want, _) = c2_ref("rk4")
    for kw in (dict(), dict(chunk=7)):
        assert np.array_equal(c2_density(rk4=True, **kw).numpy()[0], want), kw


@pytest.mark.parametrize("nx,ny", [(1440, 720), (7, 5)])
def test_c2_weighted_sum_within_the_rounding_bound(nx, ny):
    """Per bin |wsum_gpu - wsum_ref| <= 2 (n + 1) 2^-53 sum|w|: the bound of a
    sum of n terms in any order, twice (both sides are rounded sums), plus one
    rounding for a tail added as a product."""
    pts, _ = c2_ref()
    spec = DensitySpec(nx, ny, weight="amp")
    lon, lat, w = pts[..., 0], pts[..., 1], pts[..., 4]
    want, wwant = reference_bins(lon, lat, w, None, spec)
    abs_sum = reference_bins(lon, lat, np.abs(w), None, spec)[1]
    m = c2_density(spec, chunk=40)
    count, wsum = m.numpy()
    assert np.array_equal(count, want)
    err, bound = np.abs(wsum - wwant), 2.0 * (want + 1) * 2.0 ** -53 * abs_sum
    print(f"wsum {nx}x{ny}: max err {err.max():.3g}, max err/bound {np.max(err[bound > 0] / bound[bound > 0]):.3g}")
    assert np.all(err <= bound)
    # a point with a non-finite weight is in neither array
    unweighted = reference_bins(lon, lat, None, None, DensitySpec(nx, ny))[0]
    n_bad_w = int((np.isfinite(lon) & np.isfinite(lat) & ~np.isfinite(w)).sum())
    assert unweighted.sum() - count.sum() == n_bad_w
    assert np.all(np.isfinite(wsum))


def test_c2_additivity_over_shards():
    """The two halves of shard_indices(world=2), run one after the other into
    two maps, sum to the whole-set map exactly; so do the two emulated ranks
    of run_sharded (the sharded sink form, chan indexed by the shard)."""
    import shard
    _, (want, _) = c2_ref()
    g = golden("init_C2_zonal.npz")
    y0 = g["rows"][:5].reshape(5, -1)
    live = ~np.isnan(y0.mean(axis=0))
    parts = [c2_density(idx=shard.shard_indices(live, r, 2), chunk=50).numpy()[0] for r in range(2)]
    assert parts[0].sum() > 0 and parts[1].sum() > 0
    assert np.array_equal(parts[0] + parts[1], want)
    eng = engine("zonal")
    m = DensityMap(C2_SPEC, eng.device)
    for r in range(2):
        shard.run_sharded(eng, torch.as_tensor(y0), NT_C2, 7200.0, rank=r, world=2,
                          ttotal=(NT_C2 - 1) * 7200.0, sink=DensitySink(m, c2_chan()), gather=False)
    assert np.array_equal(m.numpy()[0], want)


# ------------------------------------------------------- WR.ray_density (C1)
def test_c1_ray_density_equals_the_reference_history():
    """C1, 90 days through WR.ray_density: the counts equal reference_bins of
    the reference's own golden history (rows 1..1080) plus row 0; by root,
    each map holds that root's 1 081 points; the history arrays keep row 0."""
    hist = golden("traj_C1.npz")["hist"]              # (7, 1081, 3)
    spec = DensitySpec(1440, 720)
    want = reference_bins(hist[0], hist[1], None, None, spec)[0]
    assert want.sum() == 3243
    wr = c1_wr()
    with np.errstate(all="ignore"):
        m = wr.ray_density(spec)
    assert np.array_equal(m.numpy()[0], want)
    assert np.isnan(wr.rlon[1:]).all() and not np.isnan(wr.rlon[0]).any()
    with np.errstate(all="ignore"):      # mode='numpy': the delivered history through reference_bins
        host_count, host_wsum = c1_wr().ray_density(spec, mode="numpy")
    assert host_wsum is None and np.array_equal(host_count, want)
    wr = c1_wr()
    with np.errstate(all="ignore"):
        m3 = wr.ray_density(DensitySpec(144, 72), by="root")
    count = m3.numpy()[0]
    assert count.shape == (3, 72, 144) and count.sum(axis=(1, 2)).tolist() == [1081, 1081, 1081]
    assert np.array_equal(count, reference_bins(hist[0], hist[1], None, np.arange(3)[None, :],
                                                DensitySpec(144, 72, nchan=3))[0])
    # weighted by the amplitude: root 0 is a dead root slot here (a position, but
    # a NaN amplitude on every row), so its points are in neither array
    with np.errstate(all="ignore"):
        count, wsum = c1_wr().ray_density(DensitySpec(144, 72, weight="amp"), by="root").numpy()
    assert count.sum(axis=(1, 2)).tolist() == [0, 1081, 1081] and not wsum[0].any()
    want3, w3 = reference_bins(hist[0], hist[1], hist[4], np.arange(3)[None, :],
                               DensitySpec(144, 72, nchan=3, weight="amp"))
    assert np.array_equal(count, want3)
    a3 = reference_bins(hist[0], hist[1], np.abs(hist[4]), np.arange(3)[None, :],
                        DensitySpec(144, 72, nchan=3, weight="amp"))[1]
    assert np.all(np.abs(wsum - w3) <= 2.0 * (want3 + 1) * 2.0 ** -53 * a3)
    with np.errstate(all="ignore"):
        no0 = c1_wr().ray_density(spec, include_initial=False, inte_method="")     # RK4, rows 1.. only
    assert 0 < no0.count.sum().item() <= 3240


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
    spec = DensitySpec(1440, 720, weight="amp")
    want, wwant = reference_bins(pts[..., 0], pts[..., 1], pts[..., 4], None, spec)
    assert want.sum() > 1000
    for kw in (dict(), dict(chunk=5)):
        m = DensityMap(spec, eng.device)
        eng.integrate(y0.clone(), nt, 7200.0, ttotal=(nt - 1) * 7200.0, sink=DensitySink(m), **kw)
        assert np.array_equal(m.numpy()[0], want), kw


# ------------------------------------------------------------- allreduce
def _allreduce_body(dist, calls):
    rng = np.random.default_rng(0)
    m = DensityMap(DensitySpec(144, 72, weight="amp"), "cuda:0")
    m.add_points(rng.uniform(0, 6.28, 5000), rng.uniform(-1.5, 1.5, 5000), rng.uniform(0, 2, 5000))
    before = m.numpy()
    m.allreduce(dist.group.WORLD)
    after = m.numpy()
    ncalls = len(calls)
    # WR.ray_density with a group, through the N-rank branches on one rank
    # (shard.COLLECTIVE_MIN_WORLD = 1, as tests/test_gpu_multirank.py does):
    # the shard's sink, then the all-reduce of the map
    import shard
    spec = DensitySpec(144, 72, weight="amp")
    with np.errstate(all="ignore"):
        alone = c2_wr().ray_density(spec, by="zwn").numpy()
        shard.COLLECTIVE_MIN_WORLD = 1
        grouped = c2_wr().ray_density(spec, by="zwn", group=dist.group.WORLD).numpy()
    return dist.get_backend(), ncalls, before, after, alone, grouped, len(calls) - ncalls


def test_allreduce_one_rank_group_leaves_the_map_unchanged():
    backend, ncalls, before, after, alone, grouped, ncalls_wr = one_rank(_allreduce_body)
    assert backend == "nccl" and ncalls == 2
    assert before[0].sum() == 5000
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # the grouped drop-in: same counts as the run without a group, the map all-reduced
    assert alone[0].shape == (4, 72, 144) and alone[0].sum() > 10000
    assert np.array_equal(alone[0], grouped[0]) and ncalls_wr >= 2
    assert np.allclose(alone[1], grouped[1], rtol=1e-12, atol=0.0)


def test_output_file(tmp_path):
    import ncio
    m = DensityMap(DensitySpec(8, 4, nchan=2, weight="amp"), DEV)
    m.add_points([0.1, 3.0], [0.0, 1.0], [2.0, 3.0], [0, 1])
    for name in ("map.nc", "map.npz"):
        path = str(tmp_path / name)
        m.output(path)
        d = ncio.read(path)
        assert d["count"].shape == (2, 4, 8) and d["count"].sum() == 2 and d["wsum"].sum() == 5.0
        assert d["lon"].shape == (8,) and d["lat"][0] == -67.5
