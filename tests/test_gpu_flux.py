"""Wave-ray flux maps on the GPU (``rwrt_ray_flux``, flux.py): ``count`` and
``rowsum`` equal the NumPy definition ``flux.reference_flux`` exactly and the
three sums agree within the rounding bound of a sum taken in any order -- for
crafted rows in every row layout (dense, tails, row blocks), under contention,
through ``RayEngine.integrate`` / ``integrate_rk4`` in any chunking and row
layout, next to a ``DensitySink`` in one ``Tee``, across shards, through
``WR.ray_flux`` on the reference's C1 history with and without a target
region, and on a time-varying background."""
import math

import numpy as np
import pytest
import torch

import flux as F
import synthetic as S
from conftest import golden
from density import DensityMap, DensitySink, DensitySpec
from engine import Tails
from flux import FluxMap, FluxSink, FluxSpec, reference_flux
from summary import RaySummary, Tee, reference_summary
from support.cases import NT_C2, c1_wr, c2_chan, c2_ref, c2_wr, engine, tv_engine
from support.cases_flux import VARIANTS, abs_sums, assert_flux, columns, crafted_launch, reference_of, sum_bound
from support.dist import one_rank
from support.rows import layout_device

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = {0: 1.0, 1: 0.1}   # lon lat of a row that must never be read: at rest, binnable, counted if it were


def scaled(m, factor):
    return {k: v * factor for k, v in m.items()}


@pytest.mark.parametrize("nray", [41, 130], ids=["41-rays", "130-rays"])
@pytest.mark.parametrize("shape", [(7, 5, 3), (64, 32, 1)], ids=["7x5x3", "64x32x1"])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_crafted_rows_every_layout(name, shape, nray):
    """The launch [1, 8) of the host tests (41 rays, and 130: three waves, the
    last partial), every layout: count and rowsum equal reference_flux, the
    sums agree to the bound; a second identical call doubles everything;
    launches [1, 4) and [4, 8) give what one launch [1, 8) gives."""
    nx, ny, nchan = shape
    spec = FluxSpec(nx, ny, nchan=nchan, **VARIANTS[name])
    L = crafted_launch(1, 8, seed=3, nray=nray)
    if nchan == 1:                                     # channels 0..2 are the one map; -1 and 3 stay outside
        L["chan"] = np.where((L["chan"] >= 0) & (L["chan"] < 3), 0, L["chan"]).astype(np.int32)
    assert {-1, 1, 8, 11} <= set(L["tf"].tolist()) and {-1, 3} <= set(L["chan"].tolist())
    want, a = reference_of([L], spec)
    assert 20 < want["count"].sum() < nray * 7
    chan = torch.as_tensor(L["chan"], device=DEV)
    for layout, (view, tails, slots) in layout_device(L, SENTINEL).items():
        m = FluxMap(spec, DEV)
        m.add_rows(1, 8, view, tails, slots, chan)
        assert_flux(m.numpy(), want, a, (name, layout))
        m.add_rows(1, 8, view, tails, slots, chan)
        assert_flux(m.numpy(), scaled(want, 2), 2 * a, (name, layout, "twice"))
        m2 = FluxMap(spec, DEV)
        m2.add_rows(1, 4, view[:, :3].contiguous(), tails, slots, chan)
        m2.add_rows(4, 8, view[:, 3:].contiguous(), tails, slots, chan)
        assert_flux(m2.numpy(), want, a, (name, layout, "in two launches"))


def test_contention_one_bin():
    """4 160 rays x 7 rows all in one bin, dense and all-tail: count and rowsum
    exact there and every other bin untouched; the velocity sums too (ug = 3,
    vg = -4, speed 5: small integers, exact in any order); the unit vectors
    (0.6, -0.8) within the bound."""
    nray, i0, i1 = 4160, 1, 8
    rows = np.zeros((nray, i1 - i0, 8))
    rows[..., 0], rows[..., 1], rows[..., 5], rows[..., 6] = 1.0, 0.1, 3.0, -4.0
    n = nray * (i1 - i0)
    for spec in (FluxSpec(1440, 720), FluxSpec(4320, 720, lon_range=(-360.0, 720.0)), FluxSpec(7, 5, vector="unit")):
        b = int(F.accept(1.0, 0.1, 0.0, 0.0, 3.0, -4.0, None, spec)[0])
        assert b >= 0
        want = reference_flux(*columns(rows), None, spec, row0=i0)
        a = abs_sums(*columns(rows), None, spec)
        for tailed in (False, True):
            m = FluxMap(spec, DEV)
            tails = None
            if tailed:    # every ray's rows are its tail: one run of 7 per ray
                tails = Tails(nray, DEV)
                tails.frm.fill_(i0)
                tails.row.copy_(torch.as_tensor(rows[:, 0]))
            m.add_rows(i0, i1, torch.as_tensor(rows, device=DEV), tails)
            got = m.numpy()
            assert got["count"].reshape(-1)[b] == n and got["count"].sum() == n
            assert got["rowsum"].reshape(-1)[b] == nray * 28 and got["rowsum"].sum() == nray * 28
            assert np.count_nonzero(got["sum"]) == 3
            assert_flux(got, want, a, (spec, tailed))
            if not spec.unit:
                assert got["sum"].reshape(-1, 3)[b].tolist() == [3.0 * n, -4.0 * n, 5.0 * n]


def test_add_points_derived_fields_fold_and_output(tmp_path):
    """``add_points`` is row 0; the derived fields are NaN exactly where count
    is 0; ``fold`` sums three circles onto one; ``output`` round-trips."""
    import ncio
    spec = FluxSpec(6, 4, nchan=2, lon_range=(-360.0, 720.0))
    lon = np.array([0.5, 0.5 - 2 * math.pi, 0.5 + 2 * math.pi, 3.0, 3.0, 1.0, 13.0, math.nan])
    lat = np.array([0.1, 0.1, 0.1, -1.0, -1.0, 0.1, 0.1, 0.1])
    ug = np.array([3.0, 3.0, -3.0, 0.0, 6.0, 1.0, 1.0, 1.0])
    vg = np.array([4.0, -4.0, 4.0, 2.0, 8.0, 1.0, 1.0, 1.0])
    k = np.zeros(8)
    chan = np.array([0, 0, 0, 1, 1, 2, 0, 0])          # a channel outside, a point outside the window, a NaN
    m = FluxMap(spec, DEV)
    m.add_points(lon, lat, k, k, ug, vg, chan)
    want = reference_flux(lon[:, None], lat[:, None], k[:, None], k[:, None], ug[:, None], vg[:, None], chan, spec)
    assert_flux(m.numpy(), want, None, "row 0")        # (at most two points per bin: exact)
    assert want["count"].sum() == 5 and want["rowsum"].sum() == 0
    m.add_rows(6, 7, torch.as_tensor(np.array([[[3.0, -1.0, 0, 0, 0, 0.0, -2.0, 0]]]), device=DEV),
               chan=torch.as_tensor([1], device=DEV))
    a = m.numpy()
    count = a["count"]
    b = np.unravel_index(int(F.accept(3.0, -1.0, 0, 0, 0.0, 2.0, 1, spec)[0]), spec.shape)
    assert count[b] == 3 and a["rowsum"][b] == 6 and a["sum"][b].tolist() == [6.0, 8.0, 2.0 + 10.0 + 2.0]
    fields = {"magnitude": m.magnitude(), "direction": m.direction(), "coherence": m.coherence(),
              "mean_speed": m.mean_speed(), "mean_days": m.mean_days(7200.0)}
    for name, f in fields.items():
        assert f.is_cuda and f.dtype == torch.float64 and tuple(f.shape) == spec.shape, name
        assert np.array_equal(np.isnan(f.cpu().numpy()), count == 0), name
    f = {name: v.cpu().numpy() for name, v in fields.items()}
    close = lambda x, y: abs(x - y) <= 1e-13 * abs(y)           # noqa: E731  (the device's hypot, atan2)
    assert close(f["magnitude"][b], 10.0) and f["mean_speed"][b] == 14.0 / 3.0
    assert f["mean_days"][b] == 2.0 * 7200.0 / 86400.0
    assert close(f["direction"][b], math.degrees(math.atan2(8.0, 6.0))) and close(f["coherence"][b], 10.0 / 14.0)
    east = np.unravel_index(int(F.accept(0.5, 0.1, 0, 0, 3.0, 4.0, 0, spec)[0]), spec.shape)
    assert close(f["direction"][east], math.degrees(math.atan2(4.0, 3.0))) and close(f["coherence"][east], 1.0)
    assert m.lon_edges.tolist() == [-360.0, -180.0, 0.0, 180.0, 360.0, 540.0, 720.0]
    assert m.lat_edges[0] == -90.0 and m.lat_edges[-1] == 90.0 and len(m.lat_edges) == 5
    # fold: the three points at 0.5 (+- one circle) meet in one bin of [0, 360)
    w = m.fold()
    assert w.spec == FluxSpec(2, 4, nchan=2) and w.lon_edges.tolist() == [0.0, 180.0, 360.0]
    wa = w.numpy()
    assert wa["count"].sum() == 6 and wa["count"][0, 2, 0] == 3 and wa["sum"][0, 2, 0].tolist() == [3.0, 4.0, 15.0]
    assert np.array_equal(wa["count"], count.reshape(2, 4, 3, 2).sum(axis=2))
    unit = FluxMap(FluxSpec(2, 4, vector="unit"), DEV)
    unit.add_points(lon[:3], lat[:3], k[:3], k[:3], ug[:3], vg[:3])
    assert abs(float(unit.coherence()[0, 2, 0].item()) - math.hypot(0.6, 0.8) / 3.0) < 1e-14
    with pytest.raises(ValueError):
        FluxMap(FluxSpec(7, 4, lon_range=(-360.0, 720.0)), DEV).fold()
    with pytest.raises(ValueError):
        w.fold()
    for name in ("map.nc", "map.npz"):
        path = str(tmp_path / name)
        m.output(path)
        d = ncio.read(path)
        assert d["count"].shape == (2, 4, 6) and np.array_equal(d["count"], count)
        assert np.array_equal(d["rowsum"], a["rowsum"])
        if name.endswith(".npz"):
            assert d["count"].dtype.kind == "i" and d["rowsum"].dtype.kind == "i"
        for q, v in enumerate(("fx", "fy", "fs")):
            assert np.array_equal(d[v], a["sum"][..., q])
        assert d["lon"].tolist() == [-270.0, -90.0, 90.0, 270.0, 450.0, 630.0] and d["lat"][0] == -67.5
        assert np.array_equal(d["lon_edges"], m.lon_edges)


def test_select_through():
    fields = reference_summary(np.full((5, 3, 8), np.nan), [(0, 10, 0, 10), (20, 30, 0, 10)])
    fields["first_row"] = np.array([[-1, 0, 4, -1, 7], [-1, -1, 2, 5, 0]], np.int32)
    rs = RaySummary.from_fields(fields, 3, [(0, 10, 0, 10), (20, 30, 0, 10)], DEV)
    any_, all_ = F.select_through(rs), F.select_through(rs, "all")
    assert any_.is_cuda and any_.dtype == torch.bool
    assert any_.tolist() == [False, True, True, True, True] and all_.tolist() == [False, False, True, False, True]
    with pytest.raises(ValueError):
        F.select_through(rs, "most")
    with pytest.raises(ValueError):
        F.select_through(RaySummary(5, (), DEV))


# ------------------------------------------------ C2 through the engine
C2_SPEC = FluxSpec(360, 180, nchan=4)
C2_WINDOW = FluxSpec(1080, 180, nchan=4, lon_range=(-360.0, 720.0), vector="unit", speed_range=(2.0, 60.0), wn_max=8.0)
_WANT = {}


def c2_want(method="rk45", spec=C2_SPEC):
    """reference_flux of the dense rows the density tests gathered with a
    plain sink (rows 1..), their sum|v|, and their reference density map --
    computed once."""
    key = (method, spec)
    if key not in _WANT:
        pts, (count, _) = c2_ref(method)
        _WANT[key] = (reference_flux(*columns(pts), c2_chan(), spec, row0=1),
                      abs_sums(*columns(pts), c2_chan(), spec), count)
    return _WANT[key]


def c2_flux(spec=C2_SPEC, idx=None, rk4=False, tee=False, **kw):
    g = golden("init_C2_zonal.npz")
    eng = engine("zonal")
    y0 = torch.as_tensor(g["rows"][:5].reshape(5, -1))
    chan = torch.as_tensor(c2_chan())
    if idx is not None:
        y0 = y0[:, torch.as_tensor(idx)].contiguous()
    m = FluxMap(spec, eng.device)
    sink = FluxSink(m, chan)
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
    on the row-block, the tails and the dense path: all equal reference_flux of
    the dense rows (count and rowsum exactly, the sums to the bound); the
    filtered unit-vector map on three circles too."""
    want, a, _ = c2_want()
    assert want["count"].sum() > 100000 and (want["count"].sum(axis=(1, 2)) > 0).all()
    wwant, wa, _ = c2_want(spec=C2_WINDOW)
    assert 10000 < wwant["count"].sum() < want["count"].sum()
    eng = engine("zonal")
    try:
        if path == "tails":
            eng.use_slots = False
        if path == "dense":
            eng.use_tails = False
        for kw in (dict(chunk=120), dict(chunk=5), dict(first_chunk=[6, 24], team=[64, 64, 64])):
            assert_flux(c2_flux(**kw).numpy(), want, a, (path, kw))
        assert_flux(c2_flux(C2_WINDOW, chunk=50).numpy(), wwant, wa, (path, "window"))
    finally:
        for name in ("use_slots", "use_tails"):
            eng.__dict__.pop(name, None)


def test_c2_rk4():
    want, a, _ = c2_want("rk4")
    assert_flux(c2_flux(rk4=True, chunk=7).numpy(), want, a, "rk4")


def test_c2_tee_with_a_density_sink():
    """One integration into Tee(DensitySink, FluxSink): the flux map as alone,
    the density map unchanged.  (The density map sums amp, the flux map needs
    ug and vg: a point counts in both when all three are finite.)"""
    want, a, dens_want = c2_want()
    m, dm = c2_flux(tee=True, chunk=40)
    got = m.numpy()
    assert_flux(got, want, a, "tee")
    assert np.array_equal(dm.numpy()[0], dens_want)
    err = np.abs(got["sum"] - want["sum"])
    b = sum_bound(want["count"], a)
    print(f"C2 sums: max err {err.max():.3g}, max err/bound {np.max(err[b > 0] / b[b > 0]):.3g}")


def test_c2_shards_combine():
    """The two halves of shard_indices(world=2), run into two maps through
    take(idx), sum to the whole-set map; so do the two emulated ranks of
    run_sharded into one map (the sharded sink form, chan indexed by the shard)."""
    import shard
    want, a, _ = c2_want()
    g = golden("init_C2_zonal.npz")
    y0 = g["rows"][:5].reshape(5, -1)
    live = ~np.isnan(y0.mean(axis=0))
    parts = [c2_flux(idx=shard.shard_indices(live, r, 2), chunk=50).numpy() for r in range(2)]
    assert parts[0]["count"].sum() > 0 and parts[1]["count"].sum() > 0
    assert_flux({k: parts[0][k] + parts[1][k] for k in parts[0]}, want, a, "two maps")
    eng = engine("zonal")
    m = FluxMap(C2_SPEC, eng.device)
    for r in range(2):
        shard.run_sharded(eng, torch.as_tensor(y0), NT_C2, 7200.0, rank=r, world=2,
                          ttotal=(NT_C2 - 1) * 7200.0, sink=FluxSink(m, c2_chan()), gather=False)
    assert_flux(m.numpy(), want, a, "run_sharded")


# ------------------------------------------------------------ WR.ray_flux (C1)
C1_BOX = (280.0, 284.0, 30.0, 32.0)    # chosen from traj_C1.npz: root 1 enters it at row 203, root 2 never does


def c1_reference(spec, chan, first=0):
    hist = golden("traj_C1.npz")["hist"]              # (7, 1081, 3): lon lat k l amp ug vg
    cols = [hist[c].T[:, first:] for c in (0, 1, 2, 3, 5, 6)]
    return reference_flux(*cols, chan, spec, row0=first), abs_sums(*cols, chan, spec)


def test_c1_ray_flux_equals_the_reference_history():
    """C1, 90 days through WR.ray_flux by root: equal to reference_flux of the
    reference's own golden history (row 0 included), wrapped and on three
    circles; mode='numpy' the same; include_initial=False removes exactly
    row 0; the history arrays keep row 0."""
    spec = FluxSpec(1440, 720)
    want, a = c1_reference(FluxSpec(1440, 720, nchan=3), np.arange(3))
    assert want["count"].sum(axis=(1, 2)).tolist() == [0, 1081, 1081]
    wr = c1_wr()
    with np.errstate(all="ignore"):
        m = wr.ray_flux(spec, by="root")
    assert m.spec.nchan == 3 and m.selected is None
    assert_flux(m.numpy(), want, a, "hip")
    assert np.isnan(wr.rlon[1:]).all() and not np.isnan(wr.rlon[0]).any()
    days = m.mean_days(7200.0).cpu().numpy()
    assert np.nanmax(days) <= 90.0 and np.nanmin(days) >= 0.0
    with np.errstate(all="ignore"):
        host = c1_wr().ray_flux(spec, by="root", mode="numpy")
        no0 = c1_wr().ray_flux(spec, by="root", include_initial=False).numpy()
    assert host["selected"] is None
    assert_flux(host, want, a, "numpy")
    want1, a1 = c1_reference(FluxSpec(1440, 720, nchan=3), np.arange(3), first=1)
    assert_flux(no0, want1, a1, "without row 0")
    assert (want["count"] - no0["count"]).sum() == 2 and (want["rowsum"] == no0["rowsum"]).all()
    wspec = FluxSpec(4320, 720, lon_range=(-360.0, 720.0), vector="unit")
    wwant, wa = c1_reference(FluxSpec(4320, 720, nchan=3, lon_range=(-360.0, 720.0), vector="unit"), np.arange(3))
    assert wwant["count"].sum(axis=(1, 2)).tolist() == [0, 230, 229]
    with np.errstate(all="ignore"):
        assert_flux(c1_wr().ray_flux(wspec, by="root").numpy(), wwant, wa, "three circles")
    with pytest.raises(ValueError):
        c1_wr().ray_flux(spec, by="source")
    with pytest.raises(ValueError):
        c1_wr().ray_flux(spec, through=[C1_BOX], through_mode="most")


def test_c1_ray_flux_through_a_region():
    """``through=[box]``: exactly one of the two live roots passes through the
    box, and only its points are in the map -- in 'hip' mode (two
    integrations: the summary, then the flux) and in 'numpy' mode."""
    hist = golden("traj_C1.npz")["hist"]
    rows = np.full((3, 1081, 8), np.nan)
    for c in range(7):
        rows[:, :, c] = hist[c].T
    s = reference_summary(rows, [C1_BOX])
    selected = s["first_row"][0] >= 0
    assert selected.sum() == 1 and selected.tolist() == [False, True, False] and s["first_row"][0, 1] == 203
    spec = FluxSpec(1440, 720)
    want, a = c1_reference(FluxSpec(1440, 720, nchan=3), np.where(selected, np.arange(3), -1))
    assert want["count"].sum(axis=(1, 2)).tolist() == [0, 1081, 0]
    with np.errstate(all="ignore"):
        m = c1_wr().ray_flux(spec, by="root", through=[C1_BOX])
        host = c1_wr().ray_flux(spec, by="root", through=[C1_BOX], mode="numpy")
        one = c1_wr().ray_flux(spec, through=[C1_BOX, (0.0, 1.0, -80.0, -79.0)], through_mode="all")
    assert m.selected.shape == (3, 1, 1) and m.selected.dtype == np.bool_
    assert m.selected.reshape(-1).tolist() == selected.tolist()
    assert_flux(m.numpy(), want, a, "hip")
    assert host["selected"].reshape(-1).tolist() == selected.tolist()
    assert_flux(host, want, a, "numpy")
    assert not one.selected.any() and one.numpy()["count"].sum() == 0          # nobody passes through both


# ------------------------------------------------- time-varying background
def test_time_varying_background():
    eng = tv_engine(False)
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
    spec = FluxSpec(1440, 720)
    want = reference_flux(*columns(pts), None, spec, row0=1)
    a = abs_sums(*columns(pts), None, spec)
    assert want["count"].sum() > 1000
    for kw in (dict(), dict(chunk=5)):
        m = FluxMap(spec, eng.device)
        eng.integrate(y0.clone(), nt, 7200.0, ttotal=(nt - 1) * 7200.0, sink=FluxSink(m), **kw)
        assert_flux(m.numpy(), want, a, kw)


# ------------------------------------------------------------- allreduce
def _allreduce_body(dist, ops):
    rng = np.random.default_rng(0)
    m = FluxMap(FluxSpec(144, 72), "cuda:0")
    zero = np.zeros(5000)
    m.add_points(rng.uniform(0, 6.28, 5000), rng.uniform(-1.5, 1.5, 5000), zero, zero,
                 rng.uniform(-2, 2, 5000), rng.uniform(-2, 2, 5000))
    before = m.numpy()
    m.allreduce(dist.group.WORLD)
    after = m.numpy()
    nops = len(ops)
    all_sum = all(o == dist.ReduceOp.SUM for o in ops)
    # WR.ray_flux with a group, through the N-rank branches on one rank
    # (shard.COLLECTIVE_MIN_WORLD = 1, as tests/test_gpu_multirank.py does)
    import shard
    spec = FluxSpec(144, 72)
    with np.errstate(all="ignore"):
        alone = c2_wr().ray_flux(spec, by="zwn").numpy()
        shard.COLLECTIVE_MIN_WORLD = 1
        grouped = c2_wr().ray_flux(spec, by="zwn", group=dist.group.WORLD).numpy()
    return dist.get_backend(), nops, all_sum, before, after, alone, grouped, len(ops) - nops


def test_allreduce_one_rank_group_leaves_the_map_unchanged():
    backend, nops, all_sum, before, after, alone, grouped, nops_wr = one_rank(_allreduce_body)
    assert backend == "nccl" and nops == 2 and all_sum
    assert before["count"].sum() == 5000 and before["rowsum"].sum() == 0
    assert_flux(after, before, None, "one rank")
    # the grouped drop-in: the same map as the run without a group, all-reduced
    assert alone["count"].shape == (4, 72, 144) and alone["count"].sum() > 10000
    for name in ("count", "rowsum"):
        assert np.array_equal(alone[name], grouped[name])
    assert np.allclose(alone["sum"], grouped["sum"], rtol=1e-12, atol=1e-9) and nops_wr >= 2
