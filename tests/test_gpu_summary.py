"""Per-ray path summaries on the GPU (``rwrt_ray_summary``, summary.py) equal
the NumPy definition ``summary.reference_summary`` -- integer fields exactly,
selections bit for bit, ``path`` within a relative 1e-12 -- for crafted rows
in every row layout (dense, tails, row blocks) in one call and in two, through
``RayEngine.integrate`` / ``integrate_rk4`` in any chunking and row layout, on
a time-varying background, through ``WR.ray_summary`` on the reference's C1
history, across shards and ranks, and next to a density map in one ``Tee``."""
import math
import os

import numpy as np
import pytest
import torch

from density import DensityMap, DensitySink, DensitySpec, reference_bins
from summary import RaySummary, SummarySink, Tee, reference_summary
from support.bits import bitwise
from support.cases import c1_wr, c2_hist, c2_wr, c2_y0, engine, tv_engine
from support.cases_summary import C1_BOX, REGIONS8, assert_summary, c1_rows
from support.dist import child_paths, free_port, one_rank
from support.rows import layout_device

pytestmark = pytest.mark.gpu
DEV = "cuda"
NT_C2 = 121          # 10 days
NAN = math.nan


def check(rs, want, what, cols=None):
    """``rs.numpy()`` against ``want`` (at the columns ``cols``)."""
    got = rs.numpy()
    if cols is not None:
        got = {k: v[..., cols] for k, v in got.items()}
    wp = np.asarray(want["path"])
    rel = np.abs(np.asarray(got["path"]) - wp)[wp > 0] / wp[wp > 0]
    print(f"summary {what}: max |path - want| / want = {rel.max() if rel.size else 0.0:.3g} (bound 1e-12)")
    assert_summary(got, want, what)
    assert np.array_equal(got["path_m"], got["path"] * 6.3712e6)
    return got


def _same(a, b):
    """Every field of two ``numpy()`` dicts, bit for bit."""
    for k in a:
        same = bitwise(a[k], b[k]) if a[k].dtype.kind == "f" else np.array_equal(a[k], b[k])
        assert same, k


def non_vacuous(want, what):
    """The case has reflections and, in some region, rays that arrive and rays that never do."""
    n = want["n_valid"].size
    assert want["n_turn"].max() > 0, what
    if len(want["first_row"]):
        hit = (want["first_row"].reshape(len(want["first_row"]), -1) >= 0).sum(axis=1)
        assert ((hit > 0) & (hit < n)).any(), (what, hit)


# ------------------------------------------------- crafted rows, entry point
NRAY, NROW = 130, 8          # three waves, the last partial; row 0 and rows 1..7
NCOL = 200                   # the accumulators are wider than the ray set
SENTINEL = (0.1, 1.55, -9.0, 1e6)   # lon lat l amp: valid, inside boxes, beyond every real lat and amp


def crafted(seed=0, frz=None):
    """Logical rows ``[130, 8, 8]`` and each ray's freeze row ``frz`` (rows from
    ``frz`` on repeat row ``frz``; 8: never): frozen from row 1 on (j % 3 == 0,
    no row block in the slots layout), from a row in 2..6, or live -- or the
    ``frz`` given; NaN tails, NaN first rows and NaN holes on either side of
    the split at row 4."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-3.0, 3.0, (NRAY, NROW, 8))
    rows[..., 0] = rng.uniform(-70.0, 70.0, (NRAY, NROW))
    rows[..., 1] = rng.uniform(-1.5, 1.5, (NRAY, NROW))
    j = np.arange(NRAY)
    if frz is None:
        frz = np.where(j % 3 == 0, 1, np.where(j % 3 == 1, 2 + j % 5, NROW))
    rows[j % 13 == 5, 0] = NAN                     # no initial row
    rows[0, 0] = NAN                               # (ray 0 is NaN from row 1 on too: no valid row at all)
    rows[(j % 3 == 2) & (j % 5 == 2), 3, :2] = NAN   # a hole before the split ...
    rows[(j % 3 == 2) & (j % 5 == 3), 4, 0] = np.inf   # ... and after it
    rows[j % 17 == 4, 2:5, 4] = NAN                # valid rows without an amplitude
    rows[j % 19 == 7, :, 3] = 0.0                  # l == 0 throughout
    for r in range(NRAY):
        if frz[r] < NROW:
            if r % 7 == 0:
                rows[r, frz[r]] = NAN              # frozen NaN rays
            rows[r, frz[r]:] = rows[r, frz[r]]
    return rows, frz


def layouts(rows, frz, i0, i1, seed=1, frm=None):
    """``name -> (view, tails, slots)`` device objects of the logical rows
    ``[i0, i1)``; what a launch would not write holds SENTINEL.  ``frm``: the
    ``tail_from`` handed over (default: ``frz`` clipped to the launch)."""
    tf = np.clip(frz, i0, i1).astype(np.int32)
    tail = rows[np.arange(NRAY), np.minimum(tf, i1 - 1)].copy()
    tail[tf >= i1] = [SENTINEL[0], SENTINEL[1], 0.0, SENTINEL[2], SENTINEL[3], 0.0, 0.0, 0.0]   # (no tail: unread)
    L = dict(i0=i0, i1=i1, rows=rows[:, i0:i1], tail=tail, tf=tf)
    # (here a ray has a row block when it has rows to read, whatever its number)
    out = layout_device(L, dict(zip((0, 1, 3, 4), SENTINEL)), seed + i0, DEV, live=np.where(tf > i0)[0])
    if frm is not None:
        out["tails"][1].frm.copy_(torch.as_tensor(np.asarray(frm, np.int32)))
    return out


@pytest.mark.parametrize("nreg", [0, 1, 8])
def test_crafted_rows_every_layout(nreg):
    """130 rays x (row 0 + 7 rows) through a permuted column map into 200
    columns: rows 1..7 in one call and split at row 4 (the carried previous
    row), dense, with tails and with row blocks."""
    rows, frz = crafted()
    every_layout_equals_reference_summary(rows, frz, nreg, ([(1, 8)], [(1, 4), (4, 8)]))


@pytest.mark.parametrize("nreg", [0, 1, 8])
def test_crafted_rows_tail_from_clamp_and_batch_boundary(nreg):
    """Rows 1..7 in one call with ``tail_from`` below, at and above the launch,
    handed over unclamped, and 0, 1, 3, 4, 5 and 7 rows read: on either side
    of the kernel's batch of 4."""
    i0, i1 = 1, NROW
    j = np.arange(NRAY)
    frm = np.array([i0 - 2, i0, i0 + 1, i0 + 3, i0 + 4, i0 + 5, i1, i1 + 3])[j % 8]
    frz = np.clip(frm, i0, i1)
    assert sorted(set((frz - i0).tolist())) == [0, 1, 3, 4, 5, 7]
    rows, frz = crafted(seed=4, frz=frz)
    every_layout_equals_reference_summary(rows, frz, nreg, ([(i0, i1)],), frm)


def every_layout_equals_reference_summary(rows, frz, nreg, all_splits, frm=None):
    regions = REGIONS8[:nreg]
    want = reference_summary(rows, regions)
    non_vacuous(want, nreg)
    assert (want["n_valid"] == 0).any() and (want["last_row"] < NROW - 1).any() and (want["path"] == 0.0).any()
    cols = np.random.default_rng(3).permutation(NCOL)[:NRAY]
    ray = torch.as_tensor(cols, device=DEV)
    spare = np.setdiff1d(np.arange(NCOL), cols)
    for splits in all_splits:
        for name in ("dense", "tails", "slots"):
            rs = RaySummary(NCOL, regions, DEV)
            fresh = rs.numpy()
            rs.start(rows[:, 0, 0], rows[:, 0, 1], rows[:, 0, 3], rows[:, 0, 4], ray=ray)
            for i0, i1 in splits:
                view, tails, slots = layouts(rows, frz, i0, i1, frm=frm)[name]
                rs.add_rows(i0, i1, view, tails, slots, ray)
            got = check(rs, want, (nreg, splits, name), cols)
            full = rs.numpy()
            # no rays: nothing changes
            rs.add_rows(8, 9, torch.empty((0, 1, 8), dtype=torch.float64, device=DEV), ray=ray[:0])
            _same(full, rs.numpy())
            # the columns no ray maps to keep the values of a ray without rows
            _same({k: v[..., spare] for k, v in full.items()}, {k: v[..., spare] for k, v in fresh.items()})
            assert got["n_valid"].max() == NROW and rs.owned.sum().item() == NRAY


def test_identity_columns_and_argument_checks():
    rows, frz = crafted(seed=2)
    want = reference_summary(rows, [C1_BOX])
    rs = RaySummary(NRAY, [C1_BOX], DEV)
    rs.start(rows[:, 0, 0], rows[:, 0, 1], rows[:, 0, 3], rows[:, 0, 4])
    assert not rs.owned.any()                      # (row 0 does not claim a ray)
    view, tails, slots = layouts(rows, frz, 1, 8)["slots"]
    rs.add_rows(1, 8, view, tails, slots)
    check(rs, want, "identity")
    with pytest.raises(ValueError):
        rs.add_rows(1, 8, view, None, slots)
    with pytest.raises(ValueError):
        rs.add_rows(1, 7, view, tails, slots)
    with pytest.raises(ValueError):
        RaySummary(NCOL, [C1_BOX], DEV).add_rows(1, 8, view, tails, slots)     # 130 rays, 200 columns, no map
    with pytest.raises(ValueError):
        RaySummary(NRAY, [C1_BOX] * 9, DEV)


# ------------------------------------------------ C2 through the engine
C2_REGIONS = [C1_BOX, (160.0, 220.0, 20.0, 60.0), (150.0, 160.0, 30.0, 50.0)]   # chosen from a 10-day CPU history


def c2_summary(kind, regions, rk4=False, idx=None, rs=None, extra=None, **kw):
    eng = engine(kind)
    row0, y0 = c2_y0(kind)
    if rs is None:
        rs = RaySummary(3072, regions, eng.device)
        rs.start(row0[0], row0[1], row0[3], row0[4])
    sink = SummarySink(rs)
    if extra is not None:
        sink = Tee(extra, sink)
    if idx is not None:
        y0 = y0[:, torch.as_tensor(idx)].contiguous()
        sink = sink.take(idx)
    if rk4:
        eng.integrate_rk4(y0, NT_C2, 7200.0, sink=sink, **kw)
    else:
        eng.integrate(y0, NT_C2, 7200.0, ttotal=(NT_C2 - 1) * 7200.0, sink=sink, **kw)
    return rs


@pytest.mark.parametrize("path", ["slots", "tails", "dense"])
@pytest.mark.parametrize("kind", ["zonal", "nonzonal"])
def test_c2_chunking_and_row_layouts(kind, path):
    """One launch (chunk = 120), many (chunk = 7) and short leading launches
    with the latency mode give the summary of the delivered history, on the
    row-block, the tails and the dense path."""
    regions = C2_REGIONS[:1] if path == "tails" else C2_REGIONS
    want = reference_summary(c2_hist(kind), regions)
    non_vacuous(want, (kind, path))
    assert want["path"].max() > 1.0
    eng = engine(kind)
    try:
        if path == "tails":
            eng.use_slots = False
        if path == "dense":
            eng.use_tails = False
        for kw in (dict(chunk=120), dict(chunk=7), dict(first_chunk=[6, 24], team=[64, 64, 64])):
            check(c2_summary(kind, regions, **kw), want, (kind, path, kw))
    finally:
        for a in ("use_slots", "use_tails"):
            eng.__dict__.pop(a, None)


@pytest.mark.parametrize("kind", ["zonal", "nonzonal"])
def test_c2_rk4(kind):
    want = reference_summary(c2_hist(kind, "rk4"), C2_REGIONS)
    non_vacuous(want, kind)
    for kw in (dict(), dict(chunk=7)):
        check(c2_summary(kind, C2_REGIONS, rk4=True, **kw), want, (kind, kw))


def test_time_varying_background():
    """A time-varying background (fp64 levels), built as
    test_gpu_density.py::test_time_varying_background builds it, one day."""
    import synthetic as S
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
    hist = np.full((y0.shape[1], nt, 8), NAN)
    hist[:, 0, :7] = row0[:7].T
    hist[:, 1:] = np.concatenate([got[k] for k in sorted(got)], axis=1)
    regions = [(100.0, 120.0, 15.0, 30.0), C1_BOX]     # the first holds some of the sources
    want = reference_summary(hist, regions)
    non_vacuous(want, "tv")
    for kw in (dict(), dict(chunk=5)):
        rs = RaySummary(y0.shape[1], regions, eng.device)
        rs.start(init[0], init[1], init[3], init[4])       # device tensors [3, nsource, nzwn], as they are
        eng.integrate(y0.clone(), nt, 7200.0, ttotal=(nt - 1) * 7200.0, sink=SummarySink(rs), **kw)
        check(rs, want, ("tv", kw))


# ------------------------------------------------------- WR.ray_summary (C1)
def test_c1_ray_summary_equals_the_reference_history(tmp_path):
    """C1, 90 days through WR.ray_summary: the summary of the reference's own
    golden history, the literals of tests/test_summary_host.py included."""
    import ncio
    want = reference_summary(c1_rows(), [C1_BOX])
    wr = c1_wr()
    with np.errstate(all="ignore"):
        rs = wr.ray_summary(regions=[C1_BOX])
    got = rs.numpy()
    assert got["path"].shape == (3, 1, 1) and got["first_row"].shape == (1, 3, 1, 1)
    flat = {k: v.reshape(v.shape[:-3] + (3,)) for k, v in got.items()}
    assert_summary(flat, want, "C1")
    assert flat["n_valid"].tolist() == [1081, 1081, 1081] and flat["n_turn"].tolist() == [0, 155, 111]
    assert flat["path"][0] == 0.0
    assert flat["first_row"].tolist() == [[-1, 97, 93]] and flat["rows_inside"].tolist() == [[0, 88, 93]]
    assert np.isnan(wr.rlon[1:]).all() and not np.isnan(wr.rlon[0]).any()      # no history was delivered
    with np.errstate(all="ignore"):      # mode='numpy': the delivered history through reference_summary
        host = c1_wr().ray_summary(regions=[C1_BOX], mode="numpy")
    assert isinstance(host, RaySummary) and host.i32[3].tolist() == [1, 1, 1]
    host = host.numpy()
    assert host["path"].shape == (3, 1, 1)
    assert_summary({k: v.reshape(v.shape[:-3] + (3,)) for k, v in host.items()}, want, "C1 numpy")
    for name in ("summary.nc", "summary.npz"):
        path = str(tmp_path / name)
        rs.output(path)
        d = ncio.read(path)
        assert d["path"].shape == (3, 1, 1) and d["first_row"].reshape(-1).tolist() == [-1, 97, 93]
        assert np.array_equal(d["n_turn"].reshape(-1), [0, 155, 111])
        assert np.allclose(d["lat_first"].reshape(-1), 30.0) and d["region_box"].tolist() == [list(C1_BOX)]


# ------------------------------------------------------------- shards, Tee
def test_c2_shards_give_the_whole():
    """The two halves of shard_indices(world=2), integrated one after the
    other through ``take(idx)`` into one summary, and the two emulated ranks
    of run_sharded (the sharded sink form), equal the whole set's summary."""
    import shard
    want = reference_summary(c2_hist("zonal"), C2_REGIONS)
    row0, y0 = c2_y0("zonal")
    live = ~np.isnan(row0[:5].mean(axis=0))
    rs = None
    for r in range(2):
        idx = shard.shard_indices(live, r, 2)
        rs = c2_summary("zonal", C2_REGIONS, idx=idx, rs=rs, chunk=50)
        assert rs.owned.sum().item() == (len(idx) if r == 0 else 3072)
    check(rs, want, "take")
    eng = engine("zonal")
    rs = RaySummary(3072, C2_REGIONS, eng.device)
    rs.start(row0[0], row0[1], row0[3], row0[4])
    for r in range(2):
        shard.run_sharded(eng, y0, NT_C2, 7200.0, rank=r, world=2, ttotal=(NT_C2 - 1) * 7200.0,
                          sink=SummarySink(rs), gather=False)
    check(rs, want, "run_sharded")


def test_tee_density_and_summary_share_one_integration():
    hist = c2_hist("zonal")
    want = reference_summary(hist, C2_REGIONS)
    spec = DensitySpec(360, 180, weight="amp")
    pts = hist[:, 1:]
    count_want = reference_bins(pts[..., 0], pts[..., 1], pts[..., 4], None, spec)[0]
    eng = engine("zonal")
    m = DensityMap(spec, eng.device)
    rs = c2_summary("zonal", C2_REGIONS, extra=DensitySink(m), chunk=40)
    assert eng.rows_bytes < 3072 * 40 * 64          # (the Tee took row blocks)
    check(rs, want, "tee")
    assert np.array_equal(m.numpy()[0], count_want)
    alone = DensityMap(spec, eng.device)
    row0, y0 = c2_y0("zonal")
    eng.integrate(y0, NT_C2, 7200.0, ttotal=(NT_C2 - 1) * 7200.0, sink=DensitySink(alone), chunk=40)
    assert np.array_equal(alone.numpy()[0], m.numpy()[0])


# ------------------------------------------------------------- allreduce
def _one_rank_body(dist, ops):
    import shard
    rows, frz = crafted()
    rs = RaySummary(NRAY, REGIONS8, "cuda:0")
    rs.start(rows[:, 0, 0], rows[:, 0, 1], rows[:, 0, 3], rows[:, 0, 4])
    half = torch.arange(0, NRAY, 2, device="cuda:0")          # the rays this rank integrated
    view = torch.as_tensor(rows[::2, 1:], device="cuda:0").contiguous()
    rs.add_rows(1, 8, view, ray=half)
    before = rs.numpy()
    rs.allreduce(dist.group.WORLD)
    after = rs.numpy()
    with np.errstate(all="ignore"):
        alone = c2_wr().ray_summary(regions=C2_REGIONS).numpy()
        shard.COLLECTIVE_MIN_WORLD = 1
        grouped = c2_wr().ray_summary(regions=C2_REGIONS, group=dist.group.WORLD).numpy()
    return dist.get_backend(), before, after, alone, grouped


def test_allreduce_one_rank_group_leaves_the_summary_unchanged():
    """A one-rank nccl group: the all-reduce (RCCL, device tensors) changes no
    bit -- the rays this rank integrated and the ones nobody did, which keep
    their row 0 -- and WR.ray_summary with the group, through the N-rank
    branches (shard.COLLECTIVE_MIN_WORLD = 1), equals the run without one."""
    backend, before, after, alone, grouped = one_rank(_one_rank_body)
    assert backend == "nccl"
    assert before["n_valid"][::2].max() == NROW and before["n_valid"][1::2].max() == 1
    _same(before, after)
    assert alone["path"].shape == (3, 256, 4) and alone["n_turn"].max() > 0
    _same(alone, grouped)


def _two_rank_worker(rank, port, q):
    child_paths()
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        with np.errstate(all="ignore"):
            got = c2_wr().ray_summary(regions=C2_REGIONS, group=dist.group.WORLD).numpy()
        q.put(("ok", rank, got))
    except Exception as e:  # pragma: no cover
        q.put(("err", rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_world2_ray_summary_equals_single_gpu():
    """Two processes share the GPU over gloo: each integrates its shard and
    owns those rays; after the all-reduce both hold every ray's summary, bit
    for bit the single-process one (``path`` included: one rank adds a ray's
    segments, the others add zero)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=110) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(r[0] == "ok" for r in res), res
    with np.errstate(all="ignore"):
        want = c2_wr().ray_summary(regions=C2_REGIONS).numpy()
    non_vacuous(want, "world 2")
    assert sorted(r[1] for r in res) == [0, 1]
    for r in res:
        _same(want, r[2])
