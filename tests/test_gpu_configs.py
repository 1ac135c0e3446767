"""The ray loop on the BASELINE configurations C3, C4 and C5 (BASELINE.json
configs[2..4]) against the oracle.

* C3 -- the full 2.40 M-slot C3 set integrated 12 days on the GPU; on a
  cost-stratified sample of 16 384 live rays (tests/golden/c3_sample.npz, made
  by tools/c3_sample.py: the 512 rays with the most attempts in day 1 plus
  random rays from 31 cost quantiles) every row must equal the oracle (the
  reference's own arithmetic, NumPy's transcendentals included) BIT FOR BIT:
  all 7 variables, 144 rows, accepted-step counts.  (For scale: under a
  1-ulp RHS perturbation the reference itself moves these rays by up to
  1.8e-4 rad after a day and 3.6e-2 rad after 12 days,
  tests/golden/noise_floor_C3_zonal.json.)
* C4 -- the same sample as ONE ray set split over a world-2 group by measured
  cost (shard.run_sharded: probe launch, snake deal, per-rank integration,
  gather to rank 0), bit-identical to the 1-GPU run.
* C5 -- 0.25-degree time-varying background, 4 096 live rays from the C5 seed
  grid, 2 days through 9 levels, fp64 and fp32 level storage, bit-identical to
  the oracle's TimeVaryingBackground.
"""
import os

import numpy as np
import pytest

from conftest import golden
from support.dist import free_port

pytestmark = pytest.mark.gpu
C3_DAYS = 12


def same(a, b):
    a = np.where(np.isnan(a), np.nan, np.asarray(a, np.float64))
    b = np.where(np.isnan(b), np.nan, np.asarray(b, np.float64))
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def ndiff(a, b):
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


_C3 = {}


def c3_run():
    """Full C3 on the GPU for C3_DAYS; rows (ray, row, 8) of the sample rays."""
    if "gpu" not in _C3:
        import torch
        from bench import c3_initial_state, c3_sources, make_bs
        from engine import RayEngine
        bs, bg = make_bs("zonal")
        eng = RayEngine.from_bs(bs)
        src, zcs = c3_sources(eng)
        y0 = torch.cat([eng.initial_rows_dev(src, zc)[0][:5].reshape(5, -1) for zc in zcs], dim=1)
        g = golden("c3_sample.npz")
        assert y0.shape[1] == int(g["nslot"])
        sel = torch.as_tensor(g["idx"], device=eng.device)
        nt = C3_DAYS * 12 + 1
        rows = {}
        res = eng.integrate(y0, nt, 7200.0, chunk=48, first_chunk=[6, 24],
                            sink=lambda a, b, o: rows.__setitem__(a, o[sel].cpu().numpy()))
        hist = np.concatenate([rows[k] for k in sorted(rows)], axis=1)
        y0h = c3_initial_state(bs)
        # the GPU initial rows are the host rows (tests/test_gpu_parity.py), here too
        assert same(y0[:, sel].cpu().numpy(), y0h[:, g["idx"]])
        _C3["gpu"] = (hist, res.nacc[sel].cpu().numpy(), y0h[:, g["idx"]].copy(), bg, nt)
    return _C3["gpu"]


@pytest.mark.refhost
def test_c3_sample_bitwise_with_reference_arithmetic():
    import rwrt_oracle as O
    hist, nacc, y0, bg, nt = c3_run()
    with np.errstate(all="ignore"):
        ref, rnacc, _, st = O.ray_run(O.Background(**bg), y0.copy(), nt, 7200.0)
    assert st == 0
    g = np.transpose(hist[:, :, :7], (2, 1, 0))
    assert same(g, ref[:, 1:]), f"{ndiff(g, ref[:, 1:])} values differ"
    assert np.array_equal(nacc, rnacc)
    # the nacc column of every row is the running accepted-step count
    assert np.array_equal(hist[:, -1, 7].astype(np.int64), rnacc)


# ---------------------------------------------------------------- C4
def _c4_worker(rank, world, port, q, shard_probe=False):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    sys.path[:0] = [os.path.join(root, "rossby-wave-ray-tracing_amd"), root, here]
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bench import c3_initial_state, make_bs
        from engine import RayEngine
        from shard import broadcast_array, gather_rows, run_sharded
        bs, bg = make_bs("zonal")
        # rank 0's basic state is the one every rank integrates through
        fields = broadcast_array(bs.fields if rank == 0 else None)
        eng = RayEngine(fields, bs.lon, bs.lat)
        g = np.load(os.path.join(here, "golden", "c3_sample.npz"))
        y0 = c3_initial_state(bs)[:, g["idx"]]
        nt = C3_DAYS * 12 + 1
        parts = []
        r = run_sharded(eng, y0, nt, group=dist.group.WORLD, chunk=48, shard_probe=shard_probe,
                        sink=lambda a, b, o, idx: parts.append(o.cpu()))
        mine = torch.cat(parts, dim=1)                      # (n_local, nt-1, 8)
        full = gather_rows(mine, r.idx.cpu().numpy(), y0.shape[1], group=dist.group.WORLD)
        if rank == 0:
            q.put(("ok", full.numpy(), r.counts.cpu().numpy(), r.endpoints.cpu().numpy(),
                   int(r.idx.numel())))
        else:
            q.put(("rank1", int(r.idx.numel())))
    except Exception as e:  # pragma: no cover
        q.put(("err", repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("shard_probe", [False, True])
def test_c4_cost_sharded_world2_equals_single_gpu(shard_probe):
    """``shard_probe``: each rank probes half the rays and the probe costs are
    all-gathered (shard.probe_costs), then each re-probes its own shard."""
    import torch.multiprocessing as mp
    hist, nacc, y0, bg, nt = c3_run()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_c4_worker, args=(r, 2, port, q, shard_probe)) for r in range(2)]
    for p in procs:
        p.start()
    msgs = [q.get(timeout=110) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    ok = [m for m in msgs if m[0] == "ok"]
    assert ok, msgs
    _, full, counts, ends, n0 = ok[0]
    n1 = [m for m in msgs if m[0] == "rank1"][0][1]
    assert n0 + n1 == hist.shape[0] and abs(n0 - n1) <= 2     # balanced, disjoint, complete
    assert same(full[:, :, :7], hist[:, :, :7])
    assert np.array_equal(counts[:, 0], nacc)
    assert same(ends, hist[:, -1])


@pytest.mark.parametrize("world", [8])
def test_c4_full_set_split_union_equals_single_gpu(world):
    """The WHOLE C3 set (2.40 M slots, 12 days) split ``world`` ways as
    bench.py --gpus 8 splits it -- each rank probing every ``world``-th ray,
    the costs all-gathered (here: every share probed on this GPU,
    shard.probe_costs), each rank re-probing and integrating its shard --
    each emulated rank run alone on this GPU: the union of the ranks' last
    rows and step counters equals the 1-GPU run's bit for bit, and the split
    is disjoint, complete and balanced in live rays."""
    import torch
    from bench import c3_initial_state, make_bs
    from engine import RayEngine, t_eval_of
    from shard import probe_costs, run_sharded
    bs, _ = make_bs("zonal")
    eng = RayEngine.from_bs(bs)
    y0 = torch.as_tensor(c3_initial_state(bs), device=eng.device)
    nt = C3_DAYS * 12 + 1
    one = run_sharded(eng, y0, nt, rank=0, world=1, lead=[24, 96])
    ends1, cnt1 = one.endpoints.cpu().numpy(), one.counts.cpu().numpy()
    p = eng.params(nt, 7200.0)
    st0 = eng.init(y0, p)
    tb = torch.as_tensor(t_eval_of(nt, 7200.0), dtype=torch.float64, device=eng.device)
    costs = probe_costs(eng, st0, p, tb, 6, 0, world)
    del st0
    nray = y0.shape[1]
    ends = np.full((nray, 8), -1.0)
    cnts = np.full((nray, 2), -1, dtype=np.int64)
    seen = np.zeros(nray, dtype=np.int64)
    live = []
    for r in range(world):
        rr = run_sharded(eng, y0, nt, rank=r, world=world, lead=[24, 96], costs=costs)
        idx = rr.idx.cpu().numpy()
        seen[idx] += 1
        ends[idx] = rr.endpoints.cpu().numpy()
        cnts[idx] = rr.counts.cpu().numpy()
        live.append(int((~torch.isnan(y0[:, rr.idx].sum(0))).sum().item()))
    assert (seen == 1).all()                                   # disjoint and complete
    assert max(live) - min(live) <= 2                          # balanced in live rays
    assert np.array_equal(cnts, cnt1)
    assert same(ends, ends1), f"{ndiff(ends, ends1)} values differ"


@pytest.mark.refhost
# ---------------------------------------------------------------- C5
@pytest.mark.parametrize("fp32", [False, True])
def test_c5_025deg_bitwise_with_oracle(fp32):
    import torch
    import rwrt_oracle as O
    import synthetic as S
    from engine import RayEngine
    from levels import Levels
    dt, nlev, nt = 6 * 3600.0, 9, 25          # 2 days at 2 h through 9 six-hourly levels
    bl = [S.background_level(j, res=0.25) for j in range(nlev)]
    lv = Levels(bl[0]["lat"], bl[0]["lon"], nlev, t0=0.0, dt=dt, fp32=fp32)
    for j, b in enumerate(bl):
        lv.set_level(j, b["u"], b["v"])
    eng = RayEngine.from_levels(lv)
    cfg = S.config("C5")
    slon, slat = O.source_matrix(cfg.SW_lon, cfg.SW_lat, cfg.dlon, cfg.dlat, cfg.nnx, cfg.nny)
    rows = eng.initial_rows(slon, slat, cfg.zwn, S.c3_freq(S.C5_PERIODS_DAYS[-1])).cpu().numpy()
    y0 = rows[:5].reshape(5, -1)
    live = np.where(~np.isnan(y0.mean(axis=0)))[0]
    pick = np.sort(np.random.default_rng(3).choice(live, size=4096, replace=False))
    y0 = y0[:, pick].copy()
    got = {}
    res = eng.integrate(torch.as_tensor(y0), nt, 7200.0, ttotal=(nt - 1) * 7200.0, chunk=12,
                        sink=lambda a, b, o: got.__setitem__(a, o.cpu().numpy().copy()))
    hist = np.concatenate([got[k] for k in sorted(got)], axis=1)
    del eng, lv
    torch.cuda.empty_cache()
    ob = O.TimeVaryingBackground([O.Background(**b) for b in bl], 0.0, dt, fp32=fp32)
    with np.errstate(all="ignore"):
        ref, nacc, _, st = O.ray_run(ob, y0.copy(), nt, 7200.0)
    assert st == 0
    g = np.transpose(hist[:, :, :7], (2, 1, 0))
    assert same(g, ref[:, 1:]), f"{ndiff(g, ref[:, 1:])} values differ"
    assert np.array_equal(res.nacc.cpu().numpy(), nacc)
    # the sample moves through the levels (not a static-state test in disguise)
    assert np.nanmax(np.abs(hist[:, -1, 0] - y0[0])) > 0.05
