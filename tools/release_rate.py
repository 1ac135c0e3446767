"""What a release stack buys and what it costs, on one GPU.

    python tools/release_rate.py [--releases 32] [--days 90] [--repeats 5] [--cost-days 10] [--out FILE.json]

(a) The stack against the loop it replaces: ``--releases`` release times spread
evenly over a 41-level family (``synthetic.background_level(j)``, 2.5 degrees,
6 h apart) x the C2 sources (3 072 slots each), ``--days`` days, no sink.  One
``integrate(release=)`` of a time-varying engine against one time-varying
``integrate`` per release (an engine on a shallow copy of the levels with
``t0 = -release``, this build's time-varying engine), alternating per repeat,
each timed by a host clock around work that ends in a device synchronise.
Both sides start from the same initial rows (``Levels.state_at`` per release).
With it, from the counters: every release's heaviest ray (accepted + rejected
attempts: the sequential chain a launch cannot be shorter than) -- the ratio of
the chains' sum to the largest one bounds the gain.

(b) The cost of the release path: the C5 sources (0.25-degree levels, 1-degree
seeds x k = 1..10, one period) for ``--cost-days`` days with every release 0
through the release kernels against the time-varying engine as shipped, at 32
and at 64 rays per wave.  Ray-steps per second of each.

Every result is checked: the release stack's counters equal the time-varying
engines'.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rossby-wave-ray-tracing_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _hip  # noqa: E402
import synthetic as S  # noqa: E402
from engine import RayEngine  # noqa: E402
from levels import Levels  # noqa: E402

DT = 6 * 3600.0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def sources(cfg):
    deg = np.pi / 180.0
    ix, iy = np.meshgrid(np.arange(cfg.nnx), np.arange(cfg.nny))
    return ((cfg.SW_lon + ix.ravel() * cfg.dlon) % 360.0) * deg, (cfg.SW_lat + iy.ravel() * cfg.dlat) * deg


def stack_vs_loop(nrel, days, repeats, first_chunk, nlev=41):
    bgs = [S.background_level(j) for j in range(nlev)]
    lv = Levels(bgs[0]["lat"], bgs[0]["lon"], nlev, t0=0.0, dt=DT)
    lv.set_levels(np.stack([b["u"] for b in bgs]), np.stack([b["v"] for b in bgs]))
    cfg = S.config("C2")
    slon, slat = sources(cfg)
    er = RayEngine.from_levels(lv)
    releases = np.linspace(0.0, (nlev - 1) * DT, nrel, endpoint=False)
    src, zc = er.sources(slon, slat), er.zwn_tensor(cfg.zwn, 0.0)
    nslot = cfg.nray
    loops, y0 = [], []
    for r in releases:
        lr = copy.copy(lv)
        lr.t0 = lv.t0 - float(r)
        loops.append(RayEngine.from_levels(lr))
        y0.append(er.initial_rows_dev(src, zc, packed=lv.state_at(float(r)).contiguous())[0][:5]
                  .reshape(5, nslot).contiguous())
    y0_all = torch.cat(y0, dim=1).contiguous()
    rel = np.repeat(releases, nslot)
    nt = int(round(days * 12)) + 1
    kw = dict(ttotal=(nt - 1) * 7200.0, order_policy="priority", first_chunk=first_chunk)

    def run_stack():
        return er.integrate(y0_all, nt, 7200.0, release=rel, **kw)

    def run_loop():
        return [e.integrate(y, nt, 7200.0, **kw) for e, y in zip(loops, y0)]

    run_stack(), run_loop()                                                 # warm-up: every shape timed below
    t_stack, t_loop = [], []
    for _ in range(repeats):
        ts, rs = timed(run_stack)
        tl, rl = timed(run_loop)
        t_stack.append(ts)
        t_loop.append(tl)
    att_s = (rs.nacc + rs.nrej).cpu().numpy().reshape(nrel, nslot)
    att_l = np.stack([(r.nacc + r.nrej).cpu().numpy() for r in rl])
    same = bool(np.array_equal(att_s, att_l)) and all(
        np.array_equal(rs.nanrow.cpu().numpy().reshape(nrel, nslot)[m], rl[m].nanrow.cpu().numpy())
        and np.array_equal(rs.nacc.cpu().numpy().reshape(nrel, nslot)[m], rl[m].nacc.cpu().numpy())
        for m in range(nrel))
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 4 * er.tv_lanes
    chain = att_s.max(axis=1)
    steps = int(rs.nacc.sum().item())
    return {
        "first_chunk": first_chunk, "releases": nrel, "levels": nlev, "slots": int(nrel * nslot), "days": days,
        "rows": nt, "tv_lanes": int(er.tv_lanes), "live_rays": int(sum(r.n_live for r in rl)),
        "stack_s": t_stack, "loop_s": t_loop,
        "stack_median_s": statistics.median(t_stack), "loop_median_s": statistics.median(t_loop),
        "loop_over_stack": statistics.median(t_loop) / statistics.median(t_stack),
        "ray_steps": steps,
        "stack_ray_steps_per_s": steps / statistics.median(t_stack),
        "loop_ray_steps_per_s": steps / statistics.median(t_loop),
        "counters_equal_time_varying": same,
        "heaviest_chain_attempts_per_release": chain.tolist(),
        "heaviest_chain_attempts_stack": int(chain.max()), "sum_of_release_chains_loop": int(chain.sum()),
        "chain_ratio_bound": float(chain.sum() / chain.max()),
        "attempts_total": int(att_s.sum()), "lanes": int(lanes),
        "occupancy_stack_at_chain": float(att_s.sum() / (chain.max() * lanes)),
        "occupancy_loop_at_chain": float(att_s.sum() / (chain.sum() * lanes)),
        "stack_launch_log": list(er.launch_log),
    }


def release_cost(days, repeats):
    res = 0.25
    nt = int(round(days * 12)) + 1
    nlev = int(np.ceil((nt - 1) * 7200.0 / DT)) + 1
    b0 = S.background_level(0, res=res)
    lv = Levels(b0["lat"], b0["lon"], nlev, t0=0.0, dt=DT)
    for j in range(nlev):
        b = b0 if j == 0 else S.background_level(j, res=res)
        lv.set_level(j, b["u"], b["v"])
    cfg = S.config("C5")
    slon, slat = sources(cfg)
    out = {"grid_deg": res, "levels": nlev, "days": days, "rows": nt}
    for lanes in (32, 64):
        shipped, er = RayEngine.from_levels(lv), RayEngine.from_levels(lv)
        shipped.tv_lanes = er.tv_lanes = lanes
        y0 = er.initial_rows_dev(er.sources(slon, slat), er.zwn_tensor(cfg.zwn, S.c3_freq(S.C3_PERIODS_DAYS[0])))[0][:5]
        y0 = y0.reshape(5, -1).contiguous()
        zero = np.zeros(y0.shape[1])
        kw = dict(ttotal=(nt - 1) * 7200.0, order_policy="priority", first_chunk=[24, 96])
        runs = {"release_all_zero": lambda: er.integrate(y0, nt, 7200.0, release=zero, **kw),
                "time_varying_as_shipped": lambda: shipped.integrate(y0, nt, 7200.0, **kw)}
        got, times = {}, {k: [] for k in runs}
        for fn in runs.values():
            fn()                                                            # warm-up
        for _ in range(repeats):
            for k, fn in runs.items():
                t, got[k] = timed(fn)
                times[k].append(t)
        a, b = got["release_all_zero"], got["time_varying_as_shipped"]
        steps = int(a.nacc.sum().item())
        o = {"rays": int(y0.shape[1]), "live_rays": int(a.n_live), "ray_steps": steps,
             "counters_equal_time_varying": bool(torch.equal(a.nacc, b.nacc)) and bool(torch.equal(a.nrej, b.nrej))
             and bool(torch.equal(a.nanrow, b.nanrow))}
        for k in runs:
            med = statistics.median(times[k])
            o[k] = {"s": times[k], "median_s": med, "ray_steps_per_s": steps / med}
        o["release_over_time_varying"] = o["release_all_zero"]["median_s"] / o["time_varying_as_shipped"]["median_s"]
        out[f"tv_lanes_{lanes}"] = o
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--releases", type=int, default=32)
    ap.add_argument("--days", type=float, default=90.0)
    ap.add_argument("--cost-days", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-cost", action="store_true", help="measurement (a) only")
    ap.add_argument("--skip-stack", action="store_true", help="measurement (b) only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/release_rate.py measures on the GPU: no HIP device visible")
    out = {"device": torch.cuda.get_device_name(0), "library": _hip.version()}

    def save():
        text = json.dumps(out, indent=1)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return text

    if not a.skip_stack:
        # the same integrate() arguments on both sides: its defaults (one launch), and two leading launches
        out["a_stack_vs_loop"] = stack_vs_loop(a.releases, a.days, a.repeats, None)
        save()
        out["a_stack_vs_loop_lead_24_96"] = stack_vs_loop(a.releases, a.days, a.repeats, [24, 96])
        save()
    if not a.skip_cost:
        out["b_release_cost_c5"] = release_cost(a.cost_days, a.repeats)
    print(save())


if __name__ == "__main__":
    main()
