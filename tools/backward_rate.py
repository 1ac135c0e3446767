"""The backward ray loop's rate next to the forward one's, on one GPU.

    python tools/backward_rate.py [--days 90] [--repeats 3] [--footprint] [--out FILE.json]

The C3 sources on the zonal and the non-zonal state, ``--days`` days, no sink
(row blocks for the live rays, never read).  Forward and backward run in one
process, alternating per repeat, each with the benchmark's schedule for a
whole C3 set on one GPU: a 4-row probe, leading launches of 24 and 160 rows,
the rest in one launch (split by the ``"auto"`` rule), priority order, the 64
heaviest rays of every launch after the probe in latency mode on the zonal
state and none on the non-zonal one.  Each run is timed by a host clock around
work that ends in a device synchronise (solver construction included).

The two directions integrate different ray populations (a backward ray leaves
its source the other way), so wall times and ray-steps per second are not
comparable as such; the rate per attempt (accepted + rejected, the unit of the
loop's work) is, and ``backward_over_forward_attempts_per_s`` is that ratio.

``--footprint``: the README's example, timed -- backward rays from one receptor
box over East Asia (21 x 11 receptors, 100-140E 20-40N, k = 1..7, 30 days)
through ``WR(backward=True).ray_density``.
"""
import argparse
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
import bench  # noqa: E402
from engine import RayEngine, t_eval_of  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def rate(kind, days, repeats):
    bs, _ = bench.make_bs(kind)
    eng = RayEngine.from_bs(bs)
    src, zcs = bench.c3_sources(eng)
    y0 = torch.cat([eng.initial_rows_dev(src, zc)[0][:5].reshape(5, -1) for zc in zcs], dim=1).contiguous()
    live0 = ~torch.isnan(y0.sum(0))
    nt = int(round(days * 12)) + 1
    tb = torch.as_tensor(t_eval_of(nt, 7200.0, (nt - 1) * 7200.0), dtype=torch.float64, device=eng.device)
    team = [0, 64, 64, 64] if kind == "zonal" else 0

    def run(backward):
        p = eng.params(nt, 7200.0, backward=backward)
        st = eng.init(y0, p)
        return eng.advance(st, p, tb, 1, order_policy="priority", first_chunk=[4, 24, 160], team=team, split="auto")

    run(False), run(True)                                               # warm-up: every shape timed below
    times = {False: [], True: []}
    res = {}
    for _ in range(repeats):
        for b in (False, True):
            t, res[b] = timed(lambda: run(b))
            times[b].append(t)
    out = {"state": kind, "slots": int(y0.shape[1]), "days": days, "rows": nt, "team": team}
    # one more run per direction, not timed by the host clock: every launch's device time (events), its
    # attempts in all and of its heaviest ray (the chain it cannot be shorter than), the rays handed off
    # at its drain, and the rank correlation of the two leading launches' work (the "auto" split's rule)
    launches = {}
    for b in (False, True):
        ev = []
        eng.keep_launch_work = True
        try:
            p = eng.params(nt, 7200.0, backward=b)
            r = eng.advance(eng.init(y0, p), p, tb, 1, order_policy="priority", first_chunk=[4, 24, 160], team=team,
                            split="auto", events=ev)
            torch.cuda.synchronize()
            launches[b] = [{"rows": list(bd), "ms": e0.elapsed_time(e1), "attempts": int(w.sum().item()),
                            "heaviest_ray_attempts": int(w.max().item()), "handed_off": h}
                           for bd, (e0, e1), (w, _), h in zip(r.bounds, ev, eng.launch_work, eng.handoffs())]
            launches[b].append({"split_rank_correlation": eng.split_rho})
        finally:
            eng.keep_launch_work = False
            eng.launch_work = []
    for b, name in ((False, "forward"), (True, "backward")):
        r = res[b]
        assert r.backward is b
        med = statistics.median(times[b])
        acc, rej = int(r.nacc.sum().item()), int(r.nrej.sum().item())
        att = (r.nacc + r.nrej)
        out[name] = {"s": times[b], "median_s": med, "live_rays": int(r.n_live),
                     "live_at_end": int(((r.nanrow == nt) & live0).sum().item()), "launches": [list(x) for x in r.bounds],
                     "ray_steps": acc, "rejected": rej, "attempts": acc + rej, "heaviest_ray_attempts": int(att.max().item()),
                     "ray_steps_per_s": acc / med, "attempts_per_s": (acc + rej) / med, "per_launch": launches[b]}
    out["backward_over_forward_attempts_per_s"] = out["backward"]["attempts_per_s"] / out["forward"]["attempts_per_s"]
    # a launch cannot be shorter than its heaviest ray's chain of attempts: seconds per attempt of that chain
    for name in ("forward", "backward"):
        out[name]["s_per_attempt_of_the_heaviest_ray"] = out[name]["median_s"] / out[name]["heaviest_ray_attempts"]
    return out


def footprint(repeats):
    from density import DensitySpec
    from wr import WR
    bs, _ = bench.make_bs("nonzonal")
    nnx, nny, zwn, days = 21, 11, np.arange(1.0, 8.0), 30

    def run():
        w = WR(len(zwn), nnx * nny, 7200.0, days * 86400.0, 0.0, nx=bs.nlon, ny=bs.nlat, backward=True)
        w.bs = bs
        w.set_zwn(zwn)
        w.set_source_matrix(100.0, 20.0, 2.0, 2.0, nnx, nny)           # the receptor box
        with np.errstate(all="ignore"):
            return w, w.ray_density(DensitySpec(144, 72))

    run()
    ts = []
    for _ in range(repeats):
        t, (w, dmap) = timed(run)
        ts.append(t)
    count = dmap.count[0].cpu().numpy()
    lat = -90.0 + (np.arange(72) + 0.5) * 2.5
    lon = (np.arange(144) + 0.5) * 2.5
    iy, ix = np.unravel_index(np.argsort(count, axis=None)[::-1][:5], count.shape)
    res = w.last_run
    return {"state": "nonzonal", "receptors": nnx * nny, "box": "100-140E 20-40N", "zwn": zwn.tolist(), "days": days,
            "slots": 3 * nnx * nny * len(zwn), "live_rays": int(res.n_live), "ray_steps": int(res.ray_steps),
            "map": "144 x 72", "s": ts, "median_s": statistics.median(ts), "points_counted": int(count.sum()),
            "cells_reached": int((count > 0).sum()),
            "share_of_points_outside_the_box": float(1.0 - count[np.ix_((lat >= 20) & (lat <= 40),
                                                                      (lon >= 100) & (lon <= 140))].sum() / count.sum()),
            "densest_cells_lon_lat_count": [[float(lon[i]), float(lat[j]), int(count[j, i])] for j, i in zip(iy, ix)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=float, default=90.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--footprint", action="store_true", help="the receptor-footprint example only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/backward_rate.py measures on the GPU: no HIP device visible")
    out = {"device": torch.cuda.get_device_name(0), "library": _hip.version()}
    if a.footprint:
        out["footprint"] = footprint(a.repeats)
    else:
        out["c3"] = [rate(kind, a.days, a.repeats) for kind in ("zonal", "nonzonal")]
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
