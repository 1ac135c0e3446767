"""What a member stack buys and what it costs, on one GPU.

    python tools/stack_rate.py [--members 32] [--days 90] [--repeats 5] [--out FILE.json]

(a) The stack against the loop it replaces: ``--members`` members
(``synthetic.background_level(j)``, 2.5 degrees) x the C2 sources (3 072 slots
each), ``--days`` days, no sink.  One ``integrate`` of a member-stack engine
(``RayEngine.from_levels(levels, members=True)``) against the sum of one
static ``integrate`` per member (``RayEngine.from_packed(levels.packed[m])``,
this build's static engine), alternating per repeat, each timed by a host
clock around work that ends in a device synchronise.  With it, from the
counters: every member's heaviest ray (accepted + rejected attempts: the
sequential chain a launch cannot be shorter than), all attempts, and the share
of the persistent grid's lanes (256 CUs x 256) the attempts would fill if the
launch lasted exactly its heaviest chain.

(b) The cost of the stack path: the C3 zonal rays dealt round-robin over 4
copies of the zonal state against the static engine on the same rays -- once as
shipped, once with the drain-time hand-off off (``handoff = 0``) and
``team=0``, which is what a stack launch has.  Ray-steps per second of each.

Every result is checked: the stack's counters equal the static engines'.
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
import synthetic as S  # noqa: E402
from engine import RayEngine  # noqa: E402
from levels import Levels  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def stack_vs_loop(nmember, days, repeats, first_chunk):
    bgs = [S.background_level(j) for j in range(nmember)]
    lv = Levels(bgs[0]["lat"], bgs[0]["lon"], nmember)
    lv.set_levels(np.stack([b["u"] for b in bgs]), np.stack([b["v"] for b in bgs]))
    cfg = S.config("C2")
    deg = np.pi / 180.0
    ix, iy = np.meshgrid(np.arange(cfg.nnx), np.arange(cfg.nny))
    slon = ((cfg.SW_lon + ix.ravel() * cfg.dlon) % 360.0) * deg
    slat = (cfg.SW_lat + iy.ravel() * cfg.dlat) * deg
    es = RayEngine.from_levels(lv, members=True)
    statics = [RayEngine.from_packed(lv.packed[m], lv.lon, lv.lat) for m in range(nmember)]
    rows0 = es.initial_rows(slon, slat, cfg.zwn, 0.0)                      # [nmember, 7, 3, ns, nz]
    nslot = cfg.nray
    y0 = [rows0[m, :5].reshape(5, nslot).contiguous() for m in range(nmember)]
    y0_all = torch.cat(y0, dim=1).contiguous()
    member = torch.arange(nmember).repeat_interleave(nslot)
    nt = int(round(days * 12)) + 1
    kw = dict(ttotal=(nt - 1) * 7200.0, order_policy="priority", first_chunk=first_chunk)

    def run_stack():
        return es.integrate(y0_all, nt, 7200.0, member=member, **kw)

    def run_loop():
        return [e.integrate(y, nt, 7200.0, **kw) for e, y in zip(statics, y0)]

    run_stack(), run_loop()                                                 # warm-up: every shape timed below
    t_stack, t_loop = [], []
    for _ in range(repeats):
        ts, rs = timed(run_stack)
        tl, rl = timed(run_loop)
        t_stack.append(ts)
        t_loop.append(tl)
    log = list(es.launch_log)
    att_s = (rs.nacc + rs.nrej).cpu().numpy().reshape(nmember, nslot)
    att_l = np.stack([(r.nacc + r.nrej).cpu().numpy() for r in rl])
    same = bool(np.array_equal(att_s, att_l)) and all(
        np.array_equal(rs.nanrow.cpu().numpy().reshape(nmember, nslot)[m], rl[m].nanrow.cpu().numpy())
        for m in range(nmember))
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 256
    chain = att_s.max(axis=1)
    out = {
        "first_chunk": first_chunk, "members": nmember, "slots": int(nmember * nslot), "days": days, "rows": nt,
        "live_rays": int(sum(r.n_live for r in rl)),
        "stack_s": t_stack, "loop_s": t_loop,
        "stack_median_s": statistics.median(t_stack), "loop_median_s": statistics.median(t_loop),
        "loop_over_stack": statistics.median(t_loop) / statistics.median(t_stack),
        "ray_steps": int(rs.nacc.sum().item()),
        "stack_ray_steps_per_s": int(rs.nacc.sum().item()) / statistics.median(t_stack),
        "loop_ray_steps_per_s": int(rs.nacc.sum().item()) / statistics.median(t_loop),
        "counters_equal_static": same,
        "heaviest_chain_attempts_per_member": chain.tolist(),
        "heaviest_chain_attempts": int(chain.max()), "sum_of_member_chains": int(chain.sum()),
        "attempts_total": int(att_s.sum()),
        "lanes": int(lanes),
        # the share of the lanes busy if a launch lasted exactly its heaviest chain
        "occupancy_stack_at_chain": float(att_s.sum() / (chain.max() * lanes)),
        "occupancy_loop_at_chain": float(att_s.sum() / (chain.sum() * lanes)),
        "stack_launch_log": log,
    }
    return out


def stack_cost(days, repeats):
    bs, bg = bench.make_bs("zonal")
    y0 = torch.as_tensor(bench.c3_initial_state(bs), device="cuda")
    nray = y0.shape[1]
    lv = Levels(bg["lat"], bg["lon"], 4)
    lv.set_levels(np.stack([bg["u"]] * 4), np.stack([bg["v"]] * 4))
    es = RayEngine.from_levels(lv, members=True)
    shipped = RayEngine.from_packed(lv.packed[0], lv.lon, lv.lat)
    plain = RayEngine.from_packed(lv.packed[0], lv.lon, lv.lat)
    plain.handoff = 0
    member = torch.arange(nray) % 4
    nt = int(round(days * 12)) + 1
    kw = dict(ttotal=(nt - 1) * 7200.0, order_policy="priority", first_chunk=[24, 96])
    runs = {"stack": lambda: es.integrate(y0, nt, 7200.0, member=member, **kw),
            "static_as_shipped": lambda: shipped.integrate(y0, nt, 7200.0, **kw),
            "static_no_handoff_team0": lambda: plain.integrate(y0, nt, 7200.0, team=0, **kw)}
    res, times = {}, {k: [] for k in runs}
    for k, fn in runs.items():
        fn()                                                                # warm-up
    for _ in range(repeats):
        for k, fn in runs.items():
            t, res[k] = timed(fn)
            times[k].append(t)
    steps = int(res["stack"].nacc.sum().item())
    same = all(bool(torch.equal(res["stack"].nacc, res[k].nacc)) and bool(torch.equal(res["stack"].nrej, res[k].nrej))
               and bool(torch.equal(res["stack"].nanrow, res[k].nanrow)) for k in runs)
    out = {"rays": int(nray), "live_rays": int(res["stack"].n_live), "days": days, "rows": nt, "ray_steps": steps,
           "counters_equal_static": same, "handoffs_as_shipped": shipped.handoffs()}
    for k in runs:
        med = statistics.median(times[k])
        out[k] = {"s": times[k], "median_s": med, "ray_steps_per_s": steps / med}
    out["stack_over_static_as_shipped"] = out["stack"]["median_s"] / out["static_as_shipped"]["median_s"]
    out["stack_over_static_no_handoff_team0"] = out["stack"]["median_s"] / out["static_no_handoff_team0"]["median_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=32)
    ap.add_argument("--days", type=float, default=90.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-cost", action="store_true", help="measurement (a) only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/stack_rate.py measures on the GPU: no HIP device visible")
    out = {"device": torch.cuda.get_device_name(0), "library": _hip.version(),
           # the same integrate() arguments on both sides: its defaults (one launch), and two leading launches
           "a_stack_vs_loop": stack_vs_loop(a.members, a.days, a.repeats, None),
           "a_stack_vs_loop_lead_24_96": stack_vs_loop(a.members, a.days, a.repeats, [24, 96])}
    if not a.skip_cost:
        out["b_stack_cost_c3"] = stack_cost(a.days, a.repeats)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
