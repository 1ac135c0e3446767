"""What a gate-crossing map costs on top of the ray loop: the C3 ray set through
``RayEngine.integrate`` on one GPU, in one session and interleaved,

  none       no consumer (``sink=None, out=None``: the row blocks are written and dropped);
  summary    a ``summary.SummarySink`` with one region (it reads the same rows once, no atomics);
  cross_1    a ``cross.CrossSink`` with one gate, the latitude circle 30 N;
  cross_8    a ``cross.CrossSink`` with eight gates, four latitude circles and four meridians;
  track      a ``track.TrackSink`` on 360 x 180 (about 20 deposits per segment);

the crossing maps with 360 bins, no window, no weight and the per-ray arrays.

    python tools/cross_rate.py [--days 90] [--rounds 3] [--out FILE.json]

Reports per variant every round's wall time, the added time per run (best of
``--rounds`` minus the best bare run, and the median of the same-round
differences), the reducing kernels' own time (HIP events around each call),
and for the crossing maps the crossings found -- each is one 64-bit integer
atomic and one fp64 atomic -- next to the segments the track map deposited.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rossby-wave-ray-tracing_amd")
sys.path[:0] = [ROOT, PKG]
import torch  # noqa: E402
import bench  # noqa: E402
from cross import CrossMap, CrossSink, CrossSpec, Gate  # noqa: E402
from engine import RayEngine  # noqa: E402
from summary import RaySummary, SummarySink  # noqa: E402
from track import TrackMap, TrackSink, TrackSpec  # noqa: E402

REGION = (350.0, 20.0, 20.0, 60.0)
GATES = (Gate.lat(30.0), Gate.lon(180.0), Gate.lat(0.0), Gate.lon(0.0), Gate.lat(-30.0), Gate.lon(90.0),
         Gate.lat(60.0), Gate.lon(270.0))


class Timed:
    """A sink with a pair of events around every call of ``sink``."""
    takes_tails = True
    takes_slots = True

    def __init__(self, sink, target):
        self.sink, self.target, self.events = sink, target, []

    def __call__(self, i0, i1, view, tails=None, slots=None):
        s = torch.cuda.current_stream(view.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        self.sink(i0, i1, view, tails, slots)
        e1.record(s)
        self.events.append((e0, e1))

    def kernel_s(self):
        return sum(a.elapsed_time(b) for a, b in self.events) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=float, default=90.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bs, _ = bench.make_bs("zonal")
    y0_host = bench.c3_initial_state(bs)
    y0 = torch.as_tensor(y0_host, device="cuda")
    eng = RayEngine.from_bs(bs)
    nt = int(round(a.days * 12)) + 1
    nray = int(y0.shape[1])
    kw = dict(ttotal=(nt - 1) * 7200.0, first_chunk=[24, 160], team=[64, 64, 64])

    def run(sink):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eng.integrate(y0, nt, 7200.0, sink=sink, out=None, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    def make(name):
        # row 0: lon, lat, l and the amplitude of the initial state y = lon lat k l amp
        if name == "none":
            return None
        if name == "summary":
            rs = RaySummary(nray, [REGION], "cuda")
            rs.start(y0_host[0], y0_host[1], y0_host[3], y0_host[4])
            return Timed(SummarySink(rs), rs)
        if name == "track":
            m = TrackMap(TrackSpec(360, 180), nray, "cuda").start(y0[0], y0[1], y0[4])
            return Timed(TrackSink(m), m)
        m = CrossMap(CrossSpec(GATES[:int(name.split("_")[1])], 360), nray, "cuda").start(y0[0], y0[1], y0[4])
        return Timed(CrossSink(m), m)

    names = ("none", "summary", "cross_1", "cross_8", "track")
    for name in names:                                  # warm-up: every kernel once
        _, res = run(make(name))
    n_live = int((~torch.isnan(y0.sum(0))).sum().item())
    rec = {"workload": f"C3 zonal, {a.days:g} d at 2 h, RayEngine.integrate first_chunk 24+160, team 64",
           "slots": nray, "live": n_live, "rows": nt - 1, "launches": len(res.bounds), "ray_steps": res.ray_steps,
           "device": torch.cuda.get_device_name(0), "gates": [[g.kind, g.deg] for g in GATES], "bins": 360,
           "order": f"{a.rounds} rounds x ({', '.join(names)}), interleaved, after one untimed run each",
           "variants": {}}
    wall = {n: [] for n in names}
    kern = {n: [] for n in names[1:]}
    totals = {}
    for _ in range(a.rounds):
        for name in names:
            sink = make(name)
            wall[name].append(run(sink)[0])
            if sink is None:
                continue
            kern[name].append(sink.kernel_s())
            m = sink.target
            if name.startswith("cross"):
                totals[name] = {"crossings": int(m.ncross.sum().item()), "in_the_map": int(m.cnt.sum().item()),
                                "dropped": int(m.dropped.item()),
                                "per_gate_and_direction": m.ncross.sum(dim=2).tolist(),
                                "rays_that_crossed_gate_0": int(m.crossed(0).sum().item())}
            elif name == "track":
                totals[name] = {"segments": float(m.time.sum().item()), "cells": int(m.cnt.sum().item()),
                                "dropped": int(m.dropped.item())}
    base = min(wall["none"])
    rec["variants"]["none"] = {"wall_s": wall["none"]}
    for name in names[1:]:
        same_round = [w - b for w, b in zip(wall[name], wall["none"])]
        v = {"wall_s": wall[name], "kernel_s": kern[name], "added_s_per_run": min(wall[name]) - base,
             "added_same_round_s": same_round, "added_same_round_median_s": statistics.median(same_round),
             "kernel_s_min": min(kern[name])}
        v.update(totals.get(name, {}))
        rec["variants"][name] = v
    k = {n: rec["variants"][n]["kernel_s_min"] for n in names[1:]}
    rec["cross_1_over_summary_kernel"] = k["cross_1"] / k["summary"]
    rec["cross_8_over_summary_kernel"] = k["cross_8"] / k["summary"]
    rec["track_over_cross_8_kernel"] = k["track"] / k["cross_8"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
