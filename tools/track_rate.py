"""What a residence-time map along ray segments costs on top of the ray loop:
the C3 ray set through ``RayEngine.integrate`` on one GPU, in one session and
interleaved,

  none        no consumer (``sink=None, out=None``: the row blocks are written and dropped);
  density_*   a ``density.DensitySink`` counting the rows' points on the same map;
  track_*     a ``track.TrackSink`` depositing the segments, without a weight;
  track_*_w   the same with ``weight='amp'`` (a third atomic per flush);

on 360 x 180 and on 1440 x 720.

    python tools/track_rate.py [--days 90] [--rounds 3] [--out FILE.json]

Reports per variant the added time per run (best of ``--rounds``), the
reducing kernels' own time (HIP events around each call), and for the track
maps the segments deposited (the map's time), the cells (its visits) and the
flushes -- the runs the kernel turned into atomics.  The flushes are counted by
the A/B build ``librwrt_trackcount.so`` (``make -C .../csrc variant
NAME=trackcount DEFS="-DRWRT_TRACK_COUNT_FLUSHES=1"``) in an untimed run; null
when that build is absent.  The density kernel's runs are counted as
tools/flux_rate.py counts them, from the row blocks with torch.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rossby-wave-ray-tracing_amd")
sys.path[:0] = [ROOT, PKG]
import torch  # noqa: E402
import bench  # noqa: E402
import _hip as H  # noqa: E402
from density import DensityMap, DensitySink, DensitySpec  # noqa: E402
from engine import RayEngine  # noqa: E402
from track import TrackMap, TrackSink, TrackSpec  # noqa: E402


class Timed:
    """A sink with a pair of events around every call of ``sink`` and, when
    ``bins`` (a DensitySpec) is given, a count of the equal-bin runs of the
    launch's rows."""
    takes_tails = True
    takes_slots = True

    def __init__(self, sink, bins=None):
        self.sink, self.bins = sink, bins
        self.events, self.runs = [], 0

    def __call__(self, i0, i1, view, tails=None, slots=None):
        s = torch.cuda.current_stream(view.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        self.sink(i0, i1, view, tails, slots)
        e1.record(s)
        self.events.append((e0, e1))
        if self.bins is not None:
            sp = self.bins
            n = int(slots.n_dev.item()) if slots is not None else view.shape[0]
            for a in range(0, n, 65536):
                v = view[a:min(a + 65536, n)]
                fx = torch.floor(torch.remainder(v[..., 0], 2 * math.pi) * sp.inv_dlon)
                b = torch.nan_to_num(fx + sp.nx * torch.floor((v[..., 1] - sp.lat0) * sp.inv_dlat), nan=-1.0)
                self.runs += int(((b[:, 1:] != b[:, :-1]) & (b[:, 1:] >= 0)).sum().item())
                self.runs += int((b[:, 0] >= 0).sum().item())
            if tails is not None:
                self.runs += int(((tails.frm < i1) & ~torch.isnan(tails.row[:, 0])).sum().item())

    def kernel_s(self):
        return sum(a.elapsed_time(b) for a, b in self.events) / 1e3


def counting_library():
    """The A/B build whose ``d_dropped`` receives the flushes, or None."""
    path = os.path.join(PKG, "librwrt_trackcount.so")
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    ours = H.load()
    lib.rwrt_ray_track.argtypes = ours.rwrt_ray_track.argtypes
    lib.rwrt_ray_track.restype = ctypes.c_int
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=float, default=90.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bs, _ = bench.make_bs("zonal")
    y0 = torch.as_tensor(bench.c3_initial_state(bs), device="cuda")
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

    maps = {"360": (360, 180), "1440": (1440, 720)}
    specs = {}
    for tag, (nx, ny) in maps.items():
        specs["density_" + tag] = DensitySpec(nx, ny)
        specs["track_" + tag] = TrackSpec(nx, ny)
        specs["track_" + tag + "_w"] = TrackSpec(nx, ny, weight="amp")
    names = ("none",) + tuple(specs)

    def track_map(spec, lib=None):
        m = TrackMap(spec, nray, "cuda")
        if lib is not None:
            m._lib = lib
        # row 0: lon, lat and the amplitude of the initial state (rows 0, 1, 4)
        return m.start(y0[0], y0[1], y0[4], y0[4] if spec.wcol >= 0 else None)

    def make(name, count=False):
        if name == "none":
            return None
        spec = specs[name]
        if name.startswith("density"):
            return Timed(DensitySink(DensityMap(spec, "cuda")), spec if count else None)
        return Timed(TrackSink(track_map(spec)))

    _, res = run(None)                                  # warm-up
    n_live = int((~torch.isnan(y0.sum(0))).sum().item())
    rec = {"workload": f"C3 zonal, {a.days:g} d at 2 h, RayEngine.integrate first_chunk 24+160, team 64",
           "slots": nray, "live": n_live, "rows": nt - 1, "launches": len(res.bounds), "ray_steps": res.ray_steps,
           "device": torch.cuda.get_device_name(0),
           "order": f"{a.rounds} rounds x ({', '.join(names)}), interleaved, after one untimed run each",
           "variants": {}}
    counted, flushes = {}, {}
    lib = counting_library()
    for name in names[1:]:                              # (untimed: warms the kernels, counts the runs)
        sink = make(name, count=True)
        run(sink)
        counted[name] = sink
        if name.startswith("track") and lib is not None:
            m = track_map(specs[name], lib)
            run(TrackSink(m))
            flushes[name] = int(m.dropped.item())
    wall = {n: [] for n in names}
    kern = {n: [] for n in names[1:]}
    totals = {}
    for _ in range(a.rounds):
        for name in names:
            sink = make(name)
            wall[name].append(run(sink)[0])
            if sink is not None:
                kern[name].append(sink.kernel_s())
                if name.startswith("track"):
                    m = sink.sink.map
                    totals[name] = (float(m.time.sum().item()), int(m.cnt.sum().item()), int(m.dropped.item()))
    base = min(wall["none"])
    rec["variants"]["none"] = {"wall_s": wall["none"]}
    for name in names[1:]:
        v = {"wall_s": wall[name], "kernel_s": kern[name], "added_s_per_run": min(wall[name]) - base,
             "kernel_s_min": min(kern[name])}
        if name.startswith("density"):
            runs = counted[name].runs
            v.update(runs=runs, runs_per_s=runs / v["kernel_s_min"])
        else:
            seg, cells, dropped = totals[name]
            f = flushes.get(name)
            v.update(segments=seg, cells=cells, dropped=dropped, cells_per_segment=cells / max(seg, 1.0),
                     flushes=f, flushes_per_s=None if f is None else f / v["kernel_s_min"],
                     atomics_per_flush=3 if specs[name].wcol >= 0 else 2)
        rec["variants"][name] = v
    for tag in maps:
        d, t = rec["variants"]["density_" + tag], rec["variants"]["track_" + tag]
        rec["track_over_density_kernel_" + tag] = t["kernel_s_min"] / d["kernel_s_min"]
        if t["flushes_per_s"] is not None:
            rec["s_per_flush_over_s_per_run_" + tag] = d["runs_per_s"] / t["flushes_per_s"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
