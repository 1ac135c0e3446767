"""What a ray-density map costs on top of the ray loop: the C3 ray set through
``RayEngine.integrate`` on one GPU, alternately with no consumer (``sink=None,
out=None``: the row blocks are written and dropped) and with a
``density.DensitySink`` binning them on the device -- counts only, then with
the amplitude sum.  Three interleaved pairs per variant.

    python tools/density_rate.py [--days 90] [--nx 1440 --ny 720] [--pairs 3] [--out FILE.json]

Reports per variant the added time per run and per launch, the binning
kernel's own time (HIP events around each ``rwrt_ray_density`` call; under
``rocprofv3 --kernel-trace --stats -- python tools/density_rate.py ..`` the
trace's ``ray_density_kernel`` row gives the same), the equal-bin runs the
kernel turned into atomics (counted here from the row blocks with torch, by
the same index formula in torch's arithmetic: a count, not a parity check)
and the two floors the kernel time is read against:

  rows    row bytes the kernel fetches (live rays x rows x 64 B) / HBM peak;
  atomics atomics issued / the scattered float-atomic rate of the MI355X
          (64 lanes into 64 different rows: 0.08 TB/s of 4-byte adds = 2e10
          atomics/s; 8-byte integer and fp64 adds are unmeasured there).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rossby-wave-ray-tracing_amd")]
import torch  # noqa: E402
import bench  # noqa: E402
from density import DensityMap, DensitySink, DensitySpec  # noqa: E402
from engine import RayEngine  # noqa: E402

HBM_PEAK = 8.0e12          # B/s (MI355X, HBM3E)
ATOMIC_RATE = 0.08e12 / 4  # scattered 4-byte float adds per second


class TimedSink(DensitySink):
    """DensitySink with a pair of events around every binning call and, when
    asked, a count of the equal-bin runs of the launch (atomics issued)."""

    def __init__(self, map, count_runs=False):
        super().__init__(map)
        self.events, self.runs, self.rows_read, self.count_runs = [], 0, 0, count_runs

    def __call__(self, i0, i1, view, tails=None, slots=None):
        s = torch.cuda.current_stream(view.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        super().__call__(i0, i1, view, tails, slots)
        e1.record(s)
        self.events.append((e0, e1))
        if self.count_runs:
            sp = self.map.spec
            n = int(slots.n_dev.item()) if slots is not None else view.shape[0]
            for a in range(0, n, 65536):
                v = view[a:min(a + 65536, n)]
                lam = torch.remainder(v[..., 0], 2 * math.pi)
                b = torch.floor(lam * sp.inv_dlon) + sp.nx * torch.floor((v[..., 1] - sp.lat0) * sp.inv_dlat)
                b = torch.nan_to_num(b, nan=-1.0)
                self.runs += int((b[:, 1:] != b[:, :-1]).sum().item()) + int((b[:, 0] >= 0).sum().item())
            self.rows_read += n * (i1 - i0)
            if tails is not None:
                self.runs += int(((tails.frm < i1) & ~torch.isnan(tails.row[:, 0])).sum().item())

    def kernel_ms(self):
        return [a.elapsed_time(b) for a, b in self.events]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=float, default=90.0)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--ny", type=int, default=720)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bs, _ = bench.make_bs("zonal")
    y0 = torch.as_tensor(bench.c3_initial_state(bs), device="cuda")
    eng = RayEngine.from_bs(bs)
    nt = int(round(a.days * 12)) + 1
    kw = dict(ttotal=(nt - 1) * 7200.0, first_chunk=[24, 160], team=[64, 64, 64])

    def run(sink):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eng.integrate(y0, nt, 7200.0, sink=sink, out=None, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    _, res = run(None)                                  # warm-up
    launches = len(res.bounds)
    n_live = int((~torch.isnan(y0.sum(0))).sum().item())
    rec = {"workload": f"C3 zonal, {a.days:g} d at 2 h, RayEngine.integrate first_chunk 24+160, team 64",
           "slots": int(y0.shape[1]), "live": n_live, "rows": nt - 1, "launches": launches,
           "ray_steps": res.ray_steps, "map": [a.nx, a.ny], "device": torch.cuda.get_device_name(0),
           "hbm_peak_Bps": HBM_PEAK, "scattered_atomic_rate_per_s": ATOMIC_RATE, "variants": {}}
    for weight in (None, "amp"):
        spec = DensitySpec(a.nx, a.ny, weight=weight)
        counter = TimedSink(DensityMap(spec, "cuda"), count_runs=True)
        run(counter)                                    # (untimed: counts the runs, warms the kernel)
        base, dens, kern = [], [], []
        for _ in range(a.pairs):
            base.append(run(None)[0])
            sink = TimedSink(DensityMap(spec, "cuda"))
            dens.append(run(sink)[0])
            kern.append(sum(sink.kernel_ms()) / 1e3)
        points = int(sink.map.count.sum().item())
        row_bytes = counter.rows_read * 64
        floors = {"rows_s": row_bytes / HBM_PEAK, "atomics_s": counter.runs * (2 if weight else 1) / ATOMIC_RATE}
        k = min(kern)
        rec["variants"]["counts" if weight is None else "counts+amp"] = {
            "baseline_s": base, "with_sink_s": dens, "kernel_s": kern,
            "added_s_per_run": min(dens) - min(base), "added_s_per_launch": (min(dens) - min(base)) / launches,
            "kernel_s_per_launch": k / launches, "points_binned": points, "rows_read": counter.rows_read,
            "row_bytes": row_bytes, "runs": counter.runs, "atomics": counter.runs * (2 if weight else 1),
            "rows_per_run": counter.rows_read / max(counter.runs, 1), "floors": floors,
            "kernel_over_larger_floor": k / max(floors.values()),
            "ray_steps_per_s": {"baseline": res.ray_steps / min(base), "with_sink": res.ray_steps / min(dens)}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
