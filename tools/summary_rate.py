"""What a per-ray path summary costs on top of the ray loop: the C3 ray set
through ``RayEngine.integrate`` on one GPU, interleaved per repeat in this
order -- no consumer (``sink=None, out=None``: the row blocks are written and
dropped), a ``density.DensitySink`` (counts only: the yardstick, it reads the
same rows in the same pattern), a ``summary.SummarySink``, and a ``Tee`` of
both.

    python tools/summary_rate.py [--days 90] [--nx 1440 --ny 720] [--nreg 1] [--repeats 5] [--out FILE.json]

Reports per variant every repeat's wall time, the added time per run
(median over the repeats of the same-repeat difference to the bare run, with
the spread), the sink kernels' own time (HIP events around each call; under
``rocprofv3 --kernel-trace --stats -- python tools/summary_rate.py ..`` the
trace's ``ray_summary_kernel`` row gives the same) and the effective row
bytes per second: the row bytes the kernel's lanes ask for (rows read x 64 B
-- a lane uses 48 of a row's 64 bytes, the sectors fetched are the whole
row) over the kernel time.  It ends with the summary's agreement figures on
this run: totals of the integer fields and the largest path.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rossby-wave-ray-tracing_amd")]
import torch  # noqa: E402
import bench  # noqa: E402
from density import DensityMap, DensitySink, DensitySpec  # noqa: E402
from engine import RayEngine  # noqa: E402
from summary import RaySummary, SummarySink, Tee  # noqa: E402

HBM_PEAK = 8.0e12          # B/s (MI355X, HBM3E)
REGIONS = [(350.0, 20.0, 20.0, 60.0), (160.0, 220.0, 20.0, 60.0), (150.0, 160.0, 30.0, 50.0),
           (0.0, 360.0, -90.0, 0.0), (200.0, 300.0, -30.0, 30.0), (60.0, 90.0, 0.0, 90.0),
           (100.0, 120.0, 15.0, 30.0), (180.0, 100.0, -90.0, 0.0)]


class Timed:
    """A sink with a pair of events around every call of the wrapped sink."""
    takes_tails = True
    takes_slots = True

    def __init__(self, sink):
        self.sink, self.events, self.rows_read = sink, [], 0

    def __call__(self, i0, i1, view, tails=None, slots=None):
        s = torch.cuda.current_stream(view.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        self.sink(i0, i1, view, tails, slots)
        e1.record(s)
        # (row blocks: the live rays of the launch, read from the device after the runs)
        n = slots.n_dev.clone() if slots is not None else view.shape[0]
        self.events.append((e0, e1, n, i1 - i0))

    def kernel_s(self):
        return sum(a.elapsed_time(b) for a, b, _, _ in self.events) / 1e3

    def row_bytes(self):
        """Upper bound of the rows read: every block's rows (a ray frozen
        within the launch reads fewer)."""
        return sum(int(n) * r for _, _, n, r in self.events) * 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=float, default=90.0)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--ny", type=int, default=720)
    ap.add_argument("--nreg", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bs, _ = bench.make_bs("zonal")
    y0_host = bench.c3_initial_state(bs)
    y0 = torch.as_tensor(y0_host, device="cuda")
    eng = RayEngine.from_bs(bs)
    nt = int(round(a.days * 12)) + 1
    nray = int(y0.shape[1])
    kw = dict(ttotal=(nt - 1) * 7200.0, first_chunk=[24, 160], team=[64, 64, 64])
    spec = DensitySpec(a.nx, a.ny)
    regions = REGIONS[:a.nreg]

    def new_summary():
        rs = RaySummary(nray, regions, "cuda")
        # (row 0: position, l and amplitude of the initial state y = lon lat k l amp)
        rs.start(y0_host[0], y0_host[1], y0_host[3], y0_host[4])
        return rs

    def make(variant):
        if variant == "none":
            return None, None
        if variant == "density":
            return Timed(DensitySink(DensityMap(spec, "cuda"))), None
        rs = new_summary()
        if variant == "summary":
            return Timed(SummarySink(rs)), rs
        return Timed(Tee(DensitySink(DensityMap(spec, "cuda")), SummarySink(rs))), rs

    def run(sink):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eng.integrate(y0, nt, 7200.0, sink=sink, out=None, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    variants = ("none", "density", "summary", "tee")
    for v in variants:                                   # warm-up: every kernel once
        _, res = run(make(v)[0])
    launches = len(res.bounds)
    n_live = int((~torch.isnan(y0.sum(0))).sum().item())
    wall = {v: [] for v in variants}
    kern = {v: [] for v in variants}
    rbytes, last = {}, None
    for _ in range(a.repeats):
        for v in variants:
            sink, rs = make(v)
            wall[v].append(run(sink)[0])
            if sink is not None:
                kern[v].append(sink.kernel_s())
                rbytes[v] = sink.row_bytes()
            if v == "summary":
                last = rs
    rec = {"workload": f"C3 zonal, {a.days:g} d at 2 h, RayEngine.integrate first_chunk 24+160, team 64",
           "slots": nray, "live": n_live, "rows": nt - 1, "launches": launches, "ray_steps": res.ray_steps,
           "map": [a.nx, a.ny], "regions": regions, "repeats": a.repeats, "order": list(variants),
           "device": torch.cuda.get_device_name(0), "hbm_peak_Bps": HBM_PEAK, "variants": {}}
    for v in variants:
        d = {"wall_s": wall[v], "wall_median_s": statistics.median(wall[v])}
        if v != "none":
            added = [w - b for w, b in zip(wall[v], wall["none"])]
            k = statistics.median(kern[v])
            d.update(added_s=added, added_median_s=statistics.median(added), added_min_s=min(added),
                     added_max_s=max(added), kernel_s=kern[v], kernel_median_s=k,
                     kernel_s_per_launch=k / launches, row_bytes=rbytes[v],
                     row_bytes_per_s=rbytes[v] / k, fraction_of_hbm_peak=rbytes[v] / k / HBM_PEAK)
        rec["variants"][v] = d
    dk, sk = rec["variants"]["density"]["kernel_median_s"], rec["variants"]["summary"]["kernel_median_s"]
    rec["summary_over_density_kernel"] = sk / dk
    s = last.numpy()
    rec["summary_totals"] = {"n_valid": int(s["n_valid"].astype("int64").sum()),
                             "n_turn": int(s["n_turn"].astype("int64").sum()),
                             "path_max_rad": float(s["path"].max()),
                             "rays_reaching_region": [int((f >= 0).sum()) for f in s["first_row"]]}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
