"""What a wave-ray flux map costs on top of the ray loop: the C3 ray set
through ``RayEngine.integrate`` on one GPU, in one session and interleaved,

  none      no consumer (``sink=None, out=None``: the row blocks are written and dropped);
  flux      a ``flux.FluxSink`` reducing them on the device, on the wrapped
            1440 x 720 map and on 4320 x 720 over three circles;
  pair      ``Tee(DensitySink(weight='ug'), DensitySink(weight='vg'))`` on the
            wrapped map -- how the two vector sums are obtained without
            ``rwrt_ray_flux``: each row read twice, two counts, two sums.

    python tools/flux_rate.py [--days 90] [--nx 1440 --ny 720] [--pairs 3] [--through] [--out FILE.json]

Reports per variant the added time per run, the reducing kernels' own time
(HIP events around each call) and, for the flux maps, the equal-bin runs the
kernel turned into atomics (counted here from the row blocks with torch, by
the same index formula in torch's arithmetic: a count, not a parity check).
``--through`` adds the two-pass run of ``WR.ray_flux(through=...)``'s pattern:
a ``SummarySink`` integration with one region, the selection, and the flux
integration of the selected rays.
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
from flux import FluxMap, FluxSink, FluxSpec, select_through  # noqa: E402
from summary import RaySummary, SummarySink, Tee  # noqa: E402


class Timed:
    """A sink with a pair of events around every call of ``sink`` and, when
    ``spec`` is given, a count of the equal-bin runs of the launch."""
    takes_tails = True
    takes_slots = True

    def __init__(self, sink, spec=None):
        self.sink, self.spec = sink, spec
        self.events, self.runs, self.rows_read = [], 0, 0

    def __call__(self, i0, i1, view, tails=None, slots=None):
        s = torch.cuda.current_stream(view.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        self.sink(i0, i1, view, tails, slots)
        e1.record(s)
        self.events.append((e0, e1))
        if self.spec is not None:
            sp = self.spec
            n = int(slots.n_dev.item()) if slots is not None else view.shape[0]
            for a in range(0, n, 65536):
                v = view[a:min(a + 65536, n)]
                lon = v[..., 0] - sp.lon0 if sp.unwrapped else torch.remainder(v[..., 0], 2 * math.pi)
                fx = torch.floor(lon * sp.inv_dlon)
                fx = torch.where((fx >= 0) & (fx < sp.nx), fx, torch.full_like(fx, math.nan))
                b = fx + sp.nx * torch.floor((v[..., 1] - sp.lat0) * sp.inv_dlat) + 0.0 * v[..., 5] + 0.0 * v[..., 6]
                b = torch.nan_to_num(b, nan=-1.0)
                self.runs += int(((b[:, 1:] != b[:, :-1]) & (b[:, 1:] >= 0)).sum().item())
                self.runs += int((b[:, 0] >= 0).sum().item())
            self.rows_read += n * (i1 - i0)
            if tails is not None:
                self.runs += int(((tails.frm < i1) & ~torch.isnan(tails.row[:, 0] + tails.row[:, 5])).sum().item())

    def kernel_s(self):
        return sum(a.elapsed_time(b) for a, b in self.events) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=float, default=90.0)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--ny", type=int, default=720)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--through", action="store_true")
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

    specs = {"flux_wrapped": FluxSpec(a.nx, a.ny),
             "flux_three_circles": FluxSpec(3 * a.nx, a.ny, lon_range=(-360.0, 720.0))}

    def make(name):
        if name == "none":
            return None
        if name == "pair":
            return Timed(Tee(DensitySink(DensityMap(DensitySpec(a.nx, a.ny, weight="ug"), "cuda")),
                             DensitySink(DensityMap(DensitySpec(a.nx, a.ny, weight="vg"), "cuda"))))
        return Timed(FluxSink(FluxMap(specs[name], "cuda")))

    _, res = run(None)                                  # warm-up
    n_live = int((~torch.isnan(y0.sum(0))).sum().item())
    rec = {"workload": f"C3 zonal, {a.days:g} d at 2 h, RayEngine.integrate first_chunk 24+160, team 64",
           "slots": int(y0.shape[1]), "live": n_live, "rows": nt - 1, "launches": len(res.bounds),
           "ray_steps": res.ray_steps, "map": [a.nx, a.ny], "device": torch.cuda.get_device_name(0),
           "order": "pairs x (none, flux_wrapped, flux_three_circles, pair), interleaved, after one untimed run each",
           "variants": {}}
    names = ("none", "flux_wrapped", "flux_three_circles", "pair")
    counted = {}
    for name in names[1:]:                              # (untimed: warms the kernels, counts the runs)
        sink = make(name)
        if name in specs:
            sink.spec = specs[name]
        run(sink)
        counted[name] = sink
    wall = {n: [] for n in names}
    kern = {n: [] for n in names[1:]}
    points = {}
    for _ in range(a.pairs):
        for name in names:
            sink = make(name)
            wall[name].append(run(sink)[0])
            if sink is not None:
                kern[name].append(sink.kernel_s())
                if name in specs:
                    points[name] = int(sink.sink.map.count.sum().item())
    base = min(wall["none"])
    rec["variants"]["none"] = {"wall_s": wall["none"]}
    for name in names[1:]:
        v = {"wall_s": wall[name], "kernel_s": kern[name], "added_s_per_run": min(wall[name]) - base,
             "kernel_s_min": min(kern[name])}
        if name in specs:
            c = counted[name]
            v.update(points=points[name], rows_read=c.rows_read, runs=c.runs, atomics=5 * c.runs,
                     runs_per_row=c.runs / max(c.rows_read, 1), rows_per_run=c.rows_read / max(c.runs, 1))
        rec["variants"][name] = v
    pair = rec["variants"]["pair"]["added_s_per_run"]
    rec["flux_added_over_pair_added"] = {n: rec["variants"][n]["added_s_per_run"] / pair for n in specs}
    if a.through:
        # the two passes of WR.ray_flux(through=[box]): summary with one region, selection, flux
        box = [(150.0, 210.0, 20.0, 60.0)]
        t = []
        for _ in range(a.pairs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rs = RaySummary(int(y0.shape[1]), box, "cuda").start(y0[0], y0[1], y0[3], y0[4])
            eng.integrate(y0, nt, 7200.0, sink=SummarySink(rs), out=None, **kw)
            sel = select_through(rs)
            chan = torch.where(sel, 0, -1).to(torch.int32)
            fm = FluxMap(specs["flux_wrapped"], "cuda")
            eng.integrate(y0, nt, 7200.0, sink=FluxSink(fm, chan), out=None, **kw)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        rec["through"] = {"box_deg": box[0], "total_s": t, "selected_rays": int(sel.sum().item()),
                          "points": int(fm.count.sum().item()), "over_one_flux_run": min(t) / min(wall["flux_wrapped"])}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
