"""What an arrival-time map costs on top of the ray loop: the C3 ray set through
``RayEngine.integrate`` on one GPU, in interleaved rounds of

  none          no consumer (``sink=None, out=None``: row blocks written and dropped)
  density       ``density.DensitySink``, counts only -- the yardstick, unchanged code
  arrival       ``arrival.ArrivalSink`` without windows (min and max only)
  arrival-W12   the same with one-day windows (min, max and a 64-bit add)

and, with ``--noskip-lib``, the two arrival variants again through a library
built with ``-DRWRT_ARRIVAL_SKIP=0`` (``make -C .../csrc variant NAME=noskip
DEFS=-DRWRT_ARRIVAL_SKIP=0``): every min and max atomic issued, none skipped
after a load.

    python tools/arrival_rate.py [--days 90] [--nx 1440 --ny 720] [--pairs 3]
                                 [--noskip-lib .../librwrt_noskip.so] [--out FILE.json]

Reports per variant the added time per run, the kernel's own time (HIP events
around each call) and the atomics its runs amount to, counted here from the
row blocks with torch by the same index formula in torch's arithmetic (a
count, not a parity check): ``runs`` bin runs give one atomic each in the
density kernel and min + max (+ add) in the arrival kernel, ``window_adds``
more adds where a run crosses a window bound.  With the skip the min and max
atomics actually issued are fewer by an amount that depends on timing; the
count is the no-skip one.  The measure a kernel time is read against is the
density kernel's atomics per second of the same session.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rossby-wave-ray-tracing_amd")]
import torch  # noqa: E402
import _hip as H  # noqa: E402
import bench  # noqa: E402
from arrival import ArrivalMap, ArrivalSink, ArrivalSpec  # noqa: E402
from density import DensityMap, DensitySink, DensitySpec  # noqa: E402
from engine import RayEngine  # noqa: E402
from launch_rows import row_args  # noqa: E402


class VariantMap(ArrivalMap):
    """ArrivalMap whose calls go to ``rwrt_ray_arrival`` of another build."""

    def __init__(self, spec, device, lib):
        super().__init__(spec, device)
        self.fn = lib.rwrt_ray_arrival

    def add_rows(self, i0, i1, view, tails=None, slots=None, chan=None):
        nray, rows = row_args(i0, i1, view, tails, slots)
        st = self.fn(self._c, nray, int(i0), int(i1), *rows, None, H.dptr(self.first, torch.int32),
                     H.dptr(self.last, torch.int32), H.dptr(self.count, torch.int64), H.stream(self.device))
        if st != H.RWRT_OK:
            raise H.RwrtError(f"variant rwrt_ray_arrival: status {st}")


def load_variant(path):
    lib = ctypes.CDLL(path)
    P, I32 = ctypes.c_void_p, ctypes.c_int32
    lib.rwrt_ray_arrival.argtypes = [ctypes.POINTER(H.ArrivalMap), ctypes.c_int64, I32, I32] + [P] * 9
    lib.rwrt_ray_arrival.restype = ctypes.c_int
    return lib


def count_runs(spec, window_rows, i0, i1, view, tails, slots, acc):
    """The bin runs of a launch and the adds where a run crosses a window
    bound, as csrc/arrival_rows.h forms them, into ``acc``."""
    dev = view.device
    nrow = i1 - i0
    col = spec.wcol if spec.wcol >= 0 else 0

    def bins(v):
        lam = torch.remainder(v[..., 0], 2 * math.pi)
        fy = torch.floor((v[..., 1] - spec.lat0) * spec.inv_dlat)
        b = torch.clamp(torch.floor(lam * spec.inv_dlon), max=spec.nx - 1) + spec.nx * fy
        ok = torch.isfinite(b) & (fy >= 0) & (fy < spec.ny)
        if spec.wcol >= 0:
            ok &= torch.isfinite(v[..., col])
        return torch.where(ok, b, torch.full_like(b, -1.0))

    def windows(a, b):     # windows touched by rows [a, b), b > a
        return 1 if not window_rows else (b - 1) // window_rows - a // window_rows + 1

    nray = int(slots.slot.numel()) if slots is not None else view.shape[0]
    if slots is not None:
        n = int(slots.n_dev.item())
        rays = torch.nonzero(slots.slot >= 0).reshape(-1)
        ray_of = torch.empty(n, dtype=torch.int64, device=dev)
        ray_of[slots.slot[rays].to(torch.int64)] = rays
        # rays without a block: one run, all tail
        lone = torch.nonzero(slots.slot < 0).reshape(-1)
        k = int((bins(tails.row[lone]) >= 0).sum().item())
        acc["runs"] += k
        acc["tail_runs"] += k
        acc["window_adds"] += k * (windows(i0, i1) - 1)
    else:
        n = view.shape[0]
        ray_of = torch.arange(n, device=dev)
    r = torch.arange(nrow, device=dev)
    newwin = ((r + i0) % window_rows == 0) if window_rows else torch.zeros(nrow, dtype=torch.bool, device=dev)
    for a in range(0, n, 65536):
        z = min(a + 65536, n)
        b = bins(view[a:z])
        tf = torch.full((z - a,), i1, dtype=torch.int64, device=dev)
        if tails is not None:
            tf = tails.frm[ray_of[a:z]].to(torch.int64).clamp(i0, i1)
        read = r[None, :] < (tf - i0)[:, None]
        b = torch.where(read, b, torch.full_like(b, -2.0))
        same = torch.zeros_like(read)
        same[:, 1:] = b[:, 1:] == b[:, :-1]
        counted = read & (b >= 0)
        acc["runs"] += int((counted & ~same).sum().item())
        acc["window_adds"] += int((counted & same & newwin[None, :]).sum().item())
        acc["rows_read"] += int(read.sum().item())
        if tails is not None:
            has = tf < i1
            bt = bins(tails.row[ray_of[a:z]])
            lastb = torch.gather(b, 1, (tf - i0 - 1).clamp(min=0)[:, None])[:, 0]
            cont = has & (bt >= 0) & (tf > i0) & (lastb == bt)
            new = has & (bt >= 0) & ~cont
            acc["runs"] += int(new.sum().item())
            acc["tail_runs"] += int((has & (bt >= 0)).sum().item())
            if window_rows:
                w = (i1 - 1) // window_rows - tf // window_rows        # window bounds inside the tail
                w = w + (cont & (tf % window_rows == 0)).to(torch.int64)
                acc["window_adds"] += int(w[has & (bt >= 0)].sum().item())
    acc["rays"] = nray


class Timed:
    """A sink with a pair of events around every call of ``inner``."""
    takes_tails = takes_slots = True

    def __init__(self, inner, counter=None):
        self.inner, self.events, self.counter = inner, [], counter

    def __call__(self, i0, i1, view, tails=None, slots=None):
        s = torch.cuda.current_stream(view.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        self.inner(i0, i1, view, tails, slots)
        e1.record(s)
        self.events.append((e0, e1))
        if self.counter is not None:
            self.counter(i0, i1, view, tails, slots)

    def kernel_s(self):
        return sum(a.elapsed_time(b) for a, b in self.events) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=float, default=90.0)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--ny", type=int, default=720)
    ap.add_argument("--window", type=int, default=12)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--noskip-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bs, _ = bench.make_bs("zonal")
    y0 = torch.as_tensor(bench.c3_initial_state(bs), device="cuda")
    eng = RayEngine.from_bs(bs)
    nt = int(round(a.days * 12)) + 1
    kw = dict(ttotal=(nt - 1) * 7200.0, first_chunk=[24, 160], team=[64, 64, 64])
    noskip = load_variant(a.noskip_lib) if a.noskip_lib else None

    def run(sink):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eng.integrate(y0, nt, 7200.0, sink=sink, out=None, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    dspec = DensitySpec(a.nx, a.ny)
    aspec = {"arrival": ArrivalSpec(a.nx, a.ny, nt=nt), f"arrival-W{a.window}": ArrivalSpec(a.nx, a.ny, nt=nt,
                                                                                          window_rows=a.window)}
    make = {"density": lambda: DensitySink(DensityMap(dspec, "cuda"))}
    for name, sp in aspec.items():
        make[name] = lambda sp=sp: ArrivalSink(ArrivalMap(sp, "cuda"))
        if noskip is not None:
            make[name + "-noskip"] = lambda sp=sp: ArrivalSink(VariantMap(sp, "cuda", noskip))

    _, res = run(None)                                  # warm-up
    launches = len(res.bounds)
    # the runs of each kind of map, counted once (untimed; warms the kernels)
    counts = {}
    for name, spec, W in [("density", dspec, 0)] + [(k, s.bins, s.window_rows or 0) for k, s in aspec.items()]:
        acc = dict(runs=0, tail_runs=0, window_adds=0, rows_read=0)
        run(Timed(make[name](), lambda *r, spec=spec, W=W, acc=acc: count_runs(spec, W, *r, acc)))
        counts[name] = acc
    times = {k: [] for k in ["none"] + list(make)}
    kern = {k: [] for k in make}
    for _ in range(a.pairs):
        times["none"].append(run(None)[0])
        for name, mk in make.items():
            sink = Timed(mk())
            times[name].append(run(sink)[0])
            kern[name].append(sink.kernel_s())
    rec = {"workload": f"C3 zonal, {a.days:g} d at 2 h, RayEngine.integrate first_chunk 24+160, team 64",
           "slots": int(y0.shape[1]), "live": int((~torch.isnan(y0.sum(0))).sum().item()), "rows": nt - 1,
           "launches": launches, "ray_steps": res.ray_steps, "map": [a.nx, a.ny], "window_rows": a.window,
           "device": torch.cuda.get_device_name(0), "none_s": times["none"], "variants": {}}
    for name in make:
        c = counts[name.replace("-noskip", "")]
        if name == "density":
            atomics = c["runs"]
        else:
            windows = aspec[name.replace("-noskip", "")].window_rows is not None
            atomics = 2 * c["runs"] + ((c["runs"] + c["window_adds"]) if windows else 0)
        k = min(kern[name])
        rec["variants"][name] = {
            "with_sink_s": times[name], "kernel_s": kern[name],
            "added_s_per_run": min(times[name]) - min(times["none"]),
            "kernel_s_per_launch": k / launches, **c, "atomics_no_skip": atomics,
            "atomics_per_s": atomics / k if k > 0 else None}
    rate = rec["variants"]["density"]["atomics_per_s"]
    for name, v in rec["variants"].items():
        v["kernel_over_atomics_at_density_rate"] = min(v["kernel_s"]) / (v["atomics_no_skip"] / rate)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
