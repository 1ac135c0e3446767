"""What the wavenumber map costs: ``rwrt_wn_map`` on the 0.25-degree synthetic
grid (1440 x 721 nodes), 7 zonal wavenumbers, for one level and for a batch of
levels in one call -- against the only route there was before it,
``rwrt_ray_initial`` with every node as a source (one call per level, counted
without the re-layout into the map's layout it would still need).

    python tools/wn_rate.py [--res 0.25] [--nlev 8] [--repeats 10] [--inner 5] [--out FILE.json]

Every input is resident before the timed windows; a window is ``inner`` calls
between two stream events; the routes alternate within a repeat, after a
warm-up of each.  Reports per route every window's time per call, the median,
the spread (min, max), the bytes each route stores per (node, k) -- 76 (nine
doubles and one int32) against 168 (21 doubles) -- and the store rate those
imply.  Whether either route is bound by its stores or by the eigen-solve is
NOT measured here (that needs counters); the script only reports the times.
It also checks, at this size, that the map equals the initial rows bit for bit
and times ``rwrt_wn_fill`` on the level-0 ``mwn``.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rossby-wave-ray-tracing_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _hip as H  # noqa: E402
import synthetic as S  # noqa: E402
from engine import RayEngine  # noqa: E402
from levels import Levels  # noqa: E402

ZWN = [float(k) for k in range(1, 8)]
F64 = torch.float64


def same(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=float, default=0.25)
    ap.add_argument("--nlev", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H.require_gpu()
    lib = H.load()
    b0 = S.background_level(0, res=a.res)
    lv = Levels(b0["lat"], b0["lon"], a.nlev)
    for j in range(a.nlev):
        b = b0 if j == 0 else S.background_level(j, res=a.res)
        lv.set_level(j, b["u"], b["v"])
    eng = RayEngine.from_levels(lv)
    dev, grid = eng.device, eng.grid
    nx, ny, nz = lv.nlon, lv.nlat, len(ZWN)
    nnode = nx * ny
    stream = H.stream(dev)
    zc = eng.zwn_tensor(ZWN, 0.0)
    ax = torch.as_tensor(np.concatenate([lv.lon, lv.lat, np.cos(lv.lat)]), dtype=F64).to(dev)
    src = eng.sources(np.repeat(lv.lon, ny), np.tile(lv.lat, nx))          # source s = i * ny + j
    mwn, ug, vg = (torch.empty((a.nlev, nx, ny, nz, 3), dtype=F64, device=dev) for _ in range(3))
    rootnum = torch.empty((a.nlev, nx, ny, nz), dtype=torch.int32, device=dev)
    rows = torch.empty((7, 3, nnode, nz), dtype=F64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    stride = lv.packed.stride(0)

    def wn_map(nlev):
        H.check(lib.rwrt_wn_map(grid, lv.packed.data_ptr(), nlev, stride, nx, ax.data_ptr(), ax[nx:].data_ptr(),
                                ax[nx + ny:].data_ptr(), nz, zc.data_ptr(), mwn.data_ptr(), ug.data_ptr(),
                                vg.data_ptr(), rootnum.data_ptr(), info.data_ptr(), stream))

    def initial(nlev):
        for j in range(nlev):       # (each level's rows overwrite the last: no re-layout, no second buffer)
            H.check(lib.rwrt_ray_initial(grid, lv.packed[j].data_ptr(), nnode, src[0].data_ptr(), src[1].data_ptr(),
                                         src[2].data_ptr(), nz, zc.data_ptr(), rows.data_ptr(), info.data_ptr(),
                                         stream))

    fill_out = torch.empty_like(mwn[0])

    def fill(_):
        H.check(lib.rwrt_wn_fill(nx, ny, nz * 3, 1, mwn[0].data_ptr(), fill_out.data_ptr(), stream))

    routes = {"wn_map_1": (wn_map, 1), "initial_rows_1": (initial, 1),
              f"wn_map_{a.nlev}": (wn_map, a.nlev), f"initial_rows_{a.nlev}": (initial, a.nlev),
              "wn_fill_1": (fill, 1)}

    # results first: the map equals the initial rows of every node, bit for bit, at this size
    wn_map(1)
    initial(1)
    torch.cuda.synchronize()
    n_bad = int(info.item())
    equal = all(same(m[0], rows[v].view(3, nx, ny, nz).permute(1, 2, 3, 0))
                for m, v in ((mwn, 3), (ug, 5), (vg, 6)))
    hist = torch.bincount((rootnum[0] + 1).flatten().long(), minlength=5).tolist()

    def window(fn, arg):
        s = torch.cuda.current_stream(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(a.inner):
            fn(arg)
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3 / a.inner

    for fn, arg in routes.values():                       # warm-up
        window(fn, arg)
    times = {k: [] for k in routes}
    for _ in range(a.repeats):
        for k, (fn, arg) in routes.items():
            times[k].append(window(fn, arg))
    rec = {"workload": f"synthetic background_level at {a.res:g} degrees, {nx} x {ny} nodes, k = 1..{nz}",
           "device": torch.cuda.get_device_name(0), "nodes": nnode, "nzwn": nz, "nlev": a.nlev,
           "repeats": a.repeats, "calls_per_window": a.inner, "order": list(routes),
           "map_equals_initial_rows_bitwise": equal, "n_bad_level0": n_bad,
           "rootnum_histogram_level0(-1,0,1,2,3)": hist,
           "bytes_stored_per_node_k": {"wn_map": 76, "initial_rows": 168}, "routes": {}}
    for k, (fn, nlev) in routes.items():
        t = times[k]
        med = statistics.median(t)
        d = {"s_per_call": t, "median_s": med, "min_s": min(t), "max_s": max(t),
             "spread_over_median": (max(t) - min(t)) / med}
        if k != "wn_fill_1":
            per = 76 if fn is wn_map else 168
            d.update(solves_per_s=nlev * nnode * nz / med, stored_bytes=per * nlev * nnode * nz,
                     stored_bytes_per_s=per * nlev * nnode * nz / med)
        else:
            d.update(bytes_read_and_written=2 * 8 * nnode * nz * 3, nan_entries=int(torch.isnan(mwn[0]).sum().item()),
                     nan_entries_left=int(torch.isnan(fill_out).sum().item()))
        rec["routes"][k] = d
    for n in (1, a.nlev):
        rec[f"wn_map_over_initial_rows_{n}"] = rec["routes"][f"wn_map_{n}"]["median_s"] / \
            rec["routes"][f"initial_rows_{n}"]["median_s"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
