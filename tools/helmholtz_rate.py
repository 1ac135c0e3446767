"""What the Helmholtz decomposition costs: ``rwrt_sh_helmholtz`` on the
0.25-degree grid (721 x 1440), T = 42, for ``u, v`` of 41 synthetic levels in
one call -- the rotational wind alone in float32 (the ``Levels`` path), and
all ten planes plus the Rossby-wave source ``S`` -- with ``rwrt_sh_filter`` on
the same 82 fields in the same session for comparison.

    python tools/helmholtz_rate.py [--res 0.25] [--trunc 42] [--nlev 41] [--repeats 10] [--out FILE.json]
    python tools/helmholtz_rate.py --once rotational|all|filter     (one pass of one route, for a kernel trace)

Every input is resident before the timed windows; a window is one pass of a
route between two stream events; the routes alternate within a repeat, after a
warm-up of each.  Reports per route every window's time, the median and the
spread (min, max).  Which kernel the time goes to is NOT measured here: that is
a kernel trace of a ``--once`` run, taken in a run of its own."""
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
from helmholtz import Helmholtz, plane_mask  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=float, default=0.25)
    ap.add_argument("--trunc", type=int, default=42)
    ap.add_argument("--nlev", type=int, default=41)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--once", choices=["rotational", "all", "filter"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H.require_gpu()
    lib = H.load()
    b0 = S.background_level(0, res=a.res)
    nlat, nlon = b0["u"].shape
    h = Helmholtz(nlat, nlon, a.trunc)
    dev = h.device
    host = np.empty((2, a.nlev, nlat, nlon), np.float32)
    for j in range(a.nlev):
        b = b0 if j == 0 else S.background_level(j, res=a.res)
        host[0, j], host[1, j] = b["u"], b["v"]
    uv = torch.as_tensor(host, device=dev)
    npair, n1 = a.nlev, a.trunc + 1
    all_mask, rot_mask = plane_mask(None)[0], plane_mask(("u_rot", "v_rot"))[0]
    spec = torch.empty((npair, 2, n1, n1, 2), dtype=torch.float64, device=dev)
    out64 = torch.empty((npair, 10, nlat, nlon), dtype=torch.float64, device=dev)
    rot32 = torch.empty((npair, 2, nlat, nlon), dtype=torch.float32, device=dev)
    src = torch.empty((npair, nlat, nlon), dtype=torch.float64, device=dev)
    planes = [torch.empty((npair, nlat, nlon), dtype=torch.float64, device=dev) for _ in range(6)]
    scratch = torch.empty(npair * 14 * n1 * nlat * 2, dtype=torch.float64, device=dev)
    flat = uv.view(2 * npair, nlat, nlon)
    fout = torch.empty_like(flat)
    fspec = torch.empty((2 * npair, n1, n1, 2), dtype=torch.float64, device=dev)
    stream = H.stream(dev)

    def call(mask, o64, r32):
        H.check(H.entry("rwrt_sh_helmholtz")(nlon, nlat, npair, a.trunc, mask, uv[0].data_ptr(), uv[1].data_ptr(),
                                      h.w.data_ptr(), h.x.data_ptr(), spec.data_ptr(), H.dptr(o64), H.dptr(r32),
                                      scratch.data_ptr(), stream))

    def rotational():
        call(rot_mask, None, rot32)

    def all_planes_and_source():
        call(all_mask, out64, None)
        # the six planes of S, made contiguous as Helmholtz.rws does: div, u_div, v_div, vrt, vrt_x, vrt_y
        for dst, k in zip(planes, (1, 6, 7, 0, 8, 9)):
            dst.copy_(out64[:, k])
        H.check(H.entry("rwrt_sh_rws")(nlon, nlat, npair, 1, h.x.data_ptr(), *[p.data_ptr() for p in planes],
                                src.data_ptr(), stream))

    def sh_filter():
        H.check(lib.rwrt_sh_filter(nlon, nlat, 2 * npair, a.trunc, flat.data_ptr(), h.w.data_ptr(), h.x.data_ptr(),
                                   fspec.data_ptr(), fout.data_ptr(), None, scratch.data_ptr(), stream))

    routes = {f"rotational_float32_{npair}_pairs": rotational,
              f"ten_planes_and_S_{npair}_pairs": all_planes_and_source,
              f"sh_filter_{2 * npair}_fields": sh_filter}
    if a.once:
        fn = dict(zip(("rotational", "all", "filter"), routes.values()))[a.once]
        fn()                                          # (the first pass pays the code object's load)
        torch.cuda.synchronize()
        fn()
        torch.cuda.synchronize()
        print(json.dumps({"once": a.once, "passes": 2}))
        return

    def window(fn):
        s = torch.cuda.current_stream(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3

    for fn in routes.values():                       # warm-up
        window(fn)
    times = {k: [] for k in routes}
    for _ in range(a.repeats):
        for k, fn in routes.items():
            times[k].append(window(fn))
    # results: the float32 pair is the fp64 pair rounded; the source is finite
    rotational()
    all_planes_and_source()
    torch.cuda.synchronize()
    rounded = bool(torch.equal(rot32, out64[:, 4:6].to(torch.float32)))
    rec = {"workload": f"synthetic background_level at {a.res:g} degrees, {nlat} x {nlon}, T = {a.trunc}, "
                       f"u and v of {a.nlev} levels",
           "device": torch.cuda.get_device_name(0), "nlat": nlat, "nlon": nlon, "trunc": a.trunc, "npair": npair,
           "repeats": a.repeats, "order": list(routes), "rot32_is_the_fp64_pair_rounded": rounded,
           "source_is_finite": bool(torch.isfinite(src).all()), "routes": {}}
    for k in routes:
        t = times[k]
        med = statistics.median(t)
        rec["routes"][k] = {"s_per_pass": t, "median_s": med, "min_s": min(t), "max_s": max(t),
                            "spread_over_median": (max(t) - min(t)) / med}
    keys = list(routes)
    rec["rotational_over_filter"] = rec["routes"][keys[0]]["median_s"] / rec["routes"][keys[2]]["median_s"]
    rec["all_over_filter"] = rec["routes"][keys[1]]["median_s"] / rec["routes"][keys[2]]["median_s"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
