"""What the spherical-harmonic filter costs: ``rwrt_sh_filter`` on the
0.25-degree grid (721 x 1440), T = 42, for ``u, v`` of 41 levels -- 82 fields
in one call against 82 calls of one field -- with ``rwrt_bs_ready`` for the
same 41 levels as the yardstick of what the filter adds to building a
``Levels``.

    python tools/shsf_rate.py [--res 0.25] [--trunc 42] [--nlev 41] [--repeats 10] [--out FILE.json]

Every input is resident before the timed windows; a window is one pass of a
route (all 82 fields, or all 41 levels) between two stream events; the routes
alternate within a repeat, after a warm-up of each.  Reports per route every
window's time, the median and the spread (min, max), the bytes of ``u, v``
read and written (float32 in, float32 out) and the rate those imply.  Which
of the four kernels the time goes to is NOT measured here (that needs a kernel
trace); the script only reports the times.  It also checks, at this size, that
the batch gives the bits of the single calls, and the largest difference of
one field from the NumPy definition.
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
from levels import Levels  # noqa: E402
from shsf import SHFilter, reference_filter  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=float, default=0.25)
    ap.add_argument("--trunc", type=int, default=42)
    ap.add_argument("--nlev", type=int, default=41)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H.require_gpu()
    lib = H.load()
    b0 = S.background_level(0, res=a.res)
    nlat, nlon = b0["u"].shape
    lv = Levels(b0["lat"], b0["lon"], a.nlev)
    dev = lv.device
    flt = SHFilter(nlat, nlon, a.trunc, dev)
    host = np.empty((2, a.nlev, nlat, nlon), np.float32)
    for j in range(a.nlev):
        b = b0 if j == 0 else S.background_level(j, res=a.res)
        host[0, j], host[1, j] = b["u"], b["v"]
    uv = torch.as_tensor(host, device=dev)
    nfield, n1 = 2 * a.nlev, a.trunc + 1
    flat = uv.view(nfield, nlat, nlon)
    out = torch.empty_like(flat)
    one = torch.empty_like(flat)
    spec = torch.empty((nfield, n1, n1, 2), dtype=torch.float64, device=dev)
    scratch = torch.empty(2 * nfield * n1 * nlat * 2, dtype=torch.float64, device=dev)
    stream = H.stream(dev)

    def batched():
        H.check(lib.rwrt_sh_filter(nlon, nlat, nfield, a.trunc, flat.data_ptr(), flt.w.data_ptr(), flt.x.data_ptr(),
                                   spec.data_ptr(), out.data_ptr(), None, scratch.data_ptr(), stream))

    def one_by_one():
        for i in range(nfield):
            H.check(lib.rwrt_sh_filter(nlon, nlat, 1, a.trunc, flat[i].data_ptr(), flt.w.data_ptr(),
                                       flt.x.data_ptr(), spec[i].data_ptr(), one[i].data_ptr(), None,
                                       scratch.data_ptr(), stream))

    def bs_ready():
        for j in range(a.nlev):
            lv.set_level(j, out[j], out[a.nlev + j])

    routes = {f"sh_filter_{nfield}_fields_one_call": batched, f"sh_filter_{nfield}_calls_of_one_field": one_by_one,
              f"bs_ready_{a.nlev}_levels": bs_ready}

    # results first: the batch equals the single calls bit for bit; one field against the definition
    batched()
    one_by_one()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out, one))
    f0 = host[0, 0]
    ref = reference_filter(f0, a.trunc)
    got64 = flt.filter(f0, torch.float64).cpu().numpy()
    err = float(np.abs(got64 - ref).max() / np.abs(f0).max())
    spread = float(np.abs(ref - reference_filter(f0, a.trunc, "descending")).max() / np.abs(f0).max())

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
    moved = 2 * 4 * nfield * nlat * nlon
    rec = {"workload": f"synthetic background_level at {a.res:g} degrees, {nlat} x {nlon}, T = {a.trunc}, "
                       f"u and v of {a.nlev} levels",
           "device": torch.cuda.get_device_name(0), "nlat": nlat, "nlon": nlon, "trunc": a.trunc, "nfield": nfield,
           "repeats": a.repeats, "order": list(routes), "batch_equals_single_calls_bitwise": equal,
           "field0_max_error_vs_definition_over_max": err, "field0_definition_spread_over_max": spread,
           "bytes_of_u_v_read_and_written": moved, "routes": {}}
    for k in routes:
        t = times[k]
        med = statistics.median(t)
        rec["routes"][k] = {"s_per_pass": t, "median_s": med, "min_s": min(t), "max_s": max(t),
                            "spread_over_median": (max(t) - min(t)) / med}
    keys = list(routes)
    rec["routes"][keys[0]]["u_v_bytes_per_s"] = moved / rec["routes"][keys[0]]["median_s"]
    rec["one_by_one_over_batched"] = rec["routes"][keys[1]]["median_s"] / rec["routes"][keys[0]]["median_s"]
    rec["batched_filter_over_bs_ready"] = rec["routes"][keys[0]]["median_s"] / rec["routes"][keys[2]]["median_s"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
