"""What the basic-state diagnostics cost at 0.25 degrees: ``rwrt_bs_diag`` on
``nlev`` levels of the time-varying C5 background (1440 x 721) on one GPU, in
interleaved rounds of

  betam_ks      select = {betam, KS}: no scratch, one launch
  all           all 23 planes, every level in flight (scratch_levels = nlev)
  bs_ready      ``nlev`` calls of ``rwrt_bs_ready`` on the same levels (fp64 packed
                records) -- the yardstick, unchanged code
  copy          a ``torch`` device copy of the bytes ``all`` writes

and, with ``--ab-lib``, ``betam_ks`` and ``all`` again through another build of
the library (``--ab-name`` labels it; the record in ``profiles/bsdiag/`` compares
the kept kernels with the variant without a shared-memory tile, DESIGN.md
section 16), whose results are first checked to be the same bytes.

    python tools/bsdiag_rate.py [--nlev 8] [--res 0.25] [--rounds 5] [--ab-lib .../librwrt_X.so]
                                [--out FILE.json]

Times are HIP events around ``reps`` back-to-back calls, per call; reported is
the best of the rounds and every round.  For the two diagnostics calls the
record also has the least bytes a call must move -- 8 B of ``u, v`` in and 8 B
per selected plane out, per node and level -- and those bytes over the time,
to be read against the achievable HBM rate of the card (about 6.3 TB/s); the
inputs (66 MB for 8 levels) stay in the Infinity Cache between calls, the
outputs of ``all`` (1.5 GB) do not.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rossby-wave-ray-tracing_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _hip as H  # noqa: E402
import synthetic as S  # noqa: E402
from bsdiag import BSDiag  # noqa: E402

ALL = (1 << 23) - 1
BK = (1 << 21) | (1 << 22)
HBM_ACHIEVABLE = 6.3e12


def load_variant(path):
    lib = ctypes.CDLL(path)
    P, I32, D = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    lib.rwrt_bs_diag.argtypes = [I32, I32, I32, P, P, P, D, D, ctypes.c_uint32, P, P, I32, P]
    lib.rwrt_bs_diag.restype = ctypes.c_int
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nlev", type=int, default=8)
    ap.add_argument("--res", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--ab-name", default="untiled")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H.require_gpu()
    lib = H.load()
    levels = [S.background_level(j, res=a.res) for j in range(a.nlev)]
    d = BSDiag(levels[0]["lat"], levels[0]["lon"])
    u = torch.as_tensor(np.stack([b["u"] for b in levels])).cuda()
    v = torch.as_tensor(np.stack([b["v"] for b in levels])).cuda()
    nlev, n = a.nlev, d.nlon * d.nlat
    out_all = torch.empty((nlev, 23, d.nlon, d.nlat), dtype=torch.float64, device="cuda")
    out_bk = torch.empty((nlev, 2, d.nlon, d.nlat), dtype=torch.float64, device="cuda")
    copy_dst = torch.empty_like(out_all)
    scratch = torch.empty(4 * n * nlev, dtype=torch.float64, device="cuda")
    packed = torch.empty((d.nlon + 1, d.nlat, H.NFIELD_PACK), dtype=torch.float64, device="cuda")
    st = H.stream()

    def diag(fn, select, out):
        def call():
            s = fn(d.nlon, d.nlat, nlev, u.data_ptr(), v.data_ptr(), d.trig.data_ptr(), d.dx, d.dy, select,
                   out.data_ptr(), scratch.data_ptr() if select != BK else None, nlev, st)
            if s != H.RWRT_OK:
                raise H.RwrtError(f"rwrt_bs_diag: status {s}")
        return call

    def ready():
        for k in range(nlev):
            H.check(lib.rwrt_bs_ready(d.nlon, d.nlat, u[k].data_ptr(), v[k].data_ptr(), d.trig.data_ptr(), d.dx, d.dy,
                                      scratch.data_ptr(), packed.data_ptr(), 0, st))

    work = {"betam_ks": (diag(lib.rwrt_bs_diag, BK, out_bk), 20), "all": (diag(lib.rwrt_bs_diag, ALL, out_all), 3),
            "bs_ready": (ready, 3), "copy": (lambda: copy_dst.copy_(out_all), 3)}
    if a.ab_lib:
        ab = load_variant(a.ab_lib)
        # the two builds give the same bytes at the size that is timed
        diag(lib.rwrt_bs_diag, ALL, out_all)()
        diag(ab.rwrt_bs_diag, ALL, copy_dst)()
        torch.cuda.synchronize()
        if not torch.equal(out_all.view(torch.int64), copy_dst.view(torch.int64)):
            raise SystemExit("the two builds differ")
        work[f"betam_ks-{a.ab_name}"] = (diag(ab.rwrt_bs_diag, BK, out_bk), 20)
        work[f"all-{a.ab_name}"] = (diag(ab.rwrt_bs_diag, ALL, out_all), 3)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3 / reps

    for fn, _ in work.values():                          # warm-up: every kernel, every shape
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in work}
    for _ in range(a.rounds):
        for k, (fn, reps) in work.items():
            times[k].append(timed(fn, reps))
    rec = {"workload": f"C5 levels 0..{nlev - 1} at {a.res:g} degrees", "nlon": d.nlon, "nlat": d.nlat, "nlev": nlev,
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "hbm_achievable_B_per_s": HBM_ACHIEVABLE,
           "ab_lib": os.path.basename(a.ab_lib) if a.ab_lib else None, "calls": {}}
    for k, t in times.items():
        c = {"s_per_call": min(t), "s_per_level": min(t) / nlev, "every_round_s": t}
        nsel = 2 if k.startswith("betam_ks") else (23 if k.startswith("all") else None)
        if nsel:
            c["min_bytes"] = (8 + 8 * nsel) * n * nlev
            c["min_bytes_per_s"] = c["min_bytes"] / min(t)
            c["share_of_hbm_achievable"] = c["min_bytes_per_s"] / HBM_ACHIEVABLE
        if k == "copy":
            c["bytes_read_plus_written"] = 2 * out_all.numel() * 8
            c["bytes_per_s"] = c["bytes_read_plus_written"] / min(t)
        rec["calls"][k] = c
    rec["betam_ks_over_bs_ready_per_level"] = rec["calls"]["betam_ks"]["s_per_level"] / rec["calls"]["bs_ready"]["s_per_level"]
    rec["all_over_copy"] = rec["calls"]["all"]["s_per_call"] / rec["calls"]["copy"]["s_per_call"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
