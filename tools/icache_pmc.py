"""Instruction-cache requests and misses of the ray-loop kernel from one rocprofv3 PMC pass.

    rocprofv3 --pmc SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE \\
        -d <pmc_dir> -o run --output-format csv -- python bench.py --gpus 1 --steps 5 --warmup 2 [--lib ...]
    python tools/icache_pmc.py <pmc_dir> <out.json> [kernel substring]

Sums the counters over the dispatches of rk45_run_kernel (both tiers of a
static launch: the one the device did not pick returns at its entry) and
prints the miss rate, misses / requests.  The run kernel runs one wave per
SIMD, so nothing covers an instruction fetch that misses; the rate compares
code layouts of the same instructions ("Code layout").
A counter pass serialises the kernels: its times are no timings.
"""
import csv
import glob
import json
import os
import sys

COUNTERS = ("SQC_ICACHE_REQ", "SQC_ICACHE_HITS", "SQC_ICACHE_MISSES", "SQC_ICACHE_MISSES_DUPLICATE")


def main():
    d, out = sys.argv[1:3]
    kernel = sys.argv[3] if len(sys.argv) > 3 else "rk45_run_kernel"
    files = sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True))
    if not files:
        sys.exit(f"no *counter_collection.csv under {d}")
    tot, names, disp = dict.fromkeys(COUNTERS, 0.0), {}, set()
    for f in files:
        for r in csv.DictReader(open(f)):
            if kernel not in r["Kernel_Name"] or r["Counter_Name"] not in tot:
                continue
            v = float(r["Counter_Value"])
            tot[r["Counter_Name"]] += v
            disp.add(r["Dispatch_Id"])
            k = names.setdefault(r["Kernel_Name"].split("(")[0], dict.fromkeys(COUNTERS, 0.0))
            k[r["Counter_Name"]] += v
    rate = lambda c: c["SQC_ICACHE_MISSES"] / c["SQC_ICACHE_REQ"] if c["SQC_ICACHE_REQ"] else None  # noqa: E731
    res = {"kernel": kernel, "dispatches": len(disp), **tot, "miss_rate": rate(tot),
           "miss_rate_with_duplicates": ((tot["SQC_ICACHE_MISSES"] + tot["SQC_ICACHE_MISSES_DUPLICATE"]) /
                                         tot["SQC_ICACHE_REQ"]) if tot["SQC_ICACHE_REQ"] else None,
           "per_kernel": {n: {**c, "miss_rate": rate(c)} for n, c in names.items()}}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "per_kernel"}))


if __name__ == "__main__":
    main()
