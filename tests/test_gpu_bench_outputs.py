"""bench.py's plain and ``--full`` runs and ``--dump-outputs`` (one GPU).

A plain run carries the headline figures only; ``--full`` adds the roofline
(and the CPU baselines, left out here with ``--no-cpu``).  Both write what the
last timed step returned, and since the inputs are the same from run to run
the two dumps must be the same bit for bit, whatever ``--steps`` is.  A small
workload: one C3 period over 10 days.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--days", "10", "--periods", "1"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    plain = _bench(["--steps", "2", "--warmup", "1", "--dump-outputs", str(d / "plain")])
    full = _bench(["--steps", "1", "--warmup", "0", "--full", "--no-cpu", "--dump-outputs", str(d / "full")])
    return d, plain, full


def test_plain_line_is_lean_and_full_adds_the_rest(runs):
    _, plain, full = runs
    for line in (plain, full):
        assert all(k in line for k in HEADLINE)
        assert line["unit"] == "ray-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["value"] > 0 and line["ms_per_step"] > 0
        # value = accepted ray-steps per second of timed steps
        assert abs(line["value"] * line["ms_per_step"] * 1e-3 / line["ray_steps_per_step"] - 1) < 1e-9
    assert (plain["steps"], plain["warmup"], full["steps"], full["warmup"]) == (2, 1, 1, 0)
    for k in ("roofline", "cpu_baseline", "cpu_baseline_mp", "max_dpos_vs_cpu_rad", "bitwise_vs_cpu_oracle"):
        assert k not in plain
    assert plain["init_bitwise_vs_host"] is None and plain["host_init_s"] is None
    assert full["roofline"]["bound"] == "valu_issue" and full["init_bitwise_vs_host"] is True
    assert "cpu_baseline" not in full                       # --no-cpu
    assert plain["endpoints_rank0_sha256"] == full["endpoints_rank0_sha256"]


def test_dumped_outputs_are_the_last_steps_and_repeat(runs):
    d, plain, full = runs
    names = sorted(f[:-4] for f in os.listdir(d / "plain"))
    assert names == sorted(f[:-4] for f in os.listdir(d / "full"))
    assert set(names) >= {"endpoints", "counts", "ray_index"}
    a = {k: np.load(d / "plain" / f"{k}.npy") for k in names}
    b = {k: np.load(d / "full" / f"{k}.npy") for k in names}
    n = plain["config"]["live_rays_rank0"]
    assert a["endpoints"].shape == (n, 8) and a["counts"].shape == (n, 2) and a["ray_index"].shape == (n,)
    assert a["endpoints"].dtype == np.float64 and a["counts"].dtype == np.float32
    assert sum(os.path.getsize(d / "plain" / f) for f in os.listdir(d / "plain")) <= 64_000_000
    for k in a:
        assert np.isfinite(a[k]).all(), k                  # (a masked ray's NaNs: zeros, flagged in endpoints_nan)
        assert np.array_equal(a[k], b[k]), k
    # one step's own counters: the accepted steps sum to the line's ray-steps
    # per step (slots without an initial root take none)
    assert a["counts"][:, 0].astype(np.int64).sum() == int(plain["ray_steps_per_step"])
    # rays alive at the end have a position; a flagged value is written as 0
    alive = np.ones(n, bool) if "endpoints_nan" not in a else a["endpoints_nan"].astype(np.int64) & 3 == 0
    assert alive.any() and np.any(a["endpoints"][alive, :2] != 0)
    assert np.all(a["endpoints"][~alive][:, :2].prod(axis=1) == 0)
