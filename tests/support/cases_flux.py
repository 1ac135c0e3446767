"""Crafted launches, spec variants and comparisons of the flux tests."""
import math

import numpy as np

import flux as F
from flux import reference_flux

INF, NAN = math.inf, math.nan


def abs_sums(lon, lat, k, l, ug, vg, chan, spec):
    """Per bin and component the sum of |contribution| of the accepted points
    (``[nchan, ny, nx, 3]``): the sum|v| of the rounding bound."""
    chan = None if chan is None else np.asarray(chan, np.int64).reshape(-1, 1)
    idx, vx, vy, sp = F.accept(lon, lat, k, l, ug, vg, chan, spec)
    ok = idx >= 0
    out = np.zeros((spec.nchan * spec.ny * spec.nx, 3))
    for q, v in enumerate((vx, vy, sp)):
        np.add.at(out[:, q], idx[ok], np.abs(np.broadcast_to(v, ok.shape)[ok]))
    return out.reshape(spec.shape + (3,))


def sum_bound(count, abs_sum):
    """|got - ref| <= 2 (n + 1) 2^-53 sum|v| per bin and component: the bound
    of a sum of n terms in any order, twice (both sides are rounded sums), plus
    one rounding for a tail added as a product (tests/test_gpu_density.py)."""
    return 2.0 * (count[..., None] + 1) * 2.0 ** -53 * abs_sum


def assert_flux(got, want, abs_sum=None, what=""):
    """count and rowsum exactly; the sums exactly (``abs_sum`` None) or to the bound."""
    for name in ("count", "rowsum"):
        assert got[name].dtype == np.int64 and np.array_equal(got[name], want[name]), (what, name)
    if abs_sum is None:
        assert np.array_equal(got["sum"], want["sum"]), (what, "sum")
    else:
        err = np.abs(got["sum"] - want["sum"])
        assert np.all(err <= sum_bound(want["count"], abs_sum)), (what, "sum", float(err.max()))
    assert np.all(np.isfinite(got["sum"])), what


# the spec variants of the issue: wrapped and unwrapped, both vector kinds, finite filters
VARIANTS = {
    "wrapped": dict(),
    "unit": dict(vector="unit"),
    "three-circles": dict(lon_range=(-360.0, 720.0)),
    "three-circles-unit": dict(lon_range=(-360.0, 720.0), vector="unit"),
    "speed": dict(speed_range=(0.5, 2.5)),
    "wn": dict(wn_max=2.0),
    "all-filters-unit-window": dict(lon_range=(-720.0, 360.0), vector="unit", speed_range=(0.5, 3.5), wn_max=2.5),
}


NRAY = 41


def crafted_launch(i0, i1, seed, tf=None, nray=NRAY):
    """Logical rows ``[nray, i1 - i0, 8]`` of a launch ``[i0, i1)`` that all
    three layouts can hold: ray j's rows from ``tf[j]`` on repeat its tail row.
    ``tf`` runs through values below, at, inside, at the end of and above the
    launch; the j % 3 == 0 rays (no row block in the slots layout) have at most
    i0.  Longitudes span about three circles either side of 0; every fourth ray
    drifts slowly (runs of several rows in one bin, going on into the tail),
    the others jump from bin to bin; k, l in (-3, 3), speeds up to 4.2; NaN
    and inf holes in lon, ug, vg, k and l, in rows and in tails; one ray at
    rest; channels -1 and 3 among 0..2."""
    rng = np.random.default_rng(seed)
    nrow = i1 - i0
    rows = rng.uniform(-3.0, 3.0, (nray, nrow, 8))
    rows[..., 0] = rng.uniform(-20.0, 20.0, (nray, nrow))
    rows[..., 1] = rng.uniform(-1.8, 1.8, (nray, nrow))
    slow = np.arange(nray) % 4 == 1
    rows[slow, :, 0] = rng.uniform(-6.0, 12.0, (slow.sum(), 1)) + 0.05 * np.arange(nrow)
    rows[slow, :, 1] = rng.uniform(-1.0, 1.0, (slow.sum(), 1))
    rows[3, nrow // 2, 5] = NAN                                  # holes in a run
    rows[7, 0, 0] = INF
    rows[9, nrow // 2, 6] = -INF
    rows[13, 0, 2] = NAN
    rows[17, nrow - 1, 3] = INF
    rows[21, :, 5:7] = 0.0                                       # at rest while it is read
    tail = rng.uniform(-3.0, 3.0, (nray, 8))
    tail[:, 0] = rng.uniform(-20.0, 20.0, nray)
    tail[:, 1] = rng.uniform(-1.8, 1.8, nray)
    tail[5::7, 0] = NAN
    tail[6::11, 5] = INF
    tail[8::13, 3] = NAN
    tail[:, 4] = NAN                                             # the amplitude is no criterion
    if tf is None:
        choice = sorted({i0 - 2, i0, i0 + 1, i0 + 3, i0 + 4, i0 + 5, i1 - 1, i1, i1 + 3})
        j = np.arange(nray)
        q = np.cumsum(j % 3 != 0)                                 # (the rays with a block take every value)
        tf = np.where(j % 3 == 0, np.array([i0 - 2, i0])[(j // 3) % 2], np.array(choice)[q % len(choice)])
    tf = np.asarray(tf, np.int32)
    cut = np.clip(tf, i0, i1)
    for j in range(nray):
        rows[j, cut[j] - i0:] = tail[j]
    # a slow ray whose tail continues its last bin: the run goes on into the tail
    for j in np.where(slow)[0]:
        if i0 < cut[j] < i1:
            tail[j] = rows[j, cut[j] - i0 - 1]
            rows[j, cut[j] - i0:] = tail[j]
    chan = rng.integers(-1, 4, nray).astype(np.int32)            # -1 and nchan = 3 among them
    return dict(i0=i0, i1=i1, rows=rows, tail=tail, tf=tf, chan=chan)


def columns(rows):
    return [rows[..., c] for c in (0, 1, 2, 3, 5, 6)]


def reference_of(launches, spec):
    """reference_flux of the launches' logical rows, summed; and their sum|v|."""
    parts = [reference_flux(*columns(L["rows"]), L["chan"], spec, row0=L["i0"]) for L in launches]
    want = {name: sum(p[name] for p in parts) for name in ("count", "rowsum", "sum")}
    return want, sum(abs_sums(*columns(L["rows"]), L["chan"], spec) for L in launches)
