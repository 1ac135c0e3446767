"""Corner points, random points and crafted launches of the density tests, which
the other map products' tests borrow."""
import math

import numpy as np

from density import DensitySpec

TWO_PI = 2 * math.pi
HALF_PI = math.pi / 2
INF, NAN = math.inf, math.nan


SPEC = DensitySpec(7, 5, nchan=2, weight="amp")     # 7 x 5 boxes of 51.4 x 36 degrees, two maps


def corner_points():
    """``(lon, lat, w, chan, expected)``: expected = (chan, iy, ix) written out
    by hand, None for a point that is not binned."""
    lat0, lat1 = -HALF_PI, HALF_PI
    mid = 0.1          # (0.1 + pi/2) * 5/pi = 2.66 -> iy 2
    pts = [
        # longitudes (box width 2 pi / 7 = 0.8976 rad)
        (0.0, mid, 1.0, 0, (0, 2, 0)),
        (TWO_PI, mid, 1.0, 0, (0, 2, 0)),                       # 2 pi % 2 pi = 0
        (-1e-20, mid, 1.0, 0, (0, 2, 0)),                       # % gives 2 pi, the second % gives 0
        (math.nextafter(TWO_PI, 0.0), mid, 1.0, 0, (0, 2, 6)),  # the product floors to 7.0: clamped
        (63.69, mid, 1.0, 0, (0, 2, 0)),                        # 63.69 - 10 * 2 pi = 0.858
        (-5.0, mid, 1.0, 0, (0, 2, 1)),                         # 2 pi - 5 = 1.283
        (3.2, mid, 1.0, 0, (0, 2, 3)),                          # 3.2 / 0.8976 = 3.57
        # latitudes (box height pi / 5 = 0.6283 rad), map 1, lon 1.0 -> ix 1
        (1.0, lat0, 1.0, 1, (1, 0, 1)),
        # the last double below lat1: lat - lat0 rounds (to even) to pi itself, times 5/pi is 5.0 -> outside,
        # as NumPy has it; two ulps further down the difference is below pi and the point is in the top row
        (1.0, math.nextafter(lat1, 0.0), 1.0, 1, None),
        (1.0, lat1 - 1e-9, 1.0, 1, (1, 4, 1)),
        (1.0, lat1, 1.0, 1, None),                              # the upper edge is excluded
        (1.0, math.nextafter(lat0, -INF), 1.0, 1, None),
        (1.0, -0.3, 1.0, 1, (1, 2, 1)),                         # (-0.3 + pi/2) * 5/pi = 2.02
        (1.0, -0.32, 1.0, 1, (1, 1, 1)),                        # 1.99
        # non-finite and huge values
        (NAN, mid, 1.0, 0, None), (INF, mid, 1.0, 0, None), (-INF, mid, 1.0, 0, None),
        (1.0, NAN, 1.0, 0, None), (1.0, INF, 1.0, 0, None), (1.0, -INF, 1.0, 0, None),
        (1.0, 1e300, 1.0, 0, None), (1.0, -1e300, 1.0, 0, None),
        (1.0, mid, NAN, 0, None), (1.0, mid, INF, 0, None), (1.0, mid, -INF, 0, None),
        (1.0, mid, 1e300, 0, (0, 2, 1)), (2.0, mid, -1e300, 0, (0, 2, 2)),   # finite weights count
        # channels outside [0, nchan)
        (1.0, mid, 1.0, -1, None), (1.0, mid, 1.0, 2, None),
    ]
    # a huge finite longitude is binned where Python's % puts it
    for big in (1e300, -1e300):
        lam = (big % TWO_PI) % TWO_PI
        pts.append((big, mid, 1.0, 1, (1, 2, min(math.floor(lam * SPEC.inv_dlon), 6))))
    return pts


def scalar_bin(lon, lat, w, c, spec):
    """The definition of the issue, point by point in Python floats."""
    if not (math.isfinite(lon) and math.isfinite(lat)) or not 0 <= c < spec.nchan:
        return None
    if spec.wcol >= 0 and not math.isfinite(w):
        return None
    lam = (lon % TWO_PI) % TWO_PI
    ix = min(math.floor(lam * spec.inv_dlon), spec.nx - 1)
    fy = (lat - spec.lat0) * spec.inv_dlat
    if not math.isfinite(fy) or not 0 <= math.floor(fy) < spec.ny:
        return None
    return (c, math.floor(fy), ix)


def random_points(n, spec, seed=0):
    rng = np.random.default_rng(seed)
    lon = rng.uniform(-70.0, 70.0, n)
    lat = rng.uniform(spec.lat0 - 0.2, spec.lat1 + 0.2, n)
    w = rng.uniform(-2.0, 2.0, n)
    chan = rng.integers(-1, spec.nchan + 1, n)
    # some exactly on box edges, some non-finite
    k = n // 10
    lon[:k] = rng.integers(-20, 20, k) * (TWO_PI / spec.nx)
    lat[k:2 * k] = spec.lat0 + rng.integers(-1, spec.ny + 2, k) * ((spec.lat1 - spec.lat0) / spec.ny)
    lon[2 * k:2 * k + 20] = NAN
    lat[2 * k + 20:2 * k + 40] = INF
    w[2 * k + 40:2 * k + 60] = NAN
    return lon, lat, w, chan


# ------------------------------------------------- crafted rows on the device
NRAY, I0, I1 = 130, 1, 8     # three waves, the last partial; 7 rows


def crafted(seed=0, tf=None):
    """Logical rows ``[130, 7, 8]`` that all three layouts can hold: ray j's
    rows from ``tf[j]`` on repeat its tail row; tf = it_begin / middle / it_end
    by j % 3 (the j % 3 == 0 rays have no row block in the slots layout), or
    the ``tf`` given, which may lie outside ``[I0, I1]`` (and is at most I0 for
    those rays)."""
    rng = np.random.default_rng(seed)
    nrow = I1 - I0
    rows = rng.uniform(-3.0, 3.0, (NRAY, nrow, 8))
    rows[..., 0] = rng.uniform(-70.0, 70.0, (NRAY, nrow))
    rows[..., 1] = rng.uniform(-1.8, 1.8, (NRAY, nrow))
    pts = corner_points()
    flat = rows.reshape(-1, 8)
    where = rng.choice(flat.shape[0], len(pts), replace=False)
    for k, p in zip(where, pts):
        flat[k, 0], flat[k, 1], flat[k, 4] = p[0], p[1], p[2]
    tail = rng.uniform(-3.0, 3.0, (NRAY, 8))
    tail[:, 0] = rng.uniform(-70.0, 70.0, NRAY)
    tail[:, 1] = rng.uniform(-1.8, 1.8, NRAY)
    tail[5::7, 0] = np.nan                      # frozen NaN rays
    tail[6::11, 4] = np.inf                     # a non-finite weight in a tail
    tf = np.array([I0, I0 + 3, I1], np.int32)[np.arange(NRAY) % 3] if tf is None else np.asarray(tf, np.int32)
    cut = np.clip(tf, I0, I1)
    for j in range(NRAY):
        rows[j, cut[j] - I0:] = tail[j]
    return rows, tail, tf


def launch(rows, tail, tf):
    """The crafted rows as a launch of support/rows.py."""
    return dict(i0=I0, i1=I1, rows=rows, tail=tail, tf=tf)


# tail_from below, at and above the launch, and rows read on either side of the kernel's batch of 4
BOUNDARY_TF = (I0 - 2, I0, I0 + 1, I0 + 3, I0 + 4, I0 + 5, I1, I1 + 3)
