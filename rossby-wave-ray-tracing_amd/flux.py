"""Wave-ray flux maps reduced on the GPU (``rwrt_ray_flux``, ABI 5).

The second stage of the reference's manual ("How to use the wave ray flux
program"): the traced rays, without the points of abnormal group velocity or
wavenumber and, if wanted, only those that pass through a target region,
reduced per lon-lat box to a vector -- the sum of the group velocities (or of
their directions) -- with the number of points, the sum of their row indices
and the sum of their speeds: the magnitude and the direction of wave
activity, the mean propagation time and the mean speed of the rays through
each box.  The longitude axis is the wrapped [0, 360) of the density maps or
an unwrapped window such as the manual's three circles (-360, 720), on which
eastward and westward routes across the date line stay apart (the ray loops
never wrap ``rlon``).  Accumulated from the row blocks and constant tails each
ray-loop launch leaves, like the ray-density map (density.py).  ``FluxSink``
plugs into ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume`` /
``shard.run_sharded`` through the ``sink`` protocol, alone or as a member of
``summary.Tee``; ``WR.ray_flux`` is the user entry point.

None of that stage ships with the reference, so ``reference_flux`` (NumPy) is
the definition.  The kernel reproduces ``count`` and ``rowsum`` exactly
(csrc/flux_rows.h restates the accept rule and the index arithmetic operation
for operation) and the three sums to the rounding of a sum taken in any order.
"""
import math
from dataclasses import dataclass

import numpy as np

import _hip as H
import density as D
from launch_rows import one_row, row_args
from raymap import ChannelSink, DeviceMap, GridSpec, counts_for, fold_arrays  # noqa: F401

VECTORS = ("velocity", "unit")
MODE_UNIT, MODE_UNWRAPPED = 1, 2


@dataclass(frozen=True)
class FluxSpec(GridSpec):
    """``nx`` bins over the longitude axis, ``ny`` over ``lat_range`` (degrees,
    upper edge excluded), ``nchan`` maps.  ``lon_range=None``: wrapped
    longitude, [0, 360), binned exactly like a ``density.DensitySpec``;
    ``lon_range=(a, b)`` in degrees: the unwrapped window, points outside it
    are dropped.  ``vector``: ``'velocity'`` sums ``(ug, vg)`` in m/s,
    ``'unit'`` sums ``(ug, vg) / speed``.  A point counts only with
    ``speed_range[0] <= speed <= speed_range[1]`` (compared as squares) and
    ``|k|, |l| <= wn_max``."""
    nx: int
    ny: int
    lat_range: tuple = (-90.0, 90.0)
    lon_range: tuple = None
    nchan: int = 1
    vector: str = "velocity"
    speed_range: tuple = (0.0, math.inf)
    wn_max: float = math.inf

    def __post_init__(self):
        self._check_shape()
        self._check_ranges()
        if self.vector not in VECTORS:
            raise ValueError(f"vector must be one of {VECTORS}")
        smin, smax = (float(v) for v in self.speed_range)
        if not (smin >= 0.0 and smax >= smin):
            raise ValueError("speed_range must be 0 <= smin <= smax")
        if not float(self.wn_max) >= 0.0:
            raise ValueError("wn_max must not be negative")

    # the squared speed bounds: computed here, once, in fp64, like the grid's
    # factors (raymap.GridSpec), and passed to the kernel
    @property
    def s2_min(self):
        return float(self.speed_range[0]) * float(self.speed_range[0])

    @property
    def s2_max(self):
        return float(self.speed_range[1]) * float(self.speed_range[1])

    @property
    def unit(self):
        return self.vector == "unit"

    @property
    def mode(self):
        return (MODE_UNIT if self.unit else 0) | (MODE_UNWRAPPED if self.unwrapped else 0)

    def c_struct(self):
        return H.FluxMapC(self.nx, self.ny, self.nchan, self.mode, self.lon0, self.inv_dlon, self.lat0,
                          self.inv_dlat, self.s2_min, self.s2_max, float(self.wn_max))


def accept(lon, lat, k, l, ug, vg, chan, spec):
    """``(index, vx, vy, speed)`` of every point: the flat bin index
    ``(c*ny + iy)*nx + ix``, -1 for a point that is not accepted, and what an
    accepted point contributes.  The accept rule and the index arithmetic of
    ``reference_flux``."""
    lon, lat, k, l, ug, vg = (np.asarray(a, np.float64) for a in (lon, lat, k, l, ug, vg))
    chan = np.zeros(lon.shape, np.int64) if chan is None else np.broadcast_to(np.asarray(chan, np.int64), lon.shape)
    with np.errstate(all="ignore"):
        ok = (chan >= 0) & (chan < spec.nchan)
        ok &= np.isfinite(lon) & np.isfinite(lat) & np.isfinite(ug) & np.isfinite(vg)
        ok &= (np.abs(k) <= spec.wn_max) & (np.abs(l) <= spec.wn_max)              # (false for NaN)
        s2 = ug * ug + vg * vg                                                    # two products, one sum
        ok &= np.isfinite(s2) & (s2 >= spec.s2_min) & (s2 <= spec.s2_max)
        if spec.unit:
            ok &= s2 > 0.0
        fy = np.floor((lat - spec.lat0) * spec.inv_dlat)
        ok &= (fy >= 0) & (fy < spec.ny)
        if spec.unwrapped:
            fx = np.floor((lon - spec.lon0) * spec.inv_dlon)
            ok &= (fx >= 0) & (fx < spec.nx)                                       # outside the window: dropped
        else:
            lam = np.remainder(np.remainder(lon, D.TWO_PI), D.TWO_PI)              # Python float %, twice
            fx = np.minimum(np.floor(lam * spec.inv_dlon), spec.nx - 1)
        # (the range was checked on the fp64 values; only those are converted)
        ix = np.where(ok, fx, 0).astype(np.int64)
        iy = np.where(ok, fy, 0).astype(np.int64)
        speed = np.sqrt(np.where(ok, s2, 1.0))
        vx, vy = (ug / speed, vg / speed) if spec.unit else (ug, vg)
    idx = np.where(ok, (np.where(ok, chan, 0) * spec.ny + iy) * spec.nx + ix, -1)
    return idx, vx, vy, speed


def reference_flux(lon, lat, k, l, ug, vg, chan, spec, row0=0):
    """The definition of a wave-ray flux map, in NumPy: a dict with ``count``
    and ``rowsum`` (``[nchan, ny, nx]`` int64: the accepted points of the bin
    and the sum of their global row indices) and ``sum`` (``[nchan, ny, nx, 3]``
    float64: fx, fy, fs).

    ``lon, lat`` (radians), ``k, l`` and ``ug, vg`` (m/s) are ``[nray, nrow]``,
    column ``r`` being global row ``row0 + r``; ``chan`` one channel per ray
    (None: channel 0).  A point is accepted iff ``0 <= c < nchan``; lon, lat,
    ug, vg are finite; ``|k| <= wn_max`` and ``|l| <= wn_max``;
    ``s2 = ug*ug + vg*vg`` is finite and ``s2_min <= s2 <= s2_max``; with unit
    vectors ``s2 > 0``; and it falls in a bin: ``iy = floor((lat - lat0) *
    inv_dlat)`` in ``[0, ny)`` and, wrapped, ``lam = (lon % 2pi) % 2pi``,
    ``ix = min(floor(lam * inv_dlon), nx - 1)``, or, unwrapped,
    ``ix = floor((lon - lon0) * inv_dlon)`` in ``[0, nx)`` (compared in fp64).
    It adds 1, its row index, and ``(vx, vy, speed)`` with ``speed = sqrt(s2)``
    and ``(vx, vy) = (ug, vg)`` or ``(ug, vg) / speed``.  The amplitude is no
    criterion.  Doubles as the ``mode='numpy'`` map of small runs."""
    lon = np.asarray(lon, np.float64)
    if lon.ndim != 2:
        raise ValueError("points must be [nray, nrow]")
    chan = None if chan is None else np.asarray(chan, np.int64).reshape(-1, 1)
    idx, vx, vy, speed = accept(lon, lat, k, l, ug, vg, chan, spec)
    row = np.broadcast_to(row0 + np.arange(lon.shape[1], dtype=np.int64), idx.shape)
    ok = idx >= 0
    idx = idx[ok]
    n = spec.nchan * spec.ny * spec.nx
    count = np.bincount(idx, minlength=n).astype(np.int64)
    rowsum = np.zeros(n, np.int64)
    np.add.at(rowsum, idx, row[ok])
    total = np.zeros((n, 3))
    for q, v in enumerate((vx, vy, speed)):
        np.add.at(total[:, q], idx, np.broadcast_to(v, ok.shape)[ok])
    return {"count": count.reshape(spec.shape), "rowsum": rowsum.reshape(spec.shape),
            "sum": total.reshape(spec.shape + (3,))}


class FluxMap(DeviceMap):
    """The device arrays of one map: ``cnt`` (int64 ``[nchan, ny, nx, 2]``:
    count, rowsum) and ``sum`` (fp64 ``[nchan, ny, nx, 3]``: fx, fy, fs),
    zeroed here and accumulated into by every ``add_rows`` / ``add_points``
    call (time chunks, shards).  A bin's accumulators are interleaved (the
    layout of ``rwrt_ray_flux``); ``count``, ``rowsum``, ``fx``, ``fy``, ``fs``
    are views; ``allreduce`` sums both tensors over the ranks.  ``selected``:
    set by ``WR.ray_flux(through=...)``."""
    REDUCE = (("cnt", "SUM"), ("sum", "SUM"))

    def __init__(self, spec, device=None):
        import torch
        super().__init__(spec, device)
        self.cnt = torch.zeros(spec.shape + (2,), dtype=torch.int64, device=self.device)
        self.sum = torch.zeros(spec.shape + (3,), dtype=torch.float64, device=self.device)
        self.selected = None

    count = property(lambda self: self.cnt[..., 0])
    rowsum = property(lambda self: self.cnt[..., 1])
    fx = property(lambda self: self.sum[..., 0])
    fy = property(lambda self: self.sum[..., 1])
    fs = property(lambda self: self.sum[..., 2])

    def add_rows(self, i0, i1, view, tails=None, slots=None, chan=None):
        """Reduce rows ``[i0, i1)`` of a launch (the arguments of
        ``density.DensityMap.add_rows``).  One asynchronous ``rwrt_ray_flux``
        call on the device's current stream."""
        import torch
        nray, rows = row_args(i0, i1, view, tails, slots)
        chan = self._chan(chan, nray)
        H.check(self._lib.rwrt_ray_flux(
            self._c, nray, int(i0), int(i1), *rows, H.dptr(chan, torch.int32), H.dptr(self.cnt, torch.int64),
            H.dptr(self.sum, torch.float64), H.stream(self.device)))

    def add_points(self, lon, lat, k, l, ug, vg, chan=None):
        """Single points (radians, m/s) as row 0: the initial rays, which
        sinks never receive."""
        self.add_rows(0, 1, one_row({0: lon, 1: lat, 2: k, 3: l, 5: ug, 6: vg}, self.device), chan=chan)

    def numpy(self):
        """``{'count', 'rowsum', 'sum'}`` on the host, as ``reference_flux``
        returns them (waits for the pending calls)."""
        cnt = self.cnt.cpu().numpy()
        return {"count": np.ascontiguousarray(cnt[..., 0]), "rowsum": np.ascontiguousarray(cnt[..., 1]),
                "sum": self.sum.cpu().numpy()}

    # ---- derived fields: device tensors [nchan, ny, nx], NaN where count == 0
    def _where_counted(self, x):
        import torch
        return torch.where(self.count > 0, x, torch.full_like(x, math.nan))

    def magnitude(self):
        """``|F| = hypot(fx, fy)``: m/s summed over the points, or the length
        of the summed unit vectors."""
        import torch
        return self._where_counted(torch.hypot(self.fx, self.fy))

    def direction(self):
        """The direction of F in degrees, ``atan2(fy, fx)``: 0 eastward, 90
        northward."""
        import torch
        return self._where_counted(torch.rad2deg(torch.atan2(self.fy, self.fx)))

    def coherence(self):
        """How parallel the contributions are, in [0, 1]: ``|F| / fs`` for
        velocity vectors, ``|F| / count`` for unit vectors."""
        import torch
        den = self.count.to(torch.float64) if self.spec.unit else self.fs
        return self._where_counted(torch.hypot(self.fx, self.fy) / den)

    def mean_speed(self):
        """``fs / count`` in m/s."""
        import torch
        return self._where_counted(self.fs / self.count.to(torch.float64))

    def mean_days(self, tstep):
        """The mean propagation time of the points of a bin in days:
        ``rowsum / count * tstep / 86400``."""
        import torch
        return self._where_counted(self.rowsum.to(torch.float64) / self.count.to(torch.float64)
                                   * float(tstep) / 86400.0)

    def fold(self):
        """A new wrapped map: this unwrapped map, whose window is whole
        circles, summed onto [0, 360).  Needs ``nx`` divisible by the number
        of circles."""
        spec, (cnt, total) = fold_arrays(self.spec, self.cnt, self.sum)
        m = FluxMap(spec, self.device)
        m.cnt.copy_(cnt)
        m.sum.copy_(total)
        m.selected = self.selected
        return m

    def output(self, ncfile):
        """Write the map (dims ``chan, lat, lon``; bin centres in degrees).
        netCDF-3 has no 64-bit integers: ``count`` and ``rowsum`` go out as
        float64 there (exact below 2^53), as int64 into an ``.npz``."""
        import ncio
        a = self.numpy()
        dims, v = self._grid_output()
        full = ("chan", "lat", "lon")
        what = "unit vectors" if self.spec.unit else "m s-1"
        v.update({"count": (full, counts_for(ncfile, a["count"]), "ray points"),
                  "rowsum": (full, counts_for(ncfile, a["rowsum"]), "sum of output rows"),
                  "fx": (full, np.ascontiguousarray(a["sum"][..., 0]), "sum of " + what),
                  "fy": (full, np.ascontiguousarray(a["sum"][..., 1]), "sum of " + what),
                  "fs": (full, np.ascontiguousarray(a["sum"][..., 2]), "sum of speeds, m s-1")})
        ncio.write(ncfile, dims, v)


class FluxSink(ChannelSink):
    """A ``sink`` of ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume``
    and of ``shard.run_sharded`` (``launch_rows.RowSink``) that reduces each
    launch's rows into ``map``.  ``chan``: each ray's channel (length nray;
    with ``run_sharded`` indexed by the shard's ``idx``; None: channel 0); a
    ray with channel -1 contributes nothing."""


def select_through(summary, mode="any"):
    """The rays that pass through the regions of ``summary`` (a
    ``summary.RaySummary`` with regions): a bool device tensor per ray, true
    where ``first_row[r] >= 0`` for any (``mode='any'``) or every
    (``mode='all'``) region r."""
    if mode not in ("any", "all"):
        raise ValueError("mode must be 'any' or 'all'")
    if summary.nreg == 0:
        raise ValueError("the summary has no regions")
    inside = summary.i32[H.SUMMARY_NI32:H.SUMMARY_NI32 + summary.nreg] >= 0
    return inside.any(dim=0) if mode == "any" else inside.all(dim=0)
