"""Ray-density maps binned on the GPU (``rwrt_ray_density``, ABI 5).

How many ray points fall into each box of a regular lon-lat map -- optionally
weighted by a row column (the amplitude) and split into channels per ray
(zonal wavenumber, root) -- accumulated on the device from the row blocks and
constant tails each ray-loop launch leaves, so that no output row is shipped
to the host.  ``DensitySink`` plugs into ``RayEngine.integrate`` /
``integrate_rk4`` / ``resume`` / ``shard.run_sharded`` through the ``sink``
protocol; ``WR.ray_density`` is the user entry point.

``reference_bins`` (NumPy) is the definition: the kernel reproduces its counts
exactly (csrc/density_bins.h restates its index arithmetic operation for
operation).  Sampling is the output rows, i.e. residence time at ``tstep``
resolution; NaN rays (dead root slots, masked rays) contribute nothing.
"""
import math
from dataclasses import dataclass

import numpy as np

import _hip as H
from launch_rows import one_row, row_args
from raymap import WEIGHT_COLUMNS, ChannelSink, DeviceMap, GridSpec, check_columns, counts_for, with_channels  # noqa: F401

TWO_PI = 2 * math.pi


@dataclass(frozen=True)
class DensitySpec(GridSpec):
    """``nx`` bins over longitude [0, 360), ``ny`` bins over ``lat_range``
    (degrees, upper edge excluded), ``nchan`` maps, and an optional weight:
    a row column by name (``'amp'``, ``'k'``, ``'l'``, ``'ug'``, ``'vg'``)
    whose sum per bin is kept next to the count.  The grid is
    ``raymap.GridSpec``'s."""
    nx: int
    ny: int
    lat_range: tuple = (-90.0, 90.0)
    nchan: int = 1
    weight: str = None

    def __post_init__(self):
        self._check_shape()
        check_columns(self, "weight")
        self._check_ranges()

    def c_struct(self):
        return H.DensityMap(self.nx, self.ny, self.nchan, self.wcol, self.inv_dlon, self.lat0, self.inv_dlat)


def bin_index(lon, lat, w, chan, spec):
    """Flat bin index ``(c*ny + iy)*nx + ix`` of every point (-1: not binned):
    the index arithmetic of ``reference_bins``."""
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    chan = np.zeros(lon.shape, np.int64) if chan is None else np.broadcast_to(np.asarray(chan, np.int64), lon.shape)
    with np.errstate(all="ignore"):
        lam = np.remainder(np.remainder(lon, TWO_PI), TWO_PI)     # Python float %, twice
        fx = np.minimum(np.floor(lam * spec.inv_dlon), spec.nx - 1)
        fy = np.floor((lat - spec.lat0) * spec.inv_dlat)
        ok = np.isfinite(lon) & np.isfinite(lat) & (fy >= 0) & (fy < spec.ny) & (chan >= 0) & (chan < spec.nchan)
        if spec.wcol >= 0:
            ok &= np.isfinite(np.broadcast_to(np.asarray(w, np.float64), lon.shape))
        # (the range was checked on the fp64 values; only those are converted)
        ix = np.where(ok, fx, 0).astype(np.int64)
        iy = np.where(ok, fy, 0).astype(np.int64)
    return np.where(ok, (np.where(ok, chan, 0) * spec.ny + iy) * spec.nx + ix, -1)


def reference_bins(lon, lat, w, chan, spec):
    """The definition of a ray-density map, in NumPy: ``(count, wsum)`` with
    ``count[nchan, ny, nx]`` int64 and ``wsum`` float64 (None without a weight).

    ``lon, lat`` (radians) and ``w`` have one shape; ``chan`` (None: channel 0)
    broadcasts against it (per ray: ``chan[:, None]`` for ``[nray, rows]``
    points).  For a point of a ray with channel c:
    ``lam = (lon % 2pi) % 2pi``, ``ix = min(floor(lam * inv_dlon), nx - 1)``,
    ``iy = floor((lat - lat0) * inv_dlat)``; it is binned iff lon and lat are
    finite, ``0 <= iy < ny`` (compared in fp64), ``0 <= c < nchan`` and, with a
    weight, w is finite.  Doubles as the ``mode='numpy'`` map of small runs."""
    idx = bin_index(lon, lat, w, chan, spec).reshape(-1)
    ok = idx >= 0
    n = spec.nchan * spec.ny * spec.nx
    count = np.bincount(idx[ok], minlength=n).astype(np.int64).reshape(spec.shape)
    wsum = None
    if spec.wcol >= 0:
        wv = np.broadcast_to(np.asarray(w, np.float64), np.shape(lon)).reshape(-1)
        wsum = np.zeros(n)
        np.add.at(wsum, idx[ok], wv[ok])
        wsum = wsum.reshape(spec.shape)
    return count, wsum


class DensityMap(DeviceMap):
    """The device arrays of one map: ``count`` (int64) and ``wsum`` (fp64, None
    without a weight), each ``[nchan, ny, nx]``, zeroed here and accumulated
    into by every ``add_rows`` / ``add_points`` call (time chunks, shards);
    ``allreduce`` sums both over the ranks."""
    REDUCE = (("count", "SUM"), ("wsum", "SUM"))

    def __init__(self, spec, device=None):
        import torch
        super().__init__(spec, device)
        self.count = torch.zeros(spec.shape, dtype=torch.int64, device=self.device)
        self.wsum = torch.zeros(spec.shape, dtype=torch.float64, device=self.device) if spec.wcol >= 0 else None

    def add_rows(self, i0, i1, view, tails=None, slots=None, chan=None):
        """Bin rows ``[i0, i1)`` of a launch: ``view`` its row buffer (dense
        ``[nray, i1-i0, 8]``, or the row blocks of ``slots``), ``tails`` /
        ``slots`` the launch's ``engine.Tails`` / ``engine.Slots``, ``chan``
        each ray's channel (int32 device tensor; None: channel 0).  One
        asynchronous ``rwrt_ray_density`` call on the device's current stream."""
        import torch
        nray, rows = row_args(i0, i1, view, tails, slots)
        chan = self._chan(chan, nray)
        H.check(self._lib.rwrt_ray_density(
            self._c, nray, int(i0), int(i1), *rows, H.dptr(chan, torch.int32), H.dptr(self.count, torch.int64),
            H.dptr(self.wsum), H.stream(self.device)))

    def add_points(self, lon, lat, w=None, chan=None):
        """Bin single points (radians): the same entry point on a ``[n, 1, 8]``
        row tensor.  Used for row 0 (the initial rays), which sinks never
        receive."""
        cols = {0: lon, 1: lat}
        if self.spec.wcol >= 0:
            if w is None:
                raise ValueError(f"the map sums {self.spec.weight!r}: pass w")
            cols[self.spec.wcol] = w
        self.add_rows(0, 1, one_row(cols, self.device), chan=chan)

    def numpy(self):
        """``(count, wsum)`` on the host (waits for the pending calls)."""
        return self.count.cpu().numpy(), None if self.wsum is None else self.wsum.cpu().numpy()

    def output(self, ncfile):
        """Write the map (dims ``chan, lat, lon``; bin centres in degrees).
        netCDF-3 has no 64-bit integers: counts go out as float64 there (exact
        below 2^53), as int64 into an ``.npz``."""
        import ncio
        count, wsum = self.numpy()
        dims, v = self._grid_output()
        v["count"] = (("chan", "lat", "lon"), counts_for(ncfile, count), "ray points")
        if wsum is not None:
            v["wsum"] = (("chan", "lat", "lon"), wsum, f"sum of {self.spec.weight}")
        ncio.write(ncfile, dims, v)


class DensitySink(ChannelSink):
    """A ``sink`` of ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume``
    and of ``shard.run_sharded`` (``launch_rows.RowSink``) that bins each
    launch's rows into ``map``.  ``chan``: each ray's channel (length nray;
    with ``run_sharded`` indexed by the shard's ``idx``; None: channel 0)."""
