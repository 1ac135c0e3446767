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
from dataclasses import dataclass, replace

import numpy as np

import _hip as H
from launch_rows import RowSink, one_row, row_args

WEIGHT_COLUMNS = {"k": 2, "l": 3, "amp": 4, "ug": 5, "vg": 6}   # columns of the 8-column output row
TWO_PI = 2 * math.pi


@dataclass(frozen=True)
class DensitySpec:
    """``nx`` bins over longitude [0, 360), ``ny`` bins over ``lat_range``
    (degrees, upper edge excluded), ``nchan`` maps, and an optional weight:
    a row column by name (``'amp'``, ``'k'``, ``'l'``, ``'ug'``, ``'vg'``)
    whose sum per bin is kept next to the count."""
    nx: int
    ny: int
    lat_range: tuple = (-90.0, 90.0)
    nchan: int = 1
    weight: str = None

    def __post_init__(self):
        if self.nx <= 0 or self.ny <= 0 or self.nchan <= 0:
            raise ValueError("nx, ny and nchan must be positive")
        if self.nx * self.ny * self.nchan >= 2 ** 31:
            raise ValueError("nchan*ny*nx must be below 2^31")
        if self.weight is not None and self.weight not in WEIGHT_COLUMNS:
            raise ValueError(f"weight must be None or one of {sorted(WEIGHT_COLUMNS)}")
        if not self.lat_range[1] > self.lat_range[0]:
            raise ValueError("lat_range must be ascending")

    # pi * (deg / 180): +-90 give +-pi/2 exactly
    @property
    def lat0(self):
        return math.pi * (float(self.lat_range[0]) / 180.0)

    @property
    def lat1(self):
        return math.pi * (float(self.lat_range[1]) / 180.0)

    @property
    def wcol(self):
        return -1 if self.weight is None else WEIGHT_COLUMNS[self.weight]

    # the two factors of the index arithmetic: computed here, once, in fp64,
    # and passed to the kernel (never recomputed on the device)
    @property
    def inv_dlon(self):
        return self.nx / (2 * math.pi)

    @property
    def inv_dlat(self):
        return self.ny / (self.lat1 - self.lat0)

    @property
    def shape(self):
        return (self.nchan, self.ny, self.nx)

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


class DensityMap:
    """The device arrays of one map: ``count`` (int64) and ``wsum`` (fp64, None
    without a weight), each ``[nchan, ny, nx]``, zeroed here and accumulated
    into by every ``add_rows`` / ``add_points`` call (time chunks, shards)."""

    def __init__(self, spec, device=None):
        import torch
        H.require_gpu()
        H.load()
        self.spec = spec
        self.device = torch.device(device or "cuda")
        self.count = torch.zeros(spec.shape, dtype=torch.int64, device=self.device)
        self.wsum = torch.zeros(spec.shape, dtype=torch.float64, device=self.device) if spec.wcol >= 0 else None
        self._c = spec.c_struct()

    def _chan(self, chan, nray):
        import torch
        if chan is None:
            return None
        chan = torch.as_tensor(chan, device=self.device).to(torch.int32).contiguous()
        if chan.numel() != nray:
            raise ValueError(f"chan has {chan.numel()} entries for {nray} rays")
        return chan

    def add_rows(self, i0, i1, view, tails=None, slots=None, chan=None):
        """Bin rows ``[i0, i1)`` of a launch: ``view`` its row buffer (dense
        ``[nray, i1-i0, 8]``, or the row blocks of ``slots``), ``tails`` /
        ``slots`` the launch's ``engine.Tails`` / ``engine.Slots``, ``chan``
        each ray's channel (int32 device tensor; None: channel 0).  One
        asynchronous ``rwrt_ray_density`` call on the device's current stream."""
        import torch
        nray, rows = row_args(i0, i1, view, tails, slots)
        chan = self._chan(chan, nray)
        H.check(H.load().rwrt_ray_density(
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

    def allreduce(self, group=None):
        """SUM of the maps of every rank of ``group`` (``torch.distributed.all_reduce``
        of both tensors), left on every rank."""
        import torch.distributed as dist
        from shard import _dev
        for name in ("count", "wsum"):
            t = getattr(self, name)
            if t is None:
                continue
            x = t.to(_dev(group))
            dist.all_reduce(x, op=dist.ReduceOp.SUM, group=group)
            if x is not t:
                t.copy_(x)
        return self

    def numpy(self):
        """``(count, wsum)`` on the host (waits for the pending calls)."""
        return self.count.cpu().numpy(), None if self.wsum is None else self.wsum.cpu().numpy()

    @property
    def lon_edges(self):
        """The ``nx + 1`` longitude bin edges in degrees."""
        return np.linspace(0.0, 360.0, self.spec.nx + 1)

    @property
    def lat_edges(self):
        """The ``ny + 1`` latitude bin edges in degrees."""
        return np.linspace(float(self.spec.lat_range[0]), float(self.spec.lat_range[1]), self.spec.ny + 1)

    def output(self, ncfile):
        """Write the map (dims ``chan, lat, lon``; bin centres in degrees).
        netCDF-3 has no 64-bit integers: counts go out as float64 there (exact
        below 2^53), as int64 into an ``.npz``."""
        import ncio
        count, wsum = self.numpy()
        s = self.spec
        le, la = self.lon_edges, self.lat_edges
        if not str(ncfile).endswith(".npz"):
            count = count.astype(np.float64)
        dims = {"chan": s.nchan, "lat": s.ny, "lon": s.nx, "lat_edge": s.ny + 1, "lon_edge": s.nx + 1}
        v = {"lon": (("lon",), 0.5 * (le[:-1] + le[1:]), "degrees"),
             "lat": (("lat",), 0.5 * (la[:-1] + la[1:]), "degrees"),
             "lon_edges": (("lon_edge",), le, "degrees"), "lat_edges": (("lat_edge",), la, "degrees"),
             "count": (("chan", "lat", "lon"), count, "ray points")}
        if wsum is not None:
            v["wsum"] = (("chan", "lat", "lon"), wsum, f"sum of {s.weight}")
        ncio.write(ncfile, dims, v)


class DensitySink(RowSink):
    """A ``sink`` of ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume``
    and of ``shard.run_sharded`` (``launch_rows.RowSink``) that bins each
    launch's rows into ``map``.  ``chan``: each ray's channel (length nray;
    with ``run_sharded`` indexed by the shard's ``idx``; None: channel 0)."""

    def __init__(self, map, chan=None):
        super().__init__(map, None if chan is None else map._chan(chan, len(chan)))
        self.map = map

    chan = property(lambda self: self.per_ray)

    def select(self, idx):
        return None if self.per_ray is None else self.per_ray[idx]


def with_channels(spec, nchan):
    """``spec`` with ``nchan`` maps."""
    return replace(spec, nchan=int(nchan))
