"""Arrival-time maps reduced on the GPU (``rwrt_ray_arrival``, ABI 5).

When does wave activity from the source set reach a place?  Per box of a
regular lon-lat map the first and the last output row with a ray point in it
and, per time window of ``window_rows`` rows, how many points -- a travel-time
map and a longitude-time (Hovmoeller) picture without the history ever leaving
the device.  Accumulated from the row blocks and constant tails each ray-loop
launch leaves, like the ray-density map (density.py) whose bins these are.
``ArrivalSink`` plugs into ``RayEngine.integrate`` / ``integrate_rk4`` /
``resume`` / ``shard.run_sharded`` through the ``sink`` protocol, alone or as
a member of ``summary.Tee``; ``WR.ray_arrival`` is the user entry point.

``reference_arrival`` (NumPy) is the definition.  Every output is an integer
and the kernel reproduces it exactly (csrc/arrival_rows.h).
"""
from dataclasses import dataclass

import numpy as np

import _hip as H
import density as D
from launch_rows import one_row, row_args
from raymap import ChannelSink, DeviceMap, check_columns, counts_for

INT32_MAX = 2 ** 31 - 1


@dataclass(frozen=True)
class ArrivalSpec:
    """The bins of a ``density.DensitySpec`` (``nx, ny, lat_range, nchan``) and
    the time axis: ``nt`` rows of the integration (row 0 included) in windows
    of ``window_rows`` rows (None: no time-resolved counts).  ``require``: a row
    column by name (``density.WEIGHT_COLUMNS``) that must be finite for a point
    to count, or None.  The default ``'amp'`` keeps dead root slots out: they
    hold their source position with a NaN amplitude on every row."""
    nx: int
    ny: int
    nt: int
    lat_range: tuple = (-90.0, 90.0)
    nchan: int = 1
    require: str = "amp"
    window_rows: int = None

    def __post_init__(self):
        check_columns(self, "require")
        self.bins                                        # (validates nx, ny, nchan, lat_range)
        if int(self.nt) != self.nt or not 1 <= self.nt <= INT32_MAX:
            raise ValueError("nt must be an integer of at least 1")
        if self.window_rows is not None:
            if int(self.window_rows) != self.window_rows or not 1 <= self.window_rows <= INT32_MAX:
                raise ValueError("window_rows must be None or an integer of at least 1")
            if self.nwin * self.nchan * self.ny * self.nx >= 2 ** 31:
                raise ValueError("nwin*nchan*ny*nx must be below 2^31")

    @property
    def bins(self):
        """The ``density.DensitySpec`` of the bins; its weight is ``require``,
        read as "the column that must be finite"."""
        return D.DensitySpec(self.nx, self.ny, self.lat_range, self.nchan, self.require)

    @property
    def nwin(self):
        """``ceil(nt / window_rows)``; 0 without windows."""
        return 0 if self.window_rows is None else -(-int(self.nt) // int(self.window_rows))

    @property
    def shape(self):
        return (self.nchan, self.ny, self.nx)

    @property
    def count_shape(self):
        return (self.nwin,) + self.shape

    def c_struct(self):
        return H.ArrivalMap(self.bins.c_struct(), int(self.window_rows or 0), self.nwin)


def reference_arrival(lon, lat, req, chan, spec, row0=0):
    """The definition of an arrival-time map, in NumPy: a dict with ``first``
    and ``last`` (``[nchan, ny, nx]`` int32: the smallest / largest global row
    index of a counted point of the bin, -1 where there is none) and ``count``
    (``[nwin, nchan, ny, nx]`` int64: the counted points whose row ``i`` has
    ``i // window_rows == window``; None without windows).

    ``lon, lat`` (radians) and ``req`` are ``[nray, nrow]``, column ``r`` being
    global row ``row0 + r``; ``chan`` one channel per ray (None: channel 0).  A
    point counts iff ``density.bin_index`` bins it with ``spec.require`` as the
    weight column.  Doubles as the ``mode='numpy'`` map of small runs."""
    lon = np.asarray(lon, np.float64)
    if lon.ndim != 2:
        raise ValueError("points must be [nray, nrow]")
    nrow = lon.shape[1]
    if row0 < 0 or row0 + nrow > spec.nt:
        raise ValueError(f"rows [{row0}, {row0 + nrow}) are outside the {spec.nt} rows of the spec")
    chan = None if chan is None else np.asarray(chan, np.int64).reshape(-1, 1)
    idx = D.bin_index(lon, lat, req, chan, spec.bins)
    row = np.broadcast_to(row0 + np.arange(nrow, dtype=np.int64), idx.shape)
    ok = idx >= 0
    idx, row = idx[ok], row[ok]
    n = spec.nchan * spec.ny * spec.nx
    first = np.full(n, INT32_MAX, np.int64)
    np.minimum.at(first, idx, row)
    first[first == INT32_MAX] = -1
    last = np.full(n, -1, np.int64)
    np.maximum.at(last, idx, row)
    count = None
    if spec.window_rows is not None:
        count = np.bincount((row // spec.window_rows) * n + idx, minlength=spec.nwin * n)
        count = count.astype(np.int64).reshape(spec.count_shape)
    return {"first": first.astype(np.int32).reshape(spec.shape), "last": last.astype(np.int32).reshape(spec.shape),
            "count": count}


class ArrivalMap(DeviceMap):
    """The device arrays of one map: ``first`` (int32, ``INT32_MAX``: none yet)
    and ``last`` (int32, -1: none yet), each ``[nchan, ny, nx]``, and ``count``
    (int64 ``[nwin, nchan, ny, nx]``, None without windows), initialised here
    and accumulated into by every ``add_rows`` / ``add_points`` call (time
    chunks, shards) with min, max and add; ``allreduce`` combines the ranks'
    maps the same way."""
    REDUCE = (("first", "MIN"), ("last", "MAX"), ("count", "SUM"))

    def __init__(self, spec, device=None):
        import torch
        super().__init__(spec, device)
        self.first = torch.full(spec.shape, INT32_MAX, dtype=torch.int32, device=self.device)
        self.last = torch.full(spec.shape, -1, dtype=torch.int32, device=self.device)
        self.count = None
        if spec.window_rows is not None:
            self.count = torch.zeros(spec.count_shape, dtype=torch.int64, device=self.device)

    def add_rows(self, i0, i1, view, tails=None, slots=None, chan=None):
        """Reduce rows ``[i0, i1)`` of a launch (the arguments of
        ``density.DensityMap.add_rows``).  One asynchronous
        ``rwrt_ray_arrival`` call on the device's current stream."""
        import torch
        if i1 > self.spec.nt:
            raise ValueError(f"row {i1 - 1} is outside the {self.spec.nt} rows of the spec")
        nray, rows = row_args(i0, i1, view, tails, slots)
        chan = self._chan(chan, nray)
        H.check(self._lib.rwrt_ray_arrival(
            self._c, nray, int(i0), int(i1), *rows, H.dptr(chan, torch.int32), H.dptr(self.first, torch.int32),
            H.dptr(self.last, torch.int32), H.dptr(self.count, torch.int64), H.stream(self.device)))

    def add_points(self, lon, lat, req=None, chan=None):
        """Single points (radians) as row 0: the initial rays, which sinks
        never receive."""
        cols = {0: lon, 1: lat}
        col = self.spec.bins.wcol
        if col >= 0:
            if req is None:
                raise ValueError(f"the map requires {self.spec.require!r}: pass req")
            cols[col] = req
        self.add_rows(0, 1, one_row(cols, self.device), chan=chan)

    def numpy(self):
        """``{'first', 'last', 'count'}`` on the host (waits for the pending
        calls); ``first`` is -1 where no point fell."""
        first = self.first.cpu().numpy()
        return {"first": np.where(first == INT32_MAX, np.int32(-1), first), "last": self.last.cpu().numpy(),
                "count": None if self.count is None else self.count.cpu().numpy()}

    def days(self, tstep):
        """The first arrival in days (``first * tstep / 86400``, fp64), NaN
        where no point fell."""
        first = self.numpy()["first"]
        return np.where(first >= 0, first * float(tstep) / 86400.0, np.nan)

    def hovmoller(self, lat_s, lat_n):
        """``count`` summed over the latitude rows whose bin centres lie in
        ``[lat_s, lat_n]`` degrees: a device tensor ``[nwin, nchan, nx]``."""
        import torch
        if self.count is None:
            raise ValueError("the map has no time windows (window_rows is None)")
        la = self.lat_edges
        centre = 0.5 * (la[:-1] + la[1:])
        rows = torch.as_tensor(np.nonzero((centre >= lat_s) & (centre <= lat_n))[0], device=self.device)
        return self.count.index_select(2, rows).sum(dim=2)

    def output(self, ncfile):
        """Write the map (dims ``window, chan, lat, lon``; bin centres in
        degrees).  ``first`` and ``last`` are int32; netCDF-3 has no 64-bit
        integers: counts go out as float64 there (exact below 2^53), as int64
        into an ``.npz``."""
        import ncio
        a = self.numpy()
        s = self.spec
        dims, v = self._grid_output()
        v["first"] = (("chan", "lat", "lon"), a["first"], "output row (-1: none)")
        v["last"] = (("chan", "lat", "lon"), a["last"], "output row (-1: none)")
        if a["count"] is not None:
            dims["window"] = s.nwin
            v["window_row"] = (("window",), np.arange(s.nwin, dtype=np.int32) * s.window_rows, "first output row")
            v["count"] = (("window", "chan", "lat", "lon"), counts_for(ncfile, a["count"]), "ray points")
        ncio.write(ncfile, dims, v)


class ArrivalSink(ChannelSink):
    """A ``sink`` of ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume``
    and of ``shard.run_sharded`` (``launch_rows.RowSink``) that reduces each
    launch's rows into ``map``.  ``chan``: each ray's channel (length nray;
    with ``run_sharded`` indexed by the shard's ``idx``; None: channel 0)."""
