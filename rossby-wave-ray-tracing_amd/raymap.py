"""What the products that reduce a launch's rows on the device share.

The ray-density, arrival-time, flux, residence-time, gate-crossing and
wave-field maps (density.py, arrival.py, flux.py, track.py, cross.py, phase.py)
and the per-ray summaries (summary.py) each have a kernel, a NumPy reference
and device arrays of their own.  Around those they are the same, and that part is here, once:

  ``GridSpec``      the lon-lat grid of a spec: its validation and the factors
                    of the index arithmetic (``LatBand``: the latitude part;
                    ``RowColumns``: the ``need`` / ``weight`` row columns);
  ``DeviceMap``     ``spec, device, _c, _lib``, the per-ray arguments ``_chan``
                    / ``_ray`` (``RayArgs``), the bin edges, the grid variables
                    of ``output()`` and one ``allreduce`` driven by the class's
                    ``REDUCE`` table (``allreduce_tensors``);
  ``CarriedMap``    a map with each ray's carried previous row (``prev``,
                    ``chan`` by column, ``restart``, ``start``);
  ``ChannelSink``, ``ColumnSink``
                    the two ``launch_rows.RowSink`` kinds: a channel per ray
                    (None stays None) and a column per ray (None: the ray's
                    index itself).

A new product writes its spec fields, its device arrays, its ``REDUCE`` table,
its kernel call (``add_rows``) and its reference function.
"""
import math
from dataclasses import replace

import numpy as np

import _hip as H
from launch_rows import RowSink, one_row

WEIGHT_COLUMNS = {"k": 2, "l": 3, "amp": 4, "ug": 5, "vg": 6}   # columns of the 8-column output row


def radians(deg):
    """``pi * (deg / 180)``: +-90 give +-pi/2 exactly."""
    return math.pi * (float(deg) / 180.0)


def column(name):
    """The row column called ``name``; -1 for None."""
    return -1 if name is None else WEIGHT_COLUMNS[name]


def check_columns(spec, *names):
    for name in names:
        v = getattr(spec, name)
        if v is not None and v not in WEIGHT_COLUMNS:
            raise ValueError(f"{name} must be None or one of {sorted(WEIGHT_COLUMNS)}")


def with_channels(spec, nchan):
    """``spec`` with ``nchan`` maps."""
    return replace(spec, nchan=int(nchan))


def counts_for(ncfile, a):
    """netCDF-3 has no 64-bit integers: int64 counts go out as float64 there
    (exact below 2^53), as they are into an ``.npz``."""
    return a if str(ncfile).endswith(".npz") else a.astype(np.float64)


class LatBand:
    """``lat_range`` (degrees) of a frozen spec, in radians."""

    def _check_lat_range(self):
        if not self.lat_range[1] > self.lat_range[0]:
            raise ValueError("lat_range must be ascending")

    lat0 = property(lambda self: radians(self.lat_range[0]))
    lat1 = property(lambda self: radians(self.lat_range[1]))


class RowColumns:
    """The row columns a spec names: ``need`` (must be finite for a row to be
    valid) and ``weight``, each None or a key of ``WEIGHT_COLUMNS``."""
    need = weight = None
    ncol = property(lambda self: column(self.need))
    wcol = property(lambda self: column(self.weight))


class GridSpec(LatBand, RowColumns):
    """The grid of a frozen spec with ``nx, ny, nchan, lat_range`` and, for an
    unwrapped longitude window, ``lon_range`` (degrees; None: [0, 360)).  The
    factors of the index arithmetic are computed here, once, in fp64, and
    passed to the kernel (never recomputed on the device)."""
    lon_range = None

    def _check_shape(self):
        if self.nx <= 0 or self.ny <= 0 or self.nchan <= 0:
            raise ValueError("nx, ny and nchan must be positive")
        if self.nx * self.ny * self.nchan >= 2 ** 31:
            raise ValueError("nchan*ny*nx must be below 2^31")

    def _check_ranges(self):
        self._check_lat_range()
        if self.lon_range is not None:
            a, b = (float(v) for v in self.lon_range)
            if not (math.isfinite(a) and math.isfinite(b) and b > a):
                raise ValueError("lon_range must be None or finite and ascending")

    unwrapped = property(lambda self: self.lon_range is not None)
    lon0 = property(lambda self: radians(self.lon_range[0]) if self.unwrapped else 0.0)
    lon1 = property(lambda self: radians(self.lon_range[1]) if self.unwrapped else 2 * math.pi)
    inv_dlon = property(lambda self: self.nx / (self.lon1 - self.lon0))
    inv_dlat = property(lambda self: self.ny / (self.lat1 - self.lat0))
    shape = property(lambda self: (self.nchan, self.ny, self.nx))

    @property
    def circles(self):
        """The whole circles of an unwrapped window that starts on a multiple
        of 360 degrees; None for any other axis."""
        if not self.unwrapped:
            return None
        a, b = (float(v) for v in self.lon_range)
        n = (b - a) / 360.0
        return int(n) if a % 360.0 == 0.0 and n == int(n) else None


def fold_arrays(spec, *arrays):
    """``(spec', arrays')``: an unwrapped map of ``spec.circles`` whole circles
    summed onto [0, 360) -- ``spec'`` the wrapped spec of ``nx / circles``
    bins; each array is ``[nchan, ny, nx, ...]`` (NumPy or torch)."""
    nc = spec.circles
    if nc is None:
        raise ValueError("fold() needs an unwrapped window of whole circles that starts on a multiple of 360 degrees")
    if spec.nx % nc:
        raise ValueError(f"fold() needs nx divisible by the {nc} circles of the window, got nx = {spec.nx}")
    per = spec.nx // nc
    out = [a.reshape(tuple(a.shape[:2]) + (nc, per) + tuple(a.shape[3:])).sum(2) for a in arrays]
    return replace(spec, nx=per, lon_range=None), out


def valid_rows(rows, spec):
    """``[nray, nt]`` bool: lon and lat finite and, with ``need`` / ``weight``,
    those columns finite too."""
    ok = np.isfinite(rows[..., 0]) & np.isfinite(rows[..., 1])
    for col in (spec.ncol, spec.wcol):
        if col >= 0:
            ok &= np.isfinite(rows[..., col])
    return ok


def allreduce_tensors(pairs, group=None):
    """``torch.distributed.all_reduce`` of every ``(tensor, op)`` of ``pairs``
    over the ranks of ``group``, in place and left on every rank; ``op`` is
    ``'SUM'``, ``'MIN'`` or ``'MAX'``, a tensor that is None is skipped."""
    import torch.distributed as dist
    from shard import _dev
    for t, op in pairs:
        if t is None:
            continue
        x = t.to(_dev(group))
        dist.all_reduce(x, op=getattr(dist.ReduceOp, op), group=group)
        if x is not t:
            t.copy_(x)


class RayArgs:
    """The per-ray arguments of an ``add_rows`` call, as device tensors
    (needs ``self.device``; ``_ray`` also ``self.nray``)."""

    def _chan(self, chan, nray):
        import torch
        if chan is None:
            return None
        chan = torch.as_tensor(chan, device=self.device).to(torch.int32).contiguous()
        if chan.numel() != nray:
            raise ValueError(f"chan has {chan.numel()} entries for {nray} rays")
        return chan

    def _ray(self, ray, n):
        import torch
        if ray is None:
            if n != self.nray:
                raise ValueError(f"{n} rays for {self.nray} columns: pass ray (each ray's column)")
            return None
        ray = torch.as_tensor(ray, device=self.device).to(torch.int64).contiguous()
        if ray.numel() != n:
            raise ValueError(f"ray has {ray.numel()} entries for {n} rays")
        return ray


class DeviceMap(RayArgs):
    """The base of a product's device arrays: ``spec``, ``device``, the C
    struct ``_c`` and the library ``_lib`` (tools/track_rate.py puts an A/B
    build there).  ``REDUCE``: ``(attribute, op)`` per array that ``allreduce``
    combines.  The edges and ``_grid_output`` are those of a lon-lat grid
    (``nx, ny, lat_range``); ``cross.CrossMap`` has ``bin_edges`` per gate."""
    REDUCE = ()

    def __init__(self, spec, device=None):
        import torch
        H.require_gpu()
        self._lib = H.load()
        self.spec = spec
        self.device = torch.device(device or "cuda")
        self._c = spec.c_struct()

    def allreduce(self, group=None):
        """The arrays of every rank of ``group`` combined as ``REDUCE`` says
        and left on every rank."""
        allreduce_tensors([(getattr(self, name), op) for name, op in self.REDUCE], group)
        return self

    @property
    def lon_edges(self):
        """The ``nx + 1`` longitude bin edges in degrees (those of
        ``lon_range`` for an unwrapped map)."""
        lon_range = getattr(self.spec, "lon_range", None)
        a, b = (0.0, 360.0) if lon_range is None else (float(v) for v in lon_range)
        return np.linspace(a, b, self.spec.nx + 1)

    @property
    def lat_edges(self):
        """The ``ny + 1`` latitude bin edges in degrees."""
        return np.linspace(float(self.spec.lat_range[0]), float(self.spec.lat_range[1]), self.spec.ny + 1)

    def _grid_output(self):
        """``(dims, variables)`` of the grid for ``output()``: dims ``chan,
        lat, lon`` and the edges, bin centres and edges in degrees."""
        s = self.spec
        le, la = self.lon_edges, self.lat_edges
        dims = {"chan": s.nchan, "lat": s.ny, "lon": s.nx, "lat_edge": s.ny + 1, "lon_edge": s.nx + 1}
        v = {"lon": (("lon",), 0.5 * (le[:-1] + le[1:]), "degrees"),
             "lat": (("lat",), 0.5 * (la[:-1] + la[1:]), "degrees"),
             "lon_edges": (("lon_edge",), le, "degrees"), "lat_edges": (("lat_edge",), la, "degrees")}
        return dims, v


class CarriedMap(DeviceMap):
    """A map over ``nray`` rays whose segments join consecutive rows: ``prev``
    (fp64 ``[3, nray]``: lon, lat, weight value) is each ray's carried previous
    row, NaN for none -- a running state, not a sum: a ray's rows must arrive
    once, in order, each call starting at the row the previous one ended with
    (``start`` is row 0).  ``chan``: each ray's channel, indexed by the ray's
    column (None: channel 0)."""

    def __init__(self, spec, nray, device=None, chan=None):
        import torch
        super().__init__(spec, device)
        self.nray = int(nray)
        self.prev = torch.full((3, self.nray), math.nan, dtype=torch.float64, device=self.device)
        self.chan = self._chan(chan, self.nray)

    def restart(self):
        """Forget every ray's carried row (the maps and the per-ray arrays stay)."""
        self.prev.fill_(math.nan)
        return self

    def start(self, lon, lat, need=None, v=None, ray=None):
        """Row 0, the initial rays (radians), which sinks never receive: the
        same entry point on a ``[n, 1, 8]`` row tensor; it adds nothing to the
        maps and sets the carried rows.  ``need`` / ``v``: the values of the
        ``need`` and ``weight`` columns (required when the spec names them)."""
        cols = {0: lon, 1: lat}
        for name, col, val in (("need", self.spec.ncol, need), ("weight", self.spec.wcol, v)):
            if col >= 0:
                if val is None:
                    raise ValueError(f"the map's {name} column is {getattr(self.spec, name)!r}: pass its values")
                cols[col] = val
        self.add_rows(0, 1, one_row(cols, self.device), ray=ray)
        return self


class ChannelSink(RowSink):
    """A sink whose per-ray value is the ray's channel: ``chan`` has length
    nray and is indexed by a shard's ``idx``; None (channel 0) stays None."""

    def __init__(self, map, chan=None):
        super().__init__(map, None if chan is None else map._chan(chan, len(chan)))

    map = property(lambda self: self.target)
    chan = property(lambda self: self.per_ray)

    def select(self, idx):
        return None if self.per_ray is None else self.per_ray[idx]


class ColumnSink(RowSink):
    """A sink whose per-ray value is the ray's column in the target's per-ray
    arrays: ``ray`` (None: ray j is column j); a shard's ``idx`` and
    ``take(idx)`` select from it, or are the columns themselves."""

    def __init__(self, map, ray=None):
        super().__init__(map, ray if ray is None else map._ray(ray, len(ray)))

    map = property(lambda self: self.target)
    ray = property(lambda self: self.per_ray)

    def select(self, idx):
        return idx if self.per_ray is None else self.per_ray[idx]
