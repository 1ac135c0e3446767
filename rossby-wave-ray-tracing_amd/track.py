"""Residence-time maps along ray segments, reduced on the GPU
(``rwrt_ray_track``, ABI 5).

The point maps (density.py, arrival.py, flux.py) bin one point per ray per
output row, and at a fine resolution a ray moves many boxes between two rows:
their pictures have gaps and scale with the output interval.  Here the straight
segment (in lon-lat) between every two consecutive valid rows of a ray is
deposited into every box it passes through, each box receiving the fraction of
the segment that lies in it: ``time`` is the residence time per box in units of
the row interval, ``cnt`` the number of box visits, ``wsum`` (with ``weight``)
the time integral of a row column under the trapezoidal rule per segment.
Every live segment deposits exactly one row interval, whatever the resolution.

``reference_track`` (plain Python/NumPy) is the definition.  The kernel
(csrc/track_cells.h) restates the walk operation for operation -- IEEE
divisions, no fused multiply-add -- so that every cell sequence, and therefore
``cnt`` and ``dropped``, equal it exactly; ``time`` and ``wsum`` agree to the
rounding of a sum taken in any order.  ``TrackSink`` plugs into
``RayEngine.integrate`` / ``integrate_rk4`` / ``resume`` /
``shard.run_sharded`` through the ``sink`` protocol, alone or as a member of
``summary.Tee``; ``WR.ray_track`` is the user entry point.
"""
import math
from dataclasses import dataclass

import numpy as np

import _hip as H
from launch_rows import row_args
from raymap import CarriedMap, ColumnSink, GridSpec, check_columns, counts_for, fold_arrays, valid_rows  # noqa: F401

MODE_UNWRAPPED = 2
TWO30 = float(2 ** 30)


@dataclass(frozen=True)
class TrackSpec(GridSpec):
    """``nx`` boxes over the longitude axis, ``ny`` over ``lat_range`` (degrees),
    ``nchan`` maps.  ``lon_range=None``: wrapped longitude, [0, 360);
    ``lon_range=(a, b)`` in degrees: the unwrapped window of a
    ``flux.FluxSpec``, what lies outside is not deposited.  ``need``: a row
    column by name (``density.WEIGHT_COLUMNS``) that must be finite for a row
    to be valid, or None; the default ``'amp'`` keeps dead root slots out.
    ``weight``: a row column whose time integral per box is kept in ``wsum``,
    or None.  ``max_cells``: a segment that would pass through more boxes is
    dropped and counted (None: ``nx + ny``)."""
    nx: int
    ny: int
    lat_range: tuple = (-90.0, 90.0)
    lon_range: tuple = None
    need: str = "amp"
    weight: str = None
    nchan: int = 1
    max_cells: int = None

    def __post_init__(self):
        self._check_shape()
        self._check_ranges()
        check_columns(self, "need", "weight")
        if self.max_cells is not None:
            if int(self.max_cells) != self.max_cells or not 1 <= self.max_cells < 2 ** 31:
                raise ValueError("max_cells must be None or an integer in [1, 2^31)")

    @property
    def cells(self):
        return self.nx + self.ny if self.max_cells is None else int(self.max_cells)

    @property
    def mode(self):
        return MODE_UNWRAPPED if self.unwrapped else 0

    def c_struct(self):
        return H.TrackMapC(self.nx, self.ny, self.nchan, self.mode, self.ncol, self.wcol, self.cells, 0,
                           self.lon0, self.inv_dlon, self.lat0, self.inv_dlat)


def segment_cells(X0, Y0, X1, Y1, max_cells):
    """The boxes the straight segment ``(X0, Y0) -> (X1, Y1)`` (grid
    coordinates, finite Python floats) passes through, in order, as
    ``[(ix, iy, w)]`` with ``w`` the fraction of the segment in the box; None
    for a dropped segment: a floor beyond ``2^30`` in magnitude, or more than
    ``max_cells`` boxes.

    With ``f* = floor(*)``, ``ncx = |fx1 - fx0|`` x-lines and ``ncy`` y-lines
    are crossed, line ``g`` at ``t = (g - X0) / (X1 - X0)`` (one subtraction
    and one IEEE division of the rounded difference); the lines are taken in
    ascending ``t``, a tie going to x, and a box gets the difference of the
    ``t`` at which it is left and entered -- the last one ``1.0 - t``.  A
    segment inside one box gives it exactly 1.0 and divides nothing."""
    fx0, fy0, fx1, fy1 = (float(np.floor(v)) for v in (X0, Y0, X1, Y1))
    if not (abs(fx0) <= TWO30 and abs(fy0) <= TWO30 and abs(fx1) <= TWO30 and abs(fy1) <= TWO30):
        return None
    ncx, ncy = abs(fx1 - fx0), abs(fy1 - fy0)
    if ncx + ncy + 1.0 > max_cells:        # (in fp64, before any conversion)
        return None
    ncx, ncy = int(ncx), int(ncy)
    ix, iy = int(fx0), int(fy0)
    DX, DY = X1 - X0, Y1 - Y0
    sx = 1 if fx1 > fx0 else -1
    sy = 1 if fy1 > fy0 else -1
    gx = fx0 + 1.0 if sx > 0 else fx0       # the next x-line (an exact integer in fp64)
    gy = fy0 + 1.0 if sy > 0 else fy0
    out = []
    t = 0.0
    while ncx > 0 or ncy > 0:
        tx = (gx - X0) / DX if ncx > 0 else math.inf
        ty = (gy - Y0) / DY if ncy > 0 else math.inf
        if tx <= ty:
            out.append((ix, iy, tx - t))
            t = tx
            ix += sx
            gx += sx
            ncx -= 1
        else:
            out.append((ix, iy, ty - t))
            t = ty
            iy += sy
            gy += sy
            ncy -= 1
    out.append((ix, iy, 1.0 - t))
    return out


def deposits(rows, chan, spec):
    """The deposits of ``reference_track`` one by one, in ray-then-row-then-cell
    order: yields ``(c, iy, col, w, wv)`` per deposited box (``wv`` 0.0 without
    a weight) and ``None`` per dropped segment."""
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 3 or rows.shape[1] < 1 or rows.shape[2] < 7:
        raise ValueError(f"rows must be [nray, nt >= 1, >= 7], got {rows.shape}")
    nray = rows.shape[0]
    chan = np.zeros(nray, np.int64) if chan is None else np.asarray(chan, np.int64).reshape(-1)
    if chan.size != nray:
        raise ValueError(f"chan has {chan.size} entries for {nray} rays")
    ok = valid_rows(rows, spec)
    with np.errstate(all="ignore"):
        X = (rows[..., 0] - spec.lon0) * spec.inv_dlon
        Y = (rows[..., 1] - spec.lat0) * spec.inv_dlat
    v = rows[..., spec.wcol] if spec.wcol >= 0 else None
    nx, ny, cells = spec.nx, spec.ny, spec.cells
    for j in range(nray):
        c = int(chan[j])
        if not 0 <= c < spec.nchan:
            continue
        for i in np.nonzero(ok[j, 1:] & ok[j, :-1])[0] + 1:
            seg = segment_cells(float(X[j, i - 1]), float(Y[j, i - 1]), float(X[j, i]), float(Y[j, i]), cells)
            if seg is None:
                yield None
                continue
            vm = 0.5 * (float(v[j, i - 1]) + float(v[j, i])) if v is not None else 0.0
            for ix, iy, w in seg:
                if not 0 <= iy < ny:
                    continue
                if spec.unwrapped:
                    if not 0 <= ix < nx:
                        continue
                else:
                    ix %= nx
                yield c, iy, ix, w, w * vm


def reference_track(rows, chan, spec):
    """The definition of a residence-time map, in plain Python: a dict with
    ``cnt`` (``[nchan, ny, nx]`` int64: box visits), ``time`` (float64: the
    segments' fractions, i.e. residence in row intervals), ``wsum`` (float64,
    None without ``weight``) and ``dropped`` (int).

    ``rows[nray, nt, 8]``: a logical history (columns lon lat k l amp ug vg
    nacc, row 0 the initial row); ``chan`` one channel per ray (None: channel
    0).  The grid coordinates of a row are ``X = (lon - lon0) * inv_dlon`` and
    ``Y = (lat - lat0) * inv_dlat`` (a rounded difference times a rounded
    factor; ``lon`` is never wrapped).  A row is valid iff lon and lat are
    finite and the ``need`` and ``weight`` columns, when set, are finite.
    Segment ``i`` joins rows ``i - 1`` and ``i`` of a ray; it is considered
    iff both are valid and the ray's channel c is in ``[0, nchan)``, dropped
    (``dropped += 1``, nothing else) as ``segment_cells`` says with
    ``max_cells = spec.cells``, and else every box ``(ix, iy, w)`` of
    ``segment_cells`` is deposited iff ``0 <= iy < ny`` and, wrapped, into
    column ``ix % nx`` (Python's integer ``%``) or, unwrapped, iff
    ``0 <= ix < nx``: ``cnt += 1``, ``time += w`` and ``wsum += w * (0.5 *
    (v0 + v1))`` with ``v`` the weight column at the two ends.  Each box's
    sums are taken sequentially in ray-then-row-then-cell order.  Doubles as
    the ``mode='numpy'`` map of small runs."""
    cnt = np.zeros(spec.shape, np.int64)
    time = np.zeros(spec.shape)
    wsum = np.zeros(spec.shape) if spec.wcol >= 0 else None
    dropped = 0
    for d in deposits(rows, chan, spec):
        if d is None:
            dropped += 1
            continue
        c, iy, ix, w, wv = d
        cnt[c, iy, ix] += 1
        time[c, iy, ix] += w
        if wsum is not None:
            wsum[c, iy, ix] += wv
    return {"cnt": cnt, "time": time, "wsum": wsum, "dropped": dropped}


class TrackMap(CarriedMap):
    """The device arrays of one map over ``nray`` rays: ``cnt`` (int64),
    ``time`` and ``wsum`` (fp64; ``wsum`` None without a weight), each
    ``[nchan, ny, nx]``, and ``dropped`` (int64 ``[1]``), zeroed here and
    accumulated into by every ``add_rows`` call (time chunks, shards);
    ``allreduce`` sums them over the ranks.  The carried rows (``prev``,
    ``start``, ``restart``) and ``chan`` are ``raymap.CarriedMap``'s and are
    not reduced; a ray with a channel outside ``[0, nchan)`` contributes
    nothing."""
    REDUCE = (("cnt", "SUM"), ("time", "SUM"), ("wsum", "SUM"), ("dropped", "SUM"))

    def __init__(self, spec, nray, device=None, chan=None):
        import torch
        super().__init__(spec, nray, device, chan)
        self.cnt = torch.zeros(spec.shape, dtype=torch.int64, device=self.device)
        self.time = torch.zeros(spec.shape, dtype=torch.float64, device=self.device)
        self.wsum = torch.zeros(spec.shape, dtype=torch.float64, device=self.device) if spec.wcol >= 0 else None
        self.dropped = torch.zeros(1, dtype=torch.int64, device=self.device)

    def add_rows(self, i0, i1, view, tails=None, slots=None, ray=None):
        """Deposit the segments that end on rows ``[i0, i1)`` of a launch:
        ``view`` its row buffer (dense ``[n, i1-i0, 8]``, or the row blocks of
        ``slots``), ``tails`` / ``slots`` the launch's ``engine.Tails`` /
        ``engine.Slots``, ``ray`` each ray's column (int64; None: ray j is
        column j).  One asynchronous ``rwrt_ray_track`` call on the device's
        current stream."""
        import torch
        n, rows = row_args(i0, i1, view, tails, slots)
        ray = self._ray(ray, n)
        H.check(self._lib.rwrt_ray_track(
            self._c, n, int(i0), int(i1), *rows, H.dptr(ray, torch.int64), self.nray, H.dptr(self.chan, torch.int32),
            H.dptr(self.prev, torch.float64), H.dptr(self.cnt, torch.int64), H.dptr(self.time, torch.float64),
            H.dptr(self.wsum), H.dptr(self.dropped, torch.int64), H.stream(self.device)))

    def numpy(self):
        """``{'cnt', 'time', 'wsum', 'dropped'}`` on the host, as
        ``reference_track`` returns them (waits for the pending calls)."""
        return {"cnt": self.cnt.cpu().numpy(), "time": self.time.cpu().numpy(),
                "wsum": None if self.wsum is None else self.wsum.cpu().numpy(),
                "dropped": int(self.dropped.cpu().numpy()[0])}

    # ---- derived fields: device tensors [nchan, ny, nx]
    def seconds(self, tstep):
        """The residence time per box in seconds: ``time * tstep``."""
        return self.time * float(tstep)

    def mean_weight(self):
        """The time mean of the weight column over the residence in a box:
        ``wsum / time``, NaN where ``time == 0``."""
        import torch
        if self.wsum is None:
            raise ValueError("the map has no weight")
        return torch.where(self.time == 0, torch.full_like(self.time, math.nan), self.wsum / self.time)

    def fold(self):
        """A new wrapped map: this unwrapped map, whose window is whole
        circles, summed onto [0, 360).  Needs ``nx`` divisible by the number
        of circles.  The carried rows and ``dropped`` go with it."""
        arrays = [a for a in (self.cnt, self.time, self.wsum) if a is not None]
        spec, out = fold_arrays(self.spec, *arrays)
        m = TrackMap(spec, self.nray, self.device, self.chan)
        for dst, src in zip((m.cnt, m.time, m.wsum), out):
            dst.copy_(src)
        m.dropped.copy_(self.dropped)
        m.prev.copy_(self.prev)
        return m

    def output(self, ncfile):
        """Write the map (dims ``chan, lat, lon``; box centres in degrees).
        netCDF-3 has no 64-bit integers: ``cnt`` goes out as float64 there
        (exact below 2^53), as int64 into an ``.npz``."""
        import ncio
        a = self.numpy()
        dims, v = self._grid_output()
        dims["one"] = 1
        full = ("chan", "lat", "lon")
        v.update({"cnt": (full, counts_for(ncfile, a["cnt"]), "box visits"),
                  "time": (full, a["time"], "row intervals"),
                  "dropped": (("one",), np.array([float(a["dropped"])]), "segments")})
        if a["wsum"] is not None:
            v["wsum"] = (full, a["wsum"], f"time integral of {self.spec.weight}, row intervals")
        ncio.write(ncfile, dims, v)


class TrackSink(ColumnSink):
    """A ``sink`` of ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume``
    and of ``shard.run_sharded`` (``launch_rows.RowSink``) that deposits each
    launch's segments into ``map``.  ``ray``: the column of each ray of the
    integration (None: ray j is column j); the sharded form's ``idx`` and
    ``take(idx)`` select from it, or are the columns themselves.  Channels are
    the map's (``TrackMap.chan``), indexed by column."""
