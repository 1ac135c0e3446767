"""Gate-crossing maps, reduced on the GPU (``rwrt_ray_cross``, ABI 5).

The other maps (density.py, arrival.py, flux.py, track.py) reduce per lon-lat
box; a line has no area, and a row of boxes around it mixes the two directions
and counts residence, not passages.  Here a GATE is a latitude circle or a
meridian, and every passage of a ray's segment (two consecutive valid rows)
through it is counted by direction, binned along the gate, timed -- per map bin
(``cnt``, ``tsum``, with ``weight`` ``wsum``), optionally per time window -- and
recorded per ray (``ncross``, ``tfirst``): does wave activity get from one side
of a line to the other, and where, when and in which direction.

``reference_cross`` (plain Python/NumPy) is the definition.  The kernel
(csrc/cross_lines.h) restates it operation for operation -- IEEE divisions, no
fused multiply-add -- so that ``cnt``, ``ncross`` and ``dropped`` equal it
exactly and ``tfirst`` bit for bit; ``tsum`` and ``wsum`` agree to the rounding
of a sum taken in any order.  ``CrossSink`` plugs into ``RayEngine.integrate``
/ ``integrate_rk4`` / ``resume`` / ``shard.run_sharded`` through the ``sink``
protocol, alone or as a member of ``summary.Tee``; ``WR.ray_cross`` is the user
entry point.
"""
import math
from dataclasses import dataclass

import numpy as np

import _hip as H
from launch_rows import row_args
from raymap import CarriedMap, ColumnSink, LatBand, RowColumns, check_columns, counts_for, valid_rows  # noqa: F401

MAXGATE = H.CROSS_MAXGATE
TWO_PI = 2.0 * math.pi
INV_2PI = 1.0 / (2.0 * math.pi)
TWO30 = float(2 ** 30)
DIRECTIONS = {None: None, 0: 0, 1: 1, "north": 0, "east": 0, "south": 1, "west": 1}


@dataclass(frozen=True)
class Gate:
    """A latitude circle (``kind`` 0) or a meridian (``kind`` 1) at ``deg``
    degrees; a meridian's longitude is taken modulo 360."""
    kind: int
    deg: float

    def __post_init__(self):
        if self.kind not in (0, 1):
            raise ValueError("kind must be 0 (latitude circle) or 1 (meridian)")
        if not math.isfinite(float(self.deg)):
            raise ValueError("a gate's position must be finite")
        if self.kind == 0 and not -90.0 <= float(self.deg) <= 90.0:
            raise ValueError("a latitude circle lies in [-90, 90] degrees")
        if self.kind == 1 and not 0.0 <= float(self.deg) < 360.0:
            raise ValueError("a meridian lies in [0, 360) degrees (Gate.lon wraps)")

    @classmethod
    def lat(cls, deg):
        """The latitude circle at ``deg`` degrees north."""
        return cls(0, float(deg))

    @classmethod
    def lon(cls, deg):
        """The meridian at ``deg`` degrees east."""
        return cls(1, float(deg) % 360.0)

    @property
    def pos(self):
        """Radians: pi * (deg / 180), as the map axes are taken."""
        return math.pi * (float(self.deg) / 180.0)


@dataclass(frozen=True)
class CrossSpec(LatBand, RowColumns):
    """Up to 8 ``gates`` with ``nbin`` bins along each: over longitude [0, 360)
    for a latitude circle, over ``lat_range`` (degrees) for a meridian, where
    a crossing outside the range is counted per ray and not in the map.
    ``nchan`` maps.  ``need``: a row column by name
    (``density.WEIGHT_COLUMNS``) that must be finite for a row to be valid, or
    None; the default ``'amp'`` keeps dead root slots out.  ``weight``: a row
    column whose value at the crossing (interpolated along the segment) is
    summed in ``wsum``, or None.  ``window_rows``: the length of a time window
    in rows (0: none); with windows ``nt``, the rows of the history, is
    required and gives ``nwin = ceil((nt - 1) / window_rows)``."""
    gates: tuple
    nbin: int
    lat_range: tuple = (-90.0, 90.0)
    nchan: int = 1
    need: str = "amp"
    weight: str = None
    window_rows: int = 0
    nt: int = None

    def __post_init__(self):
        gates = (self.gates,) if isinstance(self.gates, Gate) else tuple(self.gates)
        object.__setattr__(self, "gates", gates)
        if not 1 <= len(gates) <= MAXGATE or not all(isinstance(g, Gate) for g in gates):
            raise ValueError(f"gates must be 1..{MAXGATE} Gate objects")
        if self.nbin <= 0 or self.nchan <= 0:
            raise ValueError("nbin and nchan must be positive")
        self._check_lat_range()
        check_columns(self, "need", "weight")
        if int(self.window_rows) != self.window_rows or self.window_rows < 0:
            raise ValueError("window_rows must be a non-negative integer")
        if self.window_rows > 0:
            if self.nt is None or int(self.nt) != self.nt or self.nt < 2:
                raise ValueError("time windows need nt >= 2, the rows of the history")
        if self.nwin * len(gates) * 2 * self.nchan * self.nbin >= 2 ** 31:
            raise ValueError("nwin*ngate*2*nchan*nbin must be below 2^31")

    @property
    def ngate(self):
        return len(self.gates)

    @property
    def nwin(self):
        if self.window_rows == 0:
            return 1
        return -(-(int(self.nt) - 1) // int(self.window_rows))

    # the factors of the bins: computed here, once, in fp64, and passed to the
    # kernel (never recomputed on the device)
    @property
    def inv_dlon(self):
        return self.nbin / TWO_PI

    @property
    def inv_dlat(self):
        return self.nbin / (self.lat1 - self.lat0)

    def axis(self, g):
        """``(org, inv_d)`` of the bins along gate ``g``."""
        return (0.0, self.inv_dlon) if self.gates[g].kind == 0 else (self.lat0, self.inv_dlat)

    @property
    def shape(self):
        return (self.nwin, self.ngate, 2, self.nchan, self.nbin)

    def c_struct(self):
        c = H.CrossMapC(self.ngate, self.nbin, self.nchan, self.ncol, self.wcol, int(self.window_rows), self.nwin, 0)
        for g, gate in enumerate(self.gates):
            org, inv_d = self.axis(g)
            c.gate[g] = H.CrossGateC(gate.kind, 0, gate.pos, org, inv_d)
        return c


def sides(rows, gate):
    """A row's side of ``gate``, ``[nray, nt]`` float64 (garbage for an invalid
    row): ``lat >= pos`` as 0.0 / 1.0, or the circle ``floor((lon - pos) *
    INV_2PI)`` the row is on."""
    with np.errstate(all="ignore"):
        if gate.kind == 0:
            return (rows[..., 1] >= gate.pos).astype(np.float64)
        return np.floor((rows[..., 0] - gate.pos) * INV_2PI)


def segment_crossing(gate, org, inv_d, nbin, s0, s1, lon0, lat0, lon1, lat1):
    """The crossing of ``gate`` by the segment ``(lon0, lat0) -> (lon1, lat1)``
    (Python floats) whose ends lie on the sides ``s0 != s1``: ``(d, bin, t)``
    with ``bin`` -1 outside the map, or None for a dropped segment."""
    d = 0 if s1 > s0 else 1
    if gate.kind == 0:
        t = (gate.pos - lat0) / (lat1 - lat0)
        lon_c = lon0 + t * (lon1 - lon0)
        if not math.isfinite(lon_c):          # (lon1 - lon0 overflowed: no bin)
            return d, -1, t
        lam = (lon_c % TWO_PI) % TWO_PI
        return d, min(math.floor(lam * inv_d), nbin - 1), t
    if not (abs(s0) <= TWO30 and abs(s1) <= TWO30) or abs(s1 - s0) > 1.0:
        return None
    u0, u1 = lon0 - gate.pos, lon1 - gate.pos
    G = max(s0, s1) * TWO_PI
    t = (G - u0) / (u1 - u0)
    t = 0.0 if t < 0.0 else t                # (-0.0 stays)
    t = 1.0 if t > 1.0 else t
    lat_c = lat0 + t * (lat1 - lat0)
    fb = math.floor((lat_c - org) * inv_d)
    return d, (fb if 0 <= fb < nbin else -1), t


def crossings(rows, chan, spec):
    """The crossings of ``reference_cross`` one by one, in ray-then-row-then-
    gate order: yields ``(g, d, j, c, w, bin, t, tc, wv)`` per crossing
    (``bin`` -1 outside the map, ``wv`` 0.0 without a weight) and ``None`` per
    dropped segment of a gate."""
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 3 or rows.shape[1] < 1 or rows.shape[2] < 7:
        raise ValueError(f"rows must be [nray, nt >= 1, >= 7], got {rows.shape}")
    nray, nt = rows.shape[:2]
    chan = np.zeros(nray, np.int64) if chan is None else np.asarray(chan, np.int64).reshape(-1)
    if chan.size != nray:
        raise ValueError(f"chan has {chan.size} entries for {nray} rays")
    if spec.window_rows > 0 and nt - 1 > spec.nwin * spec.window_rows:
        raise ValueError(f"{nt} rows for {spec.nwin} windows of {spec.window_rows} rows")
    ok = valid_rows(rows, spec)
    seg = ok[:, 1:] & ok[:, :-1] & ((chan >= 0) & (chan < spec.nchan))[:, None]
    found = []
    side = []
    for g, gate in enumerate(spec.gates):
        s = sides(rows, gate)
        side.append(s)
        j, i = np.nonzero(seg & (s[:, 1:] != s[:, :-1]))
        found.append(np.stack([j, i + 1, np.full(len(j), g)], axis=1))
    found = np.concatenate(found)
    found = found[np.lexsort((found[:, 2], found[:, 1], found[:, 0]))]
    wcol = spec.wcol
    for j, i, g in found.tolist():
        gate = spec.gates[g]
        org, inv_d = spec.axis(g)
        a, b = rows[j, i - 1], rows[j, i]
        hit = segment_crossing(gate, org, inv_d, spec.nbin, float(side[g][j, i - 1]), float(side[g][j, i]),
                               float(a[0]), float(a[1]), float(b[0]), float(b[1]))
        if hit is None:
            yield None
            continue
        d, bin_, t = hit
        w = (i - 1) // spec.window_rows if spec.window_rows > 0 else 0
        wv = float(a[wcol]) + t * (float(b[wcol]) - float(a[wcol])) if wcol >= 0 else 0.0
        yield g, d, j, int(chan[j]), w, bin_, t, float(i - 1) + t, wv


def reference_cross(rows, chan, spec):
    """The definition of a gate-crossing map, in plain Python: a dict with
    ``cnt`` (``[nwin, ngate, 2, nchan, nbin]`` int64), ``tsum`` (float64: the
    crossing times in rows, summed), ``wsum`` (float64, None without
    ``weight``), ``dropped`` (int), ``ncross`` (``[ngate, 2, nray]`` int32) and
    ``tfirst`` (float64, NaN for none).

    ``rows[nray, nt, 8]``: a logical history (columns lon lat k l amp ug vg
    nacc, row 0 the initial row); ``chan`` one channel per ray (None: channel
    0).  A row is valid iff lon and lat are finite and the ``need`` and
    ``weight`` columns, when set, are finite.  Segment ``i`` joins rows
    ``i - 1`` and ``i`` of a ray; it is considered iff both are valid and the
    ray's channel c is in ``[0, nchan)``.  Every operation is one rounded fp64
    ``+ - * /`` or a ``floor``.

    Latitude circle ``lat = pos``: ``s(lat) = (lat >= pos)``; the segment
    crosses iff ``s0 != s1``, in direction 0 (northward) iff ``s1``, else 1;
    ``t = (pos - lat0) / (lat1 - lat0)``, ``lon_c = lon0 + t * (lon1 - lon0)``,
    bin ``min(floor(lam * inv_d), nbin - 1)`` with ``lam = (lon_c % 2 pi) %
    2 pi`` (a ``lon_c`` that is not finite -- the difference of two longitudes
    near the largest double -- has no bin).

    Meridian ``lon = pos + 2 pi n``: ``u = lon - pos``, ``m = floor(u *
    INV_2PI)``, lon never wrapped; the segment crosses iff ``m0 != m1``, in
    direction 0 (eastward) iff ``m1 > m0``, else 1.  It is dropped
    (``dropped += 1`` and nothing else for that gate) iff ``|m0| > 2^30``,
    ``|m1| > 2^30`` or ``|m1 - m0| > 1``.  Otherwise ``G = max(m0, m1) *
    TWO_PI``, ``t = min(max((G - u0) / (u1 - u0), 0.0), 1.0)``, ``lat_c = lat0
    + t * (lat1 - lat0)`` and the bin is ``floor((lat_c - org) * inv_d)``, in
    the map iff ``0 <= bin < nbin``.

    A crossing of gate g in direction d on segment i has the time ``tc = (i -
    1) + t`` rows and the window ``w = (i - 1) // window_rows`` (0 without
    windows).  Per ray, always: ``ncross[g, d, j] += 1`` and ``tfirst[g, d, j]
    = tc`` if it was NaN.  Per bin, when the crossing is in the map:
    ``cnt[w, g, d, c, bin] += 1``, ``tsum += tc`` and ``wsum += v0 + t * (v1 -
    v0)``.  Doubles as the ``mode='numpy'`` map of small runs."""
    rows = np.asarray(rows, np.float64)
    nray = rows.shape[0]
    cnt = np.zeros(spec.shape, np.int64)
    tsum = np.zeros(spec.shape)
    wsum = np.zeros(spec.shape) if spec.wcol >= 0 else None
    ncross = np.zeros((spec.ngate, 2, nray), np.int32)
    tfirst = np.full((spec.ngate, 2, nray), math.nan)
    dropped = 0
    for x in crossings(rows, chan, spec):
        if x is None:
            dropped += 1
            continue
        g, d, j, c, w, bin_, t, tc, wv = x
        ncross[g, d, j] += 1
        if math.isnan(tfirst[g, d, j]):
            tfirst[g, d, j] = tc
        if bin_ < 0:
            continue
        cnt[w, g, d, c, bin_] += 1
        tsum[w, g, d, c, bin_] += tc
        if wsum is not None:
            wsum[w, g, d, c, bin_] += wv
    return {"cnt": cnt, "tsum": tsum, "wsum": wsum, "dropped": dropped, "ncross": ncross, "tfirst": tfirst}


class CrossMap(CarriedMap):
    """The device arrays of one set of gates over ``nray`` rays: ``cnt``
    (int64), ``tsum`` and ``wsum`` (fp64; ``wsum`` None without a weight), each
    ``[nwin, ngate, 2, nchan, nbin]``, ``dropped`` (int64 ``[1]``), ``ncross``
    (int32) and ``tfirst`` (fp64, NaN for none), each ``[ngate, 2, nray]``,
    initialised here and accumulated into by every ``add_rows`` call (time
    chunks, shards).  The carried rows (``prev``, ``start``, ``restart``) and
    ``chan`` are ``raymap.CarriedMap``'s; a ray with a channel outside
    ``[0, nchan)`` contributes nothing."""
    REDUCE = (("cnt", "SUM"), ("tsum", "SUM"), ("wsum", "SUM"), ("dropped", "SUM"), ("ncross", "SUM"))

    def __init__(self, spec, nray, device=None, chan=None):
        import torch
        super().__init__(spec, nray, device, chan)
        f64 = dict(dtype=torch.float64, device=self.device)
        self.cnt = torch.zeros(spec.shape, dtype=torch.int64, device=self.device)
        self.tsum = torch.zeros(spec.shape, **f64)
        self.wsum = torch.zeros(spec.shape, **f64) if spec.wcol >= 0 else None
        self.dropped = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.ncross = torch.zeros((spec.ngate, 2, self.nray), dtype=torch.int32, device=self.device)
        self.tfirst = torch.full((spec.ngate, 2, self.nray), math.nan, **f64)

    def add_rows(self, i0, i1, view, tails=None, slots=None, ray=None):
        """Find the crossings of the segments that end on rows ``[i0, i1)`` of
        a launch: ``view`` its row buffer (dense ``[n, i1-i0, 8]``, or the row
        blocks of ``slots``), ``tails`` / ``slots`` the launch's
        ``engine.Tails`` / ``engine.Slots``, ``ray`` each ray's column (int64;
        None: ray j is column j).  One asynchronous ``rwrt_ray_cross`` call on
        the device's current stream."""
        import torch
        n, rows = row_args(i0, i1, view, tails, slots)
        ray = self._ray(ray, n)
        H.check(self._lib.rwrt_ray_cross(
            self._c, n, int(i0), int(i1), *rows, H.dptr(ray, torch.int64), self.nray, H.dptr(self.chan, torch.int32),
            H.dptr(self.prev, torch.float64), H.dptr(self.cnt, torch.int64), H.dptr(self.tsum, torch.float64),
            H.dptr(self.wsum), H.dptr(self.dropped, torch.int64), H.dptr(self.ncross, torch.int32),
            H.dptr(self.tfirst, torch.float64), H.stream(self.device)))

    def allreduce(self, group=None):
        """SUM of the maps, of ``dropped`` and of ``ncross`` over the ranks of
        ``group``, left on every rank; ``tfirst`` of a ray is the value of the
        rank that integrated it (every other rank holds NaN: a MIN over the
        ranks with NaN as +inf).  The carried rows are not reduced."""
        import torch
        import torch.distributed as dist
        from shard import _dev
        super().allreduce(group)
        x = torch.nan_to_num(self.tfirst, nan=math.inf).to(_dev(group))
        dist.all_reduce(x, op=dist.ReduceOp.MIN, group=group)
        x = x.to(self.device)
        self.tfirst.copy_(torch.where(torch.isinf(x), torch.full_like(x, math.nan), x))
        return self

    def numpy(self):
        """``{'cnt', 'tsum', 'wsum', 'dropped', 'ncross', 'tfirst'}`` on the
        host, as ``reference_cross`` returns them (waits for the pending
        calls)."""
        return {"cnt": self.cnt.cpu().numpy(), "tsum": self.tsum.cpu().numpy(),
                "wsum": None if self.wsum is None else self.wsum.cpu().numpy(),
                "dropped": int(self.dropped.cpu().numpy()[0]),
                "ncross": self.ncross.cpu().numpy(), "tfirst": self.tfirst.cpu().numpy()}

    def bin_edges(self, gate):
        """The ``nbin + 1`` bin edges along gate ``gate`` in degrees:
        longitudes 0..360 for a latitude circle, ``lat_range`` for a
        meridian."""
        a, b = (0.0, 360.0) if self.spec.gates[gate].kind == 0 else (float(v) for v in self.spec.lat_range)
        return np.linspace(a, b, self.spec.nbin + 1)

    # ---- derived fields: device tensors
    def _mean(self, s):
        import torch
        return torch.where(self.cnt == 0, torch.full_like(s, math.nan), s / self.cnt)

    def mean_rows(self):
        """The mean crossing time per bin in rows: ``tsum / cnt``, NaN where
        ``cnt == 0``."""
        return self._mean(self.tsum)

    def mean_days(self, tstep):
        """``mean_rows`` in days, a row being ``tstep`` seconds."""
        return self.mean_rows() * (float(tstep) / 86400.0)

    def mean_weight(self):
        """The mean of the weight column at the crossings of a bin: ``wsum /
        cnt``, NaN where ``cnt == 0``."""
        if self.wsum is None:
            raise ValueError("the map has no weight")
        return self._mean(self.wsum)

    def net(self):
        """Northward minus southward (eastward minus westward) crossings,
        ``[nwin, ngate, nchan, nbin]`` int64."""
        return self.cnt[:, :, 0] - self.cnt[:, :, 1]

    def crossed(self, gate, direction=None):
        """A bool per ray column: the ray crossed gate ``gate`` -- in
        ``direction`` 0 / ``'north'`` / ``'east'`` or 1 / ``'south'`` /
        ``'west'``, or (None) in either."""
        if direction not in DIRECTIONS:
            raise ValueError(f"direction must be one of {list(DIRECTIONS)}")
        d = DIRECTIONS[direction]
        n = self.ncross[gate]
        return (n.sum(dim=0) if d is None else n[d]) > 0

    def output(self, ncfile):
        """Write the maps (dims ``win, gate, dir, chan, bin``) and the per-ray
        arrays (``gate, dir, ray``); bin centres and edges per gate in degrees.
        netCDF-3 has no 64-bit integers: ``cnt`` goes out as float64 there
        (exact below 2^53), as int64 into an ``.npz``."""
        import ncio
        a = self.numpy()
        s = self.spec
        edges = np.stack([self.bin_edges(g) for g in range(s.ngate)])
        dims = {"win": s.nwin, "gate": s.ngate, "dir": 2, "chan": s.nchan, "bin": s.nbin, "bin_edge": s.nbin + 1,
                "ray": self.nray, "one": 1}
        full, per_ray = ("win", "gate", "dir", "chan", "bin"), ("gate", "dir", "ray")
        v = {"gate_kind": (("gate",), np.array([float(g.kind) for g in s.gates]), "0 latitude circle, 1 meridian"),
             "gate_pos": (("gate",), np.array([float(g.deg) for g in s.gates]), "degrees"),
             "bin_centres": (("gate", "bin"), 0.5 * (edges[:, :-1] + edges[:, 1:]), "degrees"),
             "bin_edges": (("gate", "bin_edge"), edges, "degrees"),
             "cnt": (full, counts_for(ncfile, a["cnt"]), "crossings"), "tsum": (full, a["tsum"], "rows"),
             "dropped": (("one",), np.array([float(a["dropped"])]), "segments"),
             "ncross": (per_ray, a["ncross"], "crossings"),
             "tfirst": (per_ray, a["tfirst"], "rows")}
        if a["wsum"] is not None:
            v["wsum"] = (full, a["wsum"], f"sum of {s.weight} at the crossings")
        ncio.write(ncfile, dims, v)


class CrossSink(ColumnSink):
    """A ``sink`` of ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume``
    and of ``shard.run_sharded`` (``launch_rows.RowSink``) that tests each
    launch's segments against the gates of ``map``.  ``ray``: the column of
    each ray of the integration (None: ray j is column j); the sharded form's
    ``idx`` and ``take(idx)`` select from it, or are the columns themselves.
    Channels are the map's (``CrossMap.chan``), indexed by column."""
