"""Per-ray path summaries reduced on the GPU (``rwrt_ray_summary``, ABI 5).

What a ray-density map drops is the ray: how far each one travelled, how often
it was reflected at a turning latitude, which latitudes it reached, where and
when it stopped, and whether -- and after how many rows -- it reached a given
lon-lat box.  ``RaySummary`` keeps one accumulator column per ray on the
device and updates it from the row blocks and constant tails each ray-loop
launch leaves, so that no output row is shipped to the host.  ``SummarySink``
plugs into ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume`` /
``shard.run_sharded`` through the ``sink`` protocol; ``Tee`` hands one launch
to several sinks (a density map and a summary from one integration);
``WR.ray_summary`` is the user entry point.

``reference_summary`` (NumPy) is the definition.  Counts and selections equal
it exactly; ``path`` adds the same terms in the same order with the device's
``sin / cos / atan2`` and agrees to a relative 1e-12.
"""
import math

import numpy as np

import _hip as H
from launch_rows import one_row, row_args
from raymap import ColumnSink, RayArgs

R_EARTH = 6.3712e6      # metres: path_m = path * R_EARTH
TWO_PI = 2 * math.pi
INT32_MAX = 2 ** 31 - 1
F64_FIELDS = ("lon_first", "lat_first", "lon_last", "lat_last", "l_last", "lat_min", "lat_max", "amp_max", "path")
I32_FIELDS = ("n_valid", "last_row", "n_turn", "prev_valid")
_F64_INIT = (math.nan,) * 5 + (math.inf, -math.inf, -math.inf, 0.0)
_I32_INIT = (0, -1, 0, 0)


def regions_rad(regions):
    """``[(lon_w, lon_e, lat_s, lat_n)]`` in degrees -> an ``[nreg, 4]`` array in
    radians, ``pi * (deg / 180)`` (as ``density.DensitySpec`` converts its
    latitude range: +-90 give +-pi/2 exactly)."""
    regions = [] if regions is None else list(regions)
    if len(regions) > H.SUMMARY_MAXREG:
        raise ValueError(f"at most {H.SUMMARY_MAXREG} regions, got {len(regions)}")
    out = np.empty((len(regions), 4))
    for r, box in enumerate(regions):
        if len(box) != 4:
            raise ValueError("a region is (lon_w, lon_e, lat_s, lat_n) in degrees")
        out[r] = [math.pi * (float(v) / 180.0) for v in box]
    if not np.isfinite(out).all():
        raise ValueError("region edges must be finite")
    return out


def haversine(lon_c, lat_c, lon_p, lat_p):
    """The angle of the reference's ``cal_dis`` (wr.py:97-112), as written there."""
    dlon = lon_c - lon_p
    dlat = lat_c - lat_p
    a = np.sin(dlat / 2.0) ** 2 + np.cos(lat_p) * np.cos(lat_c) * np.sin(dlon / 2.0) ** 2
    return np.abs(2 * np.arctan2(np.sqrt(a), np.sqrt(1.0 - a)))


def inside(lon, lat, box):
    """Whether the points lie in ``box`` (radians): ``lat_s <= lat < lat_n`` and,
    with ``lam = (lon % 2pi) % 2pi``, ``lon_w <= lam < lon_e`` -- or, for a box
    across 0 (``lon_w >= lon_e``), ``lam >= lon_w or lam < lon_e``."""
    w, e, s, n = (float(v) for v in box)
    with np.errstate(all="ignore"):
        lam = np.remainder(np.remainder(lon, TWO_PI), TWO_PI)
        in_lon = ((lam >= w) & (lam < e)) if w < e else ((lam >= w) | (lam < e))
        return in_lon & (lat >= s) & (lat < n)


def reference_summary(rows, regions=None):
    """The definition of a per-ray summary, in NumPy.

    ``rows[nray, nt, 8]``: a logical history, columns lon lat k l amp ug vg
    nacc, row 0 the initial row.  ``regions``: up to 8 boxes ``(lon_w, lon_e,
    lat_s, lat_n)`` in degrees.  A row is valid iff lon and lat are finite.
    Returns a dict of per-ray arrays: ``n_valid``, ``last_row`` (-1: none),
    ``lon_first lat_first`` / ``lon_last lat_last l_last`` (NaN: none),
    ``lat_min lat_max`` (+inf / -inf), ``amp_max`` (max ``|amp|`` over valid
    rows with a finite amp, -inf: none), ``n_turn`` (sign changes of l between
    two valid rows i-1, i), ``path`` (radians: the haversine angles of every
    two valid rows i-1, i, summed in row order), ``path_m``, and per region
    ``first_row[nreg, nray]`` (-1: never) and ``rows_inside[nreg, nray]``."""
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 3 or rows.shape[1] < 1 or rows.shape[2] < 5:
        raise ValueError(f"rows must be [nray, nt >= 1, >= 5], got {rows.shape}")
    nray, nt = rows.shape[:2]
    boxes = regions_rad(regions)
    lon, lat, l, amp = rows[..., 0], rows[..., 1], rows[..., 3], rows[..., 4]
    valid = np.isfinite(lon) & np.isfinite(lat)
    out = {"n_valid": valid.sum(axis=1).astype(np.int32)}
    any_valid = valid.any(axis=1)
    first = np.where(any_valid, valid.argmax(axis=1), 0)
    last = np.where(any_valid, nt - 1 - valid[:, ::-1].argmax(axis=1), 0)
    out["last_row"] = np.where(any_valid, last, -1).astype(np.int32)
    ar = np.arange(nray)
    for name, col, at in (("lon_first", lon, first), ("lat_first", lat, first), ("lon_last", lon, last),
                          ("lat_last", lat, last), ("l_last", l, last)):
        out[name] = np.where(any_valid, col[ar, at], np.nan)
    with np.errstate(all="ignore"):
        out["lat_min"] = np.min(np.where(valid, lat, np.inf), axis=1, initial=np.inf)
        out["lat_max"] = np.max(np.where(valid, lat, -np.inf), axis=1, initial=-np.inf)
        out["amp_max"] = np.max(np.where(valid & np.isfinite(amp), np.abs(amp), -np.inf), axis=1, initial=-np.inf)
        both = valid[:, 1:] & valid[:, :-1]
        lp, lc = l[:, :-1], l[:, 1:]
        out["n_turn"] = (both & (((lp > 0) & (lc < 0)) | ((lp < 0) & (lc > 0)))).sum(axis=1).astype(np.int32)
        seg = np.where(both, haversine(lon[:, 1:], lat[:, 1:], lon[:, :-1], lat[:, :-1]), 0.0)
    # sequential, in row order (np.sum would add pairwise)
    out["path"] = np.add.accumulate(seg, axis=1)[:, -1] if nt > 1 else np.zeros(nray)
    out["path_m"] = out["path"] * R_EARTH
    first_row = np.full((len(boxes), nray), -1, np.int32)
    rows_inside = np.zeros((len(boxes), nray), np.int32)
    for r, box in enumerate(boxes):
        m = valid & inside(lon, lat, box)
        rows_inside[r] = m.sum(axis=1)
        first_row[r] = np.where(m.any(axis=1), m.argmax(axis=1), -1)
    out["first_row"], out["rows_inside"] = first_row, rows_inside
    return out


class RaySummary(RayArgs):
    """The device accumulators of ``nray`` rays: ``f64[9, nray]`` and
    ``i32[4 + 2 nreg, nray]`` (the layout of ``rwrt_ray_summary``,
    include/rwrt.h), set to the values of a ray without rows here and updated
    by every ``start`` / ``add_rows`` call.  The accumulators are a running
    state, not a sum: a ray's rows must arrive once, in order, each call
    starting at the row the previous one ended with (``start`` is row 0)."""

    def __init__(self, nray, regions=(), device=None):
        import torch
        H.require_gpu()
        H.load()
        self.nray = int(nray)
        self.regions = [tuple(float(v) for v in b) for b in (regions or ())]
        self.boxes = regions_rad(self.regions)
        self.nreg = len(self.boxes)
        self.device = torch.device(device or "cuda")
        self._c = H.SummaryRegions()
        self._c.nreg = self.nreg
        for r in range(self.nreg):
            for k in range(4):
                self._c.box[r][k] = float(self.boxes[r, k])
        self.f64 = torch.empty((H.SUMMARY_NF64, self.nray), dtype=torch.float64, device=self.device)
        self.i32 = torch.empty((H.SUMMARY_NI32 + 2 * self.nreg, self.nray), dtype=torch.int32, device=self.device)
        # ownership (allreduce): the columns this object's add_rows calls have
        # updated, i.e. the rays this rank integrated
        self.owned = torch.zeros(self.nray, dtype=torch.bool, device=self.device)
        self.shape = None
        self._reset(slice(None))

    def _reset(self, cols):
        for k, v in enumerate(_F64_INIT):
            self.f64[k, cols] = v
        for k, v in enumerate(_I32_INIT):
            self.i32[k, cols] = v
        self.i32[H.SUMMARY_NI32:H.SUMMARY_NI32 + self.nreg, cols] = -1
        self.i32[H.SUMMARY_NI32 + self.nreg:, cols] = 0

    def add_rows(self, i0, i1, view, tails=None, slots=None, ray=None):
        """Update the rays with rows ``[i0, i1)`` of a launch: ``view`` its row
        buffer (dense ``[n, i1-i0, 8]``, or the row blocks of ``slots``),
        ``tails`` / ``slots`` the launch's ``engine.Tails`` / ``engine.Slots``,
        ``ray`` each ray's column (int64; None: ray j is column j).  One
        asynchronous ``rwrt_ray_summary`` call on the device's current stream."""
        ray = self._update(i0, i1, view, tails, slots, ray)
        if ray is None:
            self.owned.fill_(True)
        else:
            self.owned[ray] = True

    def _update(self, i0, i1, view, tails, slots, ray):
        import torch
        n, rows = row_args(i0, i1, view, tails, slots)
        ray = self._ray(ray, n)
        H.check(H.load().rwrt_ray_summary(
            n, int(i0), int(i1), *rows, H.dptr(ray, torch.int64), self.nray, self._c,
            H.dptr(self.f64, torch.float64), H.dptr(self.i32, torch.int32), H.stream(self.device)))
        return ray

    def start(self, lon0, lat0, l0, amp0, ray=None):
        """Row 0, the initial rays (radians), which sinks never receive: the
        same entry point on a ``[n, 1, 8]`` row tensor; host arrays or device
        tensors (``RayEngine.initial_rows``) of any shape.  Does not claim the
        rays (``owned``): with a process group every rank starts every ray and
        integrates its own."""
        self._update(0, 1, one_row({0: lon0, 1: lat0, 3: l0, 4: amp0}, self.device), None, None, ray)
        return self

    @classmethod
    def from_fields(cls, fields, nt, regions=(), device=None):
        """The summary whose accumulators hold ``fields``, a
        ``reference_summary`` dict of a history of ``nt`` rows
        (``WR.ray_summary(mode='numpy')``): ``numpy()`` returns them bit for bit."""
        import torch
        n = int(np.asarray(fields["n_valid"]).size)
        rs = cls(n, regions, device)
        f = np.stack([np.asarray(fields[k], np.float64).reshape(n) for k in F64_FIELDS])
        last = np.asarray(fields["last_row"]).reshape(n)
        i = [np.asarray(fields["n_valid"]).reshape(n), last, np.asarray(fields["n_turn"]).reshape(n), last == nt - 1]
        i += list(np.asarray(fields["first_row"]).reshape(rs.nreg, n))
        i += list(np.asarray(fields["rows_inside"]).reshape(rs.nreg, n))
        rs.f64.copy_(torch.as_tensor(f))
        rs.i32.copy_(torch.as_tensor(np.stack(i).astype(np.int32)))
        rs.owned.fill_(True)
        return rs

    def allreduce(self, group=None):
        """Combine the ranks' summaries, left on every rank.  A ray is
        integrated by one rank, its owner; the others hold its initial values.
        Ownership is ``self.owned`` -- the columns this rank's ``add_rows``
        updated; a ray nobody integrated belongs to rank 0.  Every rank first
        resets the columns it does not own to the values of a ray without
        rows, which are neutral: SUM for ``path``, ``n_valid``, ``n_turn``,
        ``rows_inside``; MAX for ``last_row``, ``lat_max``, ``amp_max``; MIN for
        ``lat_min``; MIN over "never = INT32_MAX" for ``first_row``; and
        ``*_first`` / ``*_last`` travel as bit patterns, zero from a rank that
        is not the owner, through an integer SUM -- exactly the owner's."""
        import torch
        import torch.distributed as dist
        from shard import _dev
        dev = _dev(group)
        rank = dist.get_rank(group)

        def red(t, op):
            x = t.to(dev).contiguous()
            dist.all_reduce(x, op=op, group=group)
            return x.to(self.device)

        owners = red(self.owned.to(torch.int32), dist.ReduceOp.SUM)
        if int(owners.max().item()) > 1:
            raise H.RwrtError("a ray was integrated by more than one rank")
        mine = self.owned | ((owners == 0) & (rank == 0))
        self._reset(~mine)
        f, i, nr = self.f64, self.i32, self.nreg
        bits = torch.where(mine[None, :], f[:5].view(torch.int64), torch.zeros_like(f[:5], dtype=torch.int64))
        f[:5] = red(bits, dist.ReduceOp.SUM).view(torch.float64)
        f[5] = red(f[5], dist.ReduceOp.MIN)
        f[6:8] = red(f[6:8], dist.ReduceOp.MAX)
        f[8] = red(f[8], dist.ReduceOp.SUM)
        i[0] = red(i[0], dist.ReduceOp.SUM)
        i[1] = red(i[1], dist.ReduceOp.MAX)
        i[2] = red(i[2], dist.ReduceOp.SUM)
        i[3] = red(i[3], dist.ReduceOp.MAX)
        if nr:
            fr = i[4:4 + nr]
            fr = red(torch.where(fr < 0, torch.full_like(fr, INT32_MAX), fr), dist.ReduceOp.MIN)
            i[4:4 + nr] = torch.where(fr == INT32_MAX, torch.full_like(fr, -1), fr)
            i[4 + nr:] = red(i[4 + nr:], dist.ReduceOp.SUM)
        self.owned.fill_(True)
        return self

    def numpy(self):
        """The fields of ``reference_summary`` on the host (waits for the
        pending calls); per-ray arrays take ``self.shape`` when it is set
        (``WR.ray_summary``: ``(3, nsource, nzwn)``)."""
        f, i = self.f64.cpu().numpy(), self.i32.cpu().numpy()
        shp = tuple(self.shape) if self.shape is not None else (self.nray,)
        out = {name: f[k].reshape(shp) for k, name in enumerate(F64_FIELDS)}
        out.update({name: i[k].reshape(shp) for k, name in enumerate(I32_FIELDS) if name != "prev_valid"})
        out["path_m"] = out["path"] * R_EARTH
        out["first_row"] = i[4:4 + self.nreg].reshape((self.nreg,) + shp)
        out["rows_inside"] = i[4 + self.nreg:].reshape((self.nreg,) + shp)
        return out

    def output(self, ncfile):
        """Write the fields (positions in degrees); dims ``root, source, zwn``
        with a 3-d ``self.shape``, else ``ray``; the regions as ``region_box``
        (degrees)."""
        import ncio
        d = self.numpy()
        shp = d["path"].shape
        names = ("root", "source", "zwn") if len(shp) == 3 else ("ray",)
        if len(shp) not in (1, 3):
            raise ValueError(f"shape must be (nray,) or (3, nsource, nzwn), got {shp}")
        dims = dict(zip(names, shp))
        v = {}
        deg = 180.0 / math.pi
        for name in ("lon_first", "lat_first", "lon_last", "lat_last", "lat_min", "lat_max"):
            v[name] = (names, d[name] * deg, "degrees")
        v["l_last"] = (names, d["l_last"])
        v["amp_max"] = (names, d["amp_max"])
        v["path"] = (names, d["path"], "radians")
        v["path_m"] = (names, d["path_m"], "m")
        for name in ("n_valid", "last_row", "n_turn"):
            v[name] = (names, d[name], "rows")
        if self.nreg:
            dims.update(region=self.nreg, edge=4)
            v["region_box"] = (("region", "edge"), np.array(self.regions, np.float64), "degrees: lon_w lon_e lat_s lat_n")
            v["first_row"] = (("region",) + names, d["first_row"], "rows")
            v["rows_inside"] = (("region",) + names, d["rows_inside"], "rows")
        ncio.write(ncfile, dims, v)


class SummarySink(ColumnSink):
    """A ``sink`` of ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume``
    and of ``shard.run_sharded`` (``launch_rows.RowSink``) that updates
    ``summary`` from each launch's rows.  ``ray``: the column of each ray of
    the integration (None: ray j is column j); the sharded form's ``idx`` and
    ``take(idx)`` select from it, or are the columns themselves."""
    summary = property(lambda self: self.target)


class Tee:
    """One launch's rows to several sinks, in order (a ``DensitySink`` and a
    ``SummarySink`` share one integration).  It takes tails / row blocks only
    if every member does, so that each member sees a layout it understands."""

    def __init__(self, *sinks):
        if not sinks:
            raise ValueError("Tee needs at least one sink")
        self.sinks = sinks
        self.takes_tails = all(getattr(s, "takes_tails", False) for s in sinks)
        self.takes_slots = all(getattr(s, "takes_slots", False) for s in sinks)

    def take(self, idx):
        """The Tee of every member's ``take(idx)`` (a shard integrated on its
        own); a member without one cannot follow a shard's ray numbering."""
        for s in self.sinks:
            if not hasattr(s, "take"):
                raise TypeError(f"{type(s).__name__} has no take(idx): it cannot receive a shard's rows")
        return Tee(*[s.take(idx) for s in self.sinks])

    def __call__(self, i0, i1, view, *rest, **kw):
        for s in self.sinks:
            s(i0, i1, view, *rest, **kw)
