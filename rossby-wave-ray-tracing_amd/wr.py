"""Ray tracer object: the reference's ``WR`` (wr.py:114-977) with a HIP ray loop.

Same constructor, attributes (``rlon .. rvg`` of shape ``(nt, 3, nsource,
nzwn)``, NaN-initialised) and methods as the reference.  The ray loop is
selected the same way: ``ray_run(mode, inte_method)`` builds
``mode + '_rk45'`` (wr.py:897-911) and ``core_ray_run`` dispatches it
(wr.py:889-895).  The one integrator this framework provides is
``mode='hip', inte_method='rk45'`` -> ``core_ray_run_hip_rk45``: the fused
MI355X kernel replaces ``core_ray_run_rk45`` (wr.py:767-887) and everything it
calls (RK45 stepper, ``diffun_numpy``, ``cal_bs_mercator_point``,
``cal_ugvg``).  Other modes raise: there is no CPU fallback.
"""
import sys

import numpy as np

from bs import BS, cal_ky
from constants import day, hour, rad2deg, undef, deg2rad
import ncio
from wn import cal_ugvg

SUPPORTED = ("hip_rk45", "hip")      # GPU RK45 (wr.py:767-887) and GPU RK4 (wr.py:702-765)


def progress_bar(current, total, bar_length=50):
    percent = float(current) / total
    arrow = "=" * int(round(percent * bar_length) - 1) + ">"
    sys.stdout.write(f"\rprocess: [{arrow + ' ' * (bar_length - len(arrow))}] "
                     f"{int(round(percent * 100))}%")
    sys.stdout.flush()


class WR:
    """Barotropic Rossby-wave ray tracer (constructor of wr.py:133-171)."""

    def __init__(self, nzwn, nsource, tstep=1. * hour, ttotal=20. * day, freq=0,
                 cal_dtype="float64", read_dtype="float32", rtol=1e-6, atol=1e-6,
                 cut_off=0.1, nx=None, ny=None, ncfile=None, MinStepFactor=1e-3,
                 chunk_rows=None, progress=False, backward=False):
        if cal_dtype != "float64":
            raise ValueError("cal_dtype must be 'float64' (as in main_wr.py:21)")
        self.all_dtype = cal_dtype
        if nx is None or ny is None:
            if ncfile is None:
                raise ValueError("ncfile is need")
            ny, nx = self.get_defualt_nlon_and_nlat(ncfile)
        self.bs = BS(nx, ny, read_dtype=read_dtype, cal_dtype=cal_dtype)
        self.tstep = np.array([tstep], dtype=cal_dtype)
        self.ttotal = ttotal
        self.freq = np.array([freq], dtype=cal_dtype)
        self.nzwn = nzwn
        self.zwn = np.zeros(nzwn, dtype=cal_dtype)
        self.nsource = nsource
        self.source_lon = np.zeros(nsource, dtype=cal_dtype)
        self.source_lat = np.zeros(nsource, dtype=cal_dtype)
        self.nt = int(self.ttotal / self.tstep[0]) + 1
        shape = (self.nt, 3, nsource, nzwn)
        for name in ("rlon", "rlat", "rzwn", "rmwn", "ramp", "rug", "rvg"):
            setattr(self, name, np.full(shape, undef, dtype=cal_dtype))
        self.rtol, self.atol = rtol, atol
        self.cut_off = cut_off * self.tstep / 3600.
        self.MinStepFactor = MinStepFactor
        self.chunk_rows = chunk_rows
        self.progress = progress
        self.last_run = None       # engine.RunResult of the last ray_run
        # backward ray tracing: the sources are receptors, the rays are
        # integrated towards negative time (the RK45 loop's direction = -1) and
        # row i of the history is the state at -i * tstep (rows index elapsed
        # steps; ug, vg are the true group velocity at the point)
        self.backward = bool(backward)
        # the source lattice set_source_matrix remembers (ray_tube finds a ray's neighbours from it)
        self.source_nnx = self.source_nny = self.source_dlon = self.source_cyclic_x = None

    def get_defualt_nlon_and_nlat(self, ncfile):
        """(nlat, nlon) from the file's lat/lon (or u's last two dims), wr.py:173-212."""
        d = ncio.read(ncfile)
        lat = next((d[k] for k in ("lat", "latitude", "Lat", "Latitude") if k in d), None)
        lon = next((d[k] for k in ("lon", "longitude", "Lon", "Longitude") if k in d), None)
        if lat is None or lon is None:
            print("!!!WARNING: Using u.shape[-2] and u.shape[-1] as nlat and nlon!!!")
            return d["u"].shape[-2], d["u"].shape[-1]
        return lat.shape[0], lon.shape[0]

    # ----------------------------------------------------------- sources
    def set_zwn(self, zwn_array):
        if len(zwn_array) != self.nzwn:
            raise ValueError("Length of zwn_array must equal nzwn")
        self.zwn[:] = np.array(zwn_array, dtype=self.all_dtype)

    def set_freq(self, freq):
        self.freq = np.array([freq], dtype=self.all_dtype)

    def set_source_array(self, lon_list, lat_list):
        if len(lon_list) != self.nsource or len(lat_list) != self.nsource:
            raise ValueError("Source list length mismatch nsource")
        self.source_lon = np.array(lon_list, dtype=self.all_dtype) * (1.0 * deg2rad)
        self.source_lat = np.array(lat_list, dtype=self.all_dtype) * (1.0 * deg2rad)
        self.source_nnx = self.source_nny = self.source_dlon = self.source_cyclic_x = None

    def set_source_matrix(self, SW_lon, SW_lat, dlon, dlat, nnx, nny):
        """Regular source grid, index ``iy*nnx + ix`` (wr.py:236-258)."""
        if nnx * nny != self.nsource:
            raise ValueError("nsource != nnx * nny, matrix size mismatch!")
        if SW_lat + (nny - 1) * dlat > 89.0:
            raise ValueError("source latitude out of -90~90 range!")
        SW_lon = SW_lon % 360.0
        for iy in range(nny):
            for ix in range(nnx):
                idx = iy * nnx + ix
                self.source_lon[idx] = ((SW_lon + ix * dlon) % 360.0) * deg2rad
                self.source_lat[idx] = (SW_lat + iy * dlat) * deg2rad
        self.source_nnx, self.source_nny, self.source_dlon = nnx, nny, dlon
        self.source_cyclic_x = bool(nnx * dlon == 360)   # (sources all around a latitude circle)

    def ray_info(self):
        bar = "=" * 78
        lines = [bar, " WNWR Package: Barotropic Horizontal Rossby Wave Ray Tracing Information ",
                 f" Shape of the Basic Flow (nlon x nlat): {self.bs.nlon} x {self.bs.nlat}",
                 f" Initial Zonal Wave Numbers (nzwn): {self.nzwn}",
                 " " * 15 + " ".join(f"{z:.1f}" for z in self.zwn),
                 f" Source Locations (total {self.nsource} points):"]
        lines += [" " * 15 + f"{lo * rad2deg:7.2f}, {la * rad2deg:7.2f}"
                  for lo, la in zip(self.source_lon, self.source_lat)]
        lines += [f" Time Step (s): {self.tstep[0]:.1f}",
                  f" Total Integration Time (day): {self.ttotal / day:.1f}",
                  f" Total Steps (nt): {self.nt}", bar]
        print("\n".join(lines))

    # ------------------------------------------------------ initial rays
    def ray_initial_numpy(self, root_method="numpy"):
        """Initial rows (wr.py:344-395): positions, k, the 3 m roots, amp, ug, vg."""
        rows = initial_rows(self.bs, self.source_lon, self.source_lat, self.zwn, self.freq,
                            root_method)
        for h, r in zip((self.rlon, self.rlat, self.rzwn, self.rmwn, self.ramp, self.rug,
                         self.rvg), rows):
            h[0] = r

    def ray_initial_hip(self):
        """Initial rows on the GPU (``RayEngine.initial_rows``): bit-identical to
        ``ray_initial_numpy`` -- np.roots' companion-matrix eigenvalues restated
        operation for operation on the device (csrc/nproots.h)."""
        rows = self.bs.engine().initial_rows(self.source_lon, self.source_lat, self.zwn,
                                             self.freq).cpu().numpy()
        for h, r in zip((self.rlon, self.rlat, self.rzwn, self.rmwn, self.ramp, self.rug,
                         self.rvg), rows):
            h[0] = r

    def ray_initial(self, mode="numpy", root_method="numpy"):
        """Initial rays (wr.py:417-421): ``mode='numpy'`` is the reference's
        vectorised host initialiser, ``mode='hip'`` the same on the GPU."""
        if mode == "hip":
            self.ray_initial_hip()
        else:
            self.ray_initial_numpy(root_method=root_method)

    # ---------------------------------------------------------- ray loop
    def core_ray_run_hip_rk45(self, group=None):
        """The RK45 ray loop on the GPU (replaces wr.py:767-887)."""
        return self._core_ray_run_hip("rk45", group)

    def core_ray_run_hip(self, group=None):
        """The fixed-step RK4 ray loop on the GPU (replaces wr.py:702-765)."""
        return self._core_ray_run_hip("rk4", group)

    def _core_ray_run_hip(self, method, group=None, sink=None):
        """Shared driver of the two GPU ray loops.

        ``sink`` (``ray_density``, ``ray_summary``): a device-side consumer of
        the rows (the engine's ``sink`` protocol, with ``take(idx)`` for a rank's shard)
        that replaces the delivery into the history arrays -- no row reaches
        the host and the arrays keep only row 0.

        With a torch.distributed ``group`` of one process per GPU, the rays are
        sharded over the ranks (shard.py): rank 0's basic state is broadcast,
        every rank integrates its shard, and rank 0 gathers every output row
        into its history arrays (the other ranks' arrays keep only row 0).
        """
        import torch
        import shard
        rank, world = shard.world_info(group) if group is not None else (0, 1)
        multi = group is not None and shard.collective(world)
        if multi:
            self.bs.fields = shard.broadcast_array(self.bs.fields, 0, group)
            self.bs._engine = None
        eng = self.bs.engine()
        nray = 3 * self.nsource * self.nzwn
        y0 = np.array([self.rlon[0], self.rlat[0], self.rzwn[0], self.rmwn[0],
                       self.ramp[0]], dtype=self.all_dtype).reshape(5, nray)
        idx = np.arange(nray)
        if multi:
            idx = shard.shard_indices(~np.isnan(y0.mean(axis=0)), rank, world)
        rows_shape = (3, self.nsource, self.nzwn)
        hist = (self.rlon, self.rlat, self.rzwn, self.rmwn, self.ramp, self.rug, self.rvg)
        own_sink = sink is None   # (deliver into the history arrays)

        if multi and own_sink:
            # each rank's previous rows (row 0: the initial rows), as bit patterns
            row0 = np.stack([h[0].reshape(-1)[idx] for h in hist], axis=1)
            last = torch.as_tensor(np.ascontiguousarray(row0)).view(torch.int64).to(eng.device)

        def gather_sink(i0, i1, rows):
            # rank 0 receives only the rays whose rows changed; every other
            # ray repeats its previous row (hostio.fill_rows)
            got = shard.gather_changed_rows(rows, torch.as_tensor(idx, device=rows.device), last, 0, group)
            if got is None:
                return
            cols, data = got
            host = data.permute(2, 1, 0).contiguous().cpu().numpy()        # [7][rows][n]
            cols = np.ascontiguousarray(cols.cpu().numpy())
            from hostio import fill_rows
            for v in range(7):
                dst = hist[v][i0:i1].reshape(i1 - i0, nray)
                fill_rows(dst, hist[v][i0 - 1].reshape(nray), host[v], cols if len(cols) else None)
            if self.progress:
                progress_bar(i1 - 1, self.nt)

        chunk = self.chunk_rows or _default_chunk(nray, self.nt)
        grp = group if multi else None
        out, hs = None, None
        if not own_sink:
            sink = sink.take(idx) if multi else sink
        elif multi:
            sink = gather_sink
        else:
            # single GPU: chunks reach the host arrays while the next one is
            # computed (permute on the device, pinned D2H, threaded copies)
            from hostio import HistorySink
            hs = HistorySink(hist, rows_shape, nray, min(chunk, self.nt - 1), eng.device,
                             progress=(lambda i: progress_bar(i, self.nt)) if self.progress else None)
            sink, out = hs, hs.buffers()
        try:
            if method == "rk4":
                res = eng.integrate_rk4(torch.as_tensor(y0[:, idx]), self.nt, float(self.tstep[0]),
                                        chunk=chunk, sink=sink, cut_rad=float(self.cut_off[0]),
                                        group=grp, out=out, backward=self.backward)
            else:
                res = eng.integrate(torch.as_tensor(y0[:, idx]), self.nt, float(self.tstep[0]),
                                    self.rtol, self.atol, self.MinStepFactor, ttotal=self.ttotal,
                                    chunk=chunk, sink=sink, cut_rad=float(self.cut_off[0]),
                                    group=grp, out=out, backward=self.backward)
        finally:
            if hs is not None:
                hs.finish()
                # ray-rows shipped over PCIe vs delivered (frozen rays' rows are filled on the host)
                self.last_delivery = {"shipped_ray_rows": hs.shipped, "delivered_ray_rows": hs.delivered,
                                      "host_fill_s": hs.t_fill, "host_wait_s": hs.t_wait}
        if res.break_row is not None and own_sink:
            for h in hist:
                h[res.break_row:] = np.nan     # rows never stored (wr.py:853-855, 886-887)
        self.last_run = res
        return res

    # ---- the products reduced on the device (raymap.py): what the ray_* methods share
    def _channels(self, spec, by):
        """``(spec, chan)`` for ``by``: the spec with one map per zonal
        wavenumber or root and the channel of every ray slot (None: one map)."""
        import raymap
        _check_by(by)
        if by is None:
            return spec, None
        ax = np.arange(self.nzwn)[None, None, :] if by == "zwn" else np.arange(3)[:, None, None]
        chan = np.ascontiguousarray(np.broadcast_to(ax, (3, self.nsource, self.nzwn))).reshape(-1).astype(np.int32)
        return raymap.with_channels(spec, self.nzwn if by == "zwn" else 3), chan

    def _column(self, col, rows=0):
        """Rows ``rows`` of the history array of row column ``col`` (2..6); None for -1."""
        return None if col < 0 else (self.rzwn, self.rmwn, self.ramp, self.rug, self.rvg)[col - 2][rows]

    def _history_rows(self, inte_method, root_method, group):
        """``ray_run`` on the GPU and its history as rows ``[nray, nt, 8]``
        (the ``mode='numpy'`` products apply their reference to it)."""
        self.ray_run(mode="hip", inte_method=inte_method, root_method=root_method, group=group)
        nray = 3 * self.nsource * self.nzwn
        rows = np.full((nray, self.nt, 8), np.nan)
        for c, h in enumerate((self.rlon, self.rlat, self.rzwn, self.rmwn, self.ramp, self.rug, self.rvg)):
            rows[:, :, c] = h.reshape(self.nt, nray).T
        return rows

    def _reduce_on_device(self, make, mode, inte_method, group, root_method):
        """Initialise the rays, integrate them into the sink of ``make(rank,
        device) -> (product, sink)`` -- which also hands row 0 to the product
        -- and combine the ranks' products."""
        import shard
        key = mode + "_rk45" if inte_method == "rk45" else mode
        if key not in SUPPORTED:
            self.core_ray_run(key)     # raises before any work
        self._check_direction(key)
        self.ray_initial(mode=mode, root_method=root_method)
        rank, world = shard.world_info(group) if group is not None else (0, 1)
        product, sink = make(rank, self.bs.engine().device)
        self._core_ray_run_hip("rk45" if key == "hip_rk45" else "rk4", group, sink=sink)
        if group is not None and shard.collective(world):
            product.allreduce(group)
        return product

    def ray_density(self, spec, mode="hip", inte_method="rk45", by=None, include_initial=True,
                    group=None, root_method="numpy"):
        """Initialise and integrate all rays like ``ray_run``, but bin every
        output row into a lon-lat map on the GPU (density.py) instead of
        delivering the history: returns the ``density.DensityMap``; only row 0
        of ``rlon .. rvg`` is filled.

        ``spec``: a ``density.DensitySpec``.  ``by``: one map per zonal
        wavenumber (``'zwn'``) or per root (``'root'``) -- sets the channel of
        ray slot (root, source, zwn) and the number of maps; None: one map.
        ``include_initial``: count row 0 (the sources) too.  ``mode='numpy'``
        integrates on the GPU all the same, delivers the history and bins it
        on the host with ``density.reference_bins`` (small runs; returns
        ``(count, wsum)``).  With a process ``group`` every rank ends with the
        sum over the ranks."""
        import density as D
        spec, chan = self._channels(spec, by)
        if mode == "numpy":
            rows = self._history_rows(inte_method, root_method, group)[:, 0 if include_initial else 1:]
            return D.reference_bins(rows[..., 0].T, rows[..., 1].T, None if spec.wcol < 0 else rows[..., spec.wcol].T,
                                    None if chan is None else chan[None, :], spec)

        def make(rank, device):
            dmap = D.DensityMap(spec, device)
            if include_initial and rank == 0:
                dmap.add_points(self.rlon[0], self.rlat[0], self._column(spec.wcol), chan)
            return dmap, D.DensitySink(dmap, chan)

        return self._reduce_on_device(make, mode, inte_method, group, root_method)

    def ray_arrival(self, spec, mode="hip", inte_method="rk45", by=None, include_initial=True,
                    group=None, root_method="numpy"):
        """Initialise and integrate all rays like ``ray_run``, but reduce every
        output row into an arrival-time map on the GPU (arrival.py) instead of
        delivering the history: returns the ``arrival.ArrivalMap`` -- per map
        box the first and the last row with a ray point in it and, per time
        window, how many; only row 0 of ``rlon .. rvg`` is filled.

        ``spec``: an ``arrival.ArrivalSpec`` whose ``nt`` equals this run's.
        ``by``, ``include_initial``: as in ``ray_density``.  ``mode='numpy'``
        integrates on the GPU all the same, delivers the history and applies
        ``arrival.reference_arrival`` on the host (small runs; returns its
        dict).  With a process ``group`` every rank ends with the reduced map."""
        import arrival as A
        _check_by(by)
        if spec.nt != self.nt:
            raise ValueError(f"spec.nt is {spec.nt}, the run has {self.nt} rows")
        spec, chan = self._channels(spec, by)
        col = spec.bins.wcol
        if mode == "numpy":
            first = 0 if include_initial else 1
            rows = self._history_rows(inte_method, root_method, group)[:, first:]
            return A.reference_arrival(rows[..., 0], rows[..., 1], None if col < 0 else rows[..., col], chan, spec,
                                       row0=first)

        def make(rank, device):
            amap = A.ArrivalMap(spec, device)
            if include_initial and rank == 0:
                amap.add_points(self.rlon[0], self.rlat[0], self._column(col), chan)
            return amap, A.ArrivalSink(amap, chan)

        return self._reduce_on_device(make, mode, inte_method, group, root_method)

    def ray_flux(self, spec, mode="hip", inte_method="rk45", by=None, through=None, through_mode="any",
                 include_initial=True, group=None, root_method="numpy"):
        """Initialise and integrate all rays like ``ray_run``, but reduce every
        output row into a wave-ray flux map on the GPU (flux.py) instead of
        delivering the history: returns the ``flux.FluxMap`` -- per map box
        the summed group-velocity (or unit) vectors of the accepted ray points,
        their number, the sum of their rows and of their speeds; only row 0 of
        ``rlon .. rvg`` is filled.

        ``spec``: a ``flux.FluxSpec``.  ``by``, ``include_initial``: as in
        ``ray_density``.  ``through``: up to 8 boxes ``(lon_w, lon_e, lat_s,
        lat_n)`` in degrees (the regions of ``ray_summary``); only the rays
        that pass through any (``through_mode='any'``) or every (``'all'``) box
        contribute.  That costs a second integration: the first one reduces
        the rays to a ``ray_summary`` with these regions, the rays that do not
        pass get channel -1, the second one reduces the flux (the initial rows
        are deterministic: both see the same rays).  The map's ``selected`` is
        then a bool array ``(3, nsource, nzwn)``, else None.  ``mode='numpy'``
        integrates on the GPU all the same, delivers the history and applies
        ``flux.reference_flux`` (and ``summary.reference_summary`` for the
        selection) on the host (small runs; returns the dict of
        ``reference_flux`` with ``'selected'`` added).  With a process
        ``group`` every rank ends with the sum over the ranks."""
        import flux as F
        _check_by(by)
        if through_mode not in ("any", "all"):
            raise ValueError("through_mode must be 'any' or 'all'")
        if through is not None and not 1 <= len(through) <= 8:
            raise ValueError("through must be None or 1 to 8 boxes (lon_w, lon_e, lat_s, lat_n)")
        spec, chan = self._channels(spec, by)
        shape = (3, self.nsource, self.nzwn)

        def only(selected):      # channel -1 for the rays that do not pass
            return np.where(selected, 0 if chan is None else chan, -1).astype(np.int32)

        selected = None
        if mode == "numpy":
            rows = self._history_rows(inte_method, root_method, group)
            if through is not None:
                import summary as Sm
                first_row = Sm.reference_summary(rows, through)["first_row"] >= 0
                selected = first_row.any(axis=0) if through_mode == "any" else first_row.all(axis=0)
                chan = only(selected)
            first = 0 if include_initial else 1
            out = F.reference_flux(*(rows[:, first:, c] for c in (0, 1, 2, 3, 5, 6)), chan, spec, row0=first)
            out["selected"] = None if selected is None else selected.reshape(shape)
            return out
        if through is not None:
            # (validates mode / inte_method before any work, like _reduce_on_device)
            rs = self.ray_summary(regions=through, mode=mode, inte_method=inte_method, group=group,
                                  root_method=root_method)
            selected = F.select_through(rs, through_mode).cpu().numpy()
            chan = only(selected)

        def make(rank, device):
            fmap = F.FluxMap(spec, device)
            fmap.selected = None if selected is None else selected.reshape(shape)
            if include_initial and rank == 0:
                fmap.add_points(self.rlon[0], self.rlat[0], self.rzwn[0], self.rmwn[0], self.rug[0], self.rvg[0], chan)
            return fmap, F.FluxSink(fmap, chan)

        return self._reduce_on_device(make, mode, inte_method, group, root_method)

    def _ray_segments(self, reference, Map, Sink, spec, mode, inte_method, by, group, root_method, start=None):
        """``ray_track`` / ``ray_cross`` / ``ray_phase``: the product's
        reference function, its ``raymap.CarriedMap`` and its sink.  ``start(m,
        rank)``: hands row 0 to the map where ``CarriedMap.start``'s columns
        are not all it needs."""
        spec, chan = self._channels(spec, by)
        if mode == "numpy":
            return reference(self._history_rows(inte_method, root_method, group), chan, spec)

        def make(rank, device):
            m = Map(spec, 3 * self.nsource * self.nzwn, device, chan)
            # row 0 on every rank: the rank that integrates a ray carries it into row 1
            if start is None:
                m.start(self.rlon[0], self.rlat[0], self._column(spec.ncol), self._column(spec.wcol))
            else:
                start(m, rank)
            return m, Sink(m)

        return self._reduce_on_device(make, mode, inte_method, group, root_method)

    def ray_track(self, spec, mode="hip", inte_method="rk45", by=None, group=None, root_method="numpy"):
        """Initialise and integrate all rays like ``ray_run``, but deposit the
        segment between every two consecutive output rows of a ray into every
        map box it passes through (track.py) instead of delivering the
        history: returns the ``track.TrackMap`` -- per box the residence time
        in row intervals, the number of visits and, with ``spec.weight``, the
        time integral of that column; only row 0 of ``rlon .. rvg`` is filled.

        ``spec``: a ``track.TrackSpec``.  ``by``: as in ``ray_density``.
        ``mode='numpy'`` integrates on the GPU all the same, delivers the
        history and applies ``track.reference_track`` on the host (small runs;
        returns its dict).  With a process ``group`` every rank ends with the
        sum over the ranks."""
        import track as T
        return self._ray_segments(T.reference_track, T.TrackMap, T.TrackSink, spec, mode, inte_method, by, group, root_method)

    def ray_cross(self, spec, mode="hip", inte_method="rk45", by=None, group=None, root_method="numpy"):
        """Initialise and integrate all rays like ``ray_run``, but test the
        segment between every two consecutive output rows of a ray against the
        gates of ``spec`` (cross.py) instead of delivering the history:
        returns the ``cross.CrossMap`` -- per gate, direction and bin along the
        gate the number of crossings, the sum of their times and, with
        ``spec.weight``, of that column at the crossing, and per ray the
        crossings and the first crossing time, arrays that reshape to
        ``(ngate, 2, 3, nsource, nzwn)``; only row 0 of ``rlon .. rvg`` is
        filled.

        ``spec``: a ``cross.CrossSpec``.  ``by``: as in ``ray_density``.
        ``mode='numpy'`` integrates on the GPU all the same, delivers the
        history and applies ``cross.reference_cross`` on the host (small runs;
        returns its dict).  With a process ``group`` every rank ends with the
        sum over the ranks."""
        import cross as X
        return self._ray_segments(X.reference_cross, X.CrossMap, X.CrossSink, spec, mode, inte_method, by, group, root_method)

    def ray_phase(self, spec, mode="hip", inte_method="rk45", by=None, group=None, root_method="numpy"):
        """Initialise and integrate all rays like ``ray_run``, but integrate
        the WKB phase ``theta = int k dlon + l dY`` along every ray and
        deposit every ray point's wave ``w exp(i psi)`` into its box of a
        lon-lat map (phase.py) instead of delivering the history: returns the
        ``phase.PhaseMap`` -- per box ``cnt``, ``re``, ``im`` and, with
        ``spec.weight``, ``wabs`` (``field()``, ``amplitude()``,
        ``mean_phase()``, ``coherence()``), and per ray ``theta`` and
        ``nseg``, arrays that reshape to ``(3, nsource, nzwn)``; only row 0 of
        ``rlon .. rvg`` is filled.

        ``spec``: a ``phase.PhaseSpec``; where it leaves ``omega_dt`` at 0 and
        this run's ``freq`` is not 0, ``omega_dt = freq * tstep``, negated for
        ``backward=True`` (row i is the state at ``-i * tstep`` there).  ``by``:
        as in ``ray_density``.  ``mode='numpy'`` integrates on the GPU all the
        same, delivers the history and applies ``phase.reference_phase`` on the
        host (small runs; returns its dict).  With a process ``group`` every
        rank ends with the sum over the ranks."""
        from dataclasses import replace
        import phase as P
        if spec.omega_dt == 0.0 and float(self.freq[0]) != 0.0:
            omega_dt = float(self.freq[0]) * float(self.tstep[0])
            spec = replace(spec, omega_dt=-omega_dt if self.backward else omega_dt)

        def start(m, rank):
            m.start(self.rlon[0], self.rlat[0], self._column(m.spec.ncol), self._column(m.spec.wcol),
                    k=self.rzwn[0], l=self.rmwn[0])
            if rank != 0:
                m.clear_maps()     # (row 0 is deposited once: by rank 0)

        return self._ray_segments(P.reference_phase, P.PhaseMap, P.PhaseSink, spec, mode, inte_method, by, group,
                                  root_method, start=start)

    def ray_tube(self, spec, by=None, nbr=None, mode="hip", inte_method="rk45", group=None, root_method="numpy"):
        """Initialise and integrate all rays like ``ray_run``, but follow the
        tube that every ray's neighbours in the source lattice span around it
        (tube.py) instead of delivering the history: returns the
        ``tube.TubeMap`` -- per map box the tube points ``cnt``, the sum of
        ``log|D|`` of the geometric spreading ``D`` and the caustics
        (``mean_log_spreading()``, ``geometric_amplitude()``,
        ``caustic_density()``), and per ray the Maslov index ``mu``, the row
        of the ``first`` caustic, the open rows ``nrow``, ``close_row``,
        ``dmin``, ``dlast`` and the tube's columns ``f0``, ``flast``
        (``ftle(tstep)``), arrays that reshape to ``(3, nsource, nzwn)``; only
        row 0 of ``rlon .. rvg`` is filled.

        ``spec``: a ``tube.TubeSpec``.  ``by``: as in ``ray_density``.
        ``nbr``: the W, E, S, N neighbour of every ray slot (int ``[4, 3 *
        nsource * nzwn]``, -1: none); None: those of the lattice
        ``set_source_matrix`` made (``tube.lattice_neighbours``, cyclic in x
        where ``nnx * dlon == 360``) -- sources from ``set_source_array`` have
        no lattice and need ``nbr``.  ``backward=True`` runs work unchanged:
        the tube then says how sharply a receptor's origin is determined.
        ``mode='numpy'`` integrates on the GPU all the same, delivers the
        history and applies ``tube.reference_tube`` on the host (small runs;
        returns its dict).  A process ``group`` is refused: a ray's
        neighbours live on other ranks."""
        import tube as Tu
        if group is not None:
            raise NotImplementedError("ray_tube is not sharded: a ray's neighbours live on other ranks "
                                      "(DESIGN.md section 25 says what it would take)")
        _check_by(by)
        nray = 3 * self.nsource * self.nzwn
        if nbr is None:
            if self.source_nnx is None:
                raise ValueError("sources from set_source_array have no lattice: pass nbr (int [4, nray]: the W, E, "
                                 "S, N neighbour of every ray slot, -1 for none)")
            nbr = Tu.lattice_neighbours(self.source_nnx, self.source_nny, self.nzwn, nlead=3,
                                        cyclic_x=self.source_cyclic_x)
        nbr = Tu.check_neighbours(nbr, nray)
        return self._ray_segments(lambda rows, chan, sp: Tu.reference_tube(rows, nbr, chan, sp),
                                  lambda sp, n, device, chan: Tu.TubeMap(sp, n, nbr, device, chan),
                                  Tu.TubeSink, spec, mode, inte_method, by, None, root_method)

    def ray_wave(self, spec, by=None, nbr=None, mode="hip", inte_method="rk45", group=None, root_method="numpy"):
        """Initialise and integrate all rays like ``ray_run``, but walk every
        ray's tube and its WKB phase together and deposit every point of an
        open tube as the wave ``w |D|^(-1/2) exp(i (theta - omega_dt row - mu
        pi / 2))`` into its box of a lon-lat map (wave.py) instead of
        delivering the history: the wave field of ``ray_phase`` with the
        quarter-period each caustic takes from the phase and the amplitude the
        spreading of the tube gives.  Returns the ``wave.WaveMap`` -- per box
        ``cnt``, ``re``, ``im`` and ``wabs`` (``field()``, ``amplitude()``,
        ``mean_phase()``, ``coherence()``), ``dropped`` and ``clipped``, and
        per ray ``theta``, ``nseg``, ``mu``, ``first``, ``nrow``,
        ``close_row`` and ``dlast``, arrays that reshape to ``(3, nsource,
        nzwn)``; only row 0 of ``rlon .. rvg`` is filled.

        ``spec``: a ``wave.WaveSpec``; ``omega_dt`` is filled in as in
        ``ray_phase`` (``freq * tstep``, negated for ``backward=True``).
        ``by``: as in ``ray_density``.  ``nbr``: as in ``ray_tube`` (None: the
        lattice of ``set_source_matrix``).  ``mode='numpy'`` integrates on the
        GPU all the same, delivers the history and applies
        ``wave.reference_wave`` on the host (small runs; returns its dict).  A
        process ``group`` is refused: a ray's neighbours live on other
        ranks."""
        from dataclasses import replace
        import tube as Tu
        import wave as Wv
        if group is not None:
            raise NotImplementedError("ray_wave is not sharded: a ray's neighbours live on other ranks "
                                      "(DESIGN.md section 27 says what is left out)")
        _check_by(by)
        nray = 3 * self.nsource * self.nzwn
        if nbr is None:
            if self.source_nnx is None:
                raise ValueError("sources from set_source_array have no lattice: pass nbr (int [4, nray]: the W, E, "
                                 "S, N neighbour of every ray slot, -1 for none)")
            nbr = Tu.lattice_neighbours(self.source_nnx, self.source_nny, self.nzwn, nlead=3,
                                        cyclic_x=self.source_cyclic_x)
        nbr = Tu.check_neighbours(nbr, nray)
        if spec.omega_dt == 0.0 and float(self.freq[0]) != 0.0:
            omega_dt = float(self.freq[0]) * float(self.tstep[0])
            spec = replace(spec, omega_dt=-omega_dt if self.backward else omega_dt)

        def start(m, rank):
            m.start(self.rlon[0], self.rlat[0], self._column(m.spec.ncol), self._column(m.spec.wcol),
                    k=self.rzwn[0], l=self.rmwn[0])

        return self._ray_segments(lambda rows, chan, sp: Wv.reference_wave(rows, nbr, chan, sp),
                                  lambda sp, n, device, chan: Wv.WaveMap(sp, n, nbr, device, chan),
                                  Wv.WaveSink, spec, mode, inte_method, by, None, root_method, start=start)

    def ray_summary(self, regions=None, mode="hip", inte_method="rk45", group=None, root_method="numpy"):
        """Initialise and integrate all rays like ``ray_run``, but reduce every
        ray's rows to a path summary on the GPU (summary.py) instead of
        delivering the history: returns the ``summary.RaySummary``, whose
        ``numpy()`` gives fields of shape ``(3, nsource, nzwn)`` -- path
        length, turning points, latitude range, first / last point, and per
        region the first row inside and the rows spent there; only row 0 of
        ``rlon .. rvg`` is filled.

        ``regions``: up to 8 boxes ``(lon_w, lon_e, lat_s, lat_n)`` in degrees
        (``lon_w > lon_e``: across 0).  ``mode='numpy'`` integrates on the GPU
        all the same, delivers the history and applies
        ``summary.reference_summary`` on the host (small runs; the
        ``RaySummary`` returned holds its fields).  With a process ``group`` every rank ends with every ray's
        summary."""
        import summary as Sm
        shape = (3, self.nsource, self.nzwn)
        if mode == "numpy":
            rows = self._history_rows(inte_method, root_method, group)
            rs = Sm.RaySummary.from_fields(Sm.reference_summary(rows, regions), self.nt, regions or (),
                                           self.bs.engine().device)
            rs.shape = shape
            return rs

        def make(rank, device):
            rs = Sm.RaySummary(3 * self.nsource * self.nzwn, regions or (), device)
            rs.shape = shape
            # row 0 on every rank: the rank that integrates a ray carries it into row 1
            rs.start(self.rlon[0], self.rlat[0], self.rmwn[0], self.ramp[0])
            return rs, Sm.SummarySink(rs)

        return self._reduce_on_device(make, mode, inte_method, group, root_method)

    def _check_direction(self, key):
        """Backward tracing is the RK45 loop's: the RK4 loop is refused before any work."""
        if self.backward and key != "hip_rk45":
            raise NotImplementedError("backward ray tracing needs ray_run(mode='hip', inte_method='rk45'): "
                                      "the fixed-step RK4 loop has no signed step")

    def core_ray_run(self, mode="hip_rk45", group=None):
        if mode not in SUPPORTED:
            raise NotImplementedError(
                f"ray loop {mode!r} is not provided by this framework; use "
                f"ray_run(mode='hip', inte_method='rk45') (adaptive RK45) or "
                f"ray_run(mode='hip', inte_method='') (fixed-step RK4) on the MI355X")
        if mode == "hip":
            return self.core_ray_run_hip(group=group)
        return self.core_ray_run_hip_rk45(group=group)

    def ray_run(self, mode="hip", inte_method="rk45", root_method="numpy", debug=False,
                debug_file=None, group=None):
        """Initialise and integrate all rays (wr.py:897-911).

        ``group``: optional torch.distributed process group (one rank per GPU)
        to shard the rays across GPUs; results land on rank 0.
        """
        key = mode + "_rk45" if inte_method == "rk45" else mode
        if key not in SUPPORTED:
            self.core_ray_run(key)     # raises before any work
        self._check_direction(key)
        self.ray_initial(mode=mode, root_method=root_method)   # wr.py:900 (mode 'hip': GPU)
        if debug and debug_file is not None:
            try:
                self.load_init_from_precal_nc(debug_file)
            except Exception:
                pass
        return self.core_ray_run(key, group=group)

    def load_init_from_precal_nc(self, ncfile):
        """Seed row 0 from a previously written ray file (wr.py:398-415)."""
        d = ncio.read(ncfile)
        for name in ("rlon", "rlat", "rzwn", "rmwn", "ramp", "rug", "rvg"):
            t = np.array(d[name], dtype=self.all_dtype)
            if name in ("rlon", "rlat"):
                t = t / 180 * np.pi
            t[1:] = np.nan
            t[t == 999.] = np.nan
            setattr(self, name, t)

    # ------------------------------------------------------------ output
    def output(self, ncfile):
        """Write the trajectories (lon/lat in degrees), wr.py:916-959."""
        dims = {"zwn": self.nzwn, "source": self.nsource, "root": 3, "time": self.nt}
        full = ("time", "root", "source", "zwn")
        v = {"zwn": (("zwn",), self.zwn),
             "source_index": (("source",), np.arange(self.nsource, dtype=np.int32)),
             "time_index": (("time",), np.arange(self.nt, dtype=np.int32)),
             "rlon": (full, self.rlon * rad2deg, "degrees"),
             "rlat": (full, self.rlat * rad2deg, "degrees"),
             "rzwn": (full, self.rzwn, "rad_per_meter*Rearth"),
             "rmwn": (full, self.rmwn), "ramp": (full, self.ramp),
             "rug": (full, self.rug, "m s-1"), "rvg": (full, self.rvg, "m s-1")}
        ncio.write(ncfile, dims, v)

    def clean(self):
        self.bs.clean()
        for a in ("rlon", "rlat", "rzwn", "rmwn", "ramp", "rug", "rvg", "source_lon",
                  "source_lat", "zwn"):
            if hasattr(self, a):
                delattr(self, a)


def initial_rows(bs, source_lon, source_lat, zwn, freq, root_method="numpy"):
    """The seven initial rows ``(3, nsource, nzwn)`` of ``ray_initial_numpy`` (wr.py:344-395).

    Positions = sources; k = zwn; the three meridional roots of the t = 0
    dispersion relation (``cal_ky``); amp = 1 (NaN for a missing root); the
    t = 0 group velocity (``cal_ugvg`` mode 'numpy').  Host NumPy, bit-identical
    to the reference.
    """
    source_lon = np.asarray(source_lon, np.float64)
    source_lat = np.asarray(source_lat, np.float64)
    zwn = np.asarray(zwn, np.float64)
    freq = np.atleast_1d(np.asarray(freq, np.float64))
    shape = (3, len(source_lon), len(zwn))
    lon = np.ones(shape)
    lat = np.ones(shape)
    lon *= source_lon[None, :, None]
    lat *= source_lat[None, :, None]
    res = bs.cal_bs_mercator_point(source_lon, source_lat, mode="numpy")
    fmu, fmv, fmqx, fmqy = res[0], res[1], res[6], res[7]
    k = np.ones(shape)
    k *= zwn[None, None, :]
    m, amp, ug, vg = (np.full(shape, np.nan) for _ in range(4))
    for iz in range(len(zwn)):
        kz = zwn[iz]
        m_list, _ = cal_ky(fmu, fmv, fmqx, fmqy, freq, kz, iz=iz, mode="numpy",
                           root_method=root_method)
        m_val = m_list.T
        m[:, :, iz] = m_val
        a = np.ones(m_val.shape)
        a[np.isnan(m_val)] = np.nan
        amp[:, :, iz] = a
        ug[:, :, iz], vg[:, :, iz] = cal_ugvg(fmu, fmv, fmqx, fmqy, kz, m_val, mode="numpy")
    return lon, lat, k, m, amp, ug, vg


def _check_by(by):
    if by not in (None, "zwn", "root"):
        raise ValueError("by must be None, 'zwn' or 'root'")


def _default_chunk(nray, nt):
    """Rows per device chunk: keep the device row buffer near 2 GiB."""
    per_row = nray * 8 * 8
    return int(max(1, min(nt - 1, (2 << 30) // max(per_row, 1))))
