"""Rays through a stack of static basic states in one launch: ``EnsembleWR``.

``WR`` traces its sources through one basic state.  ``EnsembleWR`` traces the
same sources and wavenumbers through every member of a ``levels.Levels`` stack
-- forty winters, the members of an ensemble, three pressure levels, one flow
at several truncations -- as ONE ray run (``RayEngine.from_levels(levels,
members=True)``, the ``rwrt_rk45_*_stack`` entry points): every ray carries the
member it lives in, nothing is interpolated between members, and member ``m``
ends exactly as a separate ``WR.ray_run(mode='hip', inte_method='rk45')`` on it
would, bit for bit.

Ray slot of (member, root, source, zwn): ``((m*3 + root)*nsource + s)*nzwn + iz``
-- the history arrays ``rlon .. rvg`` are ``[nt, nmember, 3, nsource, nzwn]`` and
``rlon[:, m]`` is member ``m``'s ``WR`` history.

The reference's two global outcomes (the solver failure of rkf45.py:423-425 and
the all-NaN early exit of wr.py:853-855) are decided per member
(``member_outcomes``): a failed member's rays are frozen before the first
launch, and ``ray_run`` NaNs the rows from ``break_row[m]`` on for that member
only.
"""
import numpy as np

from constants import day, hour, rad2deg, undef
from wr import WR, _default_chunk

HIST = ("rlon", "rlat", "rzwn", "rmwn", "ramp", "rug", "rvg")


def member_outcomes(member, live, h_abs, nanrow, nmember, nt):
    """The reference's two global outcomes, per member: ``(failed, break_row)``,
    two lists of length ``nmember``.

    ``member, live, h_abs, nanrow``: one entry per ray (torch tensors on any
    device, or arrays) -- the ray's member, whether it was live at the start
    (``init``'s ``live``), its initial step size (``state[11]``) and the first
    stored row with a NaN longitude (``nt``: never).  ``failed[m]``: the member
    has live rays and none of them a finite ``h_abs`` (rkf45.py:423-425 ->
    wr.py:886-887).  ``break_row[m]``: the member's largest ``nanrow`` if that
    is below ``nt`` (wr.py:853-855), else None; 1 for a failed member; None
    for a member without rays."""
    import torch
    member = torch.as_tensor(member).reshape(-1).to(torch.int64).cpu()
    live = torch.as_tensor(live).reshape(-1).cpu() != 0
    h_abs = torch.as_tensor(h_abs).reshape(-1).to(torch.float64).cpu()
    nanrow = torch.as_tensor(nanrow).reshape(-1).to(torch.int64).cpu()
    failed, break_row = [], []
    for m in range(int(nmember)):
        mine = member == m
        lv = mine & live
        bad = bool(lv.any()) and not bool((lv & ~torch.isnan(h_abs)).any())
        failed.append(bad)
        if bad:
            break_row.append(1)
        elif bool(mine.any()):
            mx = int(nanrow[mine].max())
            break_row.append(mx if mx < int(nt) else None)
        else:
            break_row.append(None)
    return failed, break_row


class EnsembleResult:
    """Per-ray counters (device tensors, ray-slot order) and the per-member
    outcomes of one ``EnsembleWR`` run."""

    def __init__(self, run, failed, break_row, n_live):
        self.nacc, self.nrej, self.nanrow = run.nacc, run.nrej, run.nanrow
        self.failed, self.break_row = failed, break_row
        self.n_live = n_live
        self.bounds = run.bounds

    @property
    def ray_steps(self):
        return int(self.nacc.sum().item())


class EnsembleWR:
    """``WR`` over the members of a ``levels.Levels`` stack (fp64), one launch
    for all members.  Same source and wavenumber setters as ``WR``.

    (``release.ReleaseWR`` is this class over another leading axis: ``axis``
    names it -- the ``by=`` word, the output dimension -- and ``engine``,
    ``ray_initial`` and ``_init`` are what differs.)"""

    axis = "member"

    def __init__(self, levels, nzwn, nsource, tstep=1. * hour, ttotal=20. * day, freq=0, rtol=1e-6,
                 atol=1e-6, cut_off=0.1, MinStepFactor=1e-3, chunk_rows=None):
        self.levels = levels
        self.nmember = int(levels.nlev)
        if self.nmember < 1:
            raise ValueError("an ensemble needs at least one member")
        self.all_dtype = "float64"
        self.tstep = np.array([tstep], dtype=np.float64)
        self.ttotal = ttotal
        self.freq = np.array([freq], dtype=np.float64)
        self.nzwn, self.nsource = int(nzwn), int(nsource)
        self.zwn = np.zeros(self.nzwn)
        self.source_lon = np.zeros(self.nsource)
        self.source_lat = np.zeros(self.nsource)
        self.nt = int(self.ttotal / self.tstep[0]) + 1
        self.rtol, self.atol = rtol, atol
        self.cut_off = cut_off * self.tstep / 3600.
        self.MinStepFactor = MinStepFactor
        self.chunk_rows = chunk_rows
        self.last_run = None
        self._engine = None
        self._hist = False

    # the setters are WR's own (they touch only the attributes set above)
    set_zwn = WR.set_zwn
    set_freq = WR.set_freq
    set_source_array = WR.set_source_array
    set_source_matrix = WR.set_source_matrix

    # ------------------------------------------------------------ layout
    @property
    def slot_shape(self):
        return (self.nmember, 3, self.nsource, self.nzwn)

    @property
    def nray(self):
        return self.nmember * 3 * self.nsource * self.nzwn

    def slot(self, m, root, s, iz):
        """The ray slot of (member, root, source, zwn)."""
        return ((m * 3 + root) * self.nsource + s) * self.nzwn + iz

    def members(self):
        """Each ray slot's member, ``[nray]`` int32."""
        return self.channels(self.axis)[0]

    def channels(self, by):
        """``(chan[nray] int32, nchan)`` of ``by``: 'member', 'zwn' or 'root';
        ``(None, 1)`` for None."""
        if by is None:
            return None, 1
        axes = {self.axis: (0, self.nmember), "root": (1, 3), "zwn": (3, self.nzwn)}
        if by not in axes:
            raise ValueError(f"by must be None, 'zwn', 'root' or '{self.axis}'")
        ax, n = axes[by]
        shape = [1, 1, 1, 1]
        shape[ax] = n
        chan = np.broadcast_to(np.arange(n).reshape(shape), self.slot_shape)
        return np.ascontiguousarray(chan).reshape(-1).astype(np.int32), n

    def _allocate(self):
        if not self._hist:
            shape = (self.nt,) + self.slot_shape
            for name in HIST:
                setattr(self, name, np.full(shape, undef, dtype=np.float64))
            self._hist = True
        return tuple(getattr(self, n) for n in HIST)

    # ------------------------------------------------------------ the run
    def engine(self):
        """The member-stack ``RayEngine`` of the levels (built on first use)."""
        if self._engine is None:
            from engine import RayEngine
            self._engine = RayEngine.from_levels(self.levels, members=True)
        return self._engine

    def _initial_rows(self):
        """Row 0 along the leading axis, a host array ``[nmember, 7, 3, nsource,
        nzwn]`` (``RayEngine.initial_rows``: one ``rwrt_ray_initial`` call per member)."""
        return self.engine().initial_rows(self.source_lon, self.source_lat, self.zwn, self.freq).cpu().numpy()

    def ray_initial(self):
        """Row 0 of every member (``_initial_rows``); the later rows are reset."""
        rows = self._initial_rows()
        for v, h in enumerate(self._allocate()):
            h[1:] = undef
            h[0] = rows[:, v]

    def _init(self, eng, y0, p):
        """``(st, member)``: the initialised state of every ray slot and each
        slot's index along the leading axis (a device tensor)."""
        import torch
        st = eng.init(torch.as_tensor(y0), p, torch.as_tensor(self.members()))
        return st, st["member"]

    def _run(self, sink, out=None, chunk=None):
        """Integrate every member's rays from row 0 into ``sink``."""
        import torch
        from engine import F64, t_eval_of
        eng = self.engine()
        hist = self._allocate()
        y0 = np.array([h[0] for h in hist[:5]], dtype=np.float64).reshape(5, self.nray)
        p = eng.params(self.nt, float(self.tstep[0]), self.rtol, self.atol, self.MinStepFactor,
                       cut_rad=float(self.cut_off[0]))
        tb = torch.as_tensor(t_eval_of(self.nt, float(self.tstep[0]), self.ttotal), dtype=F64, device=eng.device)
        st, member = self._init(eng, y0, p)
        live = st["live"] != 0
        failed, _ = member_outcomes(member, live, st["state"][11], st["nanrow"], self.nmember, self.nt)
        if any(failed):
            # a failed member never steps (wr.py:886-887 breaks before row 1):
            # its rays are frozen here, so its counters stay 0
            gone = torch.as_tensor(failed, device=eng.device)[member.to(torch.int64)]
            st["state"][:5, gone] = float("nan")
            live = live & ~gone
        n_live = int(live.sum().item())
        chunk = chunk or self.chunk_rows or _default_chunk(self.nray, self.nt)
        run = eng.advance(st, p, tb, 1, chunk=chunk, sink=sink, out=out, n_live=n_live, n_live_local=n_live)
        _, break_row = member_outcomes(member, st["live"], torch.zeros_like(st["state"][11]), st["nanrow"],
                                       self.nmember, self.nt)
        break_row = [1 if f else b for f, b in zip(failed, break_row)]
        self.last_run = EnsembleResult(run, failed, break_row, n_live)
        return self.last_run

    def ray_run(self):
        """Initialise and integrate every member's rays; the history arrays
        ``rlon .. rvg`` ``[nt, nmember, 3, nsource, nzwn]`` are filled as
        ``WR.ray_run`` fills them for each member.  Returns the
        ``EnsembleResult`` (``failed`` and ``break_row`` per member)."""
        from hostio import HistorySink
        self.ray_initial()
        hist = self._allocate()
        chunk = self.chunk_rows or _default_chunk(self.nray, self.nt)
        hs = HistorySink(hist, self.slot_shape, self.nray, min(chunk, self.nt - 1), self.engine().device)
        try:
            res = self._run(hs, out=hs.buffers(), chunk=chunk)
        finally:
            hs.finish()
        for m, b in enumerate(res.break_row):
            if b is not None:
                for h in hist:
                    h[b:, m] = np.nan     # rows never stored (wr.py:853-855, 886-887)
        return res

    # ---- products reduced on the device (raymap.py)
    def _column(self, col):
        """Row 0 of the history array of row column ``col`` (2..6); None for -1."""
        return None if col < 0 else getattr(self, HIST[col])[0]

    def reduce(self, make, by="member"):
        """Initialise the rays and integrate them into the sink of
        ``make(device, chan, nray) -> (product, sink)`` (any raymap product;
        ``chan``: each ray slot's channel under ``by``, an int32 array or
        None).  ``make`` also hands row 0 (``self.rlon[0]`` ..) to the
        product.  Returns the product; only row 0 of the history is filled.
        One wave-field map per member (phase.py)::

            def make(device, chan, nray):
                m = PhaseMap(with_channels(spec, ew.nmember), nray, device, chan)
                m.start(ew.rlon[0], ew.rlat[0], ew.ramp[0], ew.ramp[0], k=ew.rzwn[0], l=ew.rmwn[0])
                return m, PhaseSink(m)

        A ray-tube map (tube.py) also needs the neighbours of the stack's
        ray slots: ``lattice_neighbours(nnx, nny, nzwn, nlead=3 * nmember)``
        (the example in tube.py's docstring).
        """
        chan, _ = self.channels(by)
        self.ray_initial()
        product, sink = make(self.engine().device, chan, self.nray)
        self._run(sink)
        return product

    def ray_density(self, spec, by=None, include_initial=True):
        """As ``WR.ray_density`` over every member: ``by='member'`` gives one
        map per member (also 'zwn', 'root', None)."""
        import density as D
        import raymap
        _, nchan = self.channels(by)
        spec = spec if by is None else raymap.with_channels(spec, nchan)

        def make(device, chan, nray):
            dmap = D.DensityMap(spec, device)
            if include_initial:
                dmap.add_points(self.rlon[0], self.rlat[0], self._column(spec.wcol), chan)
            return dmap, D.DensitySink(dmap, chan)

        return self.reduce(make, by)

    def ray_summary(self, regions=None):
        """As ``WR.ray_summary`` over every member: the ``summary.RaySummary``
        whose ``numpy()`` fields are ``(nmember, 3, nsource, nzwn)``."""
        import summary as Sm

        def make(device, chan, nray):
            rs = Sm.RaySummary(nray, regions or (), device)
            rs.shape = self.slot_shape
            rs.start(self.rlon[0], self.rlat[0], self.rmwn[0], self.ramp[0])
            return rs, Sm.SummarySink(rs)

        return self.reduce(make, None)

    # ------------------------------------------------------------ output
    def output(self, ncfile):
        """``WR.output``'s variables with a ``member`` dimension."""
        import ncio
        self._allocate()
        ax = self.axis
        dims = {"zwn": self.nzwn, "source": self.nsource, "root": 3, ax: self.nmember, "time": self.nt}
        full = ("time", ax, "root", "source", "zwn")
        v = {"zwn": (("zwn",), self.zwn),
             "source_index": (("source",), np.arange(self.nsource, dtype=np.int32)),
             ax + "_index": ((ax,), np.arange(self.nmember, dtype=np.int32)),
             "time_index": (("time",), np.arange(self.nt, dtype=np.int32)),
             "rlon": (full, self.rlon * rad2deg, "degrees"),
             "rlat": (full, self.rlat * rad2deg, "degrees"),
             "rzwn": (full, self.rzwn, "rad_per_meter*Rearth"),
             "rmwn": (full, self.rmwn), "ramp": (full, self.ramp),
             "rug": (full, self.rug, "m s-1"), "rvg": (full, self.rvg, "m s-1")}
        v.update(self._output_extra())
        ncio.write(ncfile, dims, v)

    def _output_extra(self):
        """Further variables of ``output`` (none here)."""
        return {}
