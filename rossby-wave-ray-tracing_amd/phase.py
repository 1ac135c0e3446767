"""The WKB phase along rays and wave-field maps, reduced on the GPU
(``rwrt_ray_phase``, ABI 5).

A WKB wave is ``A exp(i theta)``.  The ray loops integrate the amplitude ``A``
(the ``amp`` column) and the local wavenumbers ``k, l``; the other maps
(density.py .. cross.py) are statistics of where rays go and how strong they
are.  Here the phase ``theta = int k dlon + l dY`` (``dY = dlat / cos(lat)``,
``k, l`` the Mercator wavenumbers times the earth's radius, as the rows carry
them) is integrated along every ray by the trapezoidal rule per segment, and
every ray point deposits its wave ``w exp(i psi)``, ``psi = theta - omega_dt *
row``, into its box of a lon-lat map: ``re`` is the superposed wave field --
crests and troughs, the Hoskins-Karoly wave train -- and ``hypot(re, im) /
wabs`` tells where the rays that reach a box reinforce each other (1) and where
they cancel (0).

``reference_phase`` (NumPy) is the definition.  The kernel (csrc/phase_rows.h)
restates it operation for operation -- no fused multiply-add -- so that
``cnt``, ``nseg`` and ``dropped`` equal it exactly, ``theta`` differs only
through the device library's ``cos`` (a per-ray sequential sum, like
``summary``'s ``path``), and ``re``, ``im``, ``wabs`` agree to that and to the
rounding of a sum taken in any order.  ``PhaseSink`` plugs into
``RayEngine.integrate`` / ``integrate_rk4`` / ``resume`` /
``shard.run_sharded`` through the ``sink`` protocol, alone or as a member of
``summary.Tee``; ``WR.ray_phase`` is the user entry point, and
``EnsembleWR.reduce`` takes a ``PhaseMap`` like any other raymap product.
"""
import math
from dataclasses import dataclass

import numpy as np

import _hip as H
from density import bin_index
from launch_rows import one_row, row_args
from raymap import CarriedMap, ColumnSink, GridSpec, allreduce_tensors, check_columns, counts_for, valid_rows

TWO_PI = 2.0 * math.pi
HALF_PI = 1.5707963267948966     # the double nearest pi / 2


@dataclass(frozen=True)
class PhaseSpec(GridSpec):
    """``nx`` boxes over longitude [0, 360), ``ny`` over ``lat_range``
    (degrees, upper edge excluded), ``nchan`` maps.  ``need``: a row column by
    name (``density.WEIGHT_COLUMNS``) that must be finite for a row to be
    valid, or None; the default ``'amp'`` keeps dead root slots out.
    ``weight``: the row column that weighs a deposit (default the WKB
    amplitude ``'amp'``), or None: every deposit weighs 1 and there is no
    ``wabs``.  ``omega_dt``: the wave's frequency times the row interval, in
    radians per row (0: a stationary wave; ``WR.ray_phase`` fills it in from
    ``freq * tstep``)."""
    nx: int
    ny: int
    nchan: int = 1
    lat_range: tuple = (-90.0, 90.0)
    need: str = "amp"
    weight: str = "amp"
    omega_dt: float = 0.0

    def __post_init__(self):
        self._check_shape()
        self._check_ranges()
        check_columns(self, "need", "weight")
        if not math.isfinite(float(self.omega_dt)):
            raise ValueError("omega_dt must be finite")

    def c_struct(self):
        return H.PhaseMapC(self.nx, self.ny, self.nchan, self.ncol, self.wcol, 0, self.lat0, self.inv_dlat,
                           self.inv_dlon, float(self.omega_dt))


def phase_valid(rows, spec):
    """``[nray, nt]`` bool: lon, lat, k and l finite, ``|lat| < pi/2`` (the
    double nearest pi/2) and, with ``need`` / ``weight``, those columns finite."""
    with np.errstate(all="ignore"):
        return (valid_rows(rows, spec) & np.isfinite(rows[..., 2]) & np.isfinite(rows[..., 3])
                & (np.abs(rows[..., 1]) < HALF_PI))


def phase_along(rows, chan, spec, theta0=None):
    """The phase of ``reference_phase`` at every row: ``(theta[nray, nt],
    nseg[nray] int32, S[nray], ok[nray, nt])`` with ``ok`` the rows that
    deposit (valid, the ray's channel in range)."""
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 3 or rows.shape[1] < 1 or rows.shape[2] < 7:
        raise ValueError(f"rows must be [nray, nt >= 1, >= 7], got {rows.shape}")
    nray, nt = rows.shape[:2]
    chan = np.zeros(nray, np.int64) if chan is None else np.asarray(chan, np.int64).reshape(-1)
    if chan.size != nray:
        raise ValueError(f"chan has {chan.size} entries for {nray} rays")
    theta0 = np.zeros(nray) if theta0 is None else np.asarray(theta0, np.float64).reshape(-1)
    if theta0.size != nray:
        raise ValueError(f"theta0 has {theta0.size} entries for {nray} rays")
    ok = phase_valid(rows, spec) & ((chan >= 0) & (chan < spec.nchan))[:, None]
    lon, lat, k = rows[..., 0], rows[..., 1], rows[..., 2]
    with np.errstate(all="ignore"):
        a = np.where(ok, rows[..., 3], 0.0) / np.cos(np.where(ok, lat, 0.0))
        seg = ok[:, 1:] & ok[:, :-1]
        dk = (0.5 * (k[:, :-1] + k[:, 1:])) * (lon[:, 1:] - lon[:, :-1])
        dl = (0.5 * (a[:, :-1] + a[:, 1:])) * (lat[:, 1:] - lat[:, :-1])
        d = dk + dl
        theta = np.empty((nray, nt))
        theta[:, 0] = theta0
        for i in range(1, nt):       # (a sequential sum per ray, in row order)
            theta[:, i] = np.where(seg[:, i - 1], theta[:, i - 1] + d[:, i - 1], theta[:, i - 1])
        S = np.where(seg, np.abs(dk) + np.abs(dl), 0.0).sum(axis=1)
    return theta, seg.sum(axis=1).astype(np.int32), S, ok


def reference_phase(rows, chan, spec, theta0=None):
    """The definition of the phase along rays and of a wave-field map, in
    NumPy: a dict with ``cnt`` (``[nchan, ny, nx]`` int64), ``re``, ``im``,
    ``wabs`` (float64; ``wabs`` None without ``weight``), ``theta`` (``[nray]``
    float64, the phase after the last row), ``nseg`` (int32, the segments
    joined), ``dropped`` (int) and ``S`` (``[nray]``: the sum of ``|dk| +
    |dl|`` over a ray's segments, the magnitude the error bars refer to --
    theta itself cancels).

    ``rows[nray, nt, 8]``: a logical history (columns lon lat k l amp ug vg
    nacc, lon unwrapped, radians; row 0 the initial row); ``chan`` one channel
    per ray (None: channel 0); ``theta0`` the phase at row 0 per ray (None: 0).

    A row is valid iff lon, lat, k and l are finite, ``|lat| < pi/2`` (the
    double nearest pi/2, compared in fp64) and the ``need`` and ``weight``
    columns, when set, are finite; then ``a = l / cos(lat)``.  Segment ``i``
    joins rows ``i - 1`` and ``i``; it is joined iff both are valid and the
    ray's channel c is in ``[0, nchan)``.  Then, one rounding per operation::

        dk = (0.5 * (k0 + k1)) * (lon1 - lon0)
        dl = (0.5 * (a0 + a1)) * (lat1 - lat0)
        theta_i = theta_{i-1} + (dk + dl);   nseg += 1

    else ``theta_i = theta_{i-1}``: the trapezoidal rule of ``int k dlon + l
    dY``, ``dY = dlat / cos(lat)``.  Every valid row ``i``, row 0 included, of
    a ray whose channel is in range has ``psi = theta_i - omega_dt * i`` and is
    binned exactly as ``density.reference_bins`` bins it (``lam = (lon % 2 pi)
    % 2 pi``, ``ix = min(floor(lam * inv_dlon), nx - 1)``, ``iy = floor((lat -
    lat0) * inv_dlat)`` in ``[0, ny)``).  A binned row with a finite ``psi``
    adds ``cnt += 1``, ``re += w cos(psi)``, ``im += w sin(psi)``, ``wabs +=
    |w|`` (``w`` the weight column, 1 without one); a binned row whose ``psi``
    is not finite adds 1 to ``dropped`` and nothing else.

    The rows of a constant tail after its first row are rows like any other
    here: each joins a row to itself (``dk + dl`` is +0, ``nseg`` counts it)
    and deposits again.  The kernel makes those ``n - 1`` equal deposits as one
    product ``(n - 1) * term`` per sum when ``omega_dt == 0`` -- one rounding
    instead of ``n - 2``, inside the bound of a sum taken in any order -- and
    row by row otherwise.  Doubles as the ``mode='numpy'`` product of small
    runs."""
    rows = np.asarray(rows, np.float64)
    theta, nseg, S, ok = phase_along(rows, chan, spec, theta0)
    nray, nt = rows.shape[:2]
    w = rows[..., spec.wcol] if spec.wcol >= 0 else np.ones((nray, nt))
    with np.errstate(all="ignore"):
        psi = theta - float(spec.omega_dt) * np.arange(nt, dtype=np.float64)[None, :]
        idx = bin_index(rows[..., 0], rows[..., 1], w, None if chan is None else np.asarray(chan)[:, None], spec)
        binned = ok & (idx >= 0)
        fin = np.isfinite(psi)
        put = binned & fin
        n = spec.nchan * spec.ny * spec.nx
        at = idx[put]
        cnt = np.bincount(at, minlength=n).astype(np.int64).reshape(spec.shape)
        sums = []
        for term in (w[put] * np.cos(psi[put]), w[put] * np.sin(psi[put]), np.abs(w[put])):
            s = np.zeros(n)
            np.add.at(s, at, term)
            sums.append(s.reshape(spec.shape))
    return {"cnt": cnt, "re": sums[0], "im": sums[1], "wabs": sums[2] if spec.wcol >= 0 else None,
            "theta": theta[:, -1].copy(), "nseg": nseg, "dropped": int((binned & ~fin).sum()), "S": S}


class PhaseMap(CarriedMap):
    """The device arrays of one wave-field map over ``nray`` rays: ``cnt``
    (int64), ``re``, ``im`` and ``wabs`` (fp64; ``wabs`` None without a
    weight), each ``[nchan, ny, nx]``, ``dropped`` (int64 ``[1]``), and per
    ray ``theta`` (fp64, started at ``theta0``, default 0) and ``nseg``
    (int32), initialised here and accumulated into by every ``add_rows`` call
    (time chunks, shards).  The carried row ``prev`` is four columns wide
    here (``[4, nray]``: lon, lat, k, ``a = l / cos(lat)``; NaN: none);
    ``restart`` and ``chan`` are ``raymap.CarriedMap``'s; a ray with a channel
    outside ``[0, nchan)`` contributes nothing and keeps its ``theta``."""
    REDUCE = (("cnt", "SUM"), ("re", "SUM"), ("im", "SUM"), ("wabs", "SUM"), ("dropped", "SUM"), ("nseg", "SUM"))

    def __init__(self, spec, nray, device=None, chan=None, theta0=None):
        import torch
        super().__init__(spec, nray, device, chan)
        f64 = dict(dtype=torch.float64, device=self.device)
        self.prev = torch.full((4, self.nray), math.nan, **f64)
        self.cnt = torch.zeros(spec.shape, dtype=torch.int64, device=self.device)
        self.re = torch.zeros(spec.shape, **f64)
        self.im = torch.zeros(spec.shape, **f64)
        self.wabs = torch.zeros(spec.shape, **f64) if spec.wcol >= 0 else None
        self.dropped = torch.zeros(1, dtype=torch.int64, device=self.device)
        if theta0 is None:
            self.theta0 = torch.zeros(self.nray, **f64)
        else:
            self.theta0 = torch.as_tensor(theta0, dtype=torch.float64).reshape(-1).to(self.device).contiguous()
            if self.theta0.numel() != self.nray:
                raise ValueError(f"theta0 has {self.theta0.numel()} entries for {self.nray} rays")
        self.theta = self.theta0.clone()
        self.nseg = torch.zeros(self.nray, dtype=torch.int32, device=self.device)

    def start(self, lon, lat, need=None, v=None, ray=None, k=None, l=None):   # noqa: E741
        """Row 0, the initial rays (radians), which sinks never receive: the
        same entry point on a ``[n, 1, 8]`` row tensor.  It sets the carried
        rows, deposits row 0 and leaves ``theta`` at ``theta0``.  ``k, l``: the
        wavenumber columns (required); ``need`` / ``v``: the values of the
        ``need`` and ``weight`` columns where they are neither (required
        then)."""
        if k is None or l is None:
            raise ValueError("the phase needs the wavenumbers of row 0: pass k and l")
        cols = {0: lon, 1: lat, 2: k, 3: l}
        for name, col, val in (("need", self.spec.ncol, need), ("weight", self.spec.wcol, v)):
            if col >= 4:
                if val is None:
                    raise ValueError(f"the map's {name} column is {getattr(self.spec, name)!r}: pass its values")
                cols[col] = val
        self.add_rows(0, 1, one_row(cols, self.device), ray=ray)
        return self

    def add_rows(self, i0, i1, view, tails=None, slots=None, ray=None):
        """Integrate the phase over the segments that end on rows ``[i0, i1)``
        of a launch and deposit those rows: ``view`` its row buffer (dense
        ``[n, i1-i0, 8]``, or the row blocks of ``slots``), ``tails`` /
        ``slots`` the launch's ``engine.Tails`` / ``engine.Slots``, ``ray``
        each ray's column (int64; None: ray j is column j).  One asynchronous
        ``rwrt_ray_phase`` call on the device's current stream."""
        import torch
        n, rows = row_args(i0, i1, view, tails, slots)
        ray = self._ray(ray, n)
        H.check(self._lib.rwrt_ray_phase(
            self._c, n, int(i0), int(i1), *rows, H.dptr(ray, torch.int64), self.nray, H.dptr(self.chan, torch.int32),
            H.dptr(self.prev, torch.float64), H.dptr(self.theta, torch.float64), H.dptr(self.nseg, torch.int32),
            H.dptr(self.cnt, torch.int64), H.dptr(self.re, torch.float64), H.dptr(self.im, torch.float64),
            H.dptr(self.wabs), H.dptr(self.dropped, torch.int64), H.stream(self.device)))

    def clear_maps(self):
        """Zero the maps and ``dropped`` (the per-ray arrays and the carried
        rows stay): a rank that does not own row 0 calls it after ``start``."""
        for t in (self.cnt, self.re, self.im, self.wabs, self.dropped):
            if t is not None:
                t.zero_()
        return self

    def allreduce(self, group=None):
        """SUM of the maps, of ``dropped`` and of ``nseg`` over the ranks of
        ``group``, left on every rank; ``theta`` of a ray is the value of the
        rank that integrated it (the one with segments of it, or a ``theta``
        that left ``theta0``: a SUM in which every other rank adds 0), and
        ``theta0`` for a ray no rank integrated.  The carried rows are not
        reduced."""
        import torch
        mine = (self.nseg > 0) | (self.theta != self.theta0)       # (before nseg is summed)
        own = torch.where(mine, self.theta, torch.zeros_like(self.theta))
        owners = mine.to(torch.int32)
        super().allreduce(group)
        allreduce_tensors([(own, "SUM"), (owners, "SUM")], group)
        self.theta.copy_(torch.where(owners > 0, own.to(self.device), self.theta0))
        return self

    def numpy(self):
        """``{'cnt', 're', 'im', 'wabs', 'theta', 'nseg', 'dropped'}`` on the
        host, as ``reference_phase`` returns them (waits for the pending
        calls)."""
        return {"cnt": self.cnt.cpu().numpy(), "re": self.re.cpu().numpy(), "im": self.im.cpu().numpy(),
                "wabs": None if self.wabs is None else self.wabs.cpu().numpy(),
                "theta": self.theta.cpu().numpy(), "nseg": self.nseg.cpu().numpy(),
                "dropped": int(self.dropped.cpu().numpy()[0])}

    # ---- derived fields: device tensors, NaN where cnt == 0
    def _where_hit(self, x):
        import torch
        return torch.where(self.cnt == 0, torch.full_like(x, math.nan), x)

    def field(self):
        """The superposed wave at phase 0: ``re``."""
        return self._where_hit(self.re)

    def amplitude(self):
        """``hypot(re, im)``: the amplitude of the superposed wave."""
        import torch
        return self._where_hit(torch.hypot(self.re, self.im))

    def mean_phase(self):
        """``atan2(im, re)``: the phase of the superposed wave, in (-pi, pi]."""
        import torch
        return self._where_hit(torch.atan2(self.im, self.re))

    def coherence(self):
        """``amplitude / wabs`` (``/ cnt`` without a weight): 1 where the rays
        that reach a box agree in phase, 0 where they cancel."""
        import torch
        total = self.wabs if self.wabs is not None else self.cnt.to(torch.float64)
        return self._where_hit(torch.hypot(self.re, self.im) / total)

    def cycles(self):
        """``theta / 2 pi`` per ray: the wavelengths it has run through."""
        return self.theta / TWO_PI

    def output(self, ncfile):
        """Write the maps (dims ``chan, lat, lon``; bin centres and edges in
        degrees) and the per-ray arrays (``ray``).  netCDF-3 has no 64-bit
        integers: ``cnt`` goes out as float64 there (exact below 2^53), as
        int64 into an ``.npz``."""
        import ncio
        a = self.numpy()
        dims, v = self._grid_output()
        dims.update({"ray": self.nray, "one": 1})
        full = ("chan", "lat", "lon")
        v.update({"cnt": (full, counts_for(ncfile, a["cnt"]), "ray points"),
                  "re": (full, a["re"], "sum of w cos(psi)"), "im": (full, a["im"], "sum of w sin(psi)"),
                  "theta": (("ray",), a["theta"], "radians"), "nseg": (("ray",), a["nseg"], "segments"),
                  "dropped": (("one",), np.array([float(a["dropped"])]), "ray points")})
        if a["wabs"] is not None:
            v["wabs"] = (full, a["wabs"], f"sum of |{self.spec.weight}|")
        ncio.write(ncfile, dims, v)


class PhaseSink(ColumnSink):
    """A ``sink`` of ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume``
    and of ``shard.run_sharded`` (``launch_rows.RowSink``) that integrates the
    phase over each launch's rows and deposits them into ``map``.  ``ray``:
    the column of each ray of the integration (None: ray j is column j); the
    sharded form's ``idx`` and ``take(idx)`` select from it, or are the
    columns themselves.  Channels are the map's (``PhaseMap.chan``), indexed
    by column."""
