"""Caustic-aware wave-field maps, reduced on the GPU (``rwrt_ray_wave``, ABI 5).

The WKB wave a ray carries is ``A |D|^(-1/2) exp(i (theta - mu pi / 2))``.
``phase.py`` integrates ``theta`` and deposits ``w exp(i psi)`` without knowing
of caustics; ``tube.py`` finds the geometric spreading ``D``, the caustics and
the Maslov index ``mu``, and says that behind a caustic the phase has dropped by
pi / 2 and the phase map is not to be trusted.  Running both side by side does
not mend it: the phase map deposits before ``mu`` is known, and the tube map
keeps the last ``mu`` of a ray only.  Here one lane walks both along a ray, so
every ray point deposits with the ``mu`` and the ``D`` it has there::

    psi = (theta - omega_dt * row) - mu * pi / 2
    w   = weight / sqrt(|D|)                      (spread=False: the weight alone)
    re += w cos(psi);  im += w sin(psi);  wabs += |w|;  cnt += 1

``reference_wave`` (NumPy) is the definition, and it is a composition: the
per-row tube quantities are ``tube.tube_along``'s, the ones ``reference_tube``
deposits from, and the per-row phase is ``phase.phase_along``'s.  The kernel
(csrc/wave_rows.h) composes csrc/tube_rows.h and csrc/phase_rows.h in the same
way, so ``theta`` and ``nseg`` equal ``PhaseMap``'s and ``mu``, ``first``,
``nrow``, ``close_row`` and ``dlast`` equal ``TubeMap``'s bit for bit on the
same rows; ``cnt``, ``dropped`` and ``clipped`` rest on ``jac`` alone and equal
the definition exactly.

At the caustic itself ``D -> 0`` and the WKB amplitude is singular (the uniform
Airy form is left out): a deposit with ``jac == 0`` is dropped, and ``d_floor``
clips those with ``|jac| < d_floor |jac_0|`` -- counted in ``clipped``, so that
a few near-singular points do not own a box.

A ray's neighbours must be in the same launch, so ``WaveSink`` takes whole
launches only: a shard (``take``) and a process group are refused.
``WR.ray_wave`` is the user entry point.  A member stack or a release stack
(``EnsembleWR`` / ``ReleaseWR``, rays ``[member, root, source, zwn]``) goes
through ``reduce`` with the neighbours of ``3 * nmember`` leading slots::

    nbr = lattice_neighbours(nnx, nny, ew.nzwn, nlead=3 * ew.nmember)

    def make(device, chan, nray):
        m = WaveMap(with_channels(spec, ew.nmember), nray, nbr, device, chan)
        m.start(ew.rlon[0], ew.rlat[0], ew.ramp[0], ew.ramp[0], k=ew.rzwn[0], l=ew.rmwn[0])
        return m, WaveSink(m)

    m = ew.reduce(make, by="member")                        # ReleaseWR: by="release"
"""
import math
from dataclasses import dataclass

import numpy as np

import _hip as H
from launch_rows import RowSink, one_row, row_args
from phase import PhaseSpec, phase_along
from raymap import CarriedMap, GridSpec, check_columns, counts_for
from tube import TubeSpec, check_neighbours, tube_along

TWO_PI = 2.0 * math.pi
HALF_PI = 1.5707963267948966     # the double nearest pi / 2
NSTATE_I, NSTATE_F = 6, 9        # kWaveNI, kWaveNF: the rows of ``state`` and of ``prev``


@dataclass(frozen=True)
class WaveSpec(GridSpec):
    """``nx`` boxes over longitude [0, 360), ``ny`` over ``lat_range``
    (degrees, upper edge excluded), ``nchan`` maps.  ``need``, ``max_sep``:
    ``tube.TubeSpec``'s; ``need``, ``weight``, ``omega_dt``:
    ``phase.PhaseSpec``'s (``weight`` None: every deposit weighs 1 before the
    spreading; ``WR.ray_wave`` fills ``omega_dt`` in from ``freq * tstep``).
    ``spread``: divide the weight by ``sqrt(|D|)``; False leaves the Maslov
    phase as the only change to a phase map.  ``d_floor`` (finite, >= 0): a
    deposit with ``|jac| < d_floor |jac_0|`` is counted in ``clipped`` and not
    made."""
    nx: int
    ny: int
    nchan: int = 1
    lat_range: tuple = (-90.0, 90.0)
    need: str = "amp"
    weight: str = None
    spread: bool = True
    max_sep: float = 0.5
    omega_dt: float = 0.0
    d_floor: float = 0.0

    def __post_init__(self):
        self._check_shape()
        self._check_ranges()
        check_columns(self, "need", "weight")
        if not float(self.max_sep) > 0.0:
            raise ValueError("max_sep must be positive (inf: never close a tube)")
        if not math.isfinite(float(self.omega_dt)):
            raise ValueError("omega_dt must be finite")
        if not (math.isfinite(float(self.d_floor)) and float(self.d_floor) >= 0.0):
            raise ValueError("d_floor must be finite and not negative")
        if not isinstance(self.spread, (bool, np.bool_)):
            raise ValueError("spread must be True or False")

    def tube_spec(self):
        """The ``tube.TubeSpec`` whose per-row quantities the deposits use."""
        return TubeSpec(self.nx, self.ny, need=self.need, max_sep=self.max_sep, lat_range=self.lat_range,
                        nchan=self.nchan)

    def phase_spec(self):
        """The ``phase.PhaseSpec`` whose ``theta`` and valid rows the deposits use."""
        return PhaseSpec(self.nx, self.ny, nchan=self.nchan, lat_range=self.lat_range, need=self.need,
                         weight=self.weight, omega_dt=self.omega_dt)

    def c_struct(self):
        return H.WaveMapC(self.nx, self.ny, self.nchan, self.ncol, self.wcol, int(bool(self.spread)), self.lat0,
                          self.inv_dlat, self.inv_dlon, float(self.max_sep), float(self.omega_dt),
                          float(self.d_floor))


def reference_wave(rows, nbr, chan, spec, theta0=None):
    """The definition of the caustic-aware wave-field map, in NumPy: a dict
    with the maps ``cnt`` (``[nchan, ny, nx]`` int64), ``re``, ``im``, ``wabs``
    (float64), ``dropped`` and ``clipped`` (int), per ray ``theta``, ``nseg``
    and ``S`` as ``phase.reference_phase`` gives them and ``mu``, ``first``,
    ``nrow``, ``close_row``, ``dlast`` and ``code`` as ``tube.reference_tube``
    gives them.

    ``rows[nray, nt, 8]``: a logical history (columns lon lat k l amp ug vg
    nacc, radians, row 0 the initial row); ``nbr[4, nray]``: the W, E, S, N
    neighbour of every ray, -1 for none; ``chan``: one channel per ray (None:
    channel 0); ``theta0``: the phase at row 0 per ray (None: 0).

    A composition.  Per row i of ray j, ``open_i``, ``jac_i``, ``D_i`` and the
    running ``mu_i`` (a caustic at row i counted) are ``tube.tube_along``'s for
    ``spec.tube_spec()``: the quantities ``reference_tube`` deposits from, with
    the stencil fixed at row 0, ``need``, ``max_sep``, a tube that closes for
    good and ``jac_0 == 0`` meaning no tube.  ``theta_i``, ``nseg``, ``S`` and
    the mask ``ok`` of the rows that may deposit are ``phase.phase_along``'s for
    ``spec.phase_spec()``; ``theta`` runs over every phase-valid row whether
    the tube is open or not.

    Row i of ray j deposits iff ``ok[j, i]``, ``open_i`` and its point lies in
    the map, binned by position alone (no weight enters the bin).  Then, in
    this order, one rounding per operation::

        jac_i == 0                     dropped += 1, nothing else
        |jac_i| < d_floor * |jac_0|    clipped += 1, nothing else
        w = wv                         (the weight column at the row, 1.0 without one)
        w = wv / sqrt(|D_i|)           (with spread)
        psi = (theta_i - omega_dt * i) - mu_i * HALF_PI
        psi or w not finite            dropped += 1, nothing else
        cnt += 1;  re += w cos(psi);  im += w sin(psi);  wabs += |w|

    The rows of a constant tail are rows like any other here.  The kernel
    makes the ``n - 1`` equal deposits behind the first row at which the ray
    and its whole stencil rest as one product ``(n - 1) * term`` per sum when
    ``omega_dt == 0`` -- inside the bound of a sum taken in any order -- and
    row by row otherwise.  Doubles as the ``mode='numpy'`` product of small
    runs."""
    rows = np.asarray(rows, np.float64)
    theta, nseg, S, ok = phase_along(rows, chan, spec.phase_spec(), theta0)
    nray, nt = rows.shape[:2]
    wv = rows[..., spec.wcol] if spec.wcol >= 0 else np.ones((nray, nt))
    nmap = spec.nchan * spec.ny * spec.nx
    cnt = np.zeros(nmap, np.int64)
    re, im, wabs = np.zeros(nmap), np.zeros(nmap), np.zeros(nmap)
    dropped = clipped = 0
    ray = {}
    omega_dt, d_floor = float(spec.omega_dt), float(spec.d_floor)
    with np.errstate(all="ignore"):
        for r in tube_along(rows, nbr, chan, spec.tube_spec(), ray):
            i = r.i
            put = ok[:, i] & r.open & (r.idx >= 0)
            zero = put & (r.jac == 0.0)
            dropped += int(zero.sum())
            put &= ~zero
            clip = put & (np.abs(r.jac) < d_floor * np.abs(r.jac0))
            clipped += int(clip.sum())
            put &= ~clip
            w = wv[:, i]
            if spec.spread:
                w = w / np.sqrt(np.abs(r.D))
            psi = (theta[:, i] - omega_dt * float(i)) - r.mu.astype(np.float64) * HALF_PI
            bad = put & ~(np.isfinite(psi) & np.isfinite(w))
            dropped += int(bad.sum())
            put &= ~bad
            at = r.idx[put]
            np.add.at(cnt, at, 1)
            np.add.at(re, at, w[put] * np.cos(psi[put]))
            np.add.at(im, at, w[put] * np.sin(psi[put]))
            np.add.at(wabs, at, np.abs(w[put]))
    sh = spec.shape
    return {"cnt": cnt.reshape(sh), "re": re.reshape(sh), "im": im.reshape(sh), "wabs": wabs.reshape(sh),
            "dropped": dropped, "clipped": clipped, "theta": theta[:, -1].copy(), "nseg": nseg, "S": S,
            "mu": ray["mu"], "first": ray["first"], "nrow": ray["nrow"], "close_row": ray["close_row"],
            "dlast": ray["dlast"], "code": ray["code"]}


class WaveMap(CarriedMap):
    """The device arrays of one caustic-aware wave-field map over ``nray``
    rays with the neighbours ``nbr`` (``[4, nray]``: W, E, S, N; -1: none):
    the maps ``cnt`` (int64), ``re``, ``im`` and ``wabs`` (fp64), each
    ``[nchan, ny, nx]``, ``dropped`` and ``clipped`` (int64 ``[1]``), and the
    per-ray state, which is also what is carried from a launch to the next:
    ``state`` (int32 ``[6, nray]``: the stencil choice and the open flag,
    ``mu``, ``first``, ``nrow``, ``close_row``, ``nseg``) and ``prev`` (fp64
    ``[9, nray]``: the carried row lon, lat, k, ``a = l / cos(lat)``;
    ``theta``, started at ``theta0``, default 0; ``jac_prev``, ``jac_0``,
    ``cos_0``, ``dlast``).  A running state: a ray's rows must arrive once, in
    order, with its neighbours' rows in the same launch; ``start`` (row 0 of
    all rays) fixes the stencils."""

    def __init__(self, spec, nray, nbr, device=None, chan=None, theta0=None):
        import torch
        super().__init__(spec, nray, device, chan)
        self._call = H.entry("rwrt_ray_wave")
        f64 = dict(dtype=torch.float64, device=self.device)
        self.nbr = torch.as_tensor(check_neighbours(nbr, self.nray)).to(self.device).contiguous()
        self.cnt = torch.zeros(spec.shape, dtype=torch.int64, device=self.device)
        self.re = torch.zeros(spec.shape, **f64)
        self.im = torch.zeros(spec.shape, **f64)
        self.wabs = torch.zeros(spec.shape, **f64)
        self.dropped = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.clipped = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        if theta0 is None:
            self.theta0 = torch.zeros(self.nray, **f64)
        else:
            self.theta0 = torch.as_tensor(theta0, dtype=torch.float64).reshape(-1).to(self.device).contiguous()
            if self.theta0.numel() != self.nray:
                raise ValueError(f"theta0 has {self.theta0.numel()} entries for {self.nray} rays")
        self.state = torch.zeros((NSTATE_I, self.nray), dtype=torch.int32, device=self.device)
        self.prev = torch.full((NSTATE_F, self.nray), math.nan, **f64)
        self.restart()

    def restart(self):
        """Close every tube, forget the carried rows and the per-ray results
        and put ``theta`` back to ``theta0`` (the maps stay); the next row 0
        starts them again."""
        self.state.zero_()
        self.state[2].fill_(-1)
        self.state[4].fill_(-1)
        self.prev.fill_(math.nan)
        self.prev[4].copy_(self.theta0)
        return self

    mu = property(lambda self: self.state[1])
    first = property(lambda self: self.state[2])
    nrow = property(lambda self: self.state[3])
    close_row = property(lambda self: self.state[4])
    nseg = property(lambda self: self.state[5])
    theta = property(lambda self: self.prev[4])
    dlast = property(lambda self: self.prev[8])

    def start(self, lon, lat, need=None, v=None, k=None, l=None):   # noqa: E741
        """Row 0, the initial rays (radians), which sinks never receive: the
        same entry point on a ``[nray, 1, 8]`` row tensor.  It fixes the
        stencils, sets the carried rows, deposits row 0 (``D = 1``, ``mu =
        0``) and leaves ``theta`` at ``theta0``.  ``k, l``: the wavenumber
        columns (required); ``need`` / ``v``: the values of the ``need`` and
        ``weight`` columns where they are neither (required then)."""
        if k is None or l is None:
            raise ValueError("the phase needs the wavenumbers of row 0: pass k and l")
        cols = {0: lon, 1: lat, 2: k, 3: l}
        for name, col, val in (("need", self.spec.ncol, need), ("weight", self.spec.wcol, v)):
            if col >= 4:
                if val is None:
                    raise ValueError(f"the map's {name} column is {getattr(self.spec, name)!r}: pass its values")
                cols[col] = val
        self.add_rows(0, 1, one_row(cols, self.device))
        return self

    def add_rows(self, i0, i1, view, tails=None, slots=None, ray=None):
        """Walk the tubes and integrate the phase over rows ``[i0, i1)`` of a
        launch of all ``nray`` rays and deposit those rows: ``view`` its row
        buffer (dense ``[nray, i1-i0, 8]``, or the row blocks of ``slots``),
        ``tails`` / ``slots`` the launch's ``engine.Tails`` /
        ``engine.Slots``.  One asynchronous ``rwrt_ray_wave`` call on the
        device's current stream."""
        import torch
        if ray is not None:
            raise NotImplementedError("a ray tube needs the rows of a ray's neighbours in the same launch: "
                                      "pass every ray, in column order")
        n, rows = row_args(i0, i1, view, tails, slots)
        if n != self.nray:
            raise ValueError(f"{n} rays for a wave map of {self.nray}")
        H.check(self._call(
            self._c, n, int(i0), int(i1), *rows, H.dptr(self.chan, torch.int32), H.dptr(self.nbr, torch.int32),
            H.dptr(self.state, torch.int32), H.dptr(self.prev, torch.float64), H.dptr(self.cnt, torch.int64),
            H.dptr(self.re, torch.float64), H.dptr(self.im, torch.float64), H.dptr(self.wabs, torch.float64),
            H.dptr(self.dropped, torch.int64), H.dptr(self.clipped, torch.int64), H.dptr(self.err, torch.int32),
            H.stream(self.device)))

    def allreduce(self, group=None):
        raise NotImplementedError("wave maps are not sharded: a ray's neighbours live on other ranks")

    def check(self):
        """Raise if a launch met a neighbour index outside ``[-1, nray)`` (the
        kernel sets an error word and treats the ray's tube as closed)."""
        if int(self.err.item()):
            raise H.RwrtError("rwrt_ray_wave: a neighbour index outside [-1, nray) on the device")
        return self

    def numpy(self):
        """The maps and the per-ray arrays on the host, as ``reference_wave``
        returns them (waits for the pending calls)."""
        self.check()
        st, pv = self.state.cpu().numpy(), self.prev.cpu().numpy()
        return {"cnt": self.cnt.cpu().numpy(), "re": self.re.cpu().numpy(), "im": self.im.cpu().numpy(),
                "wabs": self.wabs.cpu().numpy(), "dropped": int(self.dropped.cpu().numpy()[0]),
                "clipped": int(self.clipped.cpu().numpy()[0]), "theta": pv[4].copy(), "nseg": st[5].copy(),
                "mu": st[1].copy(), "first": st[2].copy(), "nrow": st[3].copy(), "close_row": st[4].copy(),
                "dlast": pv[8].copy(), "code": np.stack([st[0] & 3, (st[0] >> 2) & 3]).astype(np.int32)}

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
        """``amplitude / wabs``: 1 where the rays that reach a box agree in
        phase, 0 where they cancel."""
        import torch
        return self._where_hit(torch.hypot(self.re, self.im) / self.wabs)

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
                  "wabs": (full, a["wabs"], "sum of |w|"),
                  "dropped": (("one",), np.array([float(a["dropped"])]), "ray points"),
                  "clipped": (("one",), np.array([float(a["clipped"])]), "ray points"),
                  "theta": (("ray",), a["theta"], "radians"), "dlast": (("ray",), a["dlast"], "1")})
        for k, unit in (("nseg", "segments"), ("mu", "caustics"), ("first", "row"), ("nrow", "rows"),
                        ("close_row", "row")):
            v[k] = (("ray",), a[k], unit)
        ncio.write(ncfile, dims, v)


class WaveSink(RowSink):
    """A ``sink`` of ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume``
    (``launch_rows.RowSink``) that walks ``map`` over each launch's rows, alone
    or as a member of ``summary.Tee``.  Every launch must hold every ray:
    ``take`` (a shard) is refused."""

    def __init__(self, map):
        super().__init__(map, None)

    map = property(lambda self: self.target)

    def select(self, idx):
        raise NotImplementedError("wave maps are not sharded: a ray's neighbours live on other shards")
