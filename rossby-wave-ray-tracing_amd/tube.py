"""Ray-tube maps reduced on the GPU (``rwrt_ray_tube``, ABI 5): geometric
spreading, caustics and the Maslov index per ray.

Every other product reduces one ray at a time.  This one looks at a ray
together with its neighbours in the source lattice: the two difference vectors
across the ray, west to east and south to north, span the cross-section of the
ray tube.  Its area ``A`` relative to the area at the sources is the geometric
spreading ``D = A / A_0``: where ``|D|`` shrinks the rays focus, and where
``A`` changes sign neighbouring rays have crossed -- a caustic, where the WKB
amplitude is singular and the phase drops by pi / 2.  The crossings counted
along a ray are its Maslov index ``mu``.  The deformation of the tube is also
the sensitivity of the path to the source position: ``ftle`` is the
finite-time Lyapunov exponent of the ray flow.

``reference_tube`` (NumPy) is the definition.  The kernel (csrc/tube_rows.h)
restates it operation for operation -- no fused multiply-add -- so that every
integer (``cnt``, ``ncaus``, ``mu``, ``first``, ``nrow``, ``close_row``,
``dropped``) equals it: they rest on the sign of ``jac`` alone, which has no
transcendental in it.  ``D`` and the tube's columns differ only through the
device library's ``cos``, ``slog`` through its ``log`` and the order of a sum.

A ray's neighbours must be in the same launch, so ``TubeSink`` takes whole
launches only: a shard (``take``) and a process group are refused.
``WR.ray_tube`` is the user entry point.  A member stack or a release stack
(``EnsembleWR`` / ``ReleaseWR``, rays ``[member, root, source, zwn]``) goes
through ``reduce`` with the neighbours of ``3 * nmember`` leading slots::

    nbr = lattice_neighbours(nnx, nny, ew.nzwn, nlead=3 * ew.nmember)

    def make(device, chan, nray):
        m = TubeMap(with_channels(spec, ew.nmember), nray, nbr, device, chan)
        m.start(ew.rlon[0], ew.rlat[0], ew.ramp[0])         # row 0: lon, lat, the need column
        return m, TubeSink(m)

    m = ew.reduce(make, by="member")                        # ReleaseWR: by="release"
"""
import math
from dataclasses import dataclass

import numpy as np

import _hip as H
from density import bin_index
from launch_rows import RowSink, row_args
from raymap import CarriedMap, GridSpec, check_columns, counts_for

TWO_PI = 2.0 * math.pi
HALF_PI = 1.5707963267948966     # the double nearest pi / 2
NSTATE_I, NSTATE_F = 5, 13       # kTubeNI, kTubeNF: the rows of ``state`` and of ``prev``


@dataclass(frozen=True)
class TubeSpec(GridSpec):
    """``nx`` boxes over longitude [0, 360), ``ny`` over ``lat_range``
    (degrees, upper edge excluded), ``nchan`` maps.  ``need``: a row column by
    name (``raymap.WEIGHT_COLUMNS``) that must be finite for a point to be
    valid, or None; the default ``'amp'`` keeps dead root slots out.
    ``max_sep``: the largest separation (radians, in longitude or latitude)
    between the two rays of a stencil pair for which the pair still stands for
    a derivative; a tube wider than that closes.  ``inf`` never closes one."""
    nx: int
    ny: int
    need: str = "amp"
    max_sep: float = 0.5
    lat_range: tuple = (-90.0, 90.0)
    nchan: int = 1

    def __post_init__(self):
        self._check_shape()
        self._check_ranges()
        check_columns(self, "need")
        if not float(self.max_sep) > 0.0:
            raise ValueError("max_sep must be positive (inf: never close a tube)")

    def c_struct(self):
        return H.TubeMapC(self.nx, self.ny, self.nchan, self.ncol, self.lat0, self.inv_dlat, self.inv_dlon,
                          float(self.max_sep))


def lattice_neighbours(nnx, nny, nzwn, nlead=3, cyclic_x=False):
    """``nbr[4, nray]`` int32, the W, E, S, N neighbour of every ray of the
    layout ``[lead, iy * nnx + ix, zwn]`` (``WR``'s ray slots: ``nlead = 3``
    roots; a stack of n members or releases: ``nlead = 3 * n``), -1 beyond an
    edge.  A neighbour has the same ``lead`` and ``zwn`` and the next ``ix``
    or ``iy``; ``cyclic_x``: column ``nnx - 1`` and column 0 are neighbours
    (sources all around a latitude circle)."""
    nnx, nny, nzwn, nlead = int(nnx), int(nny), int(nzwn), int(nlead)
    if min(nnx, nny, nzwn, nlead) < 1:
        raise ValueError("nnx, nny, nzwn and nlead must be positive")
    if nlead * nnx * nny * nzwn >= 2 ** 31:
        raise ValueError("more than 2^31 rays")
    lead, iy, ix, z = np.meshgrid(np.arange(nlead), np.arange(nny), np.arange(nnx), np.arange(nzwn), indexing="ij")

    def at(jx, jy):
        if cyclic_x:
            jx = jx % nnx
        ok = (jx >= 0) & (jx < nnx) & (jy >= 0) & (jy < nny)
        return np.where(ok, ((lead * nny + jy) * nnx + jx) * nzwn + z, -1).reshape(-1)

    return np.stack([at(ix - 1, iy), at(ix + 1, iy), at(ix, iy - 1), at(ix, iy + 1)]).astype(np.int32)


def check_neighbours(nbr, nray):
    """``nbr`` as int32 ``[4, nray]`` with every entry in ``[-1, nray)``."""
    nbr = np.asarray(nbr)
    if nbr.shape != (4, nray) or nbr.dtype.kind not in "iu":
        raise ValueError(f"nbr must be integers [4, {nray}], got {nbr.dtype} {nbr.shape}")
    if nbr.size and (nbr.min() < -1 or nbr.max() >= nray):
        raise ValueError(f"nbr holds an index outside [-1, {nray})")
    return np.ascontiguousarray(nbr, np.int32)


def tube_valid(rows, spec):
    """``[nray, nt]`` bool: lon and lat finite, ``|lat| < pi/2`` (the double
    nearest pi/2) and, with ``need``, that column finite."""
    with np.errstate(all="ignore"):
        ok = np.isfinite(rows[..., 0]) & np.isfinite(rows[..., 1]) & (np.abs(rows[..., 1]) < HALF_PI)
        if spec.ncol >= 0:
            ok &= np.isfinite(rows[..., spec.ncol])
    return ok


def wrap(d):
    """``(d + pi) mod 2 pi - pi`` with Python's float %, taken twice as
    ``density_wrap_2pi`` does: a longitude difference in [-pi, pi)."""
    return np.remainder(np.remainder(d + math.pi, TWO_PI), TWO_PI) - math.pi


def stencil(ok0, nbr):
    """The stencil of every ray, fixed at row 0: ``(p[2, nray], q[2, nray],
    code[2, nray])`` for the directions a (W/E) and b (S/N).  ``code`` 1: the
    centred pair ``(lo, hi)``; 2: ``(j, hi)``; 3: ``(lo, j)``; 0: none (then
    ``p = q = j``).  ``ok0``: the rays valid at row 0."""
    nray = ok0.size
    j = np.arange(nray)
    p, q, code = (np.empty((2, nray), np.int64) for _ in range(3))
    for d in range(2):
        lo, hi = nbr[2 * d].astype(np.int64), nbr[2 * d + 1].astype(np.int64)
        vl = (lo >= 0) & ok0[np.maximum(lo, 0)]
        vh = (hi >= 0) & ok0[np.maximum(hi, 0)]
        code[d] = np.where(vl & vh, 1, np.where(vh, 2, np.where(vl, 3, 0)))
        p[d] = np.where(vl, lo, j)
        q[d] = np.where(vh, hi, j)
    return p, q, code


def reference_tube(rows, nbr, chan, spec):
    """The definition of the ray-tube product, in NumPy: a dict with the maps
    ``cnt``, ``ncaus`` (``[nchan, ny, nx]`` int64) and ``slog`` (float64),
    ``dropped`` (int), per ray ``mu``, ``first``, ``nrow``, ``close_row``
    (int32), ``dmin``, ``dlast`` (float64), ``f0``, ``flast`` (``[4, nray]``)
    and ``code`` (``[2, nray]``, the stencil of ``stencil``), and ``sabs``
    (per box the sum of ``|log|D||``: the magnitude ``slog``'s error bar
    refers to).

    ``rows[nray, nt, 8]``: a logical history (columns lon lat k l amp ug vg
    nacc, radians, row 0 the initial row); ``nbr[4, nray]``: the W, E, S, N
    neighbour of every ray, -1 for none; ``chan``: one channel per ray (None:
    channel 0).

    A point is valid iff lon and lat are finite, ``|lat| < pi/2`` and the
    ``need`` column, when set, is finite.  The stencil of ray j is fixed at
    row 0: in direction a the pair ``(p, q)`` is ``(W, E)`` if both are valid
    there, else ``(j, E)``, else ``(W, j)``, else none; direction b (S/N)
    likewise.  A ray that is invalid at row 0, lacks a pair in either
    direction, has a channel outside ``[0, nchan)`` or has ``jac_0 == 0`` has
    no tube: ``nrow = 0``, ``close_row = -1``, its floats NaN.

    At row i, one rounding per operation::

        dla = wrap(lon_q - lon_p);  dpa = lat_q - lat_p       (pair a; dlb, dpb: pair b)
        jac_i = dla * dpb - dlb * dpa
        A_i = jac_i * cos(lat_j);   D_i = A_i / A_0

    Row i is open iff j and its stencil rays are valid there, ``max(|dla|,
    |dpa|, |dlb|, |dpb|) <= max_sep`` and every earlier row was open; the
    first row that is not closes the tube for good (``close_row``).  An open
    row ``i >= 1`` with ``(jac_i < 0) != (jac_{i-1} < 0)`` is a caustic: ``mu
    += 1``, ``first = i`` if unset, ``ncaus += 1`` in ray j's box (binned as
    ``density.reference_bins`` bins it).  Every open row adds ``cnt += 1``,
    ``slog += log|D_i|`` to that box; one with ``jac_i == 0`` adds 1 to
    ``dropped`` instead (its sign counts as non-negative).  A row outside the
    map (``lat_range``) is open like any other and is not deposited.  Per
    ray: ``nrow`` open rows, ``dmin = min |D_i|``, ``dlast`` the last ``D_i``,
    ``f0`` / ``flast`` the columns ``(dla cos, dpa, dlb cos, dpb)`` at row 0
    and at the last open row.  Doubles as the ``mode='numpy'`` product of
    small runs."""
    nmap = spec.nchan * spec.ny * spec.nx
    cnt, ncaus = np.zeros(nmap, np.int64), np.zeros(nmap, np.int64)
    slog, sabs = np.zeros(nmap), np.zeros(nmap)
    dropped = 0
    ray = {}
    with np.errstate(all="ignore"):
        for r in tube_along(rows, nbr, chan, spec, ray):
            put = r.open & (r.idx >= 0)
            np.add.at(ncaus, r.idx[r.caustic & put], 1)
            zero = put & (r.jac == 0.0)
            dropped += int(zero.sum())
            put &= ~zero
            np.add.at(cnt, r.idx[put], 1)
            term = np.log(np.abs(r.D)[put])
            np.add.at(slog, r.idx[put], term)
            np.add.at(sabs, r.idx[put], np.abs(term))
    sh = spec.shape
    return {"cnt": cnt.reshape(sh), "ncaus": ncaus.reshape(sh), "slog": slog.reshape(sh), "sabs": sabs.reshape(sh),
            "dropped": dropped, **ray}


class TubeRow:
    """Row ``i`` of every ray's tube, as ``tube_along`` yields it: ``open``
    (``[nray]`` bool), ``jac``, ``D`` (float64; meaningful where open),
    ``caustic`` (bool), ``mu`` (the running Maslov index, a caustic at this
    row counted), ``jac0`` and ``idx`` (the box of the ray's point by position
    alone, -1 outside the map)."""
    __slots__ = ("i", "open", "jac", "D", "caustic", "mu", "jac0", "idx")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def tube_along(rows, nbr, chan, spec, ray):
    """The per-row quantities of ``reference_tube``, one ``TubeRow`` per row
    while any tube is open -- what the definition deposits from, and what
    ``wave.reference_wave`` composes with the phase.  ``ray`` (a dict) is
    filled with the per-ray results ``mu, first, nrow, close_row, dmin, dlast,
    f0, flast, code``, current after every row.  Call it under
    ``np.errstate(all='ignore')``."""
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 3 or rows.shape[1] < 1 or rows.shape[2] < 7:
        raise ValueError(f"rows must be [nray, nt >= 1, >= 7], got {rows.shape}")
    nray, nt = rows.shape[:2]
    nbr = check_neighbours(nbr, nray)
    chan = np.zeros(nray, np.int64) if chan is None else np.asarray(chan, np.int64).reshape(-1)
    if chan.size != nray:
        raise ValueError(f"chan has {chan.size} entries for {nray} rays")
    ok = tube_valid(rows, spec)
    lon, lat = rows[..., 0], rows[..., 1]
    p, q, code = stencil(ok[:, 0], nbr)
    open_ = ok[:, 0] & (code[0] > 0) & (code[1] > 0) & (chan >= 0) & (chan < spec.nchan)
    mu, nrow = np.zeros(nray, np.int32), np.zeros(nray, np.int32)
    first, close_row = np.full(nray, -1, np.int32), np.full(nray, -1, np.int32)
    dmin, dlast = np.full(nray, math.nan), np.full(nray, math.nan)
    f0, flast = np.full((4, nray), math.nan), np.full((4, nray), math.nan)
    jprev, a0, jac0 = np.zeros(nray), np.ones(nray), np.full(nray, math.nan)

    def results():
        ray.update(mu=mu, first=first, nrow=nrow, close_row=close_row, dmin=dmin, dlast=dlast, f0=f0, flast=flast,
                   code=code.astype(np.int32))

    results()
    for i in range(nt):
        if not open_.any():
            break
        dla, dpa = wrap(lon[q[0], i] - lon[p[0], i]), lat[q[0], i] - lat[p[0], i]
        dlb, dpb = wrap(lon[q[1], i] - lon[p[1], i]), lat[q[1], i] - lat[p[1], i]
        sep = np.maximum(np.maximum(np.abs(dla), np.abs(dpa)), np.maximum(np.abs(dlb), np.abs(dpb)))
        o = open_ & ok[:, i] & ok[p[0], i] & ok[q[0], i] & ok[p[1], i] & ok[q[1], i] & (sep <= float(spec.max_sep))
        close_row[open_ & ~o] = i
        jac = dla * dpb - dlb * dpa
        c = np.cos(lat[:, i])
        if i == 0:
            o &= jac != 0.0                       # (no tube: close_row stays -1)
            a0 = np.where(o, jac * c, 1.0)
            jac0 = np.where(o, jac, math.nan)
        D = (jac * c) / a0
        caus = o & ((jac < 0.0) != (jprev < 0.0)) if i else np.zeros(nray, bool)
        mu[caus] += 1
        first[caus & (first < 0)] = i
        jprev = np.where(o, jac, jprev)
        nrow[o] += 1
        aD = np.abs(D)
        dmin = np.where(o & ~(dmin <= aD), aD, dmin)
        dlast = np.where(o, D, dlast)
        cols = np.stack([dla * c, dpa, dlb * c, dpb])
        flast = np.where(o[None, :], cols, flast)
        if i == 0:
            f0 = flast.copy()
        results()
        yield TubeRow(i=i, open=o, jac=jac, D=D, caustic=caus, mu=mu, jac0=jac0,
                      idx=bin_index(lon[:, i], lat[:, i], None, chan, spec))
        open_ = o


def sigma_max(f0, flast, xp=np):
    """The largest singular value of ``F_last F_0^-1`` for the 2 x 2 matrices
    whose columns are the tube's two difference vectors (``f[0:2]``,
    ``f[2:4]``), from the closed form; NaN where ``F_0`` is singular."""
    a0, c0, b0, d0 = f0[0], f0[1], f0[2], f0[3]          # F = [[a, b], [c, d]]
    a1, c1, b1, d1 = flast[0], flast[1], flast[2], flast[3]
    det = a0 * d0 - b0 * c0
    ma, mb = (a1 * d0 - b1 * c0) / det, (b1 * a0 - a1 * b0) / det
    mc, md = (c1 * d0 - d1 * c0) / det, (d1 * a0 - c1 * b0) / det
    s = ma * ma + mb * mb + mc * mc + md * md
    t = ma * ma + mb * mb - mc * mc - md * md
    u = ma * mc + mb * md
    return xp.sqrt(0.5 * (s + xp.sqrt(t * t + 4.0 * (u * u))))


class TubeMap(CarriedMap):
    """The device arrays of one ray-tube product over ``nray`` rays with the
    neighbours ``nbr`` (``[4, nray]``: W, E, S, N; -1: none): the maps ``cnt``,
    ``ncaus`` (int64) and ``slog`` (fp64), each ``[nchan, ny, nx]``,
    ``dropped`` (int64 ``[1]``), and the per-ray state, which is also what is
    carried from a launch to the next: ``state`` (int32 ``[5, nray]``: the
    stencil choice and the open flag, ``mu``, ``first``, ``nrow``,
    ``close_row``) and ``prev`` (fp64 ``[13, nray]``: ``jac_prev``, ``jac_0``,
    ``cos_0``, ``dmin``, ``dlast``, ``f0[4]``, ``flast[4]``).  A running state:
    a ray's rows must arrive once, in order, with its neighbours' rows in the
    same launch; ``start`` (row 0 of all rays) fixes the stencils."""

    def __init__(self, spec, nray, nbr, device=None, chan=None):
        import torch
        super().__init__(spec, nray, device, chan)
        self.nbr = torch.as_tensor(check_neighbours(nbr, self.nray)).to(self.device).contiguous()
        self.cnt = torch.zeros(spec.shape, dtype=torch.int64, device=self.device)
        self.ncaus = torch.zeros(spec.shape, dtype=torch.int64, device=self.device)
        self.slog = torch.zeros(spec.shape, dtype=torch.float64, device=self.device)
        self.dropped = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.state = torch.zeros((NSTATE_I, self.nray), dtype=torch.int32, device=self.device)
        self.prev = torch.full((NSTATE_F, self.nray), math.nan, dtype=torch.float64, device=self.device)
        self.restart()

    def restart(self):
        """Close every tube and forget the per-ray results (the maps stay);
        the next row 0 starts them again."""
        self.state.zero_()
        self.state[2].fill_(-1)
        self.state[4].fill_(-1)
        self.prev.fill_(math.nan)
        return self

    mu = property(lambda self: self.state[1])
    first = property(lambda self: self.state[2])
    nrow = property(lambda self: self.state[3])
    close_row = property(lambda self: self.state[4])
    dmin = property(lambda self: self.prev[3])
    dlast = property(lambda self: self.prev[4])
    f0 = property(lambda self: self.prev[5:9])
    flast = property(lambda self: self.prev[9:13])

    def add_rows(self, i0, i1, view, tails=None, slots=None, ray=None):
        """Walk the tubes over rows ``[i0, i1)`` of a launch of all ``nray``
        rays: ``view`` its row buffer (dense ``[nray, i1-i0, 8]``, or the row
        blocks of ``slots``), ``tails`` / ``slots`` the launch's
        ``engine.Tails`` / ``engine.Slots``.  One asynchronous
        ``rwrt_ray_tube`` call on the device's current stream."""
        import torch
        if ray is not None:
            raise NotImplementedError("a ray tube needs the rows of a ray's neighbours in the same launch: "
                                      "pass every ray, in column order")
        n, rows = row_args(i0, i1, view, tails, slots)
        if n != self.nray:
            raise ValueError(f"{n} rays for a tube map of {self.nray}")
        H.check(self._lib.rwrt_ray_tube(
            self._c, n, int(i0), int(i1), *rows, H.dptr(self.chan, torch.int32), H.dptr(self.nbr, torch.int32),
            H.dptr(self.state, torch.int32), H.dptr(self.prev, torch.float64), H.dptr(self.cnt, torch.int64),
            H.dptr(self.slog, torch.float64), H.dptr(self.ncaus, torch.int64), H.dptr(self.dropped, torch.int64),
            H.dptr(self.err, torch.int32), H.stream(self.device)))

    def allreduce(self, group=None):
        raise NotImplementedError("ray tubes are not sharded: a ray's neighbours live on other ranks")

    def check(self):
        """Raise if a launch met a neighbour index outside ``[-1, nray)`` (the
        kernel sets an error word and treats the ray as closed)."""
        if int(self.err.item()):
            raise H.RwrtError("rwrt_ray_tube: a neighbour index outside [-1, nray) on the device")
        return self

    def numpy(self):
        """The maps and the per-ray arrays on the host, as ``reference_tube``
        returns them (waits for the pending calls)."""
        self.check()
        st, pv = self.state.cpu().numpy(), self.prev.cpu().numpy()
        return {"cnt": self.cnt.cpu().numpy(), "ncaus": self.ncaus.cpu().numpy(), "slog": self.slog.cpu().numpy(),
                "dropped": int(self.dropped.cpu().numpy()[0]), "mu": st[1].copy(), "first": st[2].copy(),
                "nrow": st[3].copy(), "close_row": st[4].copy(), "dmin": pv[3].copy(), "dlast": pv[4].copy(),
                "f0": pv[5:9].copy(), "flast": pv[9:13].copy(),
                "code": np.stack([st[0] & 3, (st[0] >> 2) & 3]).astype(np.int32)}

    # ---- derived fields: device tensors, NaN where undefined
    def _where_hit(self, x):
        import torch
        return torch.where(self.cnt == 0, torch.full_like(x, math.nan), x)

    def mean_log_spreading(self):
        """``slog / cnt``: the mean of ``log|D|`` over the tube points of a box."""
        return self._where_hit(self.slog / self.cnt)

    def geometric_amplitude(self):
        """``exp(-slog / (2 cnt))``: the geometric mean of ``|D|^(-1/2)``, the
        factor by which spreading changes the WKB amplitude."""
        import torch
        return self._where_hit(torch.exp(-self.slog / (2.0 * self.cnt)))

    def caustic_density(self):
        """``ncaus / cnt``: caustics per tube point of a box."""
        import torch
        return self._where_hit(self.ncaus.to(torch.float64) / self.cnt)

    def ftle(self, tstep):
        """Per ray ``log sigma_max(F_last F_0^-1) / ((nrow - 1) tstep)``: the
        finite-time Lyapunov exponent of the ray flow over the tube's open
        rows; NaN for a tube of fewer than two rows."""
        import torch
        n = self.nrow.to(torch.float64) - 1.0
        lam = torch.log(sigma_max(self.f0, self.flast, torch)) / (n * float(tstep))
        return torch.where(n > 0, lam, torch.full_like(lam, math.nan))

    def output(self, ncfile):
        """Write the maps (dims ``chan, lat, lon``; bin centres and edges in
        degrees) and the per-ray arrays (``ray``).  netCDF-3 has no 64-bit
        integers: the counts go out as float64 there (exact below 2^53), as
        int64 into an ``.npz``."""
        import ncio
        a = self.numpy()
        dims, v = self._grid_output()
        dims.update({"ray": self.nray, "one": 1, "col": 4})
        full = ("chan", "lat", "lon")
        v.update({"cnt": (full, counts_for(ncfile, a["cnt"]), "tube points"),
                  "ncaus": (full, counts_for(ncfile, a["ncaus"]), "caustics"),
                  "slog": (full, a["slog"], "sum of log|D|"),
                  "dropped": (("one",), np.array([float(a["dropped"])]), "tube points")})
        for k, unit in (("mu", "caustics"), ("first", "row"), ("nrow", "rows"), ("close_row", "row"),
                        ("dmin", "1"), ("dlast", "1")):
            v[k] = (("ray",), a[k], unit)
        for k in ("f0", "flast"):
            v[k] = (("col", "ray"), a[k], "radians")
        ncio.write(ncfile, dims, v)


class TubeSink(RowSink):
    """A ``sink`` of ``RayEngine.integrate`` / ``integrate_rk4`` / ``resume``
    (``launch_rows.RowSink``) that walks the tubes of ``map`` over each
    launch's rows.  Every launch must hold every ray: ``take`` (a shard) is
    refused."""

    def __init__(self, map):
        super().__init__(map, None)

    map = property(lambda self: self.target)

    def select(self, idx):
        raise NotImplementedError("ray tubes are not sharded: a ray's neighbours live on other shards")
