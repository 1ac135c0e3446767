"""Time-varying basic states on the GPU (BASELINE configs[4]).

The reference integrates rays through ONE basic state (``fun`` ignores ``t``,
wr.py:784-789).  ``Levels`` holds a sequence of basic states -- snapshots of
``u, v`` valid at ``t0 + j*dt`` seconds of ray time -- as packed records
``[nlev][nlon+1][nlat][12]`` in HBM, each built on the device by
``rwrt_bs_ready`` (the reference's ``BS.ready``: vorticity, finite
differences, ``smth9``; bit-identical to the host ``BS.fields``).  Storage is
fp64, or fp32 (half the gather bytes; every operation stays fp64).  The ray
kernels interpolate each level in space exactly like the static state and
then linearly in time (include/rwrt.h ``rwrt_background``).

A one-level ``Levels`` is never integrated through the time-varying kernels:
``RayEngine.from_levels`` routes it to the reference's static path.
"""
import numpy as np
import torch

import _hip as H
from bs import BS


def trig_table(lat):
    """``[3, nlat]``: ``np.cos(lat)`` (for ``u cos(lat)``) and, at ``1..nlat-2``,
    ``np.cos``/``np.sin`` of ``lat[1:-1]`` -- the arrays ``calc_absolute_vorticity``
    evaluates (bs.py:264-279), from the host libm."""
    lat = np.asarray(lat, np.float64)
    t = np.zeros((3, len(lat)))
    t[0] = np.cos(lat[None, :])[0]
    t[1, 1:-1] = np.cos(lat[1:-1])
    t[2, 1:-1] = np.sin(lat[1:-1])
    return t


def time_index(t, t0, dt, nlev):
    """``(j, w)``: level index and weight of time ``t`` for levels at ``t0 + j*dt``
    -- ``s = (t - t0) / dt``, ``j = clip(floor(s), 0, nlev - 2)`` (0 for one
    level), ``w = min(max(s - j, 0), 1)``, in fp64 like the kernels."""
    s = (np.float64(t) - np.float64(t0)) / np.float64(dt)
    f = np.floor(s)
    # (floor_i32: an index past int32 wraps to the most negative one, as NumPy's cast does)
    i = -2 ** 31 if (f > 2147483647.0 or f != f) else int(max(f, -2147483648.0))
    j = max(0, min(i, nlev - 2)) if nlev > 1 else 0
    w = float(min(max(s - np.float64(j), np.float64(0.0)), np.float64(1.0)))
    return j, w


def level_origin(t0, release):
    """A release stack's per-ray level origin: a ray released ``release``
    seconds after the first level (valid at ``t0``) starts its own time at 0, so
    its levels lie at ``(t0 - release) + j*dt``.  fp64, on the host."""
    return np.float64(t0) - np.asarray(release, dtype=np.float64)


class Levels:
    """``nlev`` basic states on one GPU, packed for the ray kernels."""

    def __init__(self, lat_deg, lon_deg, nlev, t0=0.0, dt=6 * 3600.0, fp32=False, device=None,
                 arith32=False):
        """Axes in degrees (float32, as read from a file); level ``j`` is valid
        at ``t0 + j*dt`` s of ray time (the initial rays use level 0: t0 = 0).
        ``arith32`` (fp32 levels only): the RHS computes in fp32 as well
        (rwrt_background.fp32 = 2; not the reference's arithmetic)."""
        if arith32 and not fp32:
            raise ValueError("arith32 needs fp32 levels")
        self.arith32 = bool(arith32)
        H.require_gpu()
        H.load()
        lat_deg = np.asarray(lat_deg, np.float32)
        lon_deg = np.asarray(lon_deg, np.float32)
        if not (lat_deg[0] < lat_deg[-1]):
            raise ValueError("Levels needs an ascending latitude axis (flip u, v, lat first)")
        self.nlat, self.nlon = len(lat_deg), len(lon_deg)
        self.lat_deg, self._filters, self._diag, self._helmholtz = lat_deg, {}, None, {}
        # the axes exactly as BS.loadbs_ncfile builds them (float32 arithmetic)
        b = BS(self.nlon, self.nlat)
        b.load_arrays(np.zeros((self.nlat, self.nlon), np.float32),
                      np.zeros((self.nlat, self.nlon), np.float32), lat_deg, lon_deg)
        self.lat, self.lon = b.lat.copy(), b.lon.copy()
        self.dx, self.dy = float(b.dx[0]), float(b.dy[0])
        self.device = torch.device(device or "cuda")
        self.nlev, self.t0, self.dt, self.fp32 = int(nlev), float(t0), float(dt), bool(fp32)
        dtype = torch.float32 if fp32 else torch.float64
        self.packed = torch.empty((self.nlev, self.nlon + 1, self.nlat, H.NFIELD_PACK), dtype=dtype,
                                  device=self.device)
        # the t = 0 state in fp64 for the initial rays (rwrt_ray_initial reads fp64)
        self.level0_f64 = (torch.empty((self.nlon + 1, self.nlat, H.NFIELD_PACK), dtype=torch.float64,
                                       device=self.device) if fp32 else self.packed[0])
        self.trig = torch.as_tensor(trig_table(self.lat), device=self.device)
        self.scratch = torch.empty(4 * self.nlon * self.nlat, dtype=torch.float64, device=self.device)

    @property
    def grid(self):
        from engine import grid_of
        return grid_of(self.lon, self.lat, self.nlon + 1)

    def set_level(self, j, u, v, trunc=None, rotational=False):
        """Build level ``j`` from ``u, v[nlat, nlon]`` (float32, file layout; host
        arrays or device tensors) with ``rwrt_bs_ready`` (asynchronous).
        ``trunc``: first truncate ``u, v`` at that spherical-harmonic degree
        (``shsf.SHFilter``, one two-field batch; nothing leaves the device).
        ``rotational`` (needs ``trunc``): the level is built from the rotational
        wind ``u_rot, v_rot`` at that truncation instead
        (``helmholtz.Helmholtz.rotational``, float32)."""
        self._check_rotational(trunc, rotational)
        u = torch.as_tensor(u, dtype=torch.float32).to(self.device).contiguous()
        v = torch.as_tensor(v, dtype=torch.float32).to(self.device).contiguous()
        if u.shape != (self.nlat, self.nlon) or v.shape != (self.nlat, self.nlon):
            raise ValueError(f"u, v must be [{self.nlat}, {self.nlon}]")
        if rotational:
            u, v = (t.contiguous() for t in self.helmholtz(trunc).rotational(u, v))
        elif trunc is not None:
            u, v = self.sh_filter(trunc).filter(torch.stack([u, v]))
        self._ready(j, u, v)

    @staticmethod
    def _check_rotational(trunc, rotational):
        if rotational and trunc is None:
            raise ValueError("rotational=True needs trunc (the rotational wind is a truncated expansion)")

    def _ready(self, j, u, v):
        H.check(H.load().rwrt_bs_ready(self.nlon, self.nlat, H.dptr(u), H.dptr(v),
                                       H.dptr(self.trig), self.dx, self.dy, H.dptr(self.scratch),
                                       self.packed[j].data_ptr(), int(self.fp32), H.stream(self.device)))
        if j == 0 and self.fp32:
            H.check(H.load().rwrt_bs_ready(self.nlon, self.nlat, H.dptr(u), H.dptr(v),
                                           H.dptr(self.trig), self.dx, self.dy,
                                           H.dptr(self.scratch), self.level0_f64.data_ptr(), 0,
                                           H.stream(self.device)))

    def set_levels(self, u, v, trunc=None, rotational=False):
        """Build every level from ``u, v[nlev, nlat, nlon]``; with ``trunc`` the
        whole batch of ``2 nlev`` fields is filtered in one call first, with
        ``rotational`` as well (see ``set_level``) replaced by its rotational
        wind in one call."""
        self._check_rotational(trunc, rotational)
        u = torch.as_tensor(u, dtype=torch.float32).to(self.device).contiguous()
        v = torch.as_tensor(v, dtype=torch.float32).to(self.device).contiguous()
        shape = (self.nlev, self.nlat, self.nlon)
        if u.shape != shape or v.shape != shape:
            raise ValueError(f"u, v must be [{self.nlev}, {self.nlat}, {self.nlon}]")
        if rotational:
            u, v = self.helmholtz(trunc).rotational(u, v)
        elif trunc is not None:
            u, v = self.sh_filter(trunc).filter(torch.stack([u, v]))
        for j in range(self.nlev):
            self._ready(j, u[j].contiguous(), v[j].contiguous())

    def helmholtz(self, trunc):
        """The ``helmholtz.Helmholtz`` of this grid at ``trunc`` (kept).  Raises
        ``ValueError`` when the axes are not the filter's grid."""
        import helmholtz
        import shsf
        trunc = int(trunc)
        if trunc not in self._helmholtz:
            shsf.check_grid(self.nlat, self.nlon, self.lat_deg)
            self._helmholtz[trunc] = helmholtz.Helmholtz(self.nlat, self.nlon, trunc, self.device)
        return self._helmholtz[trunc]

    def sh_filter(self, trunc):
        """The ``shsf.SHFilter`` of this grid at ``trunc`` (kept).  Raises
        ``ValueError`` when the axes are not the filter's grid."""
        import shsf
        trunc = int(trunc)
        if trunc not in self._filters:
            shsf.check_grid(self.nlat, self.nlon, self.lat_deg)
            self._filters[trunc] = shsf.SHFilter(self.nlat, self.nlon, trunc, self.device)
        return self._filters[trunc]

    def diagnostics(self, u, v, names=("betam", "KS"), trunc=None):
        """Basic-state diagnostics of ``u, v[nlev, nlat, nlon]`` (or one
        ``[nlat, nlon]`` level; any number of levels, not only ``self.nlev``) on
        this stack's axes and device: a device tensor ``[nlev, len(names), nlon,
        nlat]`` (``bsdiag.BSDiag.compute``; the names are ``bsdiag.DIAG_NAMES``).
        The stack itself keeps no ``u, v``, so they are passed in."""
        if self._diag is None:
            from bsdiag import BSDiag
            self._diag = BSDiag.from_axes(self.lat, self.lon, self.dx, self.dy, self.device, self.lat_deg)
        return self._diag.compute(u, v, names, trunc=trunc)

    def time_index(self, t):
        """``(j, w)`` of ray time ``t`` (seconds, with ``t0`` as it stands): the
        lower bracketing level and the weight of level ``j + 1``, by the
        kernels' formulas and clamps (csrc/rwrt.hip VaryingBG::level)."""
        return time_index(t, self.t0, self.dt, self.nlev)

    def state_at(self, t):
        """The fp64 packed state ``[ncol, nrow, 12]`` valid at ``t`` seconds
        after the first level: ``P_j * (1 - w) + P_{j+1} * w`` with the kernels'
        own ``j`` and ``w`` (``time_index``), as three separate tensor
        operations (mul, mul, add: nothing contracts them).  ``packed[j]``
        itself when ``w == 0.0`` and ``packed[j + 1]`` itself when ``w == 1.0``,
        so a release at a level time starts from that level's own rows bit for
        bit.  fp64 levels.  (``release.reference_state_at`` is the NumPy
        definition.)

        For ``0 < w < 1`` the initial rows' ``ug, vg`` come from this blended
        state, while a run's RHS blends the two levels AFTER the bilinear
        lookup in each: the two agree to rounding, not bit for bit."""
        if self.fp32:
            raise NotImplementedError("state_at needs fp64 level storage")
        # (ray time 0 of a ray whose level origin is t0 - t: the kernels' s of its first evaluation)
        j, w = time_index(0.0, np.float64(self.t0) - np.float64(t), self.dt, self.nlev)
        up = j + 1 if self.nlev > 1 else j   # (one level: the kernels blend it with itself)
        if w == 0.0:
            return self.packed[j]
        if w == 1.0:
            return self.packed[up]
        a = torch.mul(self.packed[j], 1.0 - w)
        b = torch.mul(self.packed[up], w)
        return torch.add(a, b)

    def background(self):
        """The ``rwrt_background`` description of these levels."""
        return H.Background(self.packed.data_ptr(), self.nlev, 2 if self.arith32 else int(self.fp32),
                            self.t0, self.dt)
