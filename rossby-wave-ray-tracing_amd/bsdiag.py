"""Basic-state diagnostics on the GPU: the 23 fields of the reference's
``BS.output`` (bs.py:461-511) for a batch of levels (``rwrt_bs_diag``).

The reference's driver writes "the full suite of basic flow diagnostics" right
after ``BS.ready`` (main_wr.py:82): ``u v q``, their derivatives, the six third
derivatives of ``q``, the Mercator ``betam`` and the stationary wavenumber
``KS = sqrt(betam cos(lat) / u) R``.  The host ``BS`` computes them for one
static state; ``BSDiag`` computes them on the device for any number of levels
of ``u, v`` and any subset of the planes -- ``betam, KS`` of a whole
time-varying run in one launch.

``reference_diag`` is the NumPy definition (our host ``BS``; pinned to the
reference by tests/golden/bsdiag_ref.npz) that every device plane equals bit
for bit, NaN for NaN.
"""
import numpy as np

DIAG_NAMES = ("u", "v", "q", "ux", "uxx", "uy", "vx", "vxx", "vy", "qx", "qy", "qxx", "qxy",
              "qyx", "qyy", "qxxx", "qxxy", "qxyy", "qyyy", "qyxx", "qyyx", "betam", "KS")
# the planes derived from q (ids 2, 9..20): they need the scratch of rwrt_bs_diag
NEEDS_Q = (1 << 2) | (0xfff << 9)
_SCRATCH_BYTES = 1 << 28          # default cap of the scratch (8 levels in flight at 0.25 degrees)


def reference_diag(u, v, lat_deg, lon_deg):
    """The NumPy definition: the host ``BS.load_arrays`` + ``ready(xcyclic=True)``
    on ``u, v[nlat, nlon]`` (float32, file layout) and degree axes; returns the
    23 planes ``[23, nlon, nlat]`` float64 in ``DIAG_NAMES`` order (``u, v``
    widened)."""
    from bs import BS
    lat_deg, lon_deg = np.asarray(lat_deg), np.asarray(lon_deg)
    b = BS(len(lon_deg), len(lat_deg))
    b.load_arrays(u, v, lat_deg, lon_deg)
    with np.errstate(all="ignore"):
        b.ready(xcyclic=True)
    return np.stack([np.asarray(getattr(b, n), np.float64) for n in DIAG_NAMES])


def select_mask(names):
    """``(mask, slots)`` of a list of plane names: the ``select`` word of
    ``rwrt_bs_diag`` and, for each name, its plane's position in the output."""
    ids = []
    for n in names:
        if n not in DIAG_NAMES:
            raise ValueError(f"unknown diagnostic {n!r}: the planes are {', '.join(DIAG_NAMES)}")
        ids.append(DIAG_NAMES.index(n))
    if not ids or len(set(ids)) != len(ids):
        raise ValueError("names must be a non-empty list of distinct planes")
    order = sorted(ids)
    mask = 0
    for p in ids:
        mask |= 1 << p
    return mask, [order.index(p) for p in ids]


class BSDiag:
    """``rwrt_bs_diag`` on one grid and device."""

    def __init__(self, lat_deg, lon_deg, device=None):
        """Axes in degrees (float32, as read from a file), latitude ascending;
        the radian axes, ``dx``, ``dy`` and the trig table are built exactly as
        ``Levels`` builds them."""
        from bs import BS
        lat_deg = np.asarray(lat_deg, np.float32)
        lon_deg = np.asarray(lon_deg, np.float32)
        if not (lat_deg[0] < lat_deg[-1]):
            raise ValueError("BSDiag needs an ascending latitude axis (flip u, v, lat first)")
        nlat, nlon = len(lat_deg), len(lon_deg)
        b = BS(nlon, nlat)
        b.load_arrays(np.zeros((nlat, nlon), np.float32), np.zeros((nlat, nlon), np.float32), lat_deg, lon_deg)
        self._setup(b.lat.copy(), b.lon.copy(), float(b.dx[0]), float(b.dy[0]), device, lat_deg)

    @classmethod
    def from_axes(cls, lat, lon, dx, dy, device=None, lat_deg=None):
        """From radian axes and steps as a ``BS`` or a ``Levels`` holds them."""
        self = cls.__new__(cls)
        self._setup(np.array(lat, np.float64), np.array(lon, np.float64), float(dx), float(dy), device, lat_deg)
        return self

    def _setup(self, lat, lon, dx, dy, device, lat_deg):
        import torch
        import _hip as H
        from levels import trig_table
        H.require_gpu()
        H.load()
        self.lat, self.lon, self.dx, self.dy, self.lat_deg = lat, lon, dx, dy, lat_deg
        self.nlat, self.nlon = len(lat), len(lon)
        if self.nlon < 3 or self.nlat < 4:
            raise ValueError("the diagnostics need nlon >= 3 and nlat >= 4")
        self.device = torch.device(device or "cuda")
        self.trig = torch.as_tensor(trig_table(lat), device=self.device)
        self._scratch = None

    def _winds(self, u, v):
        import torch

        def dev(a):
            if isinstance(a, np.ndarray) and not a.flags.writeable:
                a = a.copy()            # (torch does not wrap a read-only array)
            return torch.as_tensor(a, dtype=torch.float32).to(self.device).contiguous()
        u, v = dev(u), dev(v)
        if u.ndim == 2:
            u, v = u[None], v[None]
        if u.ndim != 3 or u.shape[1:] != (self.nlat, self.nlon) or v.shape != u.shape:
            raise ValueError(f"u, v must be [{self.nlat}, {self.nlon}] or [nlev, {self.nlat}, {self.nlon}]")
        return u, v

    def compute(self, u, v, names=None, trunc=None, scratch_levels=None):
        """The planes ``names`` (default: all 23) of ``u, v`` -- ``[nlat, nlon]``
        or ``[nlev, nlat, nlon]``, float32 in file layout, host arrays or device
        tensors -- as a device tensor ``[nlev, len(names), nlon, nlat]`` in the
        caller's order.  ``trunc``: first truncate ``u, v`` at that
        spherical-harmonic degree (``shsf.shared_filter``, one batch; nothing
        leaves the device).  ``scratch_levels``: levels in flight when a plane
        derived from ``q`` is asked for (default: as many as fit 256 MB); the
        result does not depend on it.  Asynchronous on the current stream."""
        import torch
        import _hip as H
        names = list(DIAG_NAMES if names is None else names)
        mask, slots = select_mask(names)
        u, v = self._winds(u, v)
        if trunc is not None:
            import shsf
            shsf.check_grid(self.nlat, self.nlon, self.lat_deg)
            u, v = shsf.shared_filter(self.nlat, self.nlon, int(trunc), self.device).filter(torch.stack([u, v]))
        nlev, n = u.shape[0], self.nlon * self.nlat
        scratch, sl = None, 0
        if mask & NEEDS_Q:
            sl = int(scratch_levels) if scratch_levels is not None else max(1, _SCRATCH_BYTES // (32 * n))
            if sl < 1:
                raise ValueError("scratch_levels must be at least 1")
            sl = max(1, min(sl, nlev))
            if self._scratch is None or self._scratch.numel() < 4 * n * sl:
                self._scratch = torch.empty(4 * n * sl, dtype=torch.float64, device=self.device)
            scratch = self._scratch
        out = torch.empty((nlev, len(names), self.nlon, self.nlat), dtype=torch.float64, device=self.device)
        if nlev == 0:
            return out
        with torch.cuda.device(self.device):
            H.check(H.load().rwrt_bs_diag(self.nlon, self.nlat, nlev, H.dptr(u), H.dptr(v), H.dptr(self.trig),
                                          self.dx, self.dy, mask, H.dptr(out), H.dptr(scratch), sl,
                                          H.stream(self.device)))
        if slots != list(range(len(names))):
            out = out[:, torch.as_tensor(slots, device=self.device)]
        return out

    def numpy(self, u, v, names=None, trunc=None, scratch_levels=None):
        """``compute`` brought to the host: ``{name: array}``, ``[nlev, nlon,
        nlat]`` each -- ``[nlon, nlat]``, like the attributes of a ready ``BS``,
        when ``u, v`` are one ``[nlat, nlon]`` level."""
        names = list(DIAG_NAMES if names is None else names)
        one = np.ndim(u) == 2
        out = self.compute(u, v, names, trunc, scratch_levels).cpu().numpy()
        return {n: (out[0, k] if one else out[:, k]) for k, n in enumerate(names)}

    def output(self, ncfile, u, v, names=None, trunc=None, scratch_levels=None):
        """Write the planes (netCDF-3 or .npz by suffix) with the radian axes:
        dims ``(level, lon, lat)``; one level is written with ``BS.output``'s
        variable names and dims ``(lon, lat)``."""
        import ncio
        d = self.numpy(u, v, names, trunc, scratch_levels)
        first = next(iter(d.values()))
        nlev = 1 if first.ndim == 2 else first.shape[0]
        dims = {"lon": self.nlon, "lat": self.nlat}
        node = ("lon", "lat")
        if nlev != 1:
            dims, node = dict(level=nlev, **dims), ("level", "lon", "lat")
        vars_ = {"lon": (("lon",), self.lon), "lat": (("lat",), self.lat)}
        for n, a in d.items():
            vars_[n] = (node, a.reshape([dims[k] for k in node]))
        ncio.write(ncfile, dims, vars_)
