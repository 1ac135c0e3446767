"""Helmholtz decomposition of ``u, v`` and the Rossby-wave source on the GPU.

The barotropic dispersion relation of ``BS`` and of the ray RHS holds for a
non-divergent basic state, so ray-tracing studies keep only the rotational
wind ``u_psi, v_psi`` of the upper-tropospheric flow; and they start the rays
where the Rossby-wave source of Sardeshmukh & Hoskins (1988), ``S = -div(v_chi
zeta_a)``, is large.  Both need the vector spherical-harmonic transform, stated
here on the filter's own grid (``shsf``: ``nlat`` odd with both poles, ``nlon``
even, latitude ascending; DESIGN.md sections 8, 13 and 26).

``reference_vector_basis``, ``reference_helmholtz`` and ``reference_rws`` are
the NumPy definition; ``rwrt_sh_helmholtz`` and ``rwrt_sh_rws``
(csrc/helmholtz.hip, csrc/sh_vector.h) restate it on the device and are held
to it by tests/test_gpu_helmholtz.py.  ``Helmholtz`` is the device class,
``rws_sources`` picks ray sources from a source field.

The definition, with ``a = constants.rearth``, ``p_lm``, the nodes, weights and
the DFT those of ``shsf``; for ``1 <= l <= T``, ``0 <= m <= l``::

    q_lm = p_lm / cos(lat), m >= 1: p's recurrences started one power of c lower
    b_lm = m q_lm                                   (b_l0 = 0)
    d_lm = dp_lm/dlat = ((l+1) eps_lm) q_{l-1,m} - (l eps_{l+1,m}) q_{l+1,m},  m >= 1
    d_l0 = sqrt(l (l+1)) (c q_l1),      eps_lm = sqrt((l^2 - m^2) / (4 l^2 - 1))

    vrt_lm = (1/a) sum_j w_j [ i V_m(j) b_lm(j) + U_m(j) d_lm(j) ]
    div_lm = (1/a) sum_j w_j [ i U_m(j) b_lm(j) - V_m(j) d_lm(j) ]
    psi_lm = -a^2 vrt_lm / (l (l+1)),  chi_lm = -a^2 div_lm / (l (l+1)),  l = 0: exactly 0

    plane   spec fn fac        plane   spec fn fac
    vrt     vrt  p  1          v_rot   psi  b  i/a
    div     div  p  1          u_div   chi  b  i/a
    psi     psi  p  1          v_div   chi  d  1/a
    chi     chi  p  1          vrt_x   vrt  b  i/a
    u_rot   psi  d  -1/a       vrt_y   vrt  d  1/a

``G_m(j) = fac sum_l spec_lm fn_lm(j)`` (``l`` ascending), then the filter's
inverse DFT.  ``vrt_x = (1/(a cos(lat))) d vrt/d lon``, ``vrt_y = (1/a) d vrt/d lat``.
"""
import math

import numpy as np

import shsf
from constants import omega, rearth

__all__ = ["PLANES", "reference_vector_basis", "reference_helmholtz", "reference_rws", "Helmholtz", "rws_sources"]

# the planes of a decomposition, in the order of the RWRT_SHV_* bits
PLANES = ("vrt", "div", "psi", "chi", "u_rot", "v_rot", "u_div", "v_div", "vrt_x", "vrt_y")
_ROT = ("u_rot", "v_rot")
_RWS = ("div", "u_div", "v_div", "vrt", "vrt_x", "vrt_y")


def _check_sizes(nlat, nlon=None, trunc=None):
    shsf._check_sizes(nlat, nlon, None)
    if trunc is not None and not (1 <= trunc <= (nlat - 1) // 2):
        raise ValueError(f"the truncation must be 1..(nlat-1)/2 = {(nlat - 1) // 2} (the quadrature's exact "
                         f"range), got {trunc}")


def plane_mask(planes):
    """The RWRT_SHV_* mask of plane names (``None``: all ten), and the names in bit order."""
    if planes is None:
        planes = PLANES
    if isinstance(planes, str):
        planes = (planes,)
    unknown = [p for p in planes if p not in PLANES]
    if unknown or not len(planes):
        raise ValueError(f"planes must be a non-empty subset of {PLANES}, got {tuple(planes)}")
    names = tuple(p for p in PLANES if p in planes)
    return sum(1 << PLANES.index(p) for p in names), names


# ----------------------------------------------------------------------------
# The definition (NumPy, no GPU)
# ----------------------------------------------------------------------------
def _eps(l, m):
    l2, m2 = float(l) * l, float(m) * m
    return math.sqrt((l2 - m2) / (4.0 * l2 - 1.0))


def reference_vector_basis(nlat, trunc):
    """``(q, b, d)``: ``q[l, m, j] = p_lm / cos(lat)`` for ``1 <= m <= l <= T + 1``
    (shape ``[T+2, T+2, nlat]``, zero elsewhere), and ``b[l, m, j] = m p_lm /
    cos(lat)``, ``d[l, m, j] = dp_lm/dlat`` for ``l, m <= T`` (shape ``[T+1,
    T+1, nlat]``, zero for ``l < m`` and ``l = 0``); all finite at the poles.
    ``q`` runs through the recurrences of ``shsf.reference_legendre`` (the
    ``x q`` rule included) from ``q_11 = sqrt(3/2) sqrt(1/2)``: nothing is
    divided by ``cos(lat)``."""
    _check_sizes(nlat, None, trunc)
    x, c = shsf.reference_nodes(nlat)
    sg, s = np.sign(x), (c * c) / (1.0 + np.abs(x))

    def xmul(t):
        return sg * (t - s * t)

    T = int(trunc)
    q = np.zeros((T + 2, T + 2, nlat))
    qmm = np.full(nlat, math.sqrt(1.5) * math.sqrt(0.5))
    for m in range(1, T + 2):
        if m > 1:
            qmm = (math.sqrt((2.0 * m + 1.0) / (2.0 * m)) * c) * qmm
        q[m, m] = qmm
        if m + 1 <= T + 1:
            q[m + 1, m] = math.sqrt(2.0 * m + 3.0) * xmul(qmm)
        for l in range(m + 2, T + 2):
            l2, m2, k2 = float(l) * l, float(m) * m, float(l - 1) * (l - 1)
            ra = math.sqrt((4.0 * l2 - 1.0) / (l2 - m2))
            rb = math.sqrt((k2 - m2) / (4.0 * k2 - 1.0))
            q[l, m] = ra * (xmul(q[l - 1, m]) - rb * q[l - 2, m])
    b = np.zeros((T + 1, T + 1, nlat))
    d = np.zeros((T + 1, T + 1, nlat))
    for l in range(1, T + 1):
        d[l, 0] = math.sqrt(float(l) * (l + 1.0)) * (c * q[l, 1])
        for m in range(1, l + 1):
            b[l, m] = float(m) * q[l, m]
            d[l, m] = ((l + 1.0) * _eps(l, m)) * q[l - 1, m] - (float(l) * _eps(l + 1, m)) * q[l + 1, m]
    return q, b, d


def _potential(spec):
    """``-a^2 spec_lm / (l (l+1))``, the ``l = 0`` row exactly 0 (real arrays ``[..., l, m]``)."""
    out = np.zeros_like(spec)
    for l in range(1, spec.shape[-2]):
        out[..., l, :] = (spec[..., l, :] * -(rearth * rearth)) / (float(l) * (l + 1.0))
    return out


def reference_helmholtz(u, v, trunc, order="ascending"):
    """The decomposition of ``u, v[..., nlat, nlon]`` at truncation ``trunc`` (see
    the module docstring), fp64: a dict of the ten ``PLANES`` (each ``[...,
    nlat, nlon]``) and of ``vrt_lm``, ``div_lm`` (complex ``[..., T+1, T+1]``).
    The quadrature adds one latitude after another, ``order`` ``'ascending'``
    or ``'descending'`` (the spread between the two is the definition's own
    rounding error).  Real and imaginary parts are separate real sums::

        vrt: re += (w U_re) d - (w V_im) b      im += (w U_im) d + (w V_re) b
        div: re += -((w U_im) b) - (w V_re) d   im += (w U_re) b - (w V_im) d

    each divided by ``a`` at the end; ``G = fac S`` divides the sum ``S`` by
    ``a`` and swaps or negates its parts."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    if u.shape != v.shape or u.ndim < 2:
        raise ValueError("u and v must have the same shape [..., nlat, nlon]")
    nlat, nlon = u.shape[-2:]
    _check_sizes(nlat, nlon, trunc)
    if order not in ("ascending", "descending"):
        raise ValueError("order must be 'ascending' or 'descending'")
    T = int(trunc)
    M = min(T, nlon // 2 - 1) + 1
    lead = u.shape[:-2]
    u, v = u.reshape((-1, nlat, nlon)), v.reshape((-1, nlat, nlon))
    w = shsf.reference_weights(nlat)
    p = shsf.reference_legendre(nlat, T)
    _, b, d = reference_vector_basis(nlat, T)
    E = shsf._twiddles(nlon, M)
    U, V = u @ np.conj(E), v @ np.conj(E)                     # [pair, j, m]
    acc = np.zeros((4, u.shape[0], T + 1, T + 1))             # vrt re, im; div re, im: [pair, l, m]
    rows = range(nlat) if order == "ascending" else range(nlat - 1, -1, -1)
    for j in rows:                                            # the quadrature, one latitude after another
        wur, wui = (w[j] * U[:, None, j, :].real), (w[j] * U[:, None, j, :].imag)
        wvr, wvi = (w[j] * V[:, None, j, :].real), (w[j] * V[:, None, j, :].imag)
        bj, dj = b[None, :, :M, j], d[None, :, :M, j]
        acc[0, :, :, :M] = acc[0, :, :, :M] + (wur * dj - wvi * bj)
        acc[1, :, :, :M] = acc[1, :, :, :M] + (wui * dj + wvr * bj)
        acc[2, :, :, :M] = acc[2, :, :, :M] + (-(wui * bj) - wvr * dj)
        acc[3, :, :, :M] = acc[3, :, :, :M] + (wur * bj - wvi * dj)
    acc = acc / rearth
    acc[:, :, 0, :] = 0.0
    spec = {"vrt": (acc[0], acc[1]), "div": (acc[2], acc[3])}
    spec["psi"] = (_potential(acc[0]), _potential(acc[1]))
    spec["chi"] = (_potential(acc[2]), _potential(acc[3]))
    fn = {"p": p, "b": b, "d": d}

    def plane(which, f, fac):
        sre = np.zeros((u.shape[0], nlat, M))
        sim = np.zeros((u.shape[0], nlat, M))
        cre, cim = spec[which]
        for l in range(1, T + 1):
            sre = sre + cre[:, None, l, :M] * fn[f][l, :M, :].T[None]
            sim = sim + cim[:, None, l, :M] * fn[f][l, :M, :].T[None]
        if fac == "1":
            G = sre + 1j * sim
        elif fac == "-1/a":
            G = -(sre / rearth) + 1j * -(sim / rearth)
        elif fac == "i/a":
            G = -(sim / rearth) + 1j * (sre / rearth)
        else:
            G = (sre / rearth) + 1j * (sim / rearth)
        s = (G[:, :, 1:] @ E[:, 1:].T).real if M > 1 else np.zeros(G.shape[:2] + (nlon,))
        out = (G[:, :, :1].real + 2.0 * s) / nlon
        return out.reshape(lead + out.shape[1:])

    table = {"vrt": ("vrt", "p", "1"), "div": ("div", "p", "1"), "psi": ("psi", "p", "1"), "chi": ("chi", "p", "1"),
             "u_rot": ("psi", "d", "-1/a"), "v_rot": ("psi", "b", "i/a"), "u_div": ("chi", "b", "i/a"),
             "v_div": ("chi", "d", "1/a"), "vrt_x": ("vrt", "b", "i/a"), "vrt_y": ("vrt", "d", "1/a")}
    out = {name: plane(*table[name]) for name in PLANES}
    out["vrt_lm"] = (acc[0] + 1j * acc[1]).reshape(lead + (T + 1, T + 1))
    out["div_lm"] = (acc[2] + 1j * acc[3]).reshape(lead + (T + 1, T + 1))
    return out


def reference_rws(A, B, planetary=True):
    """``S(A, B; planetary) = -(vrt_B + f) div_A - (u_div_A vrt_x_B + v_div_A
    (vrt_y_B + beta))`` pointwise from the planes (dicts as ``reference_helmholtz``
    returns them) of two decompositions, ``f = (2 Omega) x_j``, ``beta = ((2 Omega)
    c_j) / a``, both 0 with ``planetary=False``.  The total source of a flow is
    ``S(A, A)``; the linearised anomaly source ``S(anom, clim) + S(clim, anom;
    planetary=False)``."""
    nlat = A["div"].shape[-2]
    x, c = shsf.reference_nodes(nlat)
    f = ((2.0 * omega) * x if planetary else np.zeros(nlat))[:, None]
    beta = (((2.0 * omega) * c) / rearth if planetary else np.zeros(nlat))[:, None]
    stretch = (B["vrt"] + f) * A["div"]
    advect = A["u_div"] * B["vrt_x"] + A["v_div"] * (B["vrt_y"] + beta)
    return -stretch - advect


# ----------------------------------------------------------------------------
# The device class
# ----------------------------------------------------------------------------
class Helmholtz:
    """``rwrt_sh_helmholtz`` / ``rwrt_sh_rws`` for one grid and truncation.  The
    quadrature weights and the node tables are the filter's
    (``shsf.shared_filter``); the scratch is kept, and grown, per batch size."""

    def __init__(self, nlat, nlon, trunc, device=None):
        _check_sizes(nlat, nlon, trunc)
        flt = shsf.shared_filter(nlat, nlon, trunc, device)
        self.nlat, self.nlon, self.trunc = int(nlat), int(nlon), int(trunc)
        self.device, self.w, self.x = flt.device, flt.w, flt.x
        self._scratch = None

    def _pair(self, u, v):
        import torch
        out = []
        for f in (u, v):
            if isinstance(f, np.ndarray) and not f.flags.writeable:
                f = f.copy()                # (torch does not wrap a read-only array)
            f = torch.as_tensor(f)
            if f.shape[-2:] != (self.nlat, self.nlon):
                raise ValueError(f"the trailing axes must be [{self.nlat}, {self.nlon}], got {tuple(f.shape)}")
            out.append(f)
        if out[0].shape != out[1].shape:
            raise ValueError("u and v must have the same shape")
        lead = tuple(out[0].shape[:-2])
        u, v = (f.to(device=self.device, dtype=torch.float32).reshape((-1, self.nlat, self.nlon)).contiguous()
                for f in out)
        return u, v, lead

    def _run(self, u, v, mask, want64, want32):
        import torch
        import _hip as H
        u, v, lead = self._pair(u, v)
        npair, n1, nplane = u.shape[0], self.trunc + 1, bin(mask).count("1")
        need = npair * (4 + nplane) * n1 * self.nlat * 2
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(max(need, 1), dtype=torch.float64, device=self.device)
        spec = torch.empty((npair, 2, n1, n1, 2), dtype=torch.float64, device=self.device)
        out64 = (torch.empty((npair, nplane, self.nlat, self.nlon), dtype=torch.float64, device=self.device)
                 if want64 else None)
        rot32 = (torch.empty((npair, 2, self.nlat, self.nlon), dtype=torch.float32, device=self.device)
                 if want32 else None)
        with torch.cuda.device(self.device):
            H.check(H.entry("rwrt_sh_helmholtz")(self.nlon, self.nlat, npair, self.trunc, mask, u.data_ptr(),
                                               v.data_ptr(), H.dptr(self.w), H.dptr(self.x), spec.data_ptr(),
                                               H.dptr(out64), H.dptr(rot32), self._scratch.data_ptr(),
                                               H.stream(self.device)))
        return spec, out64, rot32, lead

    def decompose(self, u, v, planes=None, rot32=False):
        """The planes (names of ``PLANES``; default all ten) of ``u, v[..., nlat,
        nlon]`` (host arrays or device tensors, read as float32, latitude
        ascending): a dict of fp64 device tensors ``[..., nlat, nlon]``.
        ``rot32``: also ``"rot32"``, ``[..., 2, nlat, nlon]`` float32, ``u_rot,
        v_rot`` rounded.  Asynchronous on the current stream."""
        mask, names = plane_mask(planes)
        _, out64, r32, lead = self._run(u, v, mask, True, rot32)
        shape = lead + (self.nlat, self.nlon)
        out = {name: out64[:, k].reshape(shape) for k, name in enumerate(names)}
        if rot32:
            out["rot32"] = r32.reshape(lead + (2, self.nlat, self.nlon))
        return out

    def coefficients(self, u, v):
        """``(vrt_lm, div_lm)``, complex128 ``[..., l, m]`` on the device,
        ``l, m <= trunc``: no plane is rebuilt."""
        import torch
        n1 = self.trunc + 1
        spec, _, _, lead = self._run(u, v, 1, False, False)
        spec = torch.view_as_complex(spec)
        return spec[:, 0].reshape(lead + (n1, n1)), spec[:, 1].reshape(lead + (n1, n1))

    def rotational(self, u, v, out_dtype=None):
        """``(u_rot, v_rot)`` as device tensors of the input's shape, ``out_dtype``
        ``torch.float32`` (default: what ``rwrt_bs_ready`` reads; the fp64
        value rounded) or ``torch.float64``."""
        import torch
        out_dtype = out_dtype or torch.float32
        if out_dtype not in (torch.float32, torch.float64):
            raise ValueError("out_dtype must be torch.float32 or torch.float64")
        mask, _ = plane_mask(_ROT)
        wide = out_dtype == torch.float64
        _, out64, r32, lead = self._run(u, v, mask, wide, not wide)
        out = out64 if wide else r32
        shape = lead + (self.nlat, self.nlon)
        return out[:, 0].reshape(shape), out[:, 1].reshape(shape)

    def _rws_planes(self, u, v):
        mask, names = plane_mask(_RWS)
        _, out64, _, lead = self._run(u, v, mask, True, False)
        return {name: out64[:, k].contiguous() for k, name in enumerate(names)}, lead

    def _source(self, A, B, planetary):
        import torch
        import _hip as H
        nfield = A["div"].shape[0]
        out = torch.empty((nfield, self.nlat, self.nlon), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            H.check(H.entry("rwrt_sh_rws")(self.nlon, self.nlat, nfield, int(bool(planetary)), H.dptr(self.x),
                                         H.dptr(A["div"]), H.dptr(A["u_div"]), H.dptr(A["v_div"]), H.dptr(B["vrt"]),
                                         H.dptr(B["vrt_x"]), H.dptr(B["vrt_y"]), out.data_ptr(),
                                         H.stream(self.device)))
        return out

    def rws(self, u, v):
        """The Rossby-wave source ``S(A, A; planetary)`` of the flow ``u, v``
        (``reference_rws``): an fp64 device tensor ``[..., nlat, nlon]``."""
        A, lead = self._rws_planes(u, v)
        return self._source(A, A, True).reshape(lead + (self.nlat, self.nlon))

    def rws_anomaly(self, u_clim, v_clim, u_anom, v_anom):
        """The linearised anomaly source ``S(anom, clim; planetary) + S(clim,
        anom; not planetary)`` (one tensor addition of the two)."""
        import torch
        clim, lead = self._rws_planes(u_clim, v_clim)
        anom, lead_a = self._rws_planes(u_anom, v_anom)
        if lead != lead_a:
            raise ValueError("the climatology and the anomaly must have the same shape")
        s = torch.add(self._source(anom, clim, True), self._source(clim, anom, False))
        return s.reshape(lead + (self.nlat, self.nlon))


def _separation_deg(lon1, lat1, lon2, lat2):
    """Great-circle distance in degrees (haversine)."""
    p1, p2 = np.deg2rad(lat1), np.deg2rad(lat2)
    dl = np.deg2rad(lon2 - lon1)
    h = np.sin((p2 - p1) / 2.0) ** 2 + np.cos(p1) * np.cos(p2) * np.sin(dl / 2.0) ** 2
    return np.rad2deg(2.0 * np.arcsin(np.sqrt(np.clip(h, 0.0, 1.0))))


def rws_sources(S, lat_deg, lon_deg, n, box=None, min_sep_deg=0.0, sign=None):
    """Where to start rays: the ``n`` nodes of largest ``|S|`` of one source
    field ``S[nlat, nlon]`` (a tensor on any device, or an array).  ``sign``
    ``+1`` / ``-1``: only nodes of that sign, largest ``S`` / ``-S`` first.
    ``box = (lon_w, lon_e, lat_s, lat_n)`` in degrees, edges included, keeps the
    nodes inside it (``lon_w > lon_e``: the box crosses 0 degrees).  The
    candidates are taken largest first and one is dropped when it lies within
    ``min_sep_deg`` degrees of great circle of one already taken.  Returns
    ``(lon_deg, lat_deg, value)``, float64 arrays of at most ``n`` entries,
    for ``WR.set_source_array``.  A ``topk`` where ``S`` lives and a short loop
    on the host."""
    import torch
    S = torch.as_tensor(S)
    lat = np.asarray(lat_deg, np.float64)
    lon = np.asarray(lon_deg, np.float64)
    if S.ndim != 2 or S.shape != (len(lat), len(lon)):
        raise ValueError(f"S must be [nlat, nlon] = [{len(lat)}, {len(lon)}], got {tuple(S.shape)}")
    if n < 0 or min_sep_deg < 0.0:
        raise ValueError("n and min_sep_deg must not be negative")
    if sign not in (None, 1, -1):
        raise ValueError("sign must be None, +1 or -1")
    keep = np.ones(S.shape, bool)
    if box is not None:
        lon_w, lon_e, lat_s, lat_n = (float(t) for t in box)
        if lat_s > lat_n:
            raise ValueError("box is (lon_w, lon_e, lat_s, lat_n) with lat_s <= lat_n")
        lw, le, lo = lon_w % 360.0, lon_e % 360.0, lon % 360.0
        in_lon = (lo >= lw) & (lo <= le) if lw <= le else (lo >= lw) | (lo <= le)
        keep &= ((lat >= lat_s) & (lat <= lat_n))[:, None] & in_lon[None, :]
    score = S.abs() if sign is None else S * float(sign)
    ok = torch.as_tensor(keep, device=S.device) & torch.isfinite(S)
    if sign is not None:
        ok &= score > 0
    score = torch.where(ok, score, torch.full_like(score, -math.inf)).reshape(-1)
    nvalid = int(ok.sum())
    nlon = len(lon)
    take_lon, take_lat, take_val = [], [], []
    k = min(nvalid, max(64, 32 * int(n)))
    while n > 0 and nvalid > 0:
        idx = torch.topk(score, k).indices.cpu().numpy()
        vals = S.reshape(-1)[torch.as_tensor(idx, device=S.device)].cpu().numpy().astype(np.float64)
        take_lon, take_lat, take_val = [], [], []
        for i, val in zip(idx, vals):
            plon, plat = float(lon[i % nlon]), float(lat[i // nlon])
            if min_sep_deg > 0.0 and take_lon and \
                    (_separation_deg(np.array(take_lon), np.array(take_lat), plon, plat) < min_sep_deg).any():
                continue
            take_lon.append(plon)
            take_lat.append(plat)
            take_val.append(float(val))
            if len(take_lon) == n:
                break
        if len(take_lon) == n or k == nvalid:
            break
        k = nvalid                       # (thinning used the candidates up: take every node)
    return np.array(take_lon), np.array(take_lat), np.array(take_val)
