"""Spherical-harmonic truncation of ``u, v`` (the reference's ``SHSF.py``) on the GPU.

The reference filters a basic state before ``BS`` reads it: expand in
spherical harmonics, truncate triangularly at degree ``T``, rebuild (its
comments name NCL's ``shaec`` -> ``tri_trunc`` -> ``shsec``).  It does so with
``pyshtools``; this module states the filter on the project's own grid and
returns data on the grid it was given (the deviation from
pyshtools' DH grid is DESIGN.md section 8).

``reference_weights``, ``reference_legendre`` and ``reference_filter`` are the
NumPy definition; ``rwrt_sh_filter`` (csrc/shsf.hip, csrc/shsf_legendre.h)
restates it on the device and is held to it by tests/test_gpu_shsf.py.
``SHFilter`` is the device filter, ``SHSF`` the reference's call surface.

The grid of the definition: ``f[nlat, nlon]`` in file layout, ``nlat`` odd with
``lat_j = -pi/2 + j pi / (nlat - 1)`` (both poles are nodes), ``nlon`` even with
``lon_i = 2 pi i / nlon``.  These are the IDEAL axes in fp64 -- not the
float32-rounded ``BS.lat`` -- and their sines and cosines come from the host's
C library (``math.sin``, ``math.cos``), so that a host C++ build of
csrc/shsf_legendre.h gives the same bits.
"""
import math

import numpy as np

__all__ = ["reference_nodes", "reference_weights", "reference_legendre", "reference_coefficients",
           "reference_filter", "check_grid", "SHFilter", "SHSF"]


# ----------------------------------------------------------------------------
# The definition (NumPy, no GPU)
# ----------------------------------------------------------------------------
def _check_sizes(nlat, nlon=None, trunc=None):
    if nlat < 3 or nlat % 2 == 0:
        raise ValueError(f"nlat must be odd and at least 3 (both poles are nodes), got {nlat}")
    if nlon is not None and (nlon < 2 or nlon % 2 != 0):
        raise ValueError(f"nlon must be even, got {nlon}")
    if trunc is not None and not (0 <= trunc <= (nlat - 1) // 2):
        raise ValueError(f"the truncation must be 0..(nlat-1)/2 = {(nlat - 1) // 2} (the quadrature's exact "
                         f"range), got {trunc}")


def reference_nodes(nlat):
    """``(x, c)``: ``sin(lat_j)`` and ``cos(lat_j)`` of the ideal latitudes
    ``lat_j = -pi/2 + j pi / (nlat - 1)``, both taken from the node's distance
    from the nearer pole, ``d = min(j, n - j) pi / n``: ``c = sin(d)``, ``x =
    -+cos(d)`` -- so that ``c`` keeps its relative precision next to the poles.
    ``c`` is exactly 0 at the poles, ``x`` exactly 0 on the equator."""
    _check_sizes(nlat)
    n = nlat - 1
    d = [(min(j, n - j) * math.pi) / n for j in range(nlat)]
    c = np.array([math.sin(a) for a in d])
    x = np.array([-math.cos(a) if j < n - j else math.cos(a) for j, a in enumerate(d)])
    x[n // 2] = 0.0
    return x, c


def reference_weights(nlat):
    """Clenshaw-Curtis weights in ``x = sin(lat)`` on the ``nlat`` nodes, ``n =
    nlat - 1``: ``w_j = (c_j / n) (1 - sum_{k=1..n/2} b_k / (4 k^2 - 1) cos(2 k
    theta_j))``, ``theta_j = j pi / n``, ``b_k = 1`` for ``k = n/2`` else 2,
    ``c_j = 1`` at the poles else 2 (``k`` ascending; the cosine's argument is
    reduced in integers).  They sum to 2 and integrate polynomials of degree
    ``<= nlat - 1`` exactly."""
    _check_sizes(nlat)
    n = nlat - 1
    tab = np.array([math.cos((math.pi * t) / n) for t in range(2 * n)])
    j = np.arange(nlat)
    s = np.zeros(nlat)
    for k in range(1, n // 2 + 1):
        bk = 1.0 if 2 * k == n else 2.0
        s = s + (bk / (4.0 * k * k - 1.0)) * tab[(2 * k * j) % (2 * n)]
    cj = np.full(nlat, 2.0)
    cj[0] = cj[-1] = 1.0
    return (cj / n) * (1.0 - s)


def reference_legendre(nlat, trunc):
    """``p[l, m, j] = p_lm(x_j)`` for ``l, m <= trunc`` (0 for ``l < m``): the
    associated Legendre functions normalised to ``int p_lm^2 dx = 1``, by the
    standard forward recurrence::

        p_00 = sqrt(1/2)
        p_mm = sqrt((2m+1)/(2m)) cos(lat) p_{m-1,m-1}
        p_{m+1,m} = sqrt(2m+3) (x p_mm)
        p_lm = a_lm (x p_{l-1,m} - b_lm p_{l-2,m}),
        a_lm = sqrt((4 l^2 - 1) / (l^2 - m^2)),  b_lm = sqrt(((l-1)^2 - m^2) / (4 (l-1)^2 - 1))

    A product ``x q`` is evaluated as ``sgn(x) (q - s q)`` with ``s = 1 - |x|``
    taken as ``c^2 / (1 + |x|)``: next to +-1 an fp64 ``x`` does not hold the
    node's distance from the pole (half an ulp of ``x`` moves ``p_l0`` by
    ``l (l + 1) / 2`` half-ulps), ``c`` does.  ``cos^m`` underflows to zero
    near the poles for large ``m``; the true value is negligible there."""
    _check_sizes(nlat)
    x, c = reference_nodes(nlat)
    sg, s = np.sign(x), (c * c) / (1.0 + np.abs(x))

    def xmul(q):
        return sg * (q - s * q)

    T = int(trunc)
    p = np.zeros((T + 1, T + 1, nlat))
    pmm = np.full(nlat, math.sqrt(0.5))
    for m in range(T + 1):
        if m > 0:
            pmm = (math.sqrt((2.0 * m + 1.0) / (2.0 * m)) * c) * pmm
        p[m, m] = pmm
        if m + 1 <= T:
            p[m + 1, m] = math.sqrt(2.0 * m + 3.0) * xmul(pmm)
        for l in range(m + 2, T + 1):
            l2, m2, k2 = float(l) * l, float(m) * m, float(l - 1) * (l - 1)
            a = math.sqrt((4.0 * l2 - 1.0) / (l2 - m2))
            b = math.sqrt((k2 - m2) / (4.0 * k2 - 1.0))
            p[l, m] = a * (xmul(p[l - 1, m]) - b * p[l - 2, m])
    return p


def _twiddles(nlon, M):
    """``E[i, m] = exp(2 pi i (m i mod nlon) / nlon)``, ``m < M``."""
    k = (np.arange(nlon)[:, None] * np.arange(M)[None, :]) % nlon
    ang = (2.0 * k) / nlon
    return np.cos(np.pi * ang) + 1j * np.sin(np.pi * ang)


def _analysis(f, trunc, order):
    f = np.asarray(f, np.float64)
    nlat, nlon = f.shape[-2:]
    _check_sizes(nlat, nlon, trunc)
    if order not in ("ascending", "descending"):
        raise ValueError("order must be 'ascending' or 'descending'")
    T = int(trunc)
    M = min(T, nlon // 2 - 1) + 1
    lead = f.shape[:-2]
    f = f.reshape((-1, nlat, nlon))
    w = reference_weights(nlat)
    p = reference_legendre(nlat, T)
    E = _twiddles(nlon, M)
    F = f @ np.conj(E)                                        # [field, j, m]: the longitude DFT
    a = np.zeros((f.shape[0], T + 1, T + 1), np.complex128)   # [field, l, m]
    rows = range(nlat) if order == "ascending" else range(nlat - 1, -1, -1)
    for j in rows:                                            # the quadrature, one latitude after another
        a[:, :, :M] = a[:, :, :M] + p[None, :, :M, j] * (w[j] * F[:, None, j, :])
    return a, p, E, lead, M


def reference_coefficients(f, trunc, order="ascending"):
    """``a[..., l, m] = sum_j w_j p_lm(x_j) F_m(j)`` for ``l, m <= trunc``, with
    ``F_m(j) = sum_i f[j, i] exp(-2 pi i m i / nlon)`` the (unnormalised)
    longitude DFT of row ``j``; zero for ``l < m`` and for orders above
    ``nlon/2 - 1``.  ``order``: the latitudes are summed ``'ascending'`` or
    ``'descending'`` (the spread between the two is the definition's own
    rounding error)."""
    a, _, _, lead, _ = _analysis(f, trunc, order)
    return a.reshape(lead + a.shape[1:])


def reference_filter(f, trunc, order="ascending"):
    """The field ``f[..., nlat, nlon]`` rebuilt from its spherical harmonics of
    degree ``l <= trunc`` (triangular truncation), fp64, on the grid it was
    given (see the module docstring for the grid: the ideal axes)::

        F_m(j) = longitude DFT of row j,  m = 0..min(T, nlon/2 - 1)
        a_lm   = sum_j w_j p_lm(x_j) F_m(j)
        G_m(j) = sum_{l=m..T} a_lm p_lm(x_j)                   (l ascending)
        result = inverse DFT of G = (G_0 + 2 sum_{m>=1} Re(G_m exp(2 pi i m i / nlon))) / nlon

    ``0 <= trunc <= (nlat - 1) / 2`` keeps analysis and synthesis inside the
    quadrature's exact range for everything retained.  ``order`` as in
    ``reference_coefficients``."""
    a, p, E, lead, M = _analysis(f, trunc, order)
    T = int(trunc)
    nlat = p.shape[-1]
    G = np.zeros((a.shape[0], nlat, M), np.complex128)
    for l in range(T + 1):
        G = G + a[:, None, l, :M] * p[l, :M, :].T[None]
    s = (G[:, :, 1:] @ E[:, 1:].T).real if M > 1 else np.zeros(G.shape[:2] + (E.shape[0],))
    out = (G[:, :, :1].real + 2.0 * s) / E.shape[0]
    return out.reshape(lead + out.shape[1:])


def check_grid(nlat, nlon, lat_deg=None):
    """Raise ``ValueError`` unless the axes are the grid of the definition:
    ``nlat`` odd, ``nlon`` even and ``lat_deg`` (if given) pole to pole,
    equally spaced, within float32 rounding of the ideal axis (ascending, or
    descending as some files are)."""
    _check_sizes(nlat, nlon)
    if lat_deg is None:
        return
    lat = np.asarray(lat_deg, np.float64)
    if lat.shape != (nlat,):
        raise ValueError(f"lat must have {nlat} entries")
    ideal = -90.0 + 180.0 * np.arange(nlat) / (nlat - 1)
    if lat[0] > lat[-1]:
        ideal = ideal[::-1]
    tol = 2.0 * float(np.spacing(np.float32(90.0)))
    if not (np.abs(lat - ideal) <= tol).all():
        raise ValueError("the spherical-harmonic filter needs equally spaced latitudes from pole to pole "
                         f"(-90..90 in {nlat} nodes); lat runs {lat[0]:g}..{lat[-1]:g} and is off the ideal "
                         f"axis by up to {float(np.abs(lat - ideal).max()):.3g} degrees")


# ----------------------------------------------------------------------------
# The device filter
# ----------------------------------------------------------------------------
class SHFilter:
    """``rwrt_sh_filter`` for one grid and truncation: holds the quadrature
    weights and the ``sin/cos`` tables on the device and sizes its scratch
    (kept, and grown, per batch size)."""

    def __init__(self, nlat, nlon, trunc, device=None):
        import torch
        import _hip as H
        _check_sizes(nlat, nlon, trunc)
        H.require_gpu()
        H.load()
        self.nlat, self.nlon, self.trunc = int(nlat), int(nlon), int(trunc)
        self.device = torch.device(device or "cuda")
        self.w = torch.as_tensor(reference_weights(nlat)).to(self.device)
        self.x = torch.as_tensor(np.stack(reference_nodes(nlat))).to(self.device).contiguous()
        self._scratch = None

    def _run(self, f, want32, want64):
        import torch
        import _hip as H
        if isinstance(f, np.ndarray) and not f.flags.writeable:
            f = f.copy()                # (torch does not wrap a read-only array)
        f = torch.as_tensor(f)
        if f.shape[-2:] != (self.nlat, self.nlon):
            raise ValueError(f"the trailing axes must be [{self.nlat}, {self.nlon}], got {tuple(f.shape)}")
        lead = tuple(f.shape[:-2])
        f = f.to(device=self.device, dtype=torch.float32).reshape((-1, self.nlat, self.nlon)).contiguous()
        nfield, n1 = f.shape[0], self.trunc + 1
        need = 2 * nfield * n1 * self.nlat * 2
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(max(need, 1), dtype=torch.float64, device=self.device)
        spec = torch.empty((nfield, n1, n1, 2), dtype=torch.float64, device=self.device)
        out32 = torch.empty_like(f) if want32 else None
        out64 = torch.empty(f.shape, dtype=torch.float64, device=self.device) if want64 else None
        with torch.cuda.device(self.device):
            H.check(H.load().rwrt_sh_filter(self.nlon, self.nlat, nfield, self.trunc, f.data_ptr(), H.dptr(self.w),
                                            H.dptr(self.x), spec.data_ptr(), H.dptr(out32), H.dptr(out64),
                                            self._scratch.data_ptr(), H.stream(self.device)))
        shape = lead + (self.nlat, self.nlon)
        return (spec.reshape(lead + (n1, n1, 2)), None if out32 is None else out32.reshape(shape),
                None if out64 is None else out64.reshape(shape))

    def filter(self, f, out_dtype=None):
        """``f[..., nlat, nlon]`` (a host array or a device tensor, read as
        float32 in file layout, latitude ascending in the sense of the
        definition) truncated at ``trunc``: a device tensor of the same shape,
        ``out_dtype`` ``torch.float32`` (default) or ``torch.float64``.
        Asynchronous on the current stream."""
        import torch
        out_dtype = out_dtype or torch.float32
        if out_dtype not in (torch.float32, torch.float64):
            raise ValueError("out_dtype must be torch.float32 or torch.float64")
        _, o32, o64 = self._run(f, out_dtype == torch.float32, out_dtype == torch.float64)
        return o32 if o64 is None else o64

    def filter_both(self, f):
        """``(float32, float64)`` results of one call (the float32 one is the
        float64 one rounded)."""
        _, o32, o64 = self._run(f, True, True)
        return o32, o64

    def coefficients(self, f):
        """``a[..., l, m]`` complex128 on the device, ``l, m <= trunc``
        (``reference_coefficients``): no field is rebuilt."""
        import torch
        spec, _, _ = self._run(f, False, False)
        return torch.view_as_complex(spec)


_FILTERS = {}


def shared_filter(nlat, nlon, trunc, device=None):
    """One ``SHFilter`` per (grid, truncation, device), kept for reuse."""
    import torch
    import _hip as H
    _check_sizes(nlat, nlon, trunc)
    H.require_gpu()
    dev = torch.device(device or "cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (int(nlat), int(nlon), int(trunc), str(dev))
    if key not in _FILTERS:
        _FILTERS[key] = SHFilter(nlat, nlon, trunc, dev)
    return _FILTERS[key]


def SHSF(data, truncation_level, sampling=2):
    """The reference's ``SHSF(data, truncation_level, sampling=2)``: ``data``
    2-D ``[nlat, nlon]`` or 3-D ``[n, nlat, nlon]`` expanded in spherical
    harmonics, truncated at ``truncation_level`` and rebuilt -- on the GPU,
    and ON THE INPUT GRID (the reference's pyshtools route returns the DH grid,
    which drops a pole and resamples).  ``sampling`` is accepted and ignored:
    the grid is the input's.  The data are read as float32 (what a file
    holds); a NumPy array comes back as a NumPy array of its own floating dtype
    (float32 for any other dtype), a tensor as a device tensor."""
    import torch
    is_tensor = isinstance(data, torch.Tensor)
    arr = data if is_tensor else np.asarray(data)
    if arr.ndim not in (2, 3):
        raise ValueError("data must be 2-D [nlat, nlon] or 3-D [n, nlat, nlon]")
    nlat, nlon = arr.shape[-2:]
    flt = shared_filter(nlat, nlon, truncation_level, arr.device if is_tensor and arr.is_cuda else None)
    if is_tensor:
        return flt.filter(arr, torch.float64 if arr.dtype == torch.float64 else torch.float32)
    wide = arr.dtype == np.float64
    out = flt.filter(arr.astype(np.float32), torch.float64 if wide else torch.float32)
    return out.cpu().numpy()
