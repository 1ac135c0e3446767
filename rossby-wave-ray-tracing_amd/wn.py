"""Group velocity (the reference's wn.py:140-351) on the host.

``cal_ugvg(mode='numpy')`` is the t = 0 formula used for the initial rows
(wn.py:209-259); ``mode='extent'`` is the formula of the ray loop
(wn.py:266-342), which the HIP kernel evaluates on the device -- the host
version here serves the initial-row/diagnostic path only.

``WN`` is the reference's wavenumber-map class (wn.py:21-135) with the map
computed on the GPU (``rwrt_wn_map``, ``rwrt_wn_fill``);
``reference_wn_map`` and ``reference_fill`` are the NumPy definitions the
device results are held to.
"""
import numpy as np


def cal_ugvg_numpy(fu, fv, fqx, fqy, zwn, mwn, min_val=1e-10):
    """``fu..fqy``: ``(points,)``; ``mwn``: ``(3, points)`` -> ``ug, vg`` ``(3, points)``."""
    if zwn == 0:
        return np.zeros(mwn.shape), np.zeros(mwn.shape)
    nans = np.einsum("ij,j->ij", mwn * 0, fu * fqx * fqy * 0) + 1
    nans[np.isnan(nans)] = 0
    a = zwn * zwn - mwn * mwn
    b = 2 * zwn * mwn
    c = zwn * zwn + mwn * mwn
    ug = fu + (a * fqy - b * fqx) / c ** 2
    vg = fv + (a * fqx + b * fqy) / c ** 2
    return ug * nans, vg * nans


def cal_ugvg_extent(fu, fv, fqx, fqy, zwn, mwn, min_val=1e-10):
    """Element-wise Mercator group velocity (core_cal_ugvg_extent)."""
    kap = mwn / zwn
    kap2 = kap * kap
    kap1 = 1.0 + kap2
    denom = zwn * zwn * kap1 * kap1
    ug = fu + (((1. - kap2) * fqy) - (2. * kap * fqx)) / denom
    vg = fv + ((2. * kap * fqy) + ((1. - kap2) * fqx)) / denom
    return ug, vg


def cal_ugvg(fu, fv, fqx, fqy, zwn, mwn, mode="numpy"):
    if mode == "numpy":
        return cal_ugvg_numpy(fu, fv, fqx, fqy, zwn, mwn)
    if mode == "extent":
        return cal_ugvg_extent(fu, fv, fqx, fqy, zwn, mwn)
    raise ValueError(f"mode must be 'numpy' or 'extent', got {mode!r}")


# ----------------------------------------------------------------------------
# The wavenumber map: the reference's class WN (wn.py:21-135) on the GPU
# ----------------------------------------------------------------------------
def reference_wn_map(bs, zwn, freq=0.0):
    """The NumPy definition of the wavenumber map of a ready ``BS``: at every
    grid node ``(bs.lon[i], bs.lat[j])`` and for every zonal wavenumber the
    initial rows of a ray launched there -- the host ``cal_bs_mercator_point``,
    ``cal_ky(mode='numpy')`` and ``cal_ugvg_numpy``, one latitude row at a
    time.  Returns ``(mwn, ug, vg, rootnum)``: ``[nlon, nlat, nzwn, 3]`` and
    ``rootnum[nlon, nlat, nzwn]`` (int32), the number of non-NaN slots of
    ``mwn``.  Where ``np.roots`` raises (non-finite coefficients: the pole
    rows), ``rootnum`` is -1 and the nine values are NaN; a row that raises as
    a whole is redone point by point, so only the points that raise get -1."""
    from bs import cal_ky
    zwn = np.asarray(zwn, np.float64)
    freq = np.atleast_1d(np.asarray(freq, np.float64))
    nx, ny, nz = bs.nlon, bs.nlat, len(zwn)
    mwn, ug, vg = (np.full((nx, ny, nz, 3), np.nan) for _ in range(3))
    rootnum = np.full((nx, ny, nz), -1, np.int32)

    def solve(sel, j, iz, f):
        m, _ = cal_ky(f[0], f[1], f[2], f[3], freq, zwn[iz], iz=iz, mode="numpy")
        u, v = cal_ugvg_numpy(f[0], f[1], f[2], f[3], zwn[iz], m.T)
        mwn[sel, j, iz], ug[sel, j, iz], vg[sel, j, iz] = m, u.T, v.T
        rootnum[sel, j, iz] = (~np.isnan(m)).sum(axis=1)

    for j in range(ny):
        res = bs.cal_bs_mercator_point(bs.lon[:nx], np.full(nx, bs.lat[j]), mode="numpy")
        f = res[[0, 1, 6, 7]]
        for iz in range(nz):
            with np.errstate(all="ignore"):
                try:
                    solve(slice(None), j, iz, f)
                except np.linalg.LinAlgError:
                    for i in range(nx):
                        try:
                            solve(slice(i, i + 1), j, iz, f[:, i:i + 1])
                        except np.linalg.LinAlgError:
                            pass
    return mwn, ug, vg, rootnum


def _shifted(x, di, dj, cyclic):
    """``x[i + di, j + dj]``, zero outside (``i`` wraps when ``cyclic``)."""
    y = np.roll(x, (-di, -dj), axis=(0, 1))
    if di and not cyclic:
        y[-1 if di > 0 else 0] = 0
    if dj:
        y[:, -1 if dj > 0 else 0] = 0
    return y


def reference_fill(a, cyclic):
    """The NumPy definition of the map's NaN fill (``rwrt_wn_fill``,
    csrc/wn_fill.h) on ``a[nlon, nlat, ...]``: a non-NaN entry is kept; a NaN
    entry becomes ``acc / cnt`` over its eight neighbours in the same plane
    (``i +- 1`` wraps when ``cyclic`` and is skipped at the edge otherwise,
    ``j +- 1`` is skipped at the edge), read from ``a`` itself: ``acc`` adds the
    non-NaN neighbours (a NaN or skipped one adds +0.0) with ``di = -1, 0, 1``
    outer and ``dj = -1, 0, 1`` inner, ``cnt`` counts them (infinities count),
    and the entry stays NaN when ``cnt == 0``."""
    a = np.asarray(a, np.float64)
    nan = np.isnan(a)
    val = np.where(nan, 0.0, a)
    ok = (~nan).astype(np.int64)
    acc, cnt = np.zeros(a.shape), np.zeros(a.shape, np.int64)
    with np.errstate(all="ignore"):
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                if di or dj:
                    acc = acc + _shifted(val, di, dj, cyclic)
                    cnt = cnt + _shifted(ok, di, dj, cyclic)
        return np.where(nan & (cnt > 0), acc / cnt, a)


class WN:
    """The reference's wavenumber object (wn.py:21-135) with the map computed
    on the GPU: for every grid node and initial zonal wavenumber the meridional
    wavenumbers the dispersion relation admits (``mwn[nlon, nlat, nzwn, 3]``),
    how many there are (``rootnum[nlon, nlat, nzwn]``) and their group
    velocities (``ug, vg``).  An entry is what a ray launched at that node
    starts with (``RayEngine.wn_map``, ``reference_wn_map``); the arrays are
    device tensors, ``numpy()`` brings them to the host.

    Unlike the reference's scalar sketch, ``ug, vg`` are NaN (not 0.0) where a
    slot has no root, ``rootnum`` is -1 where ``np.roots`` would raise (the
    pole rows; ``n_bad`` counts them), and ``postprocess`` averages within one
    (k, root) plane only (``reference_fill``)."""

    def __init__(self, nx, ny, nzwn, freq=0.0):
        from bs import BS
        self.bs = BS(nx, ny)
        self.levels = None
        self.nzwn = nzwn
        self.freq = freq if freq is not None else 0.0
        self.zwn = np.zeros(nzwn, dtype=float)
        self.mwn = self.rootnum = self.ug = self.vg = self.n_bad = None
        self._info = self._engine = None

    @classmethod
    def from_bs(cls, bs, zwn, freq=0.0):
        """The map of a ready ``BS`` (``bs.ready`` was called)."""
        self = cls.__new__(cls)
        WN._setup(self, bs, None, zwn, freq)
        return self

    @classmethod
    def from_levels(cls, levels, zwn, freq=0.0):
        """The maps of a ``levels.Levels`` stack (fp64 storage): the arrays lead
        with a level axis."""
        self = cls.__new__(cls)
        WN._setup(self, None, levels, zwn, freq)
        return self

    def _setup(self, bs, levels, zwn, freq):
        self.bs, self.levels = bs, levels
        self.nzwn = len(zwn)
        self.freq = freq if freq is not None else 0.0
        self.zwn = np.array(zwn, dtype=float)
        self.mwn = self.rootnum = self.ug = self.vg = self.n_bad = None
        self._info = self._engine = None

    def set_zwn(self, zwn_array):
        if len(zwn_array) != self.nzwn:
            raise ValueError("Length of zwn_array must equal nzwn")
        self.zwn[:] = np.array(zwn_array, dtype=float)

    def set_freq(self, freq):
        self.freq = freq

    def engine(self):
        if self._engine is None:
            if self.levels is not None:
                from engine import RayEngine
                self._engine = RayEngine.from_levels(self.levels)
            else:
                if self.bs.fields is None:
                    raise ValueError("the basic state is not ready: call bs.ready() first")
                self._engine = self.bs.engine()
        return self._engine

    @property
    def axes(self):
        """``(lon, lat)`` of the map, radians."""
        src = self.levels if self.levels is not None else self.bs
        return np.asarray(src.lon, np.float64), np.asarray(src.lat, np.float64)

    def cal_wave(self, levels=None):
        """Fill ``mwn, rootnum, ug, vg`` on the device (``RayEngine.wn_map``).
        Nothing raises at the pole rows: their ``rootnum`` is -1 and ``n_bad``
        is their number.  ``levels``: a ``range`` of level indices of a
        ``from_levels`` map (default: every level)."""
        if self.levels is not None and levels is None:
            levels = range(self.levels.nlev)
        self.mwn, self.ug, self.vg, self.rootnum, self._info = self.engine().wn_map(
            self.zwn, self.freq, levels=levels)
        self.n_bad = int(self._info.item())
        return self

    def postprocess(self, cyclic=None):
        """Replace NaN entries of ``mwn, ug, vg`` by the mean of their non-NaN
        neighbours in the same (k, root) plane (``reference_fill``);
        ``rootnum`` stays as computed.  ``cyclic`` defaults to ``bs.xcyclic``
        (a ``Levels`` stack is cyclic)."""
        if self.mwn is None:
            raise ValueError("call cal_wave() first")
        if cyclic is None:
            cyclic = True if self.levels is not None else bool(self.bs.xcyclic)
        eng = self.engine()
        self.mwn, self.ug, self.vg = (eng.wn_fill(a, cyclic) for a in (self.mwn, self.ug, self.vg))
        return self

    def numpy(self):
        """Host arrays: ``lon, lat, zwn, mwn, ug, vg, rootnum``."""
        if self.mwn is None:
            raise ValueError("call cal_wave() first")
        lon, lat = self.axes
        d = dict(lon=lon, lat=lat, zwn=self.zwn.copy())
        for k in ("mwn", "ug", "vg", "rootnum"):
            d[k] = getattr(self, k).cpu().numpy()
        return d

    def output(self, ncfile):
        """Write the map (netCDF-3 or .npz by suffix): dims ``lon, lat, zwn,
        root`` (``level`` first for a levels map); NaN stays NaN."""
        import ncio
        d = self.numpy()
        lead = ("level",) if d["mwn"].ndim == 5 else ()
        dims = {"lon": len(d["lon"]), "lat": len(d["lat"]), "zwn": self.nzwn, "root": 3}
        if lead:
            dims = dict(level=d["mwn"].shape[0], **dims)
        node = lead + ("lon", "lat", "zwn")
        vars_ = {"lon": (("lon",), d["lon"], "radian"), "lat": (("lat",), d["lat"], "radian"),
                 "zwn": (("zwn",), d["zwn"]), "rootnum": (node, d["rootnum"])}
        for k in ("mwn", "ug", "vg"):
            vars_[k] = (node + ("root",), d[k])
        ncio.write(ncfile, dims, vars_, {"freq": float(np.atleast_1d(self.freq)[0])})

    def clean(self):
        if self.bs is not None:
            self.bs.clean()
        self.mwn = self.rootnum = self.ug = self.vg = self.n_bad = None
        self._info = self._engine = None
