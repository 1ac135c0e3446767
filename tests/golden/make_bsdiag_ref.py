"""Generate tests/golden/bsdiag_ref.npz from the reference itself.

Run where the reference is available (``refharness.REF_DIR``):

    python tests/golden/make_bsdiag_ref.py

The fixture is DATA: float32 ``u, v`` on a 24 x 13 grid (15 degrees) with their
degree axes, and the 23 arrays the reference's ``BS.output`` would write
(bs.py:481-505) after ``BS.loadbs_ncfile`` + ``BS.ready(xcyclic=True)``
(bs.py:202-262, 318-407) on them, in ``BS.output``'s order -- ``planes[23,
nlon, nlat]`` float64 (``u, v`` widened).  The reference is imported with the
in-memory numba / netCDF4 stubs of ``refharness.py``.

The field: a sharp westerly jet at 45N and a weaker one at 45S, a wavenumber-3
perturbation in ``u`` and ``v``, and an easterly band in the tropics -- so the
interior ``KS`` has finite values and NaNs (easterlies, and ``betam <= 0`` on
the jets' flanks).  Both properties are asserted here and in the tests.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import refharness as H          # noqa: E402

NAMES = ("u", "v", "q", "ux", "uxx", "uy", "vx", "vxx", "vy", "qx", "qy", "qxx", "qxy",
         "qyx", "qyy", "qxxx", "qxxy", "qxyy", "qyyy", "qyxx", "qyyx", "betam", "KS")


def inputs():
    lat = np.arange(-90.0, 90.0 + 7.5, 15.0).astype(np.float32)      # 13
    lon = np.arange(0.0, 360.0, 15.0).astype(np.float32)             # 24
    phi = lat.astype(np.float64)[:, None]
    lam = np.deg2rad(lon.astype(np.float64))[None, :]
    c = np.cos(np.deg2rad(phi))
    jets = (60.0 * np.exp(-((phi - 45.0) / 9.0) ** 2) + 25.0 * np.exp(-((phi + 45.0) / 14.0) ** 2)
            - 9.0 * np.exp(-(phi / 12.0) ** 2))
    u = jets * (1.0 + 0.25 * np.cos(3.0 * lam + 0.4)) * np.ones_like(lam) + 1.5 * c * np.sin(3.0 * lam)
    v = 5.0 * np.sin(3.0 * lam - 0.7) * c ** 2 + 0.8 * np.cos(lam) * c
    return u.astype(np.float32), v.astype(np.float32), lat, lon


def main():
    R = H.load_reference()
    u, v, lat, lon = inputs()
    H.put_nc("bsdiag_ref.nc", u=u, v=v, lat=lat, lon=lon)
    bs = R.bs.BS(len(lon), len(lat))
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        bs.loadbs_ncfile("bsdiag_ref.nc")
        bs.ready(xcyclic=True)
    planes = np.stack([np.asarray(getattr(bs, n), np.float64) for n in NAMES])
    assert planes.shape == (23, 24, 13)
    ks, betam = planes[22, :, 1:-1], planes[21, :, 1:-1]
    assert np.isfinite(ks).any() and np.isnan(ks).any(), "interior KS needs finite values and NaNs"
    assert (betam <= 0).any(), "betam <= 0 must occur at an interior node: sharpen the jet"
    assert np.isnan(planes[21:, :, [0, -1]]).all()
    out = os.path.join(HERE, "bsdiag_ref.npz")
    np.savez_compressed(out, u=u, v=v, lat=lat, lon=lon, planes=planes, names=np.array(NAMES))
    print(f"{out}: {os.path.getsize(out)} bytes; interior KS finite {int(np.isfinite(ks).sum())}, "
          f"NaN {int(np.isnan(ks).sum())}; betam <= 0 at {int((betam <= 0).sum())} nodes, "
          f"u <= 0 at {int((planes[0, :, 1:-1] <= 0).sum())}")


if __name__ == "__main__":
    main()
