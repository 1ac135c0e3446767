"""Inputs and references of the basic-state diagnostics tests."""
import numpy as np

import synthetic as S
from bsdiag import reference_diag
from conftest import golden

ALL = (1 << 23) - 1
_REF = {}


def fixture():
    """The reference fixture (read-only): inputs and ``planes[23, 24, 13]``."""
    if "z" not in _REF:
        z = golden("bsdiag_ref.npz")
        _REF["z"] = {k: np.array(z[k]) for k in z.files}
        for a in _REF["z"].values():
            a.setflags(write=False)
    return _REF["z"]


def axes(nlon, nlat):
    """Degree axes (float32) of an ``nlon x nlat`` grid, pole to pole."""
    lat = np.linspace(-90.0, 90.0, nlat).astype(np.float32)
    lon = (360.0 * np.arange(nlon) / nlon).astype(np.float32)
    return lat, lon


def inputs(kind, nlon, nlat):
    """``u, v, lat, lon`` of one of the test inputs: synthetic.py's zonal and
    non-zonal backgrounds on the grid, or the fixture's field (24 x 13 only)."""
    if kind == "fixture":
        z = fixture()
        assert (nlon, nlat) == (24, 13)
        return z["u"], z["v"], z["lat"], z["lon"]
    lat, lon = axes(nlon, nlat)
    bg = S.background_on(kind, lat, lon)
    return bg["u"], bg["v"], lat, lon


def reference_of(kind, nlon, nlat):
    """``reference_diag`` of a test input, computed once and shared (read-only)
    by the tests of this file and of tests/test_gpu_bsdiag.py."""
    key = (kind, nlon, nlat)
    if key not in _REF:
        u, v, lat, lon = inputs(kind, nlon, nlat)
        _REF[key] = reference_diag(u, v, lat, lon)
        _REF[key].setflags(write=False)
    return _REF[key]


def grid_steps(lat_deg, lon_deg):
    """``lat`` (radians), ``dx``, ``dy`` as ``BS`` builds them."""
    from bs import BS
    b = BS(len(lon_deg), len(lat_deg))
    z = np.zeros((len(lat_deg), len(lon_deg)), np.float32)
    b.load_arrays(z, z, lat_deg, lon_deg)
    return b.lat.copy(), float(b.dx[0]), float(b.dy[0])
