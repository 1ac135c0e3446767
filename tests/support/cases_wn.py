"""Basic states, reference maps and fill planes of the wavenumber-map tests."""
import numpy as np

import synthetic as S
from support.bits import equal_nan
from wn import reference_wn_map

NAN, INF = np.nan, np.inf
ZWN = (1.0, 3.0, 5.0, 7.0)
_MAPS = {}


def bs_of(kind, xcyclic=True, res=2.5):
    from bs import BS
    bg = S.background(kind, res=res)
    bs = BS(len(bg["lon"]), len(bg["lat"]))
    bs.load_arrays(**bg)
    bs.ready(xcyclic=xcyclic)
    return bs


def reference_map(kind, zwn=ZWN, freq=0.0, xcyclic=True, res=2.5):
    """``reference_wn_map`` of a synthetic background, computed once and shared
    (read-only) by the tests of this file and of tests/test_gpu_wn.py."""
    key = (kind, tuple(zwn), float(freq), xcyclic, res)
    if key not in _MAPS:
        out = reference_wn_map(bs_of(kind, xcyclic, res), zwn, freq)
        for a in out:
            a.setflags(write=False)
        _MAPS[key] = out
    return _MAPS[key]


# ----------------------------------------------------------- the fill's planes
def fill_planes():
    """``[7, 5, 6]``: an isolated NaN; a 3 x 3 NaN block; NaNs on both longitude
    seams and both latitude edges; an inf neighbour; an all-NaN plane; a plane
    without NaN."""
    a = np.random.default_rng(11).standard_normal((7, 5, 6))
    a[3, 2, 0] = NAN
    a[2:5, 1:4, 1] = NAN
    for i, j in ((0, 2), (6, 2), (3, 0), (3, 4), (0, 0), (6, 4), (6, 0), (0, 3)):
        a[i, j, 2] = NAN
    a[3, 2, 3] = NAN
    a[2, 2, 3] = INF
    a[6, 1, 3] = NAN
    a[0, 0, 3] = -INF
    a[:, :, 4] = NAN
    a.setflags(write=False)
    return a


def check_filled_planes(a, got, cyclic):
    """What the planes of ``fill_planes`` must show, whoever filled them."""
    keep = ~np.isnan(a)
    assert equal_nan(got[keep], a[keep])                       # non-NaN entries are copied
    assert not np.isnan(got[3, 2, 0])                          # the isolated NaN is filled
    assert np.isnan(got[3, 2, 1])                              # the block's centre stays NaN
    assert not np.isnan(np.delete(got[2:5, 1:4, 1].ravel(), 4)).any()
    assert not np.isnan(got[:, :, 2]).any()
    assert got[3, 2, 3] == INF                                 # an infinite neighbour counts
    assert got[6, 1, 3] == (-INF if cyclic else got[6, 1, 3]) and not np.isnan(got[6, 1, 3])
    assert np.isnan(got[:, :, 4]).all()
    assert equal_nan(got[:, :, 5], a[:, :, 5])
