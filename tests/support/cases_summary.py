"""Regions, the C1 rows and the comparison of the summary tests."""
import math

import numpy as np

from conftest import golden
from support.bits import bitwise

INF, NAN = math.inf, math.nan


C1_BOX = (350.0, 20.0, 20.0, 60.0)       # across 0 degrees
REGIONS8 = [C1_BOX, (0.0, 360.0, -90.0, 90.0), (30.0, 120.0, -20.0, 40.0), (200.0, 100.0, -90.0, 0.0),
            (0.0, 180.0, 0.0, 90.0), (180.0, 360.0, 0.0, 90.0), (90.0, 90.0, -45.0, 45.0), (10.0, 11.0, 5.0, 6.0)]
FLOAT_FIELDS = ("lon_first", "lat_first", "lon_last", "lat_last", "l_last", "lat_min", "lat_max", "amp_max")
INT_FIELDS = ("n_valid", "last_row", "n_turn", "first_row", "rows_inside")
PATH_RTOL = 1e-12


def c1_rows():
    """The reference's C1 history as logical rows ``[3, 1081, 8]``."""
    hist = golden("traj_C1.npz")["hist"]              # (7, 1081, 3)
    rows = np.full((3, hist.shape[1], 8), NAN)
    rows[:, :, :7] = hist.transpose(2, 1, 0)
    return rows


def assert_summary(got, want, what=""):
    """Integer fields equal, selections bitwise, ``path`` within 1e-12 of
    ``want`` (and exactly 0 where ``want`` is 0)."""
    for k in INT_FIELDS:
        assert got[k].dtype.kind == "i" and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in FLOAT_FIELDS:
        assert bitwise(got[k], want[k]), (what, k)
    gp, wp = np.asarray(got["path"]), np.asarray(want["path"])
    assert gp.shape == wp.shape and np.isfinite(wp).all(), what
    err = np.abs(gp - wp)
    assert np.all(err <= PATH_RTOL * wp), (what, float(np.max(err / np.where(wp > 0, wp, 1.0))))
    assert np.all(gp[wp == 0.0] == 0.0), what
