"""Backward ray tracing: the test-side definition and the fixture its tests share.

The oracle (oracle/rwrt_oracle.py) knows only ``direction = +1``.  The ray RHS
is autonomous and IEEE negation is exact and distributes over every sum and
product of the stepper, so the reference's loop with ``direction = -1`` is bit
for bit the forward integration of ``-f``: ``oracle_backward`` is the oracle's
own interval loop (``ray_run``: ``DP54``, the masks, ``ugvg_extent`` at the
row) run with ``fun = -rhs(bg, y)[0]``.  Row ``i`` is the state at time
``-t_eval[i]``; ``ug, vg`` of a row are the true group velocity there.
"""
import numpy as np

import rwrt_oracle as O
import synthetic as S

NT, TSTEP = 181, 7200.0
KINDS = ("zonal", "nonzonal")


def cfg():
    return S.config("C2", SW_lon=90, SW_lat=-10, dlon=25, dlat=25, nnx=4, nny=4, zwn=[1, 3, 5, 7])


def oracle_backward(bg, y0, nt, tstep, rtol=1e-6, atol=1e-6, msf=1e-3, cut_off=0.1, ttotal=None, row0=None,
                    keep=None):
    """``rwrt_oracle.ray_run`` with the negated RHS: ``(hist[7, nt, nray], nacc,
    nrej, status)``.  ``keep`` (a dict, if given) receives ``solver`` (the
    ``DP54`` after the last row: ``h_abs``, ``y``) and ``nacc_rows`` (the
    accepted-step counters after every interval, the rows' nacc column)."""
    forward, stepper = O.rhs, O.DP54

    def negated(bg_, y, t=None):
        d, bad = forward(bg_, y, t)
        return -d, bad

    class Kept(stepper):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            if keep is not None:
                keep["solver"], keep["nacc_rows"] = self, []

        def advance_to(self, t_bound):
            super().advance_to(t_bound)
            if keep is not None:
                keep["nacc_rows"].append(self.nacc.copy())

    O.rhs, O.DP54 = negated, Kept
    try:
        return O.ray_run(bg, np.array(y0, dtype=np.float64), nt, tstep, rtol=rtol, atol=atol, msf=msf,
                         cut_off=cut_off, ttotal=ttotal, row0=row0)
    finally:
        O.rhs, O.DP54 = forward, stepper


_BG, _ROW0 = {}, {}


def background(kind):
    if kind not in _BG:
        _BG[kind] = O.Background(**S.background(kind))
    return _BG[kind]


def sources():
    c = cfg()
    return O.source_matrix(c.SW_lon, c.SW_lat, c.dlon, c.dlat, c.nnx, c.nny)


def row0(kind):
    """The oracle's initial rows ``[7, 192]`` of the fixture on ``kind``."""
    if kind not in _ROW0:
        slon, slat = sources()
        with np.errstate(all="ignore"):
            r = np.array(O.ray_initial(background(kind), slon, slat, cfg().zwn, 0.0)).reshape(7, -1)
        r.setflags(write=False)
        _ROW0[kind] = r
    return _ROW0[kind]


def first_nan_row(lon_rows, nt):
    """The first row ``i >= 1`` of ``lon_rows[nt, nray]`` that is NaN, per ray (``nt``: none)."""
    bad = np.isnan(lon_rows[1:])
    return np.where(bad.any(axis=0), bad.argmax(axis=0) + 1, nt).astype(np.int32)
