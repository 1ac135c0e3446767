"""Analytic winds and the tolerance of the Helmholtz-decomposition tests.

The Rossby-Haurwitz wave of wavenumber ``R`` (a solid rotation plus one
harmonic of degree ``R + 1``) is non-divergent and has closed forms for ``u, v,
zeta, psi`` and the vorticity gradient; its divergent twin has a velocity
potential of the same shape as the wave's streamfunction, and closed forms for
``u_chi, v_chi, delta, chi``."""
import numpy as np

from constants import rearth
from helmholtz import PLANES, reference_helmholtz
from shsf import reference_nodes

# name: (nlat, nlon, R, T) -- 19 x 36 with T = 9 is the edge of the range, 19 x 8 cuts the orders at nlon/2 - 1
ANALYTIC = {"19x36_R4_T8": (19, 36, 4, 8), "19x36_R8_T9": (19, 36, 8, 9), "19x8_R2_T8": (19, 8, 2, 8),
            "73x144_R4_T21": (73, 144, 4, 21)}
OMEGA_RH = K_RH = 7.848e-6
D_TWIN = 3.0e-6
# which planes share a scale: the winds, and each pair of the issue's rule
SCALE_OF = {"u_rot": "wind", "v_rot": "wind", "u_div": "wind", "v_div": "wind", "vrt": "vrt", "div": "vrt",
            "psi": "psi", "chi": "psi", "vrt_x": "grad", "vrt_y": "grad"}
_CACHE = {}


def _grid(nlat, nlon, R):
    x, c = reference_nodes(nlat)
    ang = 2.0 * ((R * np.arange(nlon)) % nlon) / nlon         # (the argument of cos R lon reduced in integers)
    return x[:, None], c[:, None], np.cos(np.pi * ang)[None, :], np.sin(np.pi * ang)[None, :]


def zero_planes(nlat, nlon):
    return {name: np.zeros((nlat, nlon)) for name in PLANES}


def rossby_haurwitz(nlat, nlon, R):
    """The planes of the Rossby-Haurwitz wave (``u_rot, v_rot`` are its wind)."""
    s, c, cr, sr = _grid(nlat, nlon, R)
    a, w, K, n2 = rearth, OMEGA_RH, K_RH, R * R + 3 * R + 2
    out = zero_planes(nlat, nlon)
    out["u_rot"] = a * w * c + a * K * c ** (R - 1) * (R * s * s - c * c) * cr
    out["v_rot"] = -a * K * R * c ** (R - 1) * s * sr
    out["vrt"] = 2 * w * s - K * s * c ** R * n2 * cr
    out["psi"] = -a * a * w * s + a * a * K * c ** R * s * cr
    out["vrt_x"] = (K * s * c ** (R - 1) * n2 * R * sr) / a
    out["vrt_y"] = (2 * w * c - K * n2 * cr * (c ** (R + 1) - R * s * s * c ** (R - 1))) / a
    return out


def divergent_twin(nlat, nlon, R):
    """The planes of the twin: ``chi = a^2 D c^R s cos(R lon)``."""
    s, c, cr, sr = _grid(nlat, nlon, R)
    a, D, n2 = rearth, D_TWIN, R * R + 3 * R + 2
    out = zero_planes(nlat, nlon)
    out["u_div"] = -a * D * R * c ** (R - 1) * s * sr
    out["v_div"] = a * D * c ** (R - 1) * (c * c - R * s * s) * cr
    out["div"] = -D * s * c ** R * n2 * cr
    out["chi"] = a * a * D * c ** R * s * cr
    return out


def add_planes(A, B):
    return {name: A[name] + B[name] for name in PLANES}


def wind_of(P):
    return P["u_rot"] + P["u_div"], P["v_rot"] + P["v_div"]


def analytic_case(name):
    """``(rh, twin, both)`` closed-form plane dicts of a case, computed once; read-only."""
    if name not in _CACHE:
        nlat, nlon, R, _ = ANALYTIC[name]
        rh, twin = rossby_haurwitz(nlat, nlon, R), divergent_twin(nlat, nlon, R)
        both = add_planes(rh, twin)
        for d in (rh, twin, both):
            for a in d.values():
                a.setflags(write=False)
        _CACHE[name] = (rh, twin, both)
    return _CACHE[name]


def scales(planes, u, v):
    """The scale each plane's error is relative to: the maximum of the input
    wind for the four wind planes, and the maximum over the pair for ``vrt,
    div``, for ``psi, chi`` and for ``vrt_x, vrt_y`` (``planes``: a dict that
    holds the pairs, from the definition or closed forms)."""
    pair = {"wind": max(float(np.abs(u).max()), float(np.abs(v).max())),
            "vrt": max(float(np.abs(planes["vrt"]).max()), float(np.abs(planes["div"]).max())),
            "psi": max(float(np.abs(planes["psi"]).max()), float(np.abs(planes["chi"]).max())),
            "grad": max(float(np.abs(planes["vrt_x"]).max()), float(np.abs(planes["vrt_y"]).max()))}
    return {name: pair[SCALE_OF[name]] for name in PLANES}


def relative_errors(got, want, scale):
    return {name: float(np.abs(np.asarray(got[name]) - want[name]).max()) / scale[name] for name in PLANES}


def tolerances(spread):
    """DESIGN.md section 13's rule per plane: 16 x the definition's spread.  The
    planes that share a scale (the four wind planes; ``vrt, div``; ``psi, chi``;
    ``vrt_x, vrt_y``) share the tolerance, from the largest spread among them:
    they are sums of the same coefficients' rounding errors, measured against
    one scale, and the smaller plane of a pair (``div`` next to ``vrt``) has a
    spread of its own that says how small it is, not how well it is known."""
    return {name: 16.0 * max(s for other, s in spread.items() if SCALE_OF[other] == SCALE_OF[name])
            for name in PLANES}


def definition_spread(u, v, T, ref=None):
    """The definition's spread under the two summation orders of the quadrature
    on ``u, v``: ``(per plane, relative to the plane's scale; of the
    coefficients, relative to the largest |vrt_lm|, |div_lm|; the ascending
    result)``."""
    up = reference_helmholtz(u, v, T, "ascending") if ref is None else ref
    down = reference_helmholtz(u, v, T, "descending")
    sc = scales(up, u, v)
    per = relative_errors(down, up, sc)
    cmax = max(float(np.abs(up["vrt_lm"]).max()), float(np.abs(up["div_lm"]).max()))
    coef = max(float(np.abs(down["vrt_lm"] - up["vrt_lm"]).max()), float(np.abs(down["div_lm"] - up["div_lm"]).max()))
    return per, coef / cmax, up
