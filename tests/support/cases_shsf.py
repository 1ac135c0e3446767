"""Harmonic fields and the tolerance of the spherical-harmonic filter tests."""
import numpy as np
from scipy.special import sph_harm_y

from shsf import reference_filter, reference_nodes


CASES = {"small": (19, 36, 6), "mid": (73, 144, 21)}
_CACHE = {}


def harmonic_field(nlat, nlon, lmin, lmax, seed, mmax=None, sectoral=False, orders=None):
    """A real field on the ideal grid: random harmonics of degree
    ``lmin..lmax`` (orders ``0..min(l, mmax)``; ``sectoral``: ``m = l`` only;
    ``orders``: these ``m`` only), from ``scipy.special.sph_harm_y``."""
    rng = np.random.default_rng(seed)
    # The nodes are the ideal ones.  A colatitude next to pi cannot hold its distance from the
    # pole (an angle off by 4e-16 moves a degree-l harmonic by l * 4e-16), so every row is
    # evaluated at its distance from the nearer pole, min(j, n - j) pi / n, the southern ones
    # with the parity (-1)^(l+m); the longitude factor exp(i m lon_i) has its argument reduced
    # in integers for the same reason.
    x, c = reference_nodes(nlat)
    n = nlat - 1
    theta = np.minimum(np.arange(nlat), n - np.arange(nlat)) * np.pi / n
    south = x < 0
    i = np.arange(nlon)
    f = np.zeros((nlat, nlon))
    for l in range(lmin, lmax + 1):
        for m in ([l] if sectoral else orders if orders is not None
                  else range(0, min(l, l if mmax is None else mmax) + 1)):
            coef = rng.standard_normal() + 1j * rng.standard_normal()
            y = sph_harm_y(l, m, theta, 0.0).real
            y = np.where(south, (-1.0) ** (l + m) * y, y)
            ang = 2.0 * ((m * i) % nlon) / nlon
            f += (coef * y[:, None] * (np.cos(np.pi * ang) + 1j * np.sin(np.pi * ang))[None, :]).real
    return f


def case_fields(case):
    """``(low, high)`` of a case, computed once: degrees ``<= T`` and degrees
    ``T < l <= nlat - 1 - T``; read-only."""
    if case not in _CACHE:
        nlat, nlon, T = CASES[case]
        low = harmonic_field(nlat, nlon, 0, T, seed=1)
        high = harmonic_field(nlat, nlon, T + 1, nlat - 1 - T, seed=2)
        for a in (low, high):
            a.setflags(write=False)
        _CACHE[case] = (low, high)
    return _CACHE[case]


def relative_spread(fields, T):
    """The definition's spread under the two summation orders over ``fields``,
    relative to each field's max |f|: the largest."""
    worst = 0.0
    for f in fields:
        scale = float(np.abs(f).max())
        if scale == 0.0:
            continue
        d = np.abs(reference_filter(f, T, "ascending") - reference_filter(f, T, "descending")).max()
        worst = max(worst, float(d) / scale)
    return worst


def definition_tolerance(fields, T):
    """16 x the spread: ``(tolerance, spread)``, both relative to max |field|."""
    s = relative_spread(fields, T)
    assert s > 0.0
    return 16.0 * s, s
