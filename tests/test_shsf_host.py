"""The spherical-harmonic filter, host side (no GPU): the NumPy definition
``shsf.reference_weights`` / ``reference_filter`` against exact quadrature and
against fields built from scipy's spherical harmonics (independent of the
definition's recurrence), csrc/shsf_legendre.h in a stand-alone program under
the sanitizers, and the argument checks of ``rwrt_sh_filter`` and of the
Python surface.

The tolerance of the filter tests is not a figure taken from any
implementation: it is 16 times the definition's own spread under two summation
orders of the quadrature (latitudes ascending and descending), relative to
max|field|, measured on the test's own fields (``definition_tolerance``).
Measured: spread 2.7e-16 (19 x 36, T = 6) and 4.7e-16 (73 x 144, T = 21), so
tolerances 4.3e-15 and 7.5e-15."""
import subprocess

import numpy as np
import pytest

import _hip as H
import shsf
from shsf import reference_filter, reference_legendre, reference_nodes, reference_weights
from support import hostprog
from support.cases_shsf import CASES, case_fields, definition_tolerance, harmonic_field

_CACHE = {}

# ------------------------------------------------------------------ the weights
@pytest.mark.parametrize("nlat", [3, 19, 73, 721])
def test_weights_sum_to_two(nlat):
    """To 1e-15 relative (math.fsum: the weights' own sum, not the rounding of adding them up)."""
    import math
    w = reference_weights(nlat)
    assert w.shape == (nlat,) and (w > 0).all()
    err = abs(math.fsum(w) - 2.0) / 2.0
    print(f"nlat {nlat}: |sum w - 2| / 2 = {err:.3g}")
    assert err <= 1e-15
    assert np.abs(w - w[::-1]).max() <= 1e-15 * w.max()          # symmetric about the equator, to rounding


@pytest.mark.parametrize("nlat", [19, 73])
def test_weights_integrate_even_powers_exactly(nlat):
    w = reference_weights(nlat)
    x, c = reference_nodes(nlat)
    assert x[0] == -1.0 and x[-1] == 1.0 and c[0] == 0.0 and c[-1] == 0.0 and x[nlat // 2] == 0.0
    worst = 0.0
    for d in range(0, nlat, 2):
        exact = 2.0 / (d + 1)
        err = abs(float(np.sum(w * x ** d)) - exact) / exact
        worst = max(worst, err)
        assert err <= 1e-13, (d, err)
    print(f"nlat {nlat}: largest relative quadrature error of x^d, even d <= {nlat - 1}: {worst:.3g}")
    # the first degree past the rule's range is not integrated exactly on the small grid
    if nlat == 19:
        d = nlat + 1
        assert abs(float(np.sum(w * x ** d)) - 2.0 / (d + 1)) > 1e-10


def test_legendre_functions_are_orthonormal():
    nlat, T = 73, 21
    w = reference_weights(nlat)
    p = reference_legendre(nlat, T)
    for m in (0, 1, 5, 21):
        gram = np.einsum("aj,bj,j->ab", p[m:, m], p[m:, m], w)
        assert np.abs(gram - np.eye(T + 1 - m)).max() < 1e-13, m
    assert not p[3, 5].any()


# ------------------------------------------------------------------- the filter
def filter_case(case):
    """Everything the four properties need, computed once per case."""
    key = ("filter", case)
    if key not in _CACHE:
        nlat, nlon, T = CASES[case]
        low, high = case_fields(case)
        both = low + high
        tol, spread = definition_tolerance([low, high, both], T)
        _CACHE[key] = dict(T=T, low=low, high=high, both=both, tol=tol, spread=spread,
                           got_low=reference_filter(low, T), got_high=reference_filter(high, T),
                           got_both=reference_filter(both, T))
    return _CACHE[key]


@pytest.mark.parametrize("prop", ["a", "b", "c", "d"])
@pytest.mark.parametrize("case", ["small", "mid"])
def test_filter_on_harmonic_fields(case, prop):
    """(a) a field of degrees <= T is reproduced; (b) one of degrees T < l <=
    nlat - 1 - T is annihilated; (c) the filter is idempotent on their sum;
    (d) sectoral harmonics l = m > T (dropped by degree or by order alike) are
    annihilated.  Errors relative to max |field|, tolerance 16 x the spread.

    Measured (small; mid): spread 2.7e-16; 4.7e-16, tolerance 4.3e-15; 7.5e-15,
    (a) 1.6e-15; 5.0e-15, (b) 5.9e-16; 3.3e-15, (c) 4.8e-16; 1.9e-15,
    (d) 1.4e-16; 2.0e-16.

    (a) on 73 x 144 is what the recurrence's ``x q`` through the pole distance
    is for (``shsf.reference_legendre``): with the plain product ``x * q`` it is
    1.3e-14, above the tolerance, all of it in the three rows next to each
    pole."""
    nlat, nlon, T = CASES[case]
    d = filter_case(case)
    tol = d["tol"]
    assert 0.0 < tol < 1e-13                             # the tolerance is rounding, not a loose bound
    if prop == "a":
        err = np.abs(d["got_low"] - d["low"]).max() / np.abs(d["low"]).max()
    elif prop == "b":
        err = np.abs(d["got_high"]).max() / np.abs(d["high"]).max()
    elif prop == "c":
        err = np.abs(reference_filter(d["got_both"], T) - d["got_both"]).max() / np.abs(d["both"]).max()
        # ... and what is left of the sum is its low part
        assert np.abs(d["got_both"] - d["low"]).max() / np.abs(d["both"]).max() <= tol
    else:
        sect = harmonic_field(nlat, nlon, T + 1, nlon // 2 - 1, seed=3, sectoral=True)
        assert np.abs(sect).max() > 0.1
        err = np.abs(reference_filter(sect, T)).max() / np.abs(sect).max()
    print(f"{case} ({prop}): spread {d['spread']:.3g}, tolerance {tol:.3g}, error {err:.3g}")
    assert err <= tol, (case, prop, err, tol)


def test_filter_batch_axis_and_coefficients():
    d = filter_case("small")
    T = d["T"]
    stack = np.stack([d["low"], d["high"], d["both"]])
    assert np.array_equal(reference_filter(stack, T), np.stack([d["got_low"], d["got_high"], d["got_both"]]))
    a = shsf.reference_coefficients(d["low"], T)
    assert a.shape == (T + 1, T + 1) and not a[np.triu_indices(T + 1, 1)].any()
    assert shsf.reference_coefficients(stack, T).shape == (3, T + 1, T + 1)


def test_filter_edges():
    nlat, nlon = 19, 36
    low, high = case_fields("small")
    f = low + high
    # T = 0: the area mean, constant
    w = reference_weights(nlat)
    mean = float(np.sum(w[:, None] * f) / (2.0 * nlon))
    out = reference_filter(f, 0)
    assert np.abs(out - mean).max() <= 1e-14 * np.abs(f).max()
    # T = (nlat - 1) / 2, the upper edge: degrees <= 9 pass, the rest up to nlat - 1 - T = 9: nothing to drop
    top = harmonic_field(nlat, nlon, 0, 9, seed=4)
    assert np.abs(reference_filter(top, 9) - top).max() <= 1e-13 * np.abs(top).max()
    # nlon / 2 - 1 < T: orders the longitude grid cannot carry are dropped, zero coefficients
    a = shsf.reference_coefficients(harmonic_field(19, 8, 0, 3, seed=5, mmax=3), 6)
    assert a.shape == (7, 7) and not a[:, 4:].any() and a[:, :4].any()


# ------------------------------------------ csrc/shsf_legendre.h on the host
def ulps(a, b):
    """Distance in units in the last place between two float64 arrays of one sign pattern."""
    ia = np.ascontiguousarray(a).view(np.int64).astype(object)
    ib = np.ascontiguousarray(b).view(np.int64).astype(object)
    return int(np.max(np.abs(ia - ib))) if ia.size else 0


def test_legendre_host_program_under_sanitizers(tmp_path):
    """csrc/shsf_legendre.h (what the kernels call) in a stand-alone program
    built with ASan + UBSan and run directly gives the definition's weights,
    nodes and p_lm to 4 ulp (measured: 0 -- the same operations in the same
    order, sin and cos from the same C library)."""
    exe = hostprog.build("shsf_legendre", tmp_path, float_cast=False, no_warnings=True, word="shsf")
    for nlat, T in ((19, 6), (19, 9), (73, 21), (73, 36), (3, 0), (3, 1)):
        r = hostprog.run_process(exe, args=(str(nlat), str(T)))
        out = np.array([int(v, 16) for v in r.stdout.split()], np.uint64).view(np.float64)
        n1 = T + 1
        assert out.size == 3 * nlat + n1 * n1 * nlat
        w, x, c = out[:nlat], out[nlat:2 * nlat], out[2 * nlat:3 * nlat]
        p = out[3 * nlat:].reshape(n1, n1, nlat)
        rx, rc = reference_nodes(nlat)
        rp = reference_legendre(nlat, T)
        assert np.array_equal(np.signbit(p), np.signbit(rp)) and np.array_equal(p == 0, rp == 0)
        d = dict(w=ulps(w, reference_weights(nlat)), x=ulps(x, rx), c=ulps(c, rc), p=ulps(p, rp))
        print(f"nlat {nlat}, T {T}: largest differences in ulp {d}")
        assert max(d.values()) <= 4, d
    # bad arguments end the program with status 2, nothing else
    for args in (("18", "3"), ("19", "10"), ("19", "-1"), ("19",)):
        assert subprocess.run([exe, *args], capture_output=True, env=hostprog.sanitizer_env(),
                              timeout=60).returncode == 2


# --------------------------------------------------------------- argument errors
def _filter(lib, nlon=36, nlat=19, nfield=1, trunc=6, d_in=1 << 20, w=64, x=128, spec=256, out32=2 << 20,
            out64=3 << 20, scratch=512):
    """rwrt_sh_filter with fake (never dereferenced) device pointers."""
    return lib.rwrt_sh_filter(nlon, nlat, nfield, trunc, d_in, w, x, spec, out32, out64, scratch, None)


def test_sh_filter_argument_errors_without_a_gpu():
    """Every check happens before any HIP call."""
    lib = H.load()
    assert "abi 5" in H.version()                      # an additive member: the version stays
    npt = 19 * 36
    cases = [(dict(nlat=18), b"nlat"), (dict(nlat=1), b"nlat"), (dict(nlon=35), b"nlon"), (dict(nlon=0), b"nlon"),
             (dict(trunc=-1), b"trunc"), (dict(trunc=10), b"trunc"), (dict(nfield=-1), b"nfield"),
             (dict(nfield=65536), b"nfield"),
             (dict(out32=1 << 20), b"alias"), (dict(out64=1 << 20), b"alias"), (dict(out64=2 << 20), b"alias"),
             # partial overlaps: the last byte of one buffer is the first of another
             (dict(out32=(1 << 20) + 4 * npt - 4), b"alias"), (dict(out64=(2 << 20) - 8 * npt + 8), b"alias"),
             (dict(nfield=2, out32=(1 << 20) + 4 * npt), b"alias"),
             (dict(d_in=None), b"NULL"), (dict(w=None), b"NULL"), (dict(x=None), b"NULL"), (dict(spec=None), b"NULL"),
             (dict(scratch=None), b"NULL"),
             (dict(nlon=20000, nlat=19, d_in=1 << 30, out32=2 << 30, out64=3 << 30), b"LDS")]
    for kw, word in cases:
        assert _filter(lib, **kw) == H.RWRT_ERR_ARG, kw
        assert word in lib.rwrt_last_error(), (kw, lib.rwrt_last_error())
    # adjacent buffers do not alias; nfield == 0 is a no-op whatever the pointers
    assert _filter(lib, nfield=0, d_in=None, out32=None, out64=None, spec=None, scratch=None) == H.RWRT_OK
    assert _filter(lib, nfield=0, d_in=64, out32=64, out64=64) == H.RWRT_OK


def test_python_argument_errors_without_a_gpu():
    f = np.zeros((19, 36))
    for bad, T in ((np.zeros((18, 36)), 3), (np.zeros((19, 35)), 3), (f, 10), (f, -1), (np.zeros((1, 4)), 0)):
        with pytest.raises(ValueError):
            reference_filter(bad, T)
    with pytest.raises(ValueError):
        reference_filter(f, 3, order="random")
    for nlat, nlon, T in ((18, 36, 3), (19, 35, 3), (19, 36, 10), (19, 36, -1)):
        with pytest.raises(ValueError):
            shsf.SHFilter(nlat, nlon, T)               # (sizes are checked before the device is asked for)
    # the grid check: pole to pole within float32 rounding, ascending or descending
    lat = np.linspace(-90.0, 90.0, 19).astype(np.float32)
    shsf.check_grid(19, 36, lat)
    shsf.check_grid(19, 36, lat[::-1])
    shsf.check_grid(19, 36, None)
    shsf.check_grid(721, 1440, np.arange(-90.0, 90.125, 0.25).astype(np.float32))
    for nlat, nlon, bad in ((18, 36, None), (19, 35, None), (19, 36, lat[:-1]), (19, 36, lat * 0.98),
                            (19, 36, np.linspace(-80.0, 80.0, 19)), (19, 36, lat + np.float32(1e-3)),
                            (19, 36, np.rad2deg(np.arcsin(np.linspace(-1, 1, 19))))):
        with pytest.raises(ValueError):
            shsf.check_grid(nlat, nlon, bad)
    # BS.load_arrays(trunc=...) refuses a grid that is not the definition's before it asks for a device
    from bs import BS
    b = BS(36, 18)
    with pytest.raises(ValueError):
        b.load_arrays(np.zeros((18, 36), np.float32), np.zeros((18, 36), np.float32),
                      np.linspace(-85.0, 85.0, 18), np.arange(36) * 10.0, trunc=3)
    b = BS(36, 19)
    with pytest.raises(ValueError):
        b.load_arrays(np.zeros((19, 36), np.float32), np.zeros((19, 36), np.float32),
                      np.linspace(-80.0, 80.0, 19), np.arange(36) * 10.0, trunc=3)
    with pytest.raises(ValueError):
        b.load_arrays(np.zeros((19, 36), np.float32), np.zeros((19, 36), np.float32), lat, np.arange(36) * 10.0,
                      trunc=10)
