"""The Helmholtz decomposition and the Rossby-wave source, host side (no GPU):
the NumPy definition ``helmholtz.reference_helmholtz`` / ``reference_rws``
against closed forms (the Rossby-Haurwitz wave and its divergent twin), its
idempotence on the synthetic wind, csrc/sh_vector.h in a stand-alone program
under the sanitizers, the argument checks of ``rwrt_sh_helmholtz`` and
``rwrt_sh_rws`` and of the Python surface, and ``rws_sources``.

Against the closed forms the bound is 1e-12 of each quantity's scale (the
wind's maximum for the wind planes, the pair's maximum for ``vrt, div``, for
``psi, chi`` and for ``vrt_x, vrt_y``; ``S``: its own maximum): a wrong sign or
a missing ``m``, ``l (l+1)`` or ``a`` is an error of order 1 or 1/l.  Measured
(DESIGN.md section 26): at most 1.0e-14 (``vrt_y`` on 73 x 144), ``S`` at most
3.6e-15.

The idempotence tolerance is DESIGN.md section 13's rule: 16 times the
definition's own spread under the two summation orders of the quadrature,
measured on the test's own wind."""
import subprocess

import numpy as np
import pytest

import _hip as H
import helmholtz
import synthetic as S
from helmholtz import PLANES, reference_helmholtz, reference_rws, reference_vector_basis, rws_sources
from support import hostprog
from support.cases_helmholtz import (ANALYTIC, analytic_case, definition_spread, relative_errors, scales, tolerances,
                                     wind_of, zero_planes)

BOUND = 1e-12
_CACHE = {}


def decomposed(name, part):
    """The definition's planes of a part (``rh``, ``twin``, ``both``) of an analytic case, computed once."""
    key = (name, part)
    if key not in _CACHE:
        T = ANALYTIC[name][3]
        P = analytic_case(name)[("rh", "twin", "both").index(part)]
        _CACHE[key] = reference_helmholtz(*wind_of(P), T)
    return _CACHE[key]


# --------------------------------------------------------- against closed forms
@pytest.mark.parametrize("part", ["rh", "twin", "both"])
@pytest.mark.parametrize("name", list(ANALYTIC))
def test_definition_against_closed_forms(name, part):
    """Every plane of the wave, of the twin and of their sum: each part is
    recovered and the other part is zero, to 1e-12 of the plane's scale (the
    scales are those of the sum, so that a zero plane has one)."""
    rh, twin, both = analytic_case(name)
    want = dict(rh=rh, twin=twin, both=both)[part]
    got = decomposed(name, part)
    err = relative_errors(got, want, scales(both, *wind_of(both)))
    print(name, part, " ".join(f"{k} {e:.2g}" for k, e in err.items()))
    for plane, e in err.items():
        assert e <= BOUND, (name, part, plane, e)
    # the closed forms are not trivially small next to their scales
    if part == "both":
        sc = scales(both, *wind_of(both))
        for plane in PLANES:
            assert np.abs(both[plane]).max() > 1e-3 * sc[plane], plane
    # the coefficients: zero for l = 0, for l < m and for orders the longitude grid cannot carry
    nlon, T = ANALYTIC[name][1], ANALYTIC[name][3]
    M = min(T, nlon // 2 - 1) + 1
    for spec in (got["vrt_lm"], got["div_lm"]):
        assert spec.shape == (T + 1, T + 1) and not spec[0].any() and not spec[:, M:].any()
        assert not spec[np.triu_indices(T + 1, 1)].any()


@pytest.mark.parametrize("name", list(ANALYTIC))
def test_rossby_wave_source_against_closed_forms(name):
    """``S`` of the sum (wave + twin) from the definition's planes against ``S``
    from the closed-form planes, both the total source and the two terms of
    the linearised anomaly source (the twin as the anomaly)."""
    rh, twin, both = analytic_case(name)
    got, grh, gtw = decomposed(name, "both"), decomposed(name, "rh"), decomposed(name, "twin")
    pairs = {"total": (reference_rws(got, got), reference_rws(both, both)),
             "anomaly": (reference_rws(gtw, grh) + reference_rws(grh, gtw, planetary=False),
                         reference_rws(twin, rh) + reference_rws(rh, twin, planetary=False))}
    for label, (s, want) in pairs.items():
        err = float(np.abs(s - want).max() / np.abs(want).max())
        print(f"{name} {label}: |S - closed form| / max|S| = {err:.3g}")
        assert err <= BOUND, (name, label, err)
    # the planetary terms matter: without them the total source is another field
    flat = reference_rws(both, both, planetary=False)
    assert np.abs(flat - pairs["total"][1]).max() > 0.1 * np.abs(pairs["total"][1]).max()
    # a leading batch axis is carried
    st = {k: np.stack([both[k], rh[k]]) for k in PLANES}
    assert np.array_equal(reference_rws(st, st)[1], reference_rws(rh, rh))


# ------------------------------------------------------------------ idempotence
@pytest.mark.parametrize("T", [6, 9])
def test_idempotence_on_the_synthetic_wind(T):
    """Decomposing ``(u_rot + u_div, v_rot + v_div)`` returns the same parts,
    and decomposing ``(u_rot, v_rot)`` gives ``div_lm = 0``, within 16 x the
    definition's spread on the synthetic non-zonal wind (19 x 36)."""
    bg = S.background("nonzonal", res=10.0)
    u, v = bg["u"].astype(np.float64), bg["v"].astype(np.float64)
    spread, cspread, first = definition_spread(u, v, T)
    sc = scales(first, u, v)
    again = reference_helmholtz(first["u_rot"] + first["u_div"], first["v_rot"] + first["v_div"], T)
    err = relative_errors(again, first, sc)
    rot = reference_helmholtz(first["u_rot"], first["v_rot"], T)
    cmax = max(float(np.abs(first["vrt_lm"]).max()), float(np.abs(first["div_lm"]).max()))
    dleft = float(np.abs(rot["div_lm"]).max()) / cmax
    print(f"T {T}: spread " + " ".join(f"{k} {e:.2g}" for k, e in spread.items()) + f"; coefficients {cspread:.2g}")
    print(f"T {T}: again  " + " ".join(f"{k} {e:.2g}" for k, e in err.items()) + f"; div_lm left {dleft:.2g}")
    tol = tolerances(spread)
    for plane in PLANES:
        assert 0.0 < tol[plane] < 1e-13
        assert err[plane] <= tol[plane], (T, plane, err[plane], tol[plane])
    assert dleft <= 16.0 * cspread, (T, dleft, cspread)
    # the wind is not non-divergent to begin with, and the parts add up to the truncated wind
    assert np.abs(first["div_lm"]).max() > 1e-3 * cmax
    assert np.abs(first["u_div"]).max() > 1e-4 * sc["u_div"]


def test_definition_batch_axis_and_errors():
    rh, twin, both = analytic_case("19x36_R4_T8")
    u, v = wind_of(both)
    u2, v2 = np.stack([u, wind_of(rh)[0]]), np.stack([v, wind_of(rh)[1]])
    got = reference_helmholtz(u2, v2, 8)
    one, two = decomposed("19x36_R4_T8", "both"), decomposed("19x36_R4_T8", "rh")
    for k in PLANES + ("vrt_lm", "div_lm"):
        assert np.array_equal(got[k][0], one[k]) and np.array_equal(got[k][1], two[k]), k
    for bad_u, bad_v, T in ((u[:-1], v[:-1], 3), (u[:, :-1], v[:, :-1], 3), (u, v, 0), (u, v, 10), (u, v[:, ::2], 3)):
        with pytest.raises(ValueError):
            reference_helmholtz(bad_u, bad_v, T)
    with pytest.raises(ValueError):
        reference_helmholtz(u, v, 3, order="random")
    with pytest.raises(ValueError):
        reference_vector_basis(19, 10)


# ----------------------------------------------------- csrc/sh_vector.h on the host
def ulps(a, b):
    """Distance in units in the last place between two float64 arrays of one sign pattern."""
    ia = np.ascontiguousarray(a).view(np.int64).astype(object)
    ib = np.ascontiguousarray(b).view(np.int64).astype(object)
    return int(np.max(np.abs(ia - ib))) if ia.size else 0


def test_vector_basis_host_program_under_sanitizers(tmp_path):
    """csrc/sh_vector.h (what the kernels call) in a stand-alone program built
    with ASan + UBSan and run directly gives the definition's q_lm, b_lm, d_lm
    and the pointwise source to 4 ulp (expected: 0 -- the same operations in
    the same order)."""
    exe = hostprog.build("sh_vector", tmp_path, float_cast=False, no_warnings=True, word="sh_vector")
    for nlat, T in ((19, 6), (19, 9), (73, 21), (73, 36)):
        r = hostprog.run_process(exe, args=(str(nlat), str(T)))
        out = np.array([int(v, 16) for v in r.stdout.split()], np.uint64).view(np.float64)
        n1, n2 = T + 1, T + 2
        nq, nb = n2 * n2 * nlat, n1 * n1 * nlat
        assert out.size == nq + 2 * nb + 2 * nlat
        q, b, d = out[:nq].reshape(n2, n2, nlat), out[nq:nq + nb].reshape(n1, n1, nlat), \
            out[nq + nb:nq + 2 * nb].reshape(n1, n1, nlat)
        rq, rb, rd = reference_vector_basis(nlat, T)
        assert np.isfinite(out).all()                                     # the pole nodes included
        for got, want in ((q, rq), (b, rb), (d, rd)):
            assert np.array_equal(got == 0, want == 0)
            nz = want != 0
            assert np.array_equal(np.signbit(got[nz]), np.signbit(want[nz]))
        j = np.arange(nlat, dtype=np.float64)[:, None]
        A = dict(zero_planes(nlat, 1), div=1e-6 * (j + 1), u_div=2.0 + j, v_div=-3.0 + j)
        B = dict(zero_planes(nlat, 1), vrt=1e-5 * (j - 4), vrt_x=1e-11 * j, vrt_y=-2e-11 * (j + 2))
        want_s = np.concatenate([reference_rws(A, B, True)[:, 0], reference_rws(A, B, False)[:, 0]])
        dist = dict(q=ulps(np.abs(q), np.abs(rq)), b=ulps(np.abs(b), np.abs(rb)), d=ulps(np.abs(d), np.abs(rd)),
                    s=ulps(out[nq + 2 * nb:], want_s))
        print(f"nlat {nlat}, T {T}: largest differences in ulp {dist}")
        assert max(dist.values()) <= 4, dist
        # b and d at the poles: finite, and b_l1, d_l1 are the only non-zero ones there
        assert not b[:, 2:, 0].any() and not d[:, 2:, -1].any() and b[1:, 1, 0].all() and d[1:, 1, -1].all()
    # bad arguments end the program with status 2, nothing else
    for args in (("18", "3"), ("19", "10"), ("19", "0"), ("19",)):
        assert subprocess.run([exe, *args], capture_output=True, env=hostprog.sanitizer_env(),
                              timeout=60).returncode == 2


# --------------------------------------------------------------- argument errors
ALL = (1 << len(PLANES)) - 1
ROT = 0x30


def _helm(lib, nlon=36, nlat=19, npair=1, trunc=6, planes=ALL, u=1 << 20, v=2 << 20, w=64, x=128, spec=256,
          out64=3 << 20, rot32=4 << 20, scratch=512):
    """rwrt_sh_helmholtz with fake (never dereferenced) device pointers."""
    return H.entry("rwrt_sh_helmholtz")(nlon, nlat, npair, trunc, planes, u, v, w, x, spec, out64, rot32, scratch, None)


def _rws(lib, nlon=36, nlat=19, nfield=1, planetary=1, x=128, p=(1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20),
         out=7 << 20):
    return H.entry("rwrt_sh_rws")(nlon, nlat, nfield, planetary, x, *p, out, None)


def test_entry_points_argument_errors_without_a_gpu():
    """Every check happens before any HIP call, and the entry's name leads the message."""
    lib = H.load()
    assert "abi 5" in H.version()                      # additive members: the version stays
    npt = 19 * 36
    cases = [(dict(nlat=18), b"nlat"), (dict(nlat=1), b"nlat"), (dict(nlon=35), b"nlon"), (dict(nlon=0), b"nlon"),
             (dict(trunc=0), b"trunc"), (dict(trunc=-1), b"trunc"), (dict(trunc=10), b"trunc"),
             (dict(planes=0), b"empty"), (dict(planes=1 << 10), b"unknown"), (dict(planes=ALL | 0x8000), b"unknown"),
             (dict(npair=-1), b"npair"), (dict(npair=6554), b"npair"), (dict(npair=32768, planes=ROT), b"npair"),
             (dict(planes=0x10), b"d_rot32"), (dict(planes=0x2f), b"d_rot32"),
             (dict(out64=None), b"d_out64"), (dict(out64=None, planes=ROT | 1), b"d_out64"),
             (dict(v=1 << 20), b"alias"), (dict(out64=1 << 20), b"alias"), (dict(rot32=2 << 20), b"alias"),
             (dict(rot32=3 << 20), b"alias"),
             # partial overlaps: the last byte of one buffer is the first of another
             (dict(v=(1 << 20) + 4 * npt - 4), b"alias"), (dict(rot32=(3 << 20) + 80 * npt - 8), b"alias"),
             (dict(u=None), b"NULL"), (dict(v=None), b"NULL"), (dict(w=None), b"NULL"), (dict(x=None), b"NULL"),
             (dict(spec=None), b"NULL"), (dict(scratch=None), b"NULL"),
             (dict(nlon=20000, u=1 << 30, v=2 << 30, out64=3 << 30, rot32=None, planes=1), b"LDS")]
    for kw, word in cases:
        assert _helm(lib, **kw) == H.RWRT_ERR_ARG, kw
        msg = lib.rwrt_last_error()
        assert msg.startswith(b"rwrt_sh_helmholtz:") and word in msg, (kw, msg)
    # npair == 0 is a no-op whatever the pointers; adjacent buffers do not alias
    assert _helm(lib, npair=0, u=None, v=None, out64=None, rot32=None, spec=None, scratch=None) == H.RWRT_OK
    assert _helm(lib, npair=0, v=(1 << 20) + 4 * npt) == H.RWRT_OK
    cases = [(dict(nlat=18), b"nlat"), (dict(nlon=35), b"nlon"), (dict(nfield=-1), b"nfield"),
             (dict(nfield=65536), b"nfield"), (dict(planetary=2), b"planetary"), (dict(x=None), b"NULL"),
             (dict(out=None), b"NULL"), (dict(out=3 << 20), b"alias"), (dict(out=(6 << 20) + 8 * npt - 8), b"alias")]
    cases += [(dict(p=tuple(None if i == k else (i + 1) << 20 for i in range(6))), b"NULL") for k in range(6)]
    for kw, word in cases:
        assert _rws(lib, **kw) == H.RWRT_ERR_ARG, kw
        msg = lib.rwrt_last_error()
        assert msg.startswith(b"rwrt_sh_rws:") and word in msg, (kw, msg)
    assert _rws(lib, nfield=0, x=None, out=None) == H.RWRT_OK


def test_python_argument_errors_without_a_gpu():
    for nlat, nlon, T in ((18, 36, 3), (19, 35, 3), (19, 36, 10), (19, 36, 0), (19, 36, -1)):
        with pytest.raises(ValueError):
            helmholtz.Helmholtz(nlat, nlon, T)         # (sizes are checked before the device is asked for)
    for bad in ((), ("vorticity",), ("vrt", "u")):
        with pytest.raises(ValueError):
            helmholtz.plane_mask(bad)
    assert helmholtz.plane_mask(None) == (ALL, PLANES)
    assert helmholtz.plane_mask(("v_rot", "u_rot")) == (ROT, ("u_rot", "v_rot"))   # bit order, not the caller's
    assert helmholtz.plane_mask("vrt_y") == (0x200, ("vrt_y",))
    assert H.SHV_PLANES == PLANES


def test_levels_and_bs_reject_rotational_without_trunc():
    """``rotational=True`` needs ``trunc``: refused before a device is asked for."""
    from bs import BS
    from levels import Levels
    z = np.zeros((19, 36), np.float32)
    lat, lon = np.linspace(-90.0, 90.0, 19).astype(np.float32), np.arange(36) * 10.0
    b = BS(36, 19)
    with pytest.raises(ValueError, match="trunc"):
        b.load_arrays(z, z, lat, lon, rotational=True)
    with pytest.raises(ValueError, match="trunc"):
        b.load_arrays(z, z, rotational=True)
    # ... and a grid that is not the definition's is refused as the filter refuses it
    with pytest.raises(ValueError):
        BS(36, 19).load_arrays(z, z, np.linspace(-80.0, 80.0, 19), lon, trunc=3, rotational=True)
    with pytest.raises(ValueError):
        b.load_arrays(z, z, lat, lon, trunc=10, rotational=True)
    lv = Levels.__new__(Levels)                        # (no device: the check comes first)
    with pytest.raises(ValueError, match="trunc"):
        lv.set_level(0, z, z, rotational=True)
    with pytest.raises(ValueError, match="trunc"):
        lv.set_levels(z[None], z[None], rotational=True)
    # rotational=False without trunc is the path as it was: no device, the same arrays
    b.load_arrays(z + 1.0, z, lat, lon, rotational=False)
    assert np.array_equal(b.u, (z + 1.0).T)


# ------------------------------------------------------------------- rws_sources
def test_rws_sources_on_a_hand_made_field():
    lat = np.linspace(-90.0, 90.0, 19)
    lon = np.arange(36) * 10.0
    Sf = np.zeros((19, 36))

    def put(lo, la, val):
        Sf[int(round((la + 90) / 10)), int(round((lo % 360) / 10))] = val

    put(350, 30, 9.0)
    put(0, 30, -8.0)       # 10 degrees of longitude from the first at 30N: 8.65 degrees of great circle
    put(20, 40, 7.0)
    put(180, 0, -10.0)     # the largest, outside the box below
    put(10, -20, 6.0)
    put(340, 50, -5.0)
    lo, la, val = rws_sources(Sf, lat, lon, 3)
    assert list(val) == [-10.0, 9.0, -8.0] and list(lo) == [180.0, 350.0, 0.0] and list(la) == [0.0, 30.0, 30.0]
    # a box across 0 degrees, edges included
    box = (340.0, 20.0, -20.0, 50.0)
    lo, la, val = rws_sources(Sf, lat, lon, 10, box=box)
    assert list(val[:5]) == [9.0, -8.0, 7.0, 6.0, -5.0] and len(val) == 10 and not val[5:].any()
    assert ((lo >= 340.0) | (lo <= 20.0)).all() and ((la >= -20.0) & (la <= 50.0)).all()
    lo2, la2, val2 = rws_sources(Sf, lat, lon, 10, box=(-20.0, 20.0, -20.0, 50.0))      # the same box
    assert np.array_equal(val2, val) and np.array_equal(lo2, lo)
    # thinning: the node 8.65 degrees from the first is dropped at 9 degrees, kept at 8
    lo, la, val = rws_sources(Sf, lat, lon, 4, box=box, min_sep_deg=9.0)
    assert list(val) == [9.0, 7.0, 6.0, -5.0]
    assert list(rws_sources(Sf, lat, lon, 4, box=box, min_sep_deg=8.0)[2]) == [9.0, -8.0, 7.0, 6.0]
    # one sign only: fewer than n when there are no more
    lo, la, val = rws_sources(Sf, lat, lon, 5, sign=-1)
    assert list(val) == [-10.0, -8.0, -5.0]
    assert list(rws_sources(Sf, lat, lon, 2, sign=+1, box=box)[2]) == [9.0, 7.0]
    # thinning that uses the first candidates up (the 64 largest lie in one patch 28 degrees across) still finds n
    lat73, lon144 = np.linspace(-90.0, 90.0, 73), np.arange(144) * 2.5
    patch = np.ones((73, 144))
    patch[32:41, 0:9] = 2.0 + np.arange(81).reshape(9, 9) * 1e-3
    lo, la, val = rws_sources(patch, lat73, lon144, 2, min_sep_deg=40.0)
    assert list(val) == [patch.max(), 1.0] and helmholtz._separation_deg(lo[0], la[0], lo[1], la[1]) >= 40.0
    # NaN is never a source, and every pair taken is apart
    dense = np.full((19, 36), 1.0)
    dense[9, :] = 2.0 + np.arange(36) * 1e-3
    dense[0, 0] = np.nan
    lo, la, val = rws_sources(dense, lat, lon, 12, min_sep_deg=25.0)
    assert len(val) == 12 and np.isfinite(val).all()
    for i in range(12):
        for k in range(i):
            assert helmholtz._separation_deg(lo[i], la[i], lo[k], la[k]) >= 25.0
    import torch
    assert np.array_equal(rws_sources(torch.as_tensor(Sf), lat, lon, 3)[2], [-10.0, 9.0, -8.0])
    assert len(rws_sources(Sf, lat, lon, 0)[2]) == 0
    for kw in (dict(n=-1), dict(n=3, sign=2), dict(n=3, min_sep_deg=-1.0), dict(n=3, box=(0, 10, 50, 20))):
        with pytest.raises(ValueError):
            rws_sources(Sf, lat, lon, **kw)
    with pytest.raises(ValueError):
        rws_sources(Sf[:-1], lat, lon, 3)
