"""The Helmholtz decomposition and the Rossby-wave source on the GPU
(``rwrt_sh_helmholtz``, ``rwrt_sh_rws``, ``helmholtz.Helmholtz``, the
``rotational=`` hooks of ``Levels`` and ``BS``) against the NumPy definition
``helmholtz.reference_helmholtz`` / ``reference_rws``.

The tolerance is DESIGN.md section 13's rule, the definition's own: 16 x its
spread under the two summation orders of the quadrature, measured on each
pair's own (float32) inputs, relative to the scales of
``support.cases_helmholtz.scales`` -- the input wind's maximum for the four
wind planes, the pair's maximum for ``vrt, div``, for ``psi, chi`` and for
``vrt_x, vrt_y`` (``tolerances``: planes that share a scale share the
tolerance), the largest coefficient for ``d_spec``, and ``S``'s own maximum.
Nothing is taken from the kernel.

Each case has two pairs in one batch: ``u, v`` of the synthetic non-zonal
background, and the analytic wave plus its divergent twin rounded to
float32."""
import numpy as np
import pytest
import torch

import _hip as H
import synthetic as S
from helmholtz import PLANES, Helmholtz, reference_helmholtz, reference_rws, rws_sources
from support.cases_helmholtz import (add_planes, definition_spread, divergent_twin, relative_errors, rossby_haurwitz,
                                     scales, tolerances, wind_of)

pytestmark = pytest.mark.gpu

# name: (nlat, nlon, T, R of the analytic pair)
CASES = {"19x36_T6": (19, 36, 6, 4), "19x36_T9": (19, 36, 9, 8), "19x8_T6": (19, 8, 6, 2),
         "73x144_T21": (73, 144, 21, 4)}
_REF = {}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def axes(nlat, nlon):
    return (np.linspace(-90.0, 90.0, nlat).astype(np.float32),
            (np.arange(nlon) * (360.0 / nlon)).astype(np.float32))


def case_inputs(name):
    """``u, v`` float32 ``[2, nlat, nlon]`` of a case and, per pair, the
    definition's planes, the spreads and the tolerances; computed once,
    read-only."""
    if name not in _REF:
        nlat, nlon, T, R = CASES[name]
        bg = S.background_on("nonzonal", *axes(nlat, nlon))
        ua, va = wind_of(add_planes(rossby_haurwitz(nlat, nlon, R), divergent_twin(nlat, nlon, R)))
        u = np.stack([bg["u"], ua.astype(np.float32)])
        v = np.stack([bg["v"], va.astype(np.float32)])
        pairs = []
        for i in range(2):
            u64, v64 = u[i].astype(np.float64), v[i].astype(np.float64)
            up = reference_helmholtz(u64, v64, T, "ascending")
            down = reference_helmholtz(u64, v64, T, "descending")
            spread, cspread, _ = definition_spread(u64, v64, T, ref=up)
            s_up, s_down = reference_rws(up, up), reference_rws(down, down)
            pairs.append(dict(ref=up, down=down, scale=scales(up, u64, v64), tol=tolerances(spread), spread=spread,
                              ctol=16.0 * cspread, cspread=cspread, S=s_up,
                              stol=16.0 * float(np.abs(s_up - s_down).max() / np.abs(s_up).max())))
        for a in (u, v):
            a.setflags(write=False)
        _REF[name] = (u, v, pairs)
    return _REF[name]


def run(h, u, v, planes=None, rot32=False):
    return {k: t.cpu().numpy() for k, t in h.decompose(u, v, planes=planes, rot32=rot32).items()}


@pytest.mark.parametrize("name", list(CASES))
def test_decomposition_against_the_definition(name):
    nlat, nlon, T, _ = CASES[name]
    u, v, pairs = case_inputs(name)
    h = Helmholtz(nlat, nlon, T)
    got = run(h, u, v, rot32=True)
    vrt_lm, div_lm = (t.cpu().numpy() for t in h.coefficients(u, v))
    assert vrt_lm.shape == div_lm.shape == (2, T + 1, T + 1) and vrt_lm.dtype == np.complex128
    M = min(T, nlon // 2 - 1) + 1
    for i, p in enumerate(pairs):
        err = relative_errors({k: got[k][i] for k in PLANES}, p["ref"], p["scale"])
        print(f"{name} pair {i}: spread    " + " ".join(f"{k} {p['spread'][k]:.2g}" for k in PLANES))
        print(f"{name} pair {i}: |kernel - definition| " + " ".join(f"{k} {err[k]:.2g}" for k in PLANES))
        cmax = max(float(np.abs(p["ref"]["vrt_lm"]).max()), float(np.abs(p["ref"]["div_lm"]).max()))
        cerr = max(float(np.abs(vrt_lm[i] - p["ref"]["vrt_lm"]).max()),
                   float(np.abs(div_lm[i] - p["ref"]["div_lm"]).max())) / cmax
        print(f"{name} pair {i}: coefficients: spread {p['cspread']:.2g}, |kernel - definition| {cerr:.2g}")
        for k in PLANES:
            assert got[k].dtype == np.float64 and got[k].shape == (2, nlat, nlon)
            assert 0.0 < p["tol"][k] < 1e-13                 # the tolerance is rounding, not a loose bound
            assert err[k] <= p["tol"][k], (name, i, k, err[k], p["tol"][k])
        assert 0.0 < p["ctol"] < 1e-13 and cerr <= p["ctol"], (name, i, cerr, p["ctol"])
        for spec in (vrt_lm[i], div_lm[i]):
            # exactly zero: l = 0, l < m, and the orders the longitude grid cannot carry
            assert not spec[0].any() and not spec[np.triu_indices(T + 1, 1)].any() and not spec[:, M:].any()
        # d_rot32 is the fp64 pair rounded, bit for bit
        assert got["rot32"].dtype == np.float32 and got["rot32"].shape == (2, 2, nlat, nlon)
        assert same_bits(got["rot32"][i, 0], got["u_rot"][i].astype(np.float32))
        assert same_bits(got["rot32"][i, 1], got["v_rot"][i].astype(np.float32))
    # different pairs in each slot: a batch-stride slip would repeat one
    assert not same_bits(got["u_rot"][0], got["u_rot"][1])
    # the analytic pair's parts are what they were built from (to float32 rounding of the input)
    R = CASES[name][3]
    rh, tw = rossby_haurwitz(nlat, nlon, R), divergent_twin(nlat, nlon, R)
    wind = pairs[1]["scale"]["u_rot"]
    for k, want in (("u_rot", rh["u_rot"]), ("v_rot", rh["v_rot"]), ("u_div", tw["u_div"]), ("v_div", tw["v_div"])):
        assert np.abs(got[k][1] - want).max() <= 1e-5 * wind, k


def test_subsets_determinism_and_batch():
    """A mask subset gives the bits of the full mask; two calls give the same
    bits; a pair's result does not depend on its batch (1 pair against 3);
    ``rotational`` is the ``u_rot, v_rot`` of ``decompose`` in both dtypes."""
    name = "73x144_T21"
    nlat, nlon, T, _ = CASES[name]
    u, v, _ = case_inputs(name)
    u3, v3 = np.concatenate([u, u[:1, :, ::-1]]), np.concatenate([v, -v[:1, :, ::-1]])
    h = Helmholtz(nlat, nlon, T)
    du, dv = torch.as_tensor(u3, device=h.device), torch.as_tensor(v3, device=h.device)
    full = run(h, du, dv, rot32=True)
    again = run(h, du, dv, rot32=True)
    for k in full:
        assert same_bits(full[k], again[k]), k
    for subset in (("vrt",), ("u_rot", "v_rot"), ("v_rot",), ("div", "u_div", "v_div", "vrt", "vrt_x", "vrt_y"),
                   ("chi", "vrt_y"), ("psi", "u_rot", "v_rot", "vrt_x")):
        rot = "u_rot" in subset and "v_rot" in subset
        part = run(h, du, dv, planes=subset, rot32=rot)
        assert set(part) == set(subset) | ({"rot32"} if rot else set())
        for k in part:
            assert same_bits(part[k], full[k]), (subset, k)
    other = Helmholtz(nlat, nlon, T)                         # (its own scratch)
    ca = [t.cpu().numpy() for t in h.coefficients(du, dv)]
    for i in range(3):
        one = run(other, u3[i], v3[i], rot32=True)
        for k in full:
            assert one[k].shape == full[k].shape[1:] and same_bits(one[k], full[k][i]), (i, k)
        cb = [t.cpu().numpy() for t in other.coefficients(u3[i], v3[i])]
        assert same_bits(cb[0].view(np.float64), ca[0][i].view(np.float64))
        assert same_bits(cb[1].view(np.float64), ca[1][i].view(np.float64))
    r32 = [t.cpu().numpy() for t in h.rotational(du, dv)]
    r64 = [t.cpu().numpy() for t in h.rotational(du, dv, out_dtype=torch.float64)]
    assert same_bits(r32[0], full["rot32"][:, 0]) and same_bits(r32[1], full["rot32"][:, 1])
    assert same_bits(r64[0], full["u_rot"]) and same_bits(r64[1], full["v_rot"])
    # the inputs are left as they were, and an empty batch is a no-op
    assert same_bits(du.cpu().numpy(), u3) and same_bits(dv.cpu().numpy(), v3)
    z = np.zeros((0, nlat, nlon), np.float32)
    assert h.decompose(z, z)["vrt"].shape == (0, nlat, nlon)
    with pytest.raises(ValueError):
        h.decompose(u3, v3[:2])
    with pytest.raises(ValueError):
        h.decompose(u3[:, :-1], v3[:, :-1])
    with pytest.raises(ValueError):
        h.rotational(du, dv, out_dtype=torch.float16)


@pytest.mark.parametrize("pair", [0, 1], ids=["synthetic", "analytic"])
@pytest.mark.parametrize("name", ["19x36_T6", "19x8_T6", "73x144_T21"])
def test_rossby_wave_source(name, pair):
    """``rws`` against ``reference_rws`` on the definition's planes, 16 x the
    spread of ``S`` between the two summation orders, relative to max ``|S|``.

    73x144_T21-synthetic is the case that shows the forward transform's
    twiddles: 4.8e-15 against a tolerance of 1.3e-14 with the definition's own
    (``cos(pi * ang)``, the product rounded, ``shv_forward_dft_kernel``), 2.8e-14
    with ``sincospi(ang)`` -- the spread does not see the twiddles (both
    orders share them), the analysis multiplies the transform's rounding by
    ``m`` (``b_lm = m q_lm``) and ``S`` multiplies the divergence by ``f``
    (DESIGN.md section 26)."""
    nlat, nlon, T, _ = CASES[name]
    u, v, pairs = case_inputs(name)
    p = pairs[pair]
    s = Helmholtz(nlat, nlon, T).rws(u, v)
    assert s.is_cuda and s.dtype == torch.float64 and s.shape == (2, nlat, nlon)
    s = s.cpu().numpy()
    err = float(np.abs(s[pair] - p["S"]).max() / np.abs(p["S"]).max())
    print(f"{name} pair {pair}: S: tolerance {p['stol']:.2g}, |kernel - definition| / max|S| = {err:.2g}")
    assert 0.0 < p["stol"] < 1e-12 and err <= p["stol"], (name, pair, err, p["stol"])


@pytest.mark.parametrize("name", ["19x36_T6", "19x8_T6", "73x144_T21"])
def test_rossby_wave_source_of_an_anomaly(name):
    """``rws_anomaly`` (the synthetic wind as the climatology, the analytic pair
    as the anomaly) against the two ``reference_rws`` terms, by the same rule;
    and ``rws`` of one field without a batch axis."""
    nlat, nlon, T, _ = CASES[name]
    u, v, pairs = case_inputs(name)
    h = Helmholtz(nlat, nlon, T)
    clim, anom = pairs[0], pairs[1]
    want = reference_rws(anom["ref"], clim["ref"]) + reference_rws(clim["ref"], anom["ref"], planetary=False)
    down = reference_rws(anom["down"], clim["down"]) + reference_rws(clim["down"], anom["down"], planetary=False)
    tol = 16.0 * float(np.abs(want - down).max() / np.abs(want).max())
    got = h.rws_anomaly(u[0], v[0], u[1], v[1]).cpu().numpy()
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{name}: anomaly S: tolerance {tol:.2g}, |kernel - definition| / max|S| = {err:.2g}")
    assert got.shape == (nlat, nlon) and 0.0 < tol < 1e-12 and err <= tol, (name, err, tol)
    assert same_bits(h.rws(u[1], v[1]).cpu().numpy(), h.rws(u, v).cpu().numpy()[1])


def packed_of(lv):
    return lv.packed.cpu().numpy(), lv.level0_f64.cpu().numpy()


@pytest.mark.parametrize("fp32", [False, True])
def test_levels_rotational(fp32):
    """``set_levels(u, v, trunc=T, rotational=True)`` packs the levels of
    ``set_levels(u_rot32, v_rot32)``, bit for bit, as ``set_level`` does level
    by level; ``rotational=False`` gives the bits of the call without it."""
    from levels import Levels
    T = 21
    bl = [S.background_level(j) for j in range(2)]
    u = np.stack([b["u"] for b in bl])
    v = np.stack([b["v"] for b in bl]) + np.float32(0.5) * np.stack([b["u"] for b in bl])[:, :, ::-1]
    v = np.ascontiguousarray(v)

    def levels():
        return Levels(bl[0]["lat"], bl[0]["lon"], 2, fp32=fp32)

    h = Helmholtz(73, 144, T)
    ur, vr = h.rotational(u, v)
    assert ur.dtype == torch.float32 and ur.shape == (2, 73, 144)
    a, b, c = levels(), levels(), levels()
    a.set_levels(u, v, trunc=T, rotational=True)
    b.set_levels(ur, vr)
    for j in range(2):
        c.set_level(j, u[j], v[j], trunc=T, rotational=True)
    for x, y in zip(packed_of(a), packed_of(b)):
        assert same_bits(x, y)
    for x, y in zip(packed_of(a), packed_of(c)):
        assert same_bits(x, y)
    # rotational=False: the filter's path and the plain path as they were
    d, e, f, g = levels(), levels(), levels(), levels()
    d.set_levels(u, v, trunc=T, rotational=False)
    e.set_levels(u, v, trunc=T)
    f.set_levels(u, v, rotational=False)
    g.set_levels(u, v)
    assert same_bits(packed_of(d)[0], packed_of(e)[0]) and same_bits(packed_of(f)[0], packed_of(g)[0])
    # the three states differ: this wind has a divergent part
    assert not same_bits(packed_of(a)[0], packed_of(e)[0]) and not same_bits(packed_of(e)[0], packed_of(g)[0])
    with pytest.raises(ValueError):
        a.set_levels(u, v, trunc=37, rotational=True)


def test_bs_rotational_and_descending_latitude():
    """``BS.load_arrays(..., trunc=T, rotational=True)`` holds ``u_rot32,
    v_rot32``; a descending-latitude input equals the ascending one under the
    flip (the decomposition sees ascending latitude either way)."""
    from bs import BS
    T = 21
    bg = S.background("nonzonal")
    u, v = bg["u"], np.ascontiguousarray(bg["v"] + np.float32(0.3) * bg["u"][:, ::-1])
    ur, vr = (t.cpu().numpy() for t in Helmholtz(73, 144, T).rotational(u, v))
    asc = BS(144, 73)
    asc.load_arrays(u, v, bg["lat"], bg["lon"], trunc=T, rotational=True)
    assert asc.u.dtype == np.float32 and same_bits(asc.u, ur.T) and same_bits(asc.v, vr.T)
    desc = BS(144, 73)
    desc.load_arrays(u[::-1], v[::-1], bg["lat"][::-1], bg["lon"], trunc=T, rotational=True)
    # (the reference's rule flips a descending file's winds and keeps its axis)
    assert same_bits(np.ascontiguousarray(desc.u), np.ascontiguousarray(asc.u))
    assert same_bits(np.ascontiguousarray(desc.v), np.ascontiguousarray(asc.v))
    assert desc.lat[0] > desc.lat[-1]
    # rotational=False: the bits of the call without the argument, with and without trunc
    for kw in (dict(), dict(trunc=T)):
        one, two = BS(144, 73), BS(144, 73)
        one.load_arrays(u, v, bg["lat"], bg["lon"], rotational=False, **kw)
        two.load_arrays(u, v, bg["lat"], bg["lon"], **kw)
        assert same_bits(np.ascontiguousarray(one.u), np.ascontiguousarray(two.u))
        assert same_bits(np.ascontiguousarray(one.v), np.ascontiguousarray(two.v))
    assert not same_bits(np.ascontiguousarray(two.v), np.ascontiguousarray(asc.v))


def test_rays_from_rws_sources_on_a_rotational_state():
    """The plumbing end to end on 19 x 36: the rotational state into ``BS``,
    sources from ``rws_sources`` on the device's ``S``, a few rows of ``WR``;
    rows are finite where ``amp`` is."""
    from bs import BS
    from wr import WR
    nlat, nlon, T = 19, 36, 9
    lat, lon = axes(nlat, nlon)
    bg = S.background_on("nonzonal", lat, lon)
    src = Helmholtz(nlat, nlon, T).rws(bg["u"], bg["v"])
    slon, slat, sval = rws_sources(src, lat, lon, 6, box=(300.0, 200.0, -60.0, 60.0), min_sep_deg=15.0)
    assert len(sval) == 6 and np.abs(sval).min() > 0.0 and (np.abs(slat) <= 60.0).all()
    bs = BS(nlon, nlat)
    bs.load_arrays(bg["u"], bg["v"], lat, lon, trunc=T, rotational=True)
    bs.ready(xcyclic=True)
    nt = 6
    w = WR(1, 6, 7200.0, (nt - 1) * 7200.0, 0.0, nx=nlon, ny=nlat)
    w.bs = bs
    w.set_zwn([3.0])
    w.set_source_array(slon, slat)
    with np.errstate(all="ignore"):
        w.ray_run(mode="hip", inte_method="rk45")
    rows = np.array([w.rlon, w.rlat, w.rzwn, w.rmwn, w.ramp, w.rug, w.rvg]).reshape(7, nt, -1)
    alive = np.isfinite(rows[4])
    assert rows.shape[2] >= 6 and alive[0].any()
    for k in range(7):
        assert np.isfinite(rows[k][alive]).all(), k


def test_argument_errors_on_the_device():
    lib = H.load()
    dev = torch.device("cuda")
    u = torch.zeros((1, 19, 36), dtype=torch.float32, device=dev)
    v = torch.zeros_like(u)
    out = torch.zeros((1, 10, 19, 36), dtype=torch.float64, device=dev)
    r32 = torch.zeros((1, 2, 19, 36), dtype=torch.float32, device=dev)
    w = torch.zeros(19, dtype=torch.float64, device=dev)
    x = torch.zeros((2, 19), dtype=torch.float64, device=dev)
    spec = torch.ones((1, 2, 7, 7, 2), dtype=torch.float64, device=dev)
    scratch = torch.zeros(14 * 7 * 19 * 2, dtype=torch.float64, device=dev)

    def call(nlon=36, nlat=19, npair=1, trunc=6, planes=0x3ff, d_u=u, d_v=v, out64=out, rot32=r32):
        return H.entry("rwrt_sh_helmholtz")(nlon, nlat, npair, trunc, planes, d_u.data_ptr(), d_v.data_ptr(), w.data_ptr(),
                                     x.data_ptr(), spec.data_ptr(), None if out64 is None else out64.data_ptr(),
                                     None if rot32 is None else rot32.data_ptr(), scratch.data_ptr(), H.stream(dev))

    for kw, word in ((dict(nlat=18), b"nlat"), (dict(trunc=0), b"trunc"), (dict(trunc=10), b"trunc"),
                     (dict(planes=0), b"empty"), (dict(planes=0x400), b"unknown"), (dict(d_v=u), b"alias"),
                     (dict(rot32=u), b"alias"), (dict(planes=0x0f), b"d_rot32"), (dict(out64=None), b"d_out64"),
                     (dict(nlon=35), b"nlon"), (dict(npair=-1), b"npair")):
        assert call(**kw) == H.RWRT_ERR_ARG, kw
        assert word in lib.rwrt_last_error(), (kw, lib.rwrt_last_error())
    assert call(npair=0) == H.RWRT_OK and call() == H.RWRT_OK
    assert call(out64=None, rot32=None) == H.RWRT_OK         # coefficients only
    assert call(planes=0x30, out64=None) == H.RWRT_OK        # nothing but the float32 pair
    torch.cuda.synchronize()
    assert not out.any() and not r32.any() and not spec.any()  # a zero wind stays zero
