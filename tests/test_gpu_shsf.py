"""The spherical-harmonic filter on the GPU (``rwrt_sh_filter``, ``shsf.SHFilter``,
``SHSF``, ``Levels.set_level(..., trunc=)``, ``BS.load_arrays(..., trunc=)``)
against the NumPy definition ``shsf.reference_filter``.

The fp64 tolerance is the definition's own: 16 x its spread under the two
summation orders of the quadrature, relative to max |field|, measured on the
fields of each case (tests/test_shsf_host.py ``definition_tolerance``) -- not
a figure taken from the kernel.

The float32 output is held to the definition rounded to float32, except where
the definition's value lies within that tolerance of a float32 rounding
boundary (the midpoint of two neighbouring float32 numbers).  The premise of
this check, that the definition alone has fewer than 1 such point in 10 000,
was checked against the host definition first and does NOT hold on these
inputs: a point's chance of lying within the tolerance of a boundary is
tolerance / half-spacing, which is small only where the value is large.  The
filtered v is zero up to rounding at the poles and on its nodal meridians
(714 of 10 512 points on 73 x 144, and every point of its T = 0 mean): there
float32 is finer than the tolerance and every point is within it of a
boundary; and u falls smoothly to zero towards the poles (116 points of u at
T = 36 with a half-spacing of only 2 to 10 000 tolerances lie within the
tolerance of a boundary, for the definition alone).  So:
  * wherever the half-spacing exceeds twice the tolerance ("resolved"), a
    difference from the rounded definition is allowed only within the
    tolerance of a boundary -- asserted at every such point;
  * the count of 1 in 10 000 is asserted over the points whose half-spacing is
    at least 10 000 tolerances ("wide": a point's own chance is then under 1 in
    10 000), for the definition alone and for the kernel's differences;
  * at the unresolved points the float32 output is held to the fp64
    tolerance plus its own half-spacing."""
import numpy as np
import pytest
import torch

import _hip as H
import synthetic as S
from shsf import SHSF, SHFilter, reference_coefficients, reference_filter
from support.cases_shsf import case_fields, definition_tolerance, harmonic_field

pytestmark = pytest.mark.gpu

_REF = {}
CASES = {"19x36_T6": (19, 36, 6, 1), "73x144_T21": (73, 144, 21, 3), "73x144_T36": (73, 144, 36, 3),
         "73x144_T0": (73, 144, 0, 3)}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def case_inputs(name):
    """``(fields float32 [n, nlat, nlon], reference fp64, tolerance relative to
    max |field|)`` of a case, computed once; read-only.  The fields are u and
    v of the non-zonal synthetic background and the sum of the random harmonic
    fields (degrees up to nlat - 1 - T of the host cases), all different."""
    if name not in _REF:
        nlat, nlon, T, _ = CASES[name]
        bg = S.background("nonzonal", res=10.0 if nlat == 19 else 2.5)
        low, high = case_fields("small" if nlat == 19 else "mid")
        f = np.stack([bg["u"], bg["v"], (low + high).astype(np.float32)])
        assert f.shape == (3, nlat, nlon) and f.dtype == np.float32
        ref = reference_filter(f, T)
        tol, spread = definition_tolerance(list(f.astype(np.float64)), T)
        for a in (f, ref):
            a.setflags(write=False)
        _REF[name] = (f, ref, tol)
    return _REF[name]


def boundary_distance(r):
    """Distance of fp64 values from the nearest float32 rounding boundary (the
    midpoints between neighbouring float32 numbers), and the half-spacing."""
    with np.errstate(over="ignore"):
        r32 = r.astype(np.float32)
    up = (r32.astype(np.float64) + np.nextafter(r32, np.float32(np.inf)).astype(np.float64)) / 2
    dn = (r32.astype(np.float64) + np.nextafter(r32, np.float32(-np.inf)).astype(np.float64)) / 2
    return np.minimum(np.abs(r - up), np.abs(r - dn)), (up - dn) / 2


def check_float32(out32, ref, tol_abs, what):
    """``out32`` against the definition ``ref`` (fp64) rounded to float32."""
    dist, half = boundary_distance(ref)
    near = dist <= tol_abs
    resolved = half > 2.0 * tol_abs
    wide = half >= 1e4 * tol_abs
    miss = out32 != ref.astype(np.float32)
    n = ref.size
    print(f"{what}: {int(miss.sum())} of {n} float32 values differ from the rounded definition "
          f"({int((miss & wide).sum())} of them among the {int(wide.sum())} wide points); "
          f"{int((near & wide).sum())} wide points of the definition lie within the tolerance of a boundary; "
          f"{int((~resolved).sum())} points are not resolved by float32")
    assert not (miss & resolved & ~near).any(), what         # a difference only next to a boundary
    assert (near & wide).sum() * 10000 < n, what             # the definition alone: fewer than 1 in 10 000
    assert (miss & wide).sum() * 10000 < n, what             # ... and so the kernel's differences
    # where float32 is finer than the tolerance, the fp64 bound and the rounding of the output itself
    bad = ~resolved
    assert (np.abs(out32.astype(np.float64) - ref)[bad] <= (tol_abs + half)[bad]).all(), what


def run_case(name):
    nlat, nlon, T, nfield = CASES[name]
    f, ref, tol = case_inputs(name)
    flt = SHFilter(nlat, nlon, T)
    groups = [f] if nfield == 3 else [f[i:i + 1] for i in range(3)]
    o32 = np.concatenate([flt.filter_both(g)[0].cpu().numpy() for g in groups])
    o64 = np.concatenate([flt.filter_both(g)[1].cpu().numpy() for g in groups])
    return f, ref, tol, o32, o64


@pytest.mark.parametrize("name", list(CASES))
def test_filter_against_the_definition(name):
    nlat, nlon, T, nfield = CASES[name]
    f, ref, tol, o32, o64 = run_case(name)
    assert o64.dtype == np.float64 and o32.dtype == np.float32 and o64.shape == f.shape == o32.shape
    assert 0.0 < tol < 1e-13
    for i in range(3):
        scale = float(np.abs(f[i]).max())
        err = float(np.abs(o64[i] - ref[i]).max()) / scale
        print(f"{name} field {i}: |fp64 - definition| / max|f| = {err:.3g}, tolerance {tol:.3g}")
        assert err <= tol, (name, i, err, tol)
        # the float32 output is the fp64 output rounded ...
        assert same_bits(o32[i], o64[i].astype(np.float32))
        # ... and the definition rounded, except next to a rounding boundary
        check_float32(o32[i], ref[i], tol * scale, f"{name} field {i}")
    # different fields in each slot: a batch-stride slip would repeat one
    assert not same_bits(o64[0], o64[1]) and not same_bits(o64[1], o64[2])
    if T == 0:
        # the area mean, constant
        for i in range(3):
            assert np.ptp(o64[i]) <= tol * np.abs(f[i]).max()
        assert abs(o64[0].mean()) > 1.0                      # (u has a mean; v's is zero to rounding)


@pytest.mark.parametrize("shape", [(19, 3600, 6), (263, 12, 4), (19, 8, 6)])
def test_filter_other_paths(shape):
    """A row and its twiddles beyond the default LDS limit (19 x 3600); more
    latitudes than a block has threads (263); orders above nlon/2 - 1 dropped
    (19 x 8 with T = 6: M = 4)."""
    nlat, nlon, T = shape
    f = harmonic_field(nlat, nlon, 0, min(nlat - 1, 12), seed=7, mmax=min(T + 2, nlon // 2 - 1)).astype(np.float32)
    ref = reference_filter(f, T)
    tol, _ = definition_tolerance([f.astype(np.float64)], T)
    flt = SHFilter(nlat, nlon, T)
    out = flt.filter(f, torch.float64).cpu().numpy()
    err = float(np.abs(out - ref).max() / np.abs(f).max())
    print(f"{shape}: |fp64 - definition| / max|f| = {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol, (shape, err, tol)
    assert np.abs(out - f).max() > 1e-3 * np.abs(f).max()    # (something was filtered away)
    a = flt.coefficients(f).cpu().numpy()
    want = reference_coefficients(f, T)
    assert a.shape == want.shape == (T + 1, T + 1)
    assert np.abs(a - want).max() <= tol * np.abs(f).max() * nlon * np.sqrt(2.0)
    if nlon == 8:
        assert not a[:, 4:].any()


def test_coefficients_of_one_harmonic():
    """(l, m) = (5, 3) on 19 x 36, T = 6: one non-zero entry.  The float32
    input is the harmonic to 2^-24 max|f| per point, which moves a coefficient
    by at most 2^-24 max|f| nlon sqrt(2) (sum_j w_j |p_lm| <= sqrt 2)."""
    f = harmonic_field(19, 36, 5, 5, seed=9, orders=[3]).astype(np.float32)
    flt = SHFilter(19, 36, 6)
    a = flt.coefficients(f)
    assert a.is_cuda and a.dtype == torch.complex128 and a.shape == (7, 7)
    a = a.cpu().numpy()
    noise = 2.0 ** -24 * float(np.abs(f).max()) * 36 * np.sqrt(2.0)
    big = np.abs(a) > noise
    assert big.sum() == 1 and big[5, 3], np.argwhere(big)
    assert abs(a[5, 3]) > 1e5 * noise
    assert not a[np.triu_indices(7, 1)].any()                # exactly zero for l < m
    tol, _ = definition_tolerance([f.astype(np.float64)], 6)
    assert np.abs(a - reference_coefficients(f, 6)).max() <= tol * np.abs(f).max() * 36 * np.sqrt(2.0)
    # a leading batch axis
    assert flt.coefficients(np.stack([f, f])).shape == (2, 7, 7)


def test_determinism_and_batch():
    """Two calls give the same bits; one call with four fields gives the bits
    of four calls with one (no atomics, every sum has one order)."""
    f, _, _ = case_inputs("73x144_T21")
    f4 = np.concatenate([f, f[:1][:, ::-1].copy()])
    flt = SHFilter(73, 144, 21)
    dev = torch.as_tensor(f4, device=flt.device)
    a32, a64 = (t.cpu().numpy() for t in flt.filter_both(dev))
    b32, b64 = (t.cpu().numpy() for t in flt.filter_both(dev))
    assert same_bits(a32, b32) and same_bits(a64, b64)
    ca, cb = flt.coefficients(dev).cpu().numpy(), flt.coefficients(dev).cpu().numpy()
    assert same_bits(ca.view(np.float64), cb.view(np.float64))
    other = SHFilter(73, 144, 21)                            # (its own tables and scratch)
    for i in range(4):
        o32, o64 = (t.cpu().numpy() for t in other.filter_both(f4[i:i + 1]))
        assert same_bits(o32[0], a32[i]) and same_bits(o64[0], a64[i]), i
        assert same_bits(other.coefficients(f4[i]).cpu().numpy().view(np.float64), ca[i].view(np.float64)), i
    # the input is left as it was, and an empty batch is a no-op
    assert same_bits(dev.cpu().numpy(), f4)
    assert flt.filter(np.zeros((0, 73, 144), np.float32)).shape == (0, 73, 144)


def test_shsf_call_surface():
    """The reference's ``SHSF(data, truncation_level, sampling=2)``: 2-D or 3-D,
    the result on the input grid, ``sampling`` ignored."""
    f, ref, tol = case_inputs("73x144_T21")
    flt = SHFilter(73, 144, 21)
    want32 = flt.filter(f).cpu().numpy()
    got = SHSF(f[0], 21)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and same_bits(got, want32[0])
    assert same_bits(SHSF(f, 21, sampling=1), want32)
    wide = SHSF(f.astype(np.float64), 21)
    assert wide.dtype == np.float64 and same_bits(wide, flt.filter(f, torch.float64).cpu().numpy())
    t = SHSF(torch.as_tensor(f, device=flt.device), 21)
    assert t.is_cuda and t.dtype == torch.float32 and same_bits(t.cpu().numpy(), want32)
    with pytest.raises(ValueError):
        SHSF(f[0, 0], 21)
    with pytest.raises(ValueError):
        SHSF(f, 37)
    with pytest.raises(ValueError):
        flt.filter(f[:, :-1])


def packed_by_hand(lv, u, v, out):
    """The parent's ``Levels.set_level``: ``rwrt_bs_ready`` on ``u, v``."""
    u = torch.as_tensor(u, dtype=torch.float32).to(lv.device).contiguous()
    v = torch.as_tensor(v, dtype=torch.float32).to(lv.device).contiguous()
    H.check(H.load().rwrt_bs_ready(lv.nlon, lv.nlat, H.dptr(u), H.dptr(v), H.dptr(lv.trig), lv.dx, lv.dy,
                                   H.dptr(lv.scratch), out.data_ptr(), int(lv.fp32), H.stream(lv.device)))


@pytest.mark.parametrize("fp32", [False, True])
def test_levels(fp32):
    from levels import Levels
    bl = [S.background_level(j) for j in range(3)]
    u = np.stack([b["u"] for b in bl])
    v = np.stack([b["v"] for b in bl])
    flt = SHFilter(73, 144, 21)

    def levels():
        return Levels(bl[0]["lat"], bl[0]["lon"], 3, fp32=fp32)

    a, b, c, d = levels(), levels(), levels(), levels()
    for j in range(3):
        a.set_level(j, u[j], v[j], trunc=21)
        uf, vf = flt.filter(np.stack([u[j], v[j]]))
        b.set_level(j, uf, vf)
    c.set_levels(u, v, trunc=21)
    d.set_levels(torch.as_tensor(u, device=d.device), torch.as_tensor(v, device=d.device), trunc=21)
    pa = a.packed.cpu().numpy()
    assert same_bits(pa, b.packed.cpu().numpy())
    assert same_bits(pa, c.packed.cpu().numpy()) and same_bits(pa, d.packed.cpu().numpy())
    assert same_bits(a.level0_f64.cpu().numpy(), c.level0_f64.cpu().numpy())
    assert same_bits(a.level0_f64.cpu().numpy(), b.level0_f64.cpu().numpy())
    assert not same_bits(pa[0], pa[1])
    # trunc=None: the parent's behaviour, built both ways
    e, g = levels(), levels()
    hand = torch.empty_like(e.packed)
    for j in range(3):
        e.set_level(j, u[j], v[j])
        packed_by_hand(e, u[j], v[j], hand[j])
    g.set_levels(u, v)
    pe = e.packed.cpu().numpy()
    assert same_bits(pe, hand.cpu().numpy()) and same_bits(pe, g.packed.cpu().numpy())
    assert not same_bits(pe, pa)                             # (the filter changed the state)
    with pytest.raises(ValueError):
        g.set_levels(u[:2], v[:2])
    with pytest.raises(ValueError):
        g.set_level(0, u[0], v[0], trunc=37)
    # a grid that is not the definition's is refused by the filter, and only by it
    lat = np.linspace(-87.5, 87.5, 71).astype(np.float32)
    off = Levels(lat, bl[0]["lon"], 1)
    z = np.zeros((71, 144), np.float32)
    off.set_level(0, z, z)
    with pytest.raises(ValueError):
        off.set_level(0, z, z, trunc=10)


def test_end_to_end_rays():
    """``BS.load_arrays(..., trunc=21)`` -> ``ready`` -> an RK45 run of 10
    sources, 20 rows: the rows of the run on ``u, v`` filtered beforehand with
    ``SHSF()``.  A descending file is filtered in its own order."""
    from bs import BS
    from wr import WR
    bg = S.background("nonzonal")
    cfg = S.config("C2", nnx=5, nny=2, zwn=[4.0])
    nt = 20

    def run(bs):
        bs.ready(xcyclic=True)
        w = WR(cfg.nzwn, cfg.nsource, 7200.0, (nt - 1) * 7200.0, 0.0, nx=bs.nlon, ny=bs.nlat)
        w.bs = bs
        w.set_zwn(cfg.zwn)
        w.set_source_matrix(cfg.SW_lon, cfg.SW_lat, cfg.dlon, cfg.dlat, cfg.nnx, cfg.nny)
        with np.errstate(all="ignore"):
            w.ray_run(mode="hip", inte_method="rk45")
        return np.array([w.rlon, w.rlat, w.rzwn, w.rmwn, w.ramp, w.rug, w.rvg])

    one = BS(144, 73)
    one.load_arrays(**bg, trunc=21)
    two = BS(144, 73)
    two.load_arrays(SHSF(bg["u"], 21), SHSF(bg["v"], 21), bg["lat"], bg["lon"])
    assert same_bits(one.u, two.u) and same_bits(one.v, two.v) and one.u.dtype == np.float32
    rows1, rows2 = run(one), run(two)
    assert rows1.shape[1] == nt and same_bits(rows1, rows2)
    assert np.isfinite(rows1[0, -1]).any()                   # rays are alive at the last row
    plain = BS(144, 73)
    plain.load_arrays(**bg)
    assert not same_bits(plain.u, one.u)
    assert np.abs(plain.u - one.u).max() < 0.2 * np.abs(plain.u).max()
    # a descending file: filtered in its own order, then flipped as always
    desc = BS(144, 73)
    desc.load_arrays(bg["u"][::-1], bg["v"][::-1], bg["lat"][::-1], bg["lon"], trunc=21)
    want = SHSF(np.ascontiguousarray(bg["u"][::-1]), 21)[::-1]
    assert same_bits(desc.u, np.ascontiguousarray(want).T)
    f, ref, tol = case_inputs("73x144_T21")
    assert np.abs(desc.u.T.astype(np.float64) - ref[0]).max() <= tol * np.abs(f[0]).max() + 2.0 ** -24 * 64


def test_argument_errors_on_the_device():
    lib = H.load()
    dev = torch.device("cuda")
    f = torch.zeros((1, 19, 36), dtype=torch.float32, device=dev)
    o32, o64 = torch.zeros_like(f), torch.zeros((1, 19, 36), dtype=torch.float64, device=dev)
    w = torch.zeros(19, dtype=torch.float64, device=dev)
    x = torch.zeros((2, 19), dtype=torch.float64, device=dev)
    spec = torch.zeros((1, 7, 7, 2), dtype=torch.float64, device=dev)
    scratch = torch.zeros(2 * 7 * 19 * 2, dtype=torch.float64, device=dev)

    def call(nlon=36, nlat=19, nfield=1, trunc=6, d_in=f, out32=o32, out64=o64):
        return lib.rwrt_sh_filter(nlon, nlat, nfield, trunc, d_in.data_ptr(), w.data_ptr(), x.data_ptr(),
                                  spec.data_ptr(), None if out32 is None else out32.data_ptr(),
                                  None if out64 is None else out64.data_ptr(), scratch.data_ptr(), H.stream(dev))

    for kw, word in ((dict(nlat=18), b"nlat"), (dict(trunc=10), b"trunc"), (dict(out32=f), b"alias"),
                     (dict(out64=o32.view(torch.float64)[:, :, :1], out32=o32), b"alias"),
                     (dict(nlon=35), b"nlon"), (dict(nfield=-1), b"nfield")):
        assert call(**kw) == H.RWRT_ERR_ARG, kw
        assert word in lib.rwrt_last_error(), (kw, lib.rwrt_last_error())
    assert call(nfield=0) == H.RWRT_OK and call() == H.RWRT_OK
    assert call(out32=None, out64=None) == H.RWRT_OK         # coefficients only
    torch.cuda.synchronize()
    assert not o32.any() and not o64.any() and not spec.any()  # a zero field stays zero
