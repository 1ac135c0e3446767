"""Basic-state diagnostics on the GPU (``rwrt_bs_diag``, ``bsdiag.BSDiag``):
every plane bit for bit (NaN for NaN) the reference's ``BS.output`` array on
the fixture, the NumPy definition ``bsdiag.reference_diag`` on every grid and
input, and ``rwrt_bs_ready``'s packed record on the planes both compute.

Grids ``(nlon, nlat)``: (3, 4) the smallest accepted; (8, 5) where smth9's
interior is small but not empty; (24, 13) the fixture; (70, 37) ragged against
a 32 x 32 tile in both directions (3 x 2 tiles, the halo crossing tile borders
and the longitude seam inside the last, partial tile)."""
import numpy as np
import pytest
import torch

import _hip as H
from bsdiag import DIAG_NAMES, NEEDS_Q, BSDiag, reference_diag
from support.bits import bitwise as same_bits
from support.cases_bsdiag import ALL, axes, fixture, grid_steps, inputs, reference_of

pytestmark = pytest.mark.gpu

GRIDS = [(3, 4), (8, 5), (24, 13), (70, 37)]
CASES = [(k, nx, ny) for nx, ny in GRIDS for k in ("zonal", "nonzonal")] + [("fixture", 24, 13)]
BK = (1 << 21) | (1 << 22)
SENTINEL = -777.25
_DIAG = {}


def diag_of(kind, nlon, nlat):
    """One ``BSDiag`` per grid (the fixture's axes are the 24 x 13 grid's)."""
    _, _, lat, lon = inputs(kind, nlon, nlat)
    key = (nlon, nlat, lat.tobytes(), lon.tobytes())
    if key not in _DIAG:
        _DIAG[key] = BSDiag(lat, lon)
    return _DIAG[key]


def assert_planes(got, want, names=DIAG_NAMES, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for k, n in enumerate(names):
        assert same_bits(got[k], want[k]), (what, n)


def three_levels(nlon, nlat):
    """Three distinct levels ``u, v[3, nlat, nlon]`` and their definition."""
    lat, lon = axes(nlon, nlat)
    kinds = ("nonzonal", "zonal", "superrotation")
    from synthetic import background_on
    bg = [background_on(k, lat, lon) for k in kinds]
    u, v = np.stack([b["u"] for b in bg]), np.stack([b["v"] for b in bg])
    v[2] = 0.5 * bg[0]["v"][:, ::-1]
    want = np.stack([reference_diag(u[k], v[k], lat, lon) for k in range(3)])
    return u, v, lat, lon, want


_THREE = {}


def three(nlon=70, nlat=37):
    if (nlon, nlat) not in _THREE:
        _THREE[(nlon, nlat)] = three_levels(nlon, nlat)
    return _THREE[(nlon, nlat)]


def raw_call(d, u, v, select, scratch=True, scratch_levels=1, pad=64):
    """``rwrt_bs_diag`` called directly into an output buffer over-allocated by
    ``pad`` doubles of a sentinel; returns ``(planes[nlev, nsel, nlon, nlat],
    the pad)`` on the host."""
    u = torch.as_tensor(np.ascontiguousarray(u), device=d.device)
    v = torch.as_tensor(np.ascontiguousarray(v), device=d.device)
    nlev, nsel, n = u.shape[0], bin(select).count("1"), d.nlon * d.nlat
    out = torch.full((nlev * nsel * n + pad,), SENTINEL, dtype=torch.float64, device=d.device)
    sc = torch.empty(4 * n * scratch_levels, dtype=torch.float64, device=d.device) if scratch else None
    H.check(H.load().rwrt_bs_diag(d.nlon, d.nlat, nlev, H.dptr(u), H.dptr(v), H.dptr(d.trig), d.dx, d.dy, select,
                                  H.dptr(out), H.dptr(sc), scratch_levels, H.stream(d.device)))
    out = out.cpu().numpy()
    return out[:nlev * nsel * n].reshape(nlev, nsel, d.nlon, d.nlat), out[nlev * nsel * n:]


# (a) ------------------------------------------------------------ the reference
def test_all_planes_equal_the_reference_fixture():
    z = fixture()
    ks = z["planes"][22][:, 1:-1]
    assert np.isfinite(ks).any() and np.isnan(ks).any() and (z["planes"][21][:, 1:-1] <= 0).any()
    got = BSDiag(z["lat"], z["lon"]).compute(z["u"], z["v"])
    assert got.shape == (1, 23, 24, 13) and got.dtype == torch.float64 and got.is_cuda
    assert_planes(got[0].cpu().numpy(), z["planes"], what="fixture")


# (b) ----------------------------------------------------------- the definition
@pytest.mark.parametrize("kind,nlon,nlat", CASES)
def test_all_planes_equal_reference_diag(kind, nlon, nlat):
    u, v, _, _ = inputs(kind, nlon, nlat)
    got = diag_of(kind, nlon, nlat).compute(u, v)[0].cpu().numpy()
    assert_planes(got, reference_of(kind, nlon, nlat), what=(kind, nlon, nlat))


# (c) ---------------------------------------------- the restated stencils' cross-pin
@pytest.mark.parametrize("kind,nlon,nlat", CASES)
def test_hot_planes_equal_bs_ready(kind, nlon, nlat):
    """u v ux uy vx vy qx qy qxx qxy qyy are columns 0..nlon-1 of
    ``rwrt_bs_ready``'s fp64 packed record of the same u, v."""
    from levels import Levels
    u, v, lat, lon = inputs(kind, nlon, nlat)
    names = ["u", "v", "ux", "uy", "vx", "vy", "qx", "qy", "qxx", "qxy", "qyy"]
    lv = Levels(lat, lon, 1)
    lv.set_level(0, u, v)
    packed = lv.packed[0].cpu().numpy()                  # [nlon + 1, nlat, 12]
    got = diag_of(kind, nlon, nlat).compute(u, v, names)[0].cpu().numpy()
    for k, n in enumerate(names):
        assert same_bits(got[k], packed[:nlon, :, k]), (kind, nlon, nlat, n)


# (d) ------------------------------------------------------------------ batches
def test_batches_do_not_change_a_level():
    u, v, lat, lon, want = three()
    d = diag_of("zonal", 70, 37)
    whole = d.compute(u, v, scratch_levels=3).cpu().numpy()
    assert whole.shape == (3, 23, 70, 37)
    for k in range(3):
        assert_planes(whole[k], want[k], what=("level", k))
        one = d.compute(u[k], v[k]).cpu().numpy()
        assert one.shape == (1, 23, 70, 37) and one.tobytes() == whole[k].tobytes(), k
    assert not same_bits(whole[0], whole[1]) and not same_bits(whole[0], whole[2])
    for sl in (1, 2, None):                               # (2: a last group of one level)
        assert d.compute(u, v, scratch_levels=sl).cpu().numpy().tobytes() == whole.tobytes(), sl
    assert d.compute(u, v, scratch_levels=3).cpu().numpy().tobytes() == whole.tobytes()      # twice the same
    # device tensors go in as they are
    assert d.compute(torch.as_tensor(u).cuda(), torch.as_tensor(v).cuda()).cpu().numpy().tobytes() == whole.tobytes()


# (e) ----------------------------------------------------------------- selects
def test_betam_ks_need_no_scratch():
    u, v, lat, lon, want = three()
    d = diag_of("zonal", 70, 37)
    got, pad = raw_call(d, u, v, BK, scratch=False, scratch_levels=-5)
    assert got.shape == (3, 2, 70, 37) and (pad == SENTINEL).all()
    for k in range(3):
        assert_planes(got[k], want[k, 21:], DIAG_NAMES[21:], what=k)
    assert np.isnan(got[:, :, :, [0, -1]]).all() and np.isfinite(got[:, 0, :, 1:-1]).all()
    assert np.isfinite(got[:, 1]).any() and np.isnan(got[:, 1, :, 1:-1]).any()
    # every mask without a q plane runs without scratch
    sel = ALL & ~NEEDS_Q
    got, pad = raw_call(d, u, v, sel, scratch=False)
    ids = [p for p in range(23) if sel >> p & 1]
    assert ids == [0, 1, 3, 4, 5, 6, 7, 8, 21, 22] and (pad == SENTINEL).all()
    for k in range(3):
        assert_planes(got[k], want[k, ids], [DIAG_NAMES[p] for p in ids], what=k)


@pytest.mark.parametrize("nlon,nlat", [(70, 37), (3, 4)])
def test_every_single_plane_and_the_sentinel(nlon, nlat):
    u, v, lat, lon, want = three(nlon, nlat)
    d = diag_of("zonal", nlon, nlat)
    full, pad = raw_call(d, u, v, ALL, scratch_levels=2)
    assert (pad == SENTINEL).all()
    for k in range(3):
        assert_planes(full[k], want[k], what=("all", k))
    for p in range(23):
        got, pad = raw_call(d, u, v, 1 << p, scratch=bool(NEEDS_Q >> p & 1), scratch_levels=2)
        assert got.shape == (3, 1, nlon, nlat) and (pad == SENTINEL).all(), DIAG_NAMES[p]
        assert same_bits(got[:, 0], want[:, p]), DIAG_NAMES[p]


def test_names_come_back_in_the_callers_order():
    u, v, _, _ = inputs("fixture", 24, 13)
    z = fixture()
    d = diag_of("fixture", 24, 13)
    names = ["KS", "u", "qyx", "betam", "qxx"]
    got = d.compute(u, v, names)[0].cpu().numpy()
    assert_planes(got, z["planes"][[DIAG_NAMES.index(n) for n in names]], names)
    h = d.numpy(u, v, names)
    assert list(h) == names and all(same_bits(h[n], z["planes"][DIAG_NAMES.index(n)]) for n in names)
    with pytest.raises(ValueError):
        d.compute(u, v, ["uyy"])
    with pytest.raises(ValueError):
        d.compute(u[:, :-1], v[:, :-1])
    with pytest.raises(ValueError):
        BSDiag(z["lat"][::-1], z["lon"])
    assert d.compute(np.zeros((0, 13, 24), np.float32), np.zeros((0, 13, 24), np.float32)).shape == (0, 23, 24, 13)


# (f) --------------------------------------------------------- argument errors
def test_argument_errors_with_device_buffers():
    lib = H.load()
    d = diag_of("fixture", 24, 13)
    z = fixture()
    n = 24 * 13
    u = torch.as_tensor(np.stack([z["u"], z["u"]])).cuda()
    v = torch.as_tensor(np.stack([z["v"], z["v"]])).cuda()
    out = torch.full((2 * 23 * n + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    sc = torch.empty(4 * n, dtype=torch.float64, device="cuda")
    base = dict(nlon=24, nlat=13, nlev=2, u=u.data_ptr(), v=v.data_ptr(), trig=d.trig.data_ptr(), select=ALL,
                out=out.data_ptr(), scratch=sc.data_ptr(), scratch_levels=1)

    def call(**kw):
        a = dict(base, **kw)
        return lib.rwrt_bs_diag(a["nlon"], a["nlat"], a["nlev"], a["u"], a["v"], a["trig"], d.dx, d.dy, a["select"],
                                a["out"], a["scratch"], a["scratch_levels"], H.stream())

    bad = [dict(nlon=2), dict(nlat=3), dict(nlev=-1), dict(select=0), dict(select=1 << 23), dict(select=ALL | 1 << 30),
           dict(u=None), dict(v=None), dict(trig=None), dict(out=None), dict(scratch=None), dict(scratch_levels=0),
           dict(select=1 << 2, scratch=None), dict(select=1 << 13, scratch_levels=-1),
           dict(out=u.data_ptr()), dict(out=v.data_ptr() + 2 * n * 4 - 8), dict(out=d.trig.data_ptr()),
           dict(u=out.data_ptr() + 2 * 23 * n * 8 - 4)]              # d_out's last bytes are u's first
    for kw in bad:
        assert call(**kw) == H.RWRT_ERR_ARG, kw
        assert lib.rwrt_last_error().startswith(b"rwrt_bs_diag: ") and len(lib.rwrt_last_error()) > 20, kw
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                        # nothing ran
    assert call(nlev=0) == H.RWRT_OK and call(nlev=0, select=BK, scratch=None) == H.RWRT_OK
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert call() == H.RWRT_OK                            # and the good call is good
    got = out.cpu().numpy()
    assert (got[2 * 23 * n:] == SENTINEL).all()
    assert_planes(got[:23 * n].reshape(23, 24, 13), z["planes"])
    with pytest.raises(H.RwrtError, match="rwrt_bs_diag"):
        H.check(call(select=0))


# (g) ------------------------------------------------ Levels, BS and the files
def test_levels_and_bs_diagnostics_and_output(tmp_path):
    import ncio
    from bs import BS
    from levels import Levels
    u, v, lat, lon, want = three()
    lv = Levels(lat, lon, 2)
    got = lv.diagnostics(u, v)                            # three levels through a two-level stack's axes
    assert got.shape == (3, 2, 70, 37) and got.device == lv.packed.device
    assert_planes(got[:, 0].cpu().numpy(), want[:, 21], range(3), "betam")
    assert_planes(got[:, 1].cpu().numpy(), want[:, 22], range(3), "KS")
    got = lv.diagnostics(u[1], v[1], names=("qy", "KS", "uxx")).cpu().numpy()
    assert_planes(got[0], want[1, [10, 22, 4]], ("qy", "KS", "uxx"))
    # BS.diagnostics: the static state's own u, v; BS itself is unchanged
    z = fixture()
    bs = BS(24, 13)
    bs.load_arrays(z["u"], z["v"], z["lat"], z["lon"])
    assert_planes(bs.diagnostics().cpu().numpy(), z["planes"], what="BS, before ready")
    bs.ready(xcyclic=True)
    got = bs.diagnostics(["KS", "q"]).cpu().numpy()
    assert_planes(got, np.stack([bs.KS, bs.q]), ("KS", "q"))
    # a descending-latitude file: BS flips u, v and keeps lat (bs.py:251-256); the device follows
    bd = BS(24, 13)
    bd.load_arrays(z["u"][::-1], z["v"][::-1], z["lat"][::-1], z["lon"])
    with np.errstate(all="ignore"):
        bd.ready(xcyclic=True)
    got = bd.diagnostics().cpu().numpy()
    assert_planes(got, np.stack([np.asarray(getattr(bd, n), np.float64) for n in DIAG_NAMES]), what="descending")
    # BSDiag.output -> ncio.read: one level like BS.output, several with a level axis
    d = diag_of("fixture", 24, 13)
    for suffix in (".nc", ".npz"):
        one, ref = str(tmp_path / ("one" + suffix)), str(tmp_path / ("ref" + suffix))
        d.output(one, z["u"], z["v"])
        bs.output(ref)
        a, b = ncio.read(one), ncio.read(ref)
        assert list(a) == list(b) and set(a) == set(DIAG_NAMES) | {"lon", "lat"}
        for k in b:
            assert same_bits(a[k], b[k]), (suffix, k)
    many = str(tmp_path / "many.nc")
    diag_of("zonal", 70, 37).output(many, u, v, names=["KS", "qyx"])
    a = ncio.read(many)
    assert set(a) == {"lon", "lat", "KS", "qyx"} and a["KS"].shape == (3, 70, 37)
    assert same_bits(a["KS"], want[:, 22]) and same_bits(a["qyx"], want[:, 13])
    assert same_bits(a["lat"], grid_steps(lat, lon)[0])


# (h) -------------------------------------------------------------- truncation
def test_trunc_equals_filtering_first():
    import shsf
    u, v, lat, lon, _ = three()
    d = diag_of("zonal", 70, 37)
    uv = shsf.shared_filter(37, 70, 5).filter(np.stack([u, v]))
    assert not torch.equal(uv[0].cpu(), torch.as_tensor(u))
    want = d.compute(uv[0], uv[1]).cpu().numpy()
    assert d.compute(u, v, trunc=5).cpu().numpy().tobytes() == want.tobytes()
    from levels import Levels
    got = Levels(lat, lon, 1).diagnostics(u, v, trunc=5).cpu().numpy()
    assert got.tobytes() == want[:, 21:].tobytes()
    assert_planes(want[0], reference_diag(uv[0, 0].cpu().numpy(), uv[1, 0].cpu().numpy(), lat, lon), what="filtered")
    with pytest.raises(ValueError):
        diag_of("zonal", 3, 4).compute(*inputs("zonal", 3, 4)[:2], trunc=1)      # (not the filter's grid: nlat is even)
