"""The wavenumber map on the GPU (``rwrt_wn_map``, ``rwrt_wn_fill``, ``wn.WN``).

A map entry is, bit for bit, what ``rwrt_ray_initial`` writes for a source at
that node, and what the NumPy definition ``wn.reference_wn_map`` gives -- both
get ``cos(lat)`` from this host's libm, so no test here depends on which libm
that is.  The fill equals ``wn.reference_fill`` exactly (a fixed order of
additions and one division)."""
import numpy as np
import pytest
import torch

import synthetic as S
from constants import deg2rad
from support.bits import equal_nan as same_bits
from support.cases import engine
from support.cases_wn import ZWN, bs_of, check_filled_planes, fill_planes, reference_map
from wn import WN, reference_fill, reference_wn_map

pytestmark = pytest.mark.gpu

_DEV = {}


def host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def nonzonal_map():
    """The device map of the non-zonal 2.5-degree state, computed once."""
    if "nonzonal" not in _DEV:
        _DEV["nonzonal"] = host(*engine("nonzonal").wn_map(ZWN, 0.0))
    return _DEV["nonzonal"]


def assert_map(got, want, what=None):
    for g, w, name in zip(got, want, ("mwn", "ug", "vg", "rootnum")):
        assert same_bits(g, w), (what, name)


def test_map_equals_the_initial_rows_and_the_reference():
    eng = engine("nonzonal")
    mwn, ug, vg, rootnum, info = nonzonal_map()
    assert mwn.shape == (144, 73, 4, 3) and rootnum.shape == (144, 73, 4) and rootnum.dtype == np.int32
    # every node as a source: s = i * 73 + j
    rows = eng.initial_rows(np.repeat(eng.lon, 73), np.tile(eng.lat, 144), ZWN, 0.0, check=False).cpu().numpy()
    for got, v in ((mwn, 3), (ug, 5), (vg, 6)):
        assert same_bits(got, rows[v].reshape(3, 144, 73, 4).transpose(1, 2, 3, 0)), v
    assert_map((mwn, ug, vg, rootnum), reference_map("nonzonal"))
    pole = np.zeros((144, 73, 4), bool)
    pole[:, [0, 72]] = True
    assert np.array_equal(rootnum == -1, pole)
    assert info.tolist() == [2 * 144 * 4]
    assert np.isnan(mwn[pole]).all() and np.isnan(ug[pole]).all() and np.isnan(vg[pole]).all()
    assert np.array_equal(rootnum[~pole], (~np.isnan(mwn)).sum(axis=-1)[~pole])
    assert np.array_equal(np.isnan(ug), np.isnan(mwn))          # NaN, not 0.0, where a slot has no root


@pytest.mark.parametrize("case", ["k0", "freq", "noncyclic", "zonal10"])
def test_map_other_inputs(case):
    from engine import RayEngine
    kw = dict(k0=dict(kind="nonzonal", zwn=(0.0, 2.0)), freq=dict(kind="nonzonal", freq=S.c3_freq(20.0)),
              noncyclic=dict(kind="nonzonal", xcyclic=False), zonal10=dict(kind="zonal", res=10.0))[case]
    kind = kw.pop("kind")
    zwn, freq = kw.pop("zwn", ZWN), kw.pop("freq", 0.0)
    if kw:
        bs = bs_of(kind, **kw)
        eng = RayEngine.from_bs(bs)
        assert eng.grid.ncol == (bs.nlon if case == "noncyclic" else bs.nlon + 1)
    else:
        eng = engine(kind)
    mwn, ug, vg, rootnum, info = host(*eng.wn_map(zwn, freq))
    want = reference_map(kind, zwn=zwn, freq=freq, **kw)
    assert_map((mwn, ug, vg, rootnum), want, case)
    assert info[0] == (want[3] == -1).sum()
    if case == "k0":
        assert (rootnum[:, :, 0] == 0).all() and np.isnan(mwn[:, :, 0]).all()
        assert not ug[:, :, 0].any() and not vg[:, :, 0].any()
        assert info[0] == 2 * 144
    if case == "freq":
        assert not same_bits(mwn, nonzonal_map()[0])
    if case == "zonal10":
        assert (mwn.shape[0] * mwn.shape[1] * len(zwn)) % 256 != 0
    # a map of the leading columns only
    part = host(*eng.wn_map(zwn, freq, nlon=5))
    assert_map(part[:4], [a[:5] for a in want], case)


def test_levels_batch():
    from engine import RayEngine
    from levels import Levels
    bl = [S.background_level(j) for j in range(3)]
    lv = Levels(bl[0]["lat"], bl[0]["lon"], 3)
    for j, b in enumerate(bl):
        lv.set_level(j, b["u"], b["v"])
    eng = RayEngine.from_levels(lv)
    batch = host(*eng.wn_map(ZWN, 0.0, levels=range(3)))
    assert batch[0].shape == (3, 144, 73, 4, 3) and batch[3].shape == (3, 144, 73, 4)
    assert batch[4].tolist() == [3 * 2 * 144 * 4]
    for j in range(3):
        one = host(*eng.wn_map(ZWN, 0.0, levels=range(j, j + 1)))
        assert one[0].shape == (1, 144, 73, 4, 3)
        assert_map([a[0] for a in one[:4]], [a[j] for a in batch[:4]], j)
        packed = host(*RayEngine.from_packed(lv.packed[j], lv.lon, lv.lat).wn_map(ZWN, 0.0))
        assert_map(packed[:4], [a[j] for a in batch[:4]], j)
    assert not same_bits(batch[0][0], batch[0][1]) and not same_bits(batch[0][1], batch[0][2])
    assert_map(host(*eng.wn_map(ZWN, 0.0))[:4], [a[0] for a in batch[:4]], "default level")
    # the device's levels are the host's BS.fields bit for bit, so the NumPy definition holds per level
    from bs import BS
    bs = BS(144, 73)
    bs.load_arrays(**bl[1])
    bs.ready(xcyclic=True)
    assert_map([a[1] for a in batch[:4]], reference_wn_map(bs, ZWN, 0.0), "level 1")
    with pytest.raises(ValueError):
        eng.wn_map(ZWN, 0.0, levels=range(2, 4))
    with pytest.raises(ValueError):
        engine("nonzonal").wn_map(ZWN, 0.0, levels=range(1))
    lv32 = Levels(bl[0]["lat"], bl[0]["lon"], 2, fp32=True)
    with pytest.raises(NotImplementedError):
        RayEngine.from_levels(lv32).wn_map(ZWN, 0.0)
    with pytest.raises(NotImplementedError):
        WN.from_levels(lv32, ZWN).cal_wave()
    # WN over the stack: every level by default, the level axis first
    w = WN.from_levels(lv, ZWN).cal_wave()
    assert w.n_bad == 3 * 2 * 144 * 4
    assert_map(host(w.mwn, w.ug, w.vg, w.rootnum), batch[:4], "WN.from_levels")
    w.postprocess()
    for j in range(3):
        assert same_bits(w.mwn[j].cpu().numpy(), reference_fill(batch[0][j].reshape(144, 73, 12), True).reshape(144, 73, 4, 3))


@pytest.mark.parametrize("cyclic", [True, False])
def test_fill(cyclic):
    eng = engine("nonzonal")
    a = fill_planes()
    got = eng.wn_fill(torch.as_tensor(a.copy(), device=eng.device), cyclic).cpu().numpy()
    assert same_bits(got, reference_fill(a, cyclic))
    check_filled_planes(a, got, cyclic)
    mwn = nonzonal_map()[0]
    got = eng.wn_fill(torch.as_tensor(mwn, device=eng.device), cyclic).cpu().numpy()
    assert got.shape == mwn.shape
    assert same_bits(got, reference_fill(mwn.reshape(144, 73, 12), cyclic).reshape(mwn.shape))
    assert (np.isnan(mwn) & ~np.isnan(got)).any() and np.isnan(got).any()
    assert same_bits(got[~np.isnan(mwn)], mwn[~np.isnan(mwn)])


def exact_degrees(rad):
    """Degrees ``d`` with ``d * deg2rad == rad`` exactly (None: there is none
    nearby), so that ``WR.set_source_array`` lands on a float32-rounded node."""
    d = np.float64(rad) / deg2rad
    for step in sorted(range(-8, 9), key=abs):
        x = d
        for _ in range(abs(step)):
            x = np.nextafter(x, np.inf if step > 0 else -np.inf)
        if x * (1.0 * deg2rad) == rad and np.signbit(x) == np.signbit(rad):
            return float(x)
    return None


def test_wn_surface(tmp_path):
    import ncio
    from wr import WR
    bs = bs_of("nonzonal")
    w = WN.from_bs(bs, ZWN)
    assert w.mwn is None and w.nzwn == 4
    w.set_freq(0.0)
    w.set_zwn(ZWN)
    with pytest.raises(ValueError):
        w.set_zwn((1.0, 2.0))
    assert w.cal_wave() is w                      # (does not raise at the pole rows)
    assert w.n_bad == 2 * 144 * 4 and w.mwn.is_cuda
    d = w.numpy()
    assert_map([d[k] for k in ("mwn", "ug", "vg", "rootnum")], nonzonal_map()[:4])
    assert same_bits(d["lon"], bs.lon) and same_bits(d["lat"], bs.lat) and d["zwn"].tolist() == list(ZWN)
    path = str(tmp_path / "wn.nc")
    w.output(path)
    back = ncio.read(path)
    for k in ("lon", "lat", "zwn", "mwn", "ug", "vg", "rootnum"):
        assert same_bits(back[k], d[k]), k
    assert np.isnan(back["mwn"]).any()
    # rays launched at grid nodes start with the map's entries
    nodes = []
    for i, j in ((0, 36), (10, 20), (37, 50), (77, 12), (143, 60), (100, 44), (5, 5), (60, 30), (120, 66)):
        deg = exact_degrees(bs.lon[i]), exact_degrees(bs.lat[j])
        if None not in deg and len(nodes) < 5:
            nodes.append((i, j) + deg)
    assert len(nodes) == 5
    wr = WR(4, 5, 7200.0, 86400.0, 0.0, nx=bs.nlon, ny=bs.nlat)
    wr.bs = bs
    wr.set_zwn(ZWN)
    wr.set_source_array([n[2] for n in nodes], [n[3] for n in nodes])
    ii, jj = [n[0] for n in nodes], [n[1] for n in nodes]
    assert same_bits(wr.source_lon, bs.lon[ii]) and same_bits(wr.source_lat, bs.lat[jj])
    wr.ray_initial(mode="hip")
    for hist, name in ((wr.rmwn, "mwn"), (wr.rug, "ug"), (wr.rvg, "vg")):
        assert same_bits(hist[0], d[name][ii, jj].transpose(2, 0, 1)), name     # [3, nsource, nzwn]
    assert (d["rootnum"][ii, jj] > 0).any()
    # the fill leaves rootnum as computed
    before = w.rootnum.clone()
    w.postprocess()
    assert torch.equal(w.rootnum, before)
    assert same_bits(w.mwn.cpu().numpy(), reference_fill(d["mwn"].reshape(144, 73, 12), True).reshape(144, 73, 4, 3))
    assert same_bits(w.ug.cpu().numpy(), reference_fill(d["ug"].reshape(144, 73, 12), bs.xcyclic).reshape(144, 73, 4, 3))
    w.clean()
    assert w.mwn is None
