"""The grid part the map specs share (raymap.GridSpec), no GPU: what
``DensitySpec``, ``ArrivalSpec``, ``FluxSpec`` and ``TrackSpec`` hand to the
kernels equals, bit for bit, the formulas written out here -- ``pi * (deg /
180)``, ``nx / (lon1 - lon0)``, ``ny / (lat1 - lat0)`` -- and the same bad
inputs raise the same messages for every spec."""
import math

import numpy as np
import pytest

from arrival import ArrivalSpec
from density import DensitySpec
from flux import FluxSpec
from raymap import DeviceMap
from track import TrackSpec

NX, NY = 7, 5
LON_RANGES = [None, (-360, 720), (10, 50)]
LAT_RANGES = [(-90, 90), (-30.5, 61.25)]
NCHANS = [1, 3]
GRIDS = [(lon, lat, nchan) for lon in LON_RANGES for lat in LAT_RANGES for nchan in NCHANS]


def fields(c):
    return {name: getattr(c, name) for name, _ in c._fields_}


def grid(lon_range, lat_range):
    """The parent's arithmetic, operation for operation."""
    lat0 = math.pi * (float(lat_range[0]) / 180.0)
    lat1 = math.pi * (float(lat_range[1]) / 180.0)
    if lon_range is None:
        lon0, lon1 = 0.0, 2 * math.pi
    else:
        lon0, lon1 = math.pi * (float(lon_range[0]) / 180.0), math.pi * (float(lon_range[1]) / 180.0)
    return lon0, lon1, lat0, lat1, NX / (lon1 - lon0), NY / (lat1 - lat0)


class EdgesOf(DeviceMap):
    """The edge properties of a device map, without its device."""

    def __init__(self, spec):
        self.spec = spec


def check_shared(spec, lon_range, lat_range, nchan):
    lon0, lon1, lat0, lat1, inv_dlon, inv_dlat = grid(lon_range, lat_range)
    assert spec.shape == (nchan, NY, NX)
    g = spec.bins if isinstance(spec, ArrivalSpec) else spec       # (an ArrivalSpec delegates to its DensitySpec)
    assert (g.lat0, g.lat1, g.inv_dlat) == (lat0, lat1, inv_dlat)
    assert (g.lon0, g.lon1, g.inv_dlon, g.unwrapped) == (lon0, lon1, inv_dlon, lon_range is not None)
    assert g.circles == {None: None, (-360, 720): 3, (10, 50): None}[lon_range]
    m = EdgesOf(spec)
    a, b = (0.0, 360.0) if lon_range is None else (float(v) for v in lon_range)
    assert np.array_equal(m.lon_edges, np.linspace(a, b, NX + 1))
    assert np.array_equal(m.lat_edges, np.linspace(float(lat_range[0]), float(lat_range[1]), NY + 1))


@pytest.mark.parametrize("lat_range", LAT_RANGES)
@pytest.mark.parametrize("nchan", NCHANS)
def test_density_and_arrival_structs(lat_range, nchan):
    _, _, lat0, _, _, inv_dlat = grid(None, lat_range)
    for weight, wcol in ((None, -1), ("amp", 4), ("vg", 6)):
        d = DensitySpec(NX, NY, lat_range, nchan, weight)
        want = dict(nx=NX, ny=NY, nchan=nchan, wcol=wcol, inv_dlon=NX / (2 * math.pi), lat0=lat0, inv_dlat=inv_dlat)
        assert fields(d.c_struct()) == want
        check_shared(d, None, lat_range, nchan)
        a = ArrivalSpec(NX, NY, 11, lat_range, nchan, weight, window_rows=4)
        c = a.c_struct()
        assert fields(c.bins) == want and (c.window_rows, c.nwin) == (4, 3)
        assert a.bins == d and a.count_shape == (3, nchan, NY, NX)
        check_shared(a, None, lat_range, nchan)
    assert ArrivalSpec(NX, NY, 11, lat_range, nchan).c_struct().bins.wcol == 4          # require defaults to 'amp'
    c = ArrivalSpec(NX, NY, 11, lat_range, nchan, None).c_struct()
    assert (c.bins.wcol, c.window_rows, c.nwin) == (-1, 0, 0)


@pytest.mark.parametrize("lon_range,lat_range,nchan", GRIDS)
def test_flux_struct(lon_range, lat_range, nchan):
    lon0, _, lat0, _, inv_dlon, inv_dlat = grid(lon_range, lat_range)
    unwrapped = 2 if lon_range is not None else 0
    for vector, unit in (("velocity", 0), ("unit", 1)):
        s = FluxSpec(NX, NY, lat_range, lon_range, nchan, vector, (1.5, 80.0), 30.0)
        assert fields(s.c_struct()) == dict(nx=NX, ny=NY, nchan=nchan, mode=unit | unwrapped, lon0=lon0,
                                            inv_dlon=inv_dlon, lat0=lat0, inv_dlat=inv_dlat, s2_min=1.5 * 1.5,
                                            s2_max=80.0 * 80.0, wn_max=30.0)
        check_shared(s, lon_range, lat_range, nchan)
    c = FluxSpec(NX, NY, lat_range, lon_range, nchan).c_struct()
    assert (c.s2_min, c.s2_max, c.wn_max) == (0.0, math.inf, math.inf)


@pytest.mark.parametrize("lon_range,lat_range,nchan", GRIDS)
def test_track_struct(lon_range, lat_range, nchan):
    lon0, _, lat0, _, inv_dlon, inv_dlat = grid(lon_range, lat_range)
    for need, weight, max_cells, cols in (("amp", None, None, (4, -1, NX + NY)), (None, "ug", 9, (-1, 5, 9)),
                                          ("k", "l", 1, (2, 3, 1))):
        s = TrackSpec(NX, NY, lat_range, lon_range, need, weight, nchan, max_cells)
        assert fields(s.c_struct()) == dict(nx=NX, ny=NY, nchan=nchan, mode=2 if lon_range is not None else 0,
                                            need=cols[0], wcol=cols[1], max_cells=cols[2], reserved=0, lon0=lon0,
                                            inv_dlon=inv_dlon, lat0=lat0, inv_dlat=inv_dlat)
        check_shared(s, lon_range, lat_range, nchan)


def test_the_right_angle_is_exact_and_density_is_the_wrapped_axis():
    assert DensitySpec(NX, NY).lat0 == -math.pi / 2 and DensitySpec(NX, NY).lat1 == math.pi / 2
    for n in (1, 7, 360, 1440, 2 ** 20 + 1):
        assert DensitySpec(n, NY).inv_dlon == n / (2 * math.pi) == FluxSpec(n, NY).inv_dlon == TrackSpec(n, NY).inv_dlon


def _spec(kind, nx=NX, ny=NY, nchan=1, lat_range=(-90, 90), **kw):
    if kind == "density":
        return DensitySpec(nx, ny, lat_range, nchan, **kw)
    if kind == "arrival":
        return ArrivalSpec(nx, ny, 11, lat_range, nchan, **kw)
    return {"flux": FluxSpec, "track": TrackSpec}[kind](nx, ny, lat_range, nchan=nchan, **kw)


@pytest.mark.parametrize("kind", ["density", "arrival", "flux", "track"])
def test_bad_grids_raise_the_same_messages(kind):
    def make(**kw):
        return _spec(kind, **kw)

    for bad in (dict(nx=0), dict(ny=-1), dict(nchan=0)):
        with pytest.raises(ValueError, match="^nx, ny and nchan must be positive$"):
            make(**bad)
    for bad in (dict(nx=2 ** 16, ny=2 ** 15), dict(nx=2 ** 10, ny=2 ** 10, nchan=2 ** 11)):
        with pytest.raises(ValueError, match=r"^nchan\*ny\*nx must be below 2\^31$"):
            make(**bad)
    make(nx=2 ** 10, ny=2 ** 10, nchan=2 ** 11 - 1)
    for bad in ((10, 10), (20, -20), (0, math.nan)):
        with pytest.raises(ValueError, match="^lat_range must be ascending$"):
            make(lat_range=bad)
    if kind in ("flux", "track"):
        for bad in ((10, 10), (50, 10), (0, math.inf), (math.nan, 5)):
            with pytest.raises(ValueError, match="^lon_range must be None or finite and ascending$"):
                make(lon_range=bad)
    columns = r"None or one of \['amp', 'k', 'l', 'ug', 'vg'\]$"
    for name in {"density": ["weight"], "arrival": ["require"], "flux": [], "track": ["need", "weight"]}[kind]:
        with pytest.raises(ValueError, match=f"^{name} must be " + columns):
            make(**{name: "lon"})
