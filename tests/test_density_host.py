"""Ray-density maps, host side (no GPU): the NumPy definition
``density.reference_bins`` on hand-made corner points and on the reference's
own C1 history, the shared index function csrc/density_bins.h in a
stand-alone program under the sanitizers, and the argument checks of
``rwrt_ray_density``."""
import ctypes
import math

import numpy as np
import pytest

import _hip as H
from conftest import golden
from density import DensitySpec, bin_index, reference_bins
from support import hostprog
from support.abi import refused
from support.cases_density import HALF_PI, INF, NAN, SPEC, TWO_PI, corner_points, random_points, scalar_bin


def test_spec_factors():
    s = DensitySpec(1440, 720)
    assert (s.lat0, s.lat1) == (-HALF_PI, HALF_PI)
    assert s.inv_dlon == 1440 / (2 * math.pi) and s.inv_dlat == 720 / (s.lat1 - s.lat0)
    assert s.wcol == -1 and SPEC.wcol == 4
    c = SPEC.c_struct()
    assert (c.nx, c.ny, c.nchan, c.wcol, c.inv_dlon, c.lat0, c.inv_dlat) == \
        (7, 5, 2, 4, SPEC.inv_dlon, SPEC.lat0, SPEC.inv_dlat)
    with pytest.raises(ValueError):
        DensitySpec(0, 5)
    with pytest.raises(ValueError):
        DensitySpec(7, 5, weight="nacc")


def test_reference_bins_corner_points():
    pts = corner_points()
    lon, lat, w, chan = (np.array([p[k] for p in pts]) for k in range(4))
    want = np.zeros(SPEC.shape, np.int64)
    wsum_want = np.zeros(SPEC.shape)
    for p in pts:
        assert scalar_bin(*p[:4], SPEC) == p[4], p
        if p[4] is not None:
            want[p[4]] += 1
            wsum_want[p[4]] += p[2]
    count, wsum = reference_bins(lon, lat, w, chan.astype(np.int64), SPEC)
    assert count.dtype == np.int64 and np.array_equal(count, want)
    # written out: map 0, latitude row 2: 4 points at ix 0 (0, 2 pi, -1e-20, 63.69), the clamped one at 6
    assert count[0, 2].tolist() == [4, 2, 1, 1, 0, 0, 1]
    assert count[1, :, 1].tolist()[:2] == [1, 1] and count[1, 4, 1] == 1
    assert count.sum() == sum(p[4] is not None for p in pts) == 15
    assert np.array_equal(wsum, wsum_want)
    # the clamp is needed at nx = 7 ...
    assert math.floor(math.nextafter(TWO_PI, 0.0) * SPEC.inv_dlon) == 7
    # ... and counts only: the same points with no weight bin the non-finite w too
    s0 = DensitySpec(7, 5, nchan=2)
    c0, w0 = reference_bins(lon, lat, None, chan.astype(np.int64), s0)
    assert w0 is None and c0.sum() == 15 + 3


def test_reference_bins_random_against_scalar_definition():
    lon, lat, w, chan = random_points(4000, SPEC, seed=3)
    idx = bin_index(lon, lat, w, chan, SPEC)
    for i in range(len(lon)):
        b = scalar_bin(float(lon[i]), float(lat[i]), float(w[i]), int(chan[i]), SPEC)
        assert idx[i] == (-1 if b is None else (b[0] * SPEC.ny + b[1]) * SPEC.nx + b[2]), i


@pytest.mark.parametrize("nx,ny", [(7, 5), (144, 72), (1440, 720)])
def test_reference_bins_c1_history(nx, ny):
    """The reference's own 90-day C1 history (rows 1..1080, 3 rays), full
    latitude range: every one of the 3 240 points is binned; at 1440 x 720 the
    fullest bin holds 1 080 (the contention case of the GPU tests)."""
    g = golden("traj_C1.npz")
    hist = g["hist"]                                  # (7, 1081, 3)
    lon, lat = hist[0, 1:], hist[1, 1:]
    assert np.nanmax(lon) > 63.0                      # stored longitudes are not wrapped
    spec = DensitySpec(nx, ny)
    count, wsum = reference_bins(lon, lat, None, None, spec)
    assert wsum is None and count.shape == (1, ny, nx)
    assert count.sum() == 3240
    if (nx, ny) == (1440, 720):
        assert count.max() == 1080
    # per root through the channels: each root's 1 080 rows
    by_root = reference_bins(lon, lat, None, np.arange(3)[None, :], DensitySpec(nx, ny, nchan=3))[0]
    assert by_root.sum(axis=(1, 2)).tolist() == [1080, 1080, 1080]
    assert np.array_equal(by_root.sum(0), count[0])


@pytest.mark.parametrize("spec", [SPEC, DensitySpec(1440, 720), DensitySpec(144, 72, lat_range=(-30, 60), nchan=3,
                                                                            weight="k")],
                         ids=["7x5", "1440x720", "144x72-band"])
def test_index_function_host_program_under_sanitizers(tmp_path, spec):
    """csrc/density_bins.h (what the kernel calls) in a stand-alone program
    built with ASan + UBSan + float-cast-overflow and run directly: the corner
    points and 10^5 random ones give reference_bins' indices, and the wrapped
    longitude equals Python's ``(lon % 2 pi) % 2 pi`` bit for bit."""
    exe = hostprog.build("density_bins", tmp_path)
    pts = corner_points()
    rl, rt, rw, rc = random_points(100000, spec, seed=11)
    lon = np.concatenate([[p[0] for p in pts], rl])
    lat = np.concatenate([[p[1] for p in pts], rt])
    w = np.concatenate([[p[2] for p in pts], rw])
    chan = np.concatenate([[p[3] for p in pts], rc]).astype(np.int64)
    lines = [f"{spec.nx} {spec.ny} {spec.nchan} {spec.wcol} {spec.inv_dlon.hex()} {spec.lat0.hex()} "
             f"{spec.inv_dlat.hex()}"]
    lines += [f"{float(a).hex()} {float(b).hex()} {float(c).hex()} {int(d)}" for a, b, c, d in zip(lon, lat, w, chan)]
    out = hostprog.run_process(exe, lines).stdout.split()
    got = np.array(out[0::2], dtype=np.int64)
    lam = np.array([float.fromhex(x) if "nan" not in x else NAN for x in out[1::2]])
    assert len(got) == len(lon)
    want = bin_index(lon, lat, w, chan, spec)
    bad = np.where(got != want)[0]
    assert bad.size == 0, [(lon[i], lat[i], w[i], chan[i], got[i], want[i]) for i in bad[:5]]
    with np.errstate(all="ignore"):
        lam_want = np.remainder(np.remainder(lon, TWO_PI), TWO_PI)
    assert np.array_equal(np.where(np.isnan(lam), NAN, lam).view(np.int64),
                          np.where(np.isnan(lam_want), NAN, lam_want).view(np.int64))
    for i in range(len(pts)):     # Python's own float %, point by point
        if math.isfinite(pts[i][0]):
            assert lam[i] == (pts[i][0] % TWO_PI) % TWO_PI


# ----------------------------------------------------------- C entry point
def _call(lib, m, nray=16, i0=1, i1=5, rows=64, slot=None, tfrom=None, trow=None, chan=None, count=64, wsum=None):
    """rwrt_ray_density with fake (never dereferenced) device pointers."""
    return lib.rwrt_ray_density(None if m is None else ctypes.byref(m), nray, i0, i1, rows, slot, tfrom, trow,
                                chan, count, wsum, None)


def test_density_argument_errors_without_a_gpu():
    """Every check happens before any HIP call and names the argument."""
    lib = H.load()
    assert ctypes.sizeof(H.DensityMap) == 40
    assert "abi 5" in H.version()
    good = SPEC.c_struct()

    def m(**kw):
        c = SPEC.c_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    cases = [
        (dict(m=None), b"map"),
        (dict(m=m(nx=0)), b"nx"), (dict(m=m(ny=-1)), b"ny"), (dict(m=m(nchan=0)), b"nchan"),
        (dict(m=m(nx=65536, ny=32768, nchan=1)), b"2^31"), (dict(m=m(nx=1 << 20, ny=1 << 10, nchan=2)), b"2^31"),
        (dict(m=m(wcol=0)), b"wcol"), (dict(m=m(wcol=1)), b"wcol"), (dict(m=m(wcol=7)), b"wcol"),
        (dict(m=m(wcol=-2)), b"wcol"),
        (dict(m=good, wsum=None), b"d_wsum"),
        (dict(m=good, wsum=64, i0=5, i1=5), b"it_begin"), (dict(m=good, wsum=64, i0=6, i1=5), b"it_begin"),
        (dict(m=good, wsum=64, slot=64), b"d_row_slot"),
        (dict(m=good, wsum=64, tfrom=64), b"d_tail_row"), (dict(m=good, wsum=64, trow=64), b"d_tail_from"),
        (dict(m=good, wsum=64, rows=None), b"d_rows"),
        (dict(m=good, wsum=64, count=None), b"d_count"),
        (dict(m=m(inv_dlon=0.0), wsum=64), b"inv_dlon"), (dict(m=m(inv_dlon=-1.0), wsum=64), b"inv_dlon"),
        (dict(m=m(inv_dlon=INF), wsum=64), b"inv_dlon"), (dict(m=m(inv_dlon=NAN), wsum=64), b"inv_dlon"),
        (dict(m=m(inv_dlat=0.0), wsum=64), b"inv_dlat"), (dict(m=m(inv_dlat=NAN), wsum=64), b"inv_dlat"),
        (dict(m=m(inv_dlat=INF), wsum=64), b"inv_dlat"),
        (dict(m=good, wsum=64, nray=-1), b"nray"), (dict(m=good, wsum=64, nray=1 << 31), b"nray"),
        (dict(m=good, wsum=64, rows=72), b"16-byte"), (dict(m=good, wsum=64, tfrom=64, trow=72), b"16-byte"),
    ]
    for kw, word in cases:
        refused(lib, _call, kw, word, b"rwrt_ray_density: ")
    # no rays: a no-op (no device is touched; there is none on the build host)
    assert _call(lib, good, nray=0, rows=None, wsum=64) == H.RWRT_OK
    assert _call(lib, m(wcol=-1), nray=0, rows=None, wsum=None) == H.RWRT_OK
