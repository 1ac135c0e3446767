"""The wavenumber map, host side (no GPU): the NumPy definition
``wn.reference_wn_map`` against the CPU oracle's initial rays at every grid
node, the fill definition ``wn.reference_fill`` against a plain scalar loop,
the shared per-entry arithmetic csrc/wn_fill.h in a stand-alone program under
the sanitizers, and the argument checks of ``rwrt_wn_map`` / ``rwrt_wn_fill``."""
import ctypes

import numpy as np
import pytest

import _hip as H
import rwrt_oracle as O
import synthetic as S
from support import hostprog
from support.bits import equal_nan
from support.cases_wn import ZWN, bs_of, check_filled_planes, fill_planes, reference_map
from wn import reference_fill

NAN, INF = np.nan, np.inf


# ------------------------------------------------- the map against the oracle
def test_reference_map_equals_the_oracles_initial_rays():
    """Rows 1..71 of the non-zonal 2.5-degree map are, bit for bit, the oracle's
    initial rays of sources (bs.lon, lat_j); the pole rows, where np.roots
    raises, are -1 / NaN; all four branches of the root ordering occur."""
    b = S.background("nonzonal")
    bs = bs_of("nonzonal")
    assert (bs.nlon, bs.nlat) == (144, 73)
    mwn, ug, vg, rootnum = reference_map("nonzonal")
    assert mwn.shape == ug.shape == vg.shape == (144, 73, 4, 3) and rootnum.shape == (144, 73, 4)
    bg = O.Background(**b)
    zwn = np.array(ZWN)
    with np.errstate(all="ignore"):
        for j in range(1, 72):
            rows = O.ray_initial(bg, bs.lon, np.full(144, bs.lat[j]), zwn, 0.0)
            for got, v in ((mwn, 3), (ug, 5), (vg, 6)):
                assert equal_nan(got[:, j], rows[v].transpose(1, 2, 0)), (j, v)
            assert np.array_equal(rootnum[:, j], (~np.isnan(rows[3])).sum(axis=0)), j
        for j in (0, 72):
            with pytest.raises(np.linalg.LinAlgError):
                O.ray_initial(bg, bs.lon, np.full(144, bs.lat[j]), zwn, 0.0)
    for j in (0, 72):
        assert (rootnum[:, j] == -1).all()
        assert np.isnan(mwn[:, j]).all() and np.isnan(ug[:, j]).all() and np.isnan(vg[:, j]).all()
    inner = rootnum[:, 1:72]
    assert inner.min() >= 0 and inner.max() <= 3
    hist = np.bincount(inner.ravel(), minlength=4)
    assert (hist >= 1000).all(), hist          # (measured: 1935 31533 1923 5505)
    # ug, vg are NaN exactly where a slot has no root
    assert np.array_equal(np.isnan(ug), np.isnan(mwn)) and np.array_equal(np.isnan(vg), np.isnan(mwn))
    assert np.array_equal(rootnum[:, 1:72], (~np.isnan(mwn[:, 1:72])).sum(axis=-1))


def test_reference_map_zonal_has_zero_or_two_roots():
    mwn, ug, vg, rootnum = reference_map("zonal")
    assert (rootnum[:, [0, 72]] == -1).all()
    assert set(np.unique(rootnum[:, 1:72]).tolist()) == {0, 2}


def test_reference_map_k_zero():
    """k == 0: no roots and zero group velocity, as in the initial rays."""
    mwn, ug, vg, rootnum = reference_map("nonzonal", zwn=(0.0, 2.0))
    assert np.isnan(mwn[:, :, 0]).all() and (rootnum[:, :, 0] == 0).all()
    assert not ug[:, :, 0].any() and not vg[:, :, 0].any()
    assert (rootnum[:, [0, 72], 1] == -1).all() and (rootnum[:, 1:72, 1] >= 0).all()


def scalar_fill(a, cyclic):
    """The definition as a plain triple loop."""
    nx, ny, npl = a.shape
    out = a.copy()
    for i in range(nx):
        for j in range(ny):
            for p in range(npl):
                if not np.isnan(a[i, j, p]):
                    continue
                acc, cnt = 0.0, 0
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        ii, jj = i + di, j + dj
                        if (di == 0 and dj == 0) or jj < 0 or jj >= ny:
                            continue
                        if ii < 0 or ii >= nx:
                            if not cyclic:
                                continue
                            ii %= nx
                        w = a[ii, jj, p]
                        with np.errstate(invalid="ignore"):
                            acc = acc + (w if not np.isnan(w) else 0.0)
                        cnt += 0 if np.isnan(w) else 1
                if cnt:
                    with np.errstate(invalid="ignore"):
                        out[i, j, p] = acc / cnt
    return out


@pytest.mark.parametrize("cyclic", [True, False])
def test_reference_fill_against_the_scalar_definition(cyclic):
    a = fill_planes()
    got = reference_fill(a, cyclic)
    assert equal_nan(got, scalar_fill(a, cyclic))
    check_filled_planes(a, got, cyclic)
    # the seam: (0, 2) of plane 2 sees column 6 only when cyclic
    other = reference_fill(a, not cyclic)
    assert not equal_nan(got[[0, 6], :, 2], other[[0, 6], :, 2])
    # a trailing axis of any shape is a set of planes
    assert equal_nan(reference_fill(a.reshape(7, 5, 2, 3), cyclic), got.reshape(7, 5, 2, 3))


# ------------------------------------------------- csrc/wn_fill.h on the host
def run_host_program(exe, a, cyclic):
    lines = ["%d %d %d %d" % (a.shape + (int(cyclic),))]
    lines += ["%016x" % u for u in np.ascontiguousarray(a).view(np.uint64).ravel().tolist()]
    r = hostprog.run_process(exe, lines)
    out = np.array([int(x, 16) for x in r.stdout.split()], np.uint64).view(np.float64)
    return out.reshape(a.shape)


def test_fill_host_program_under_sanitizers(tmp_path):
    """csrc/wn_fill.h (what the kernel calls) in a stand-alone program built
    with ASan + UBSan and run directly reproduces reference_fill exactly, on
    the crafted planes and on one-column and one-row arrays."""
    exe = hostprog.build("wn_fill", tmp_path, float_cast=False, no_warnings=True)
    a = fill_planes()
    thin = np.array([[[NAN], [1.0], [NAN], [NAN], [4.0]]])          # [1, 5, 1]
    for arr in (a, thin, np.ascontiguousarray(thin.transpose(1, 0, 2)), a[:2]):
        for cyclic in (True, False):
            got = run_host_program(exe, np.ascontiguousarray(arr), cyclic)
            assert equal_nan(got, reference_fill(arr, cyclic)), (arr.shape, cyclic)
    check_filled_planes(a, run_host_program(exe, a, True), True)


# ----------------------------------------------------------- C entry points
def _grid():
    return H.Grid(145, 73, 0.0, 0.04363323, -1.5707964, 0.04363323)


def _map(lib, g="ok", packed=64, nlev=1, stride=0, nlon=144, lon=64, lat=64, cos=64, nzwn=4, zwn=64, mwn=64,
         ug=64, vg=64, rootnum=64, info=64):
    """rwrt_wn_map with fake (never dereferenced) device pointers."""
    g = _grid() if isinstance(g, str) else g
    return lib.rwrt_wn_map(None if g is None else ctypes.byref(g), packed, nlev, stride, nlon, lon, lat, cos, nzwn,
                           zwn, mwn, ug, vg, rootnum, info, None)


def test_wn_map_argument_errors_without_a_gpu():
    """Every check happens before any HIP call."""
    lib = H.load()
    assert "abi 5" in H.version()                      # additive members: the version stays
    level = 145 * 73 * 12
    cases = [dict(g=None), dict(packed=None)]
    cases += [{k: None} for k in ("lon", "lat", "cos", "zwn", "mwn", "ug", "vg", "rootnum", "info")]
    cases += [dict(nlev=0), dict(nlev=-1), dict(nzwn=0), dict(nlon=0), dict(nlon=146),
              dict(nlev=2, stride=level - 1), dict(nlev=2, stride=0), dict(nlev=3, stride=-level)]
    # the conditions of a packed state (make_field)
    cases += [dict(g=H.Grid(1, 73, 0.0, 0.04, -1.57, 0.04), nlon=1), dict(g=H.Grid(145, 1, 0.0, 0.04, -1.57, 0.04)),
              dict(g=H.Grid(145, 73, 0.0, 0.0, -1.57, 0.04)), dict(g=H.Grid(145, 73, 0.0, 0.04, -1.57, 0.0)),
              dict(packed=72), dict(g=H.Grid(65536, 73, 0.0, 0.04, -1.57, 0.04)),
              dict(g=H.Grid(65535, 257, 0.0, 0.04, -1.57, 0.04))]
    for kw in cases:
        assert _map(lib, **kw) == H.RWRT_ERR_ARG, kw
        assert lib.rwrt_last_error(), kw
    assert b"level_stride" in (_map(lib, nlev=2, stride=level - 1), lib.rwrt_last_error())[1]
    assert b"nlon" in (_map(lib, nlon=146), lib.rwrt_last_error())[1]


def test_wn_fill_argument_errors_without_a_gpu():
    lib = H.load()
    for args, word in (((7, 5, 6, 1, None, 64), b"d_in"), ((7, 5, 6, 1, 64, None), b"d_out"),
                       ((7, 5, 6, 1, 64, 64), b"d_in"), ((0, 5, 6, 1, 64, 128), b"nlon"),
                       ((7, 0, 6, 0, 64, 128), b"nlat"), ((7, 5, 0, 0, 64, 128), b"nplane"),
                       ((-1, 5, 6, 1, 64, 128), b"nlon")):
        assert lib.rwrt_wn_fill(*args, None) == H.RWRT_ERR_ARG, args
        assert word in lib.rwrt_last_error(), (args, lib.rwrt_last_error())
