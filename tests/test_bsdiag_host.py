"""Basic-state diagnostics, host side (no GPU): the NumPy definition
``bsdiag.reference_diag`` (our host ``BS``) against the reference's own 23
``BS.output`` arrays (tests/golden/bsdiag_ref.npz), the shared per-node
arithmetic csrc/bs_diag.h in a stand-alone program under the sanitizers, and
the argument checks of ``rwrt_bs_diag``."""
import struct

import numpy as np
import pytest

import _hip as H
from bsdiag import DIAG_NAMES, NEEDS_Q, reference_diag, select_mask
from levels import trig_table
from support import hostprog
from support.bits import bitwise
from support.cases_bsdiag import ALL, fixture, grid_steps, inputs, reference_of


# ------------------------------------------- the definition against the reference
def test_fixture_has_every_case():
    z = fixture()
    assert tuple(z["names"]) == DIAG_NAMES and z["planes"].shape == (23, 24, 13)
    assert z["u"].dtype == np.float32 and z["u"].shape == (13, 24)
    betam, ks, u = z["planes"][21], z["planes"][22], z["planes"][0]
    assert np.isfinite(ks[:, 1:-1]).any() and np.isnan(ks[:, 1:-1]).any()
    assert (betam[:, 1:-1] <= 0).any()
    assert ((betam[:, 1:-1] <= 0) & (u[:, 1:-1] > 0)).any()      # NaN for betam's sake alone
    assert (u[:, 1:-1] <= 0).any()
    assert np.isnan(betam[:, [0, -1]]).all() and np.isnan(ks[:, [0, -1]]).all()
    assert np.isfinite(z["planes"][:21]).all() and np.isfinite(betam[:, 1:-1]).all()
    # qyx is the unsmoothed copy: it differs from qxy on smth9's interior only
    d = z["planes"][12] != z["planes"][13]
    assert d[1:-2, 1:-2].any() and not d[[0, -2, -1]].any() and not d[:, [0, -2, -1]].any()


def test_reference_diag_equals_the_reference():
    """Our host ``BS`` on the fixture's inputs gives the reference's 23 arrays
    bit for bit -- the planes outside the hot path (uxx, vxx, the third
    derivatives, the unsmoothed qyx, betam, KS) included."""
    z = fixture()
    got = reference_diag(z["u"], z["v"], z["lat"], z["lon"])
    assert got.shape == (23, 24, 13) and got.dtype == np.float64
    for k, n in enumerate(DIAG_NAMES):
        assert bitwise(got[k], z["planes"][k]), n


def test_select_mask():
    assert select_mask(DIAG_NAMES) == (ALL, list(range(23)))
    assert select_mask(["KS", "betam"]) == ((1 << 21) | (1 << 22), [1, 0])
    assert select_mask(["qy", "u", "KS"]) == ((1 << 10) | 1 | (1 << 22), [1, 0, 2])
    assert [n for k, n in enumerate(DIAG_NAMES) if NEEDS_Q >> k & 1] == [n for n in DIAG_NAMES if n[0] == "q"]
    for bad in ([], ["u", "u"], ["uyy"], ["ks"]):
        with pytest.raises(ValueError):
            select_mask(bad)


# ------------------------------------------------ csrc/bs_diag.h on the host
host_program = hostprog.fixture("bs_diag")


def run_host_program(exe, tmp_path, u, v, lat_deg, lon_deg, select):
    """The planes ``[popcount(select), nlon, nlat]`` of the stand-alone program."""
    lat, dx, dy = grid_steps(lat_deg, lon_deg)
    nlat, nlon = u.shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<iiIidd", nlon, nlat, select, 0, dx, dy))
        f.write(np.ascontiguousarray(trig_table(lat), "<f8").tobytes())
        f.write(np.ascontiguousarray(u, "<f4").tobytes())
        f.write(np.ascontiguousarray(v, "<f4").tobytes())
    r = hostprog.run_process(exe, args=(src, dst))
    assert "bs_diag_main ok" in r.stderr
    return np.fromfile(dst, "<f8").reshape(bin(select).count("1"), nlon, nlat)


def test_host_program_equals_the_reference_fixture(host_program, tmp_path):
    """csrc/bs_diag.h (what the kernels call) built with ASan + UBSan and run
    directly over the fixture's inputs: all 23 planes equal the reference's."""
    z = fixture()
    got = run_host_program(host_program, tmp_path, z["u"], z["v"], z["lat"], z["lon"], ALL)
    for k, n in enumerate(DIAG_NAMES):
        assert bitwise(got[k], z["planes"][k]), n


@pytest.mark.parametrize("kind", ["zonal", "nonzonal"])
def test_host_program_minimum_grid(host_program, tmp_path, kind):
    """The 3 x 4 minimum grid (smth9's interior is empty, every latitude row
    is an edge row or next to one), all 23 planes."""
    u, v, lat, lon = inputs(kind, 3, 4)
    want = reference_of(kind, 3, 4)
    got = run_host_program(host_program, tmp_path, u, v, lat, lon, ALL)
    for k, n in enumerate(DIAG_NAMES):
        assert bitwise(got[k], want[k]), n


@pytest.mark.parametrize("plane", [2, 13, 18, 21, 22])
def test_host_program_single_plane(host_program, tmp_path, plane):
    z = fixture()
    got = run_host_program(host_program, tmp_path, z["u"], z["v"], z["lat"], z["lon"], 1 << plane)
    assert got.shape == (1, 24, 13) and bitwise(got[0], z["planes"][plane]), DIAG_NAMES[plane]


def test_host_program_odd_grid(host_program, tmp_path):
    """8 x 5: smth9's interior [1:-2, 1:-2] is small but not empty."""
    u, v, lat, lon = inputs("nonzonal", 8, 5)
    want = reference_of("nonzonal", 8, 5)
    got = run_host_program(host_program, tmp_path, u, v, lat, lon, ALL)
    for k, n in enumerate(DIAG_NAMES):
        assert bitwise(got[k], want[k]), n
    assert not bitwise(want[12], want[13])          # smth9 changed something


# ----------------------------------------------------------- C entry point
def _call(lib, nlon=24, nlat=13, nlev=2, u=4096, v=8192, trig=1 << 20, select=ALL, out=1 << 24, scratch=1 << 28,
          scratch_levels=1):
    """rwrt_bs_diag with fake (never dereferenced) device pointers."""
    return lib.rwrt_bs_diag(nlon, nlat, nlev, u, v, trig, 0.26, 0.26, select, out, scratch, scratch_levels, None)


def test_bs_diag_argument_errors_without_a_gpu():
    """Every check happens before any HIP call and names the argument."""
    lib = H.load()
    assert "abi 5" in H.version()                      # an additive member: the version stays
    bk = (1 << 21) | (1 << 22)
    cases = [
        (dict(nlon=2), b"nlon"), (dict(nlat=3), b"nlat"), (dict(nlev=-1), b"nlev"),
        (dict(select=0), b"select"), (dict(select=1 << 23), b"select"), (dict(select=ALL | (1 << 31)), b"select"),
        (dict(u=None), b"d_u"), (dict(v=None), b"d_v"), (dict(trig=None), b"d_trig"), (dict(out=None), b"d_out"),
        (dict(scratch=None), b"d_scratch"), (dict(select=1 << 2, scratch=None), b"d_scratch"),
        (dict(select=1 << 20, scratch=None), b"d_scratch"),
        (dict(scratch_levels=0), b"scratch_levels"), (dict(scratch_levels=-3), b"scratch_levels"),
        (dict(out=4096), b"overlaps"),                                  # d_out == d_u
        (dict(out=4096 + 2 * 24 * 13 * 4 - 8), b"overlaps"),           # the last double of u's two levels
        (dict(out=(1 << 22) - 2 * 23 * 24 * 13 * 8 + 8, v=1 << 22), b"overlaps"),   # d_out's last double is v's first
        (dict(out=(1 << 20) + 3 * 13 * 8 - 8), b"overlaps"),           # the last entry of the trig table
        (dict(scratch=1 << 24), b"overlaps"),                           # the scratch on d_out
    ]
    for kw, word in cases:
        assert _call(lib, **kw) == H.RWRT_ERR_ARG, kw
        assert word in lib.rwrt_last_error(), (kw, lib.rwrt_last_error())
        assert lib.rwrt_last_error().startswith(b"rwrt_bs_diag: ")
    # just clear of the inputs: fine (no levels, so no device is touched)
    assert _call(lib, nlev=0) == H.RWRT_OK
    assert _call(lib, nlev=0, out=4096) == H.RWRT_OK                    # nothing is written: nothing overlaps
    assert _call(lib, nlev=0, select=bk, scratch=None, scratch_levels=-1) == H.RWRT_OK
    # no q plane: the scratch and scratch_levels are not looked at
    for sel in (bk, 1, (1 << 9) - 1 - (1 << 2), bk | (1 << 4)):
        assert _call(lib, nlev=0, select=sel, scratch=None, scratch_levels=0) == H.RWRT_OK, sel
