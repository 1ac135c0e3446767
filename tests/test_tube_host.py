"""Ray-tube maps, host side (no GPU): the definition ``tube.reference_tube``
against a slow per-ray loop and on written-out tubes, ``lattice_neighbours``,
the spec, the shared per-row code csrc/tube_rows.h in a stand-alone program
under the sanitizers (crafted launches in all three row layouts and in several
splits), the argument checks of ``rwrt_ray_tube`` and what ``WR.ray_tube``
refuses before any work."""
import ctypes
import math

import numpy as np
import pytest

import _hip as H
import tube as T
from support import hostprog
from support.abi import refused
from support.cases_tube import (NNX, NRAY, NZ, SPECS, assert_same_run, assert_tube, crafted_history,
                                crafted_nbr, crafted_spec, launches_of, run_host_program)
from support.rows import LAYOUTS
from tube import TubeSpec, lattice_neighbours, reference_tube

INF, NAN = math.inf, math.nan
PI = math.pi


# ------------------------------------------------ the definition, once more
def _wrap(d):
    return ((d + PI) % (2 * PI)) % (2 * PI) - PI


def _valid(r, spec):
    ok = math.isfinite(r[0]) and math.isfinite(r[1]) and abs(r[1]) < T.HALF_PI
    return ok and (spec.ncol < 0 or math.isfinite(r[spec.ncol]))


def slow_tube(rows, nbr, chan, spec):
    """The definition as the issue words it, one ray and one row at a time, in
    Python floats (``np.cos`` / ``np.log`` on one value, so that the
    transcendentals are the reference's)."""
    nray, nt = rows.shape[:2]
    sh = spec.shape
    out = dict(cnt=np.zeros(sh, np.int64), ncaus=np.zeros(sh, np.int64), slog=np.zeros(sh), dropped=0,
               mu=np.zeros(nray, np.int32), first=np.full(nray, -1, np.int32), nrow=np.zeros(nray, np.int32),
               close_row=np.full(nray, -1, np.int32), dmin=np.full(nray, NAN), dlast=np.full(nray, NAN),
               f0=np.full((4, nray), NAN), flast=np.full((4, nray), NAN))
    terms = [[] for _ in range(sh[0] * sh[1] * sh[2])]
    for j in range(nray):
        c = 0 if chan is None else int(chan[j])
        if not (0 <= c < spec.nchan and _valid(rows[j, 0], spec)):
            continue
        pairs = []
        for lo, hi in ((nbr[0, j], nbr[1, j]), (nbr[2, j], nbr[3, j])):
            vl = lo >= 0 and _valid(rows[lo, 0], spec)
            vh = hi >= 0 and _valid(rows[hi, 0], spec)
            pairs.append((lo, hi) if vl and vh else (j, hi) if vh else (lo, j) if vl else None)
        if None in pairs:
            continue
        (pa, qa), (pb, qb) = pairs
        a0 = jprev = None
        for i in range(nt):
            pts = [rows[k, i] for k in (j, pa, qa, pb, qb)]
            dla, dpa = _wrap(float(pts[2][0]) - float(pts[1][0])), float(pts[2][1]) - float(pts[1][1])
            dlb, dpb = _wrap(float(pts[4][0]) - float(pts[3][0])), float(pts[4][1]) - float(pts[3][1])
            if not (all(_valid(r, spec) for r in pts) and max(abs(dla), abs(dpa), abs(dlb), abs(dpb)) <= spec.max_sep):
                out["close_row"][j] = i
                break
            jac = dla * dpb - dlb * dpa
            cs = float(np.cos(np.float64(pts[0][1])))
            if i == 0:
                if jac == 0.0:
                    break
                a0 = jac * cs
            caustic = i > 0 and (jac < 0.0) != (jprev < 0.0)
            jprev = jac
            D = (jac * cs) / a0
            out["nrow"][j] += 1
            out["dmin"][j] = abs(D) if not out["dmin"][j] <= abs(D) else out["dmin"][j]
            out["dlast"][j] = D
            out["flast"][:, j] = (dla * cs, dpa, dlb * cs, dpb)
            if i == 0:
                out["f0"][:, j] = out["flast"][:, j]
            if caustic:
                out["mu"][j] += 1
                if out["first"][j] < 0:
                    out["first"][j] = i
            lam = (float(pts[0][0]) % (2 * PI)) % (2 * PI)
            fy = math.floor((float(pts[0][1]) - spec.lat0) * spec.inv_dlat)
            if not 0 <= fy < spec.ny:
                continue
            at = (c, int(fy), int(min(math.floor(lam * spec.inv_dlon), spec.nx - 1)))
            if caustic:
                out["ncaus"][at] += 1
            if jac == 0.0:
                out["dropped"] += 1
                continue
            out["cnt"][at] += 1
            terms[(at[0] * sh[1] + at[1]) * sh[2] + at[2]].append(float(np.log(np.float64(abs(D)))))
    out["slog"] = np.array([math.fsum(t) for t in terms]).reshape(sh)
    return out


def _rich(want, h, spec):
    """What the crafted history has to show (printed: the numbers behind the asserts)."""
    nbr = crafted_nbr()
    one_sided = ((want["code"] > 1) & (want["nrow"] > 0)[None, :]).any(axis=0)
    st = dict(tubes=int((want["nrow"] > 0).sum()), closing=int((want["close_row"] > 0).sum()),
              caustics=int(want["mu"].sum()), in_map=int(want["ncaus"].sum()), dropped=int(want["dropped"]),
              one_sided=int(one_sided.sum()), deposits=int(want["cnt"].sum()), edge=int((nbr < 0).any(axis=0).sum()))
    print(spec, st)
    return st


@pytest.mark.parametrize("name", sorted(SPECS))
def test_reference_equals_the_slow_loop_on_the_crafted_history(name):
    """reference_tube (vectorised over the rays) against the per-ray loop:
    every integer and every per-ray float the same value, slog within the
    rounding of a sum (the loop's is exact: fsum)."""
    spec = crafted_spec(name)
    h = crafted_history(24, seed=3)
    nbr = crafted_nbr()
    want = reference_tube(h["rows"], nbr, h["chan"], spec)
    slow = slow_tube(h["rows"], nbr, h["chan"], spec)
    st = _rich(want, h, name)
    assert st["tubes"] >= 20 and st["caustics"] >= 10 and st["one_sided"] >= 8 and st["closing"] >= 5
    assert st["deposits"] >= 100 and st["edge"] >= 20
    if name == "7x5":
        assert st["dropped"] >= 1                       # jac == 0 in an open row
    for k in ("cnt", "ncaus", "mu", "first", "nrow", "close_row"):
        assert np.array_equal(want[k], slow[k]), k
    assert want["dropped"] == slow["dropped"]
    for k in ("dmin", "dlast", "f0", "flast"):
        assert np.array_equal(want[k], slow[k], equal_nan=True), k
    assert np.all(np.abs(want["slog"] - slow["slog"]) <= (want["cnt"] + 1) * 2.0 ** -53 * want["sabs"])
    # a channel outside [0, nchan), a ray invalid at row 0: no tube
    off = ~((h["chan"] >= 0) & (h["chan"] < 3))
    assert off.sum() == 2 and (want["nrow"][off] == 0).all() and (want["close_row"][off] == -1).all()
    if spec.need == "amp":
        assert want["nrow"][13] == 0 and np.isnan(want["dmin"][13]) and want["nrow"][26] == 0


def test_written_out_tubes():
    """A 3 x 3 lattice, one wavenumber, the centre ray's tube: D == 1 at row
    0; a uniform stretch by 2 in longitude doubles it; a reflection is a
    caustic; differences across 0 degrees wrap; jac_0 == 0 is no tube; max_sep
    closes."""
    nbr = lattice_neighbours(3, 3, 1, nlead=1)
    assert nbr[:, 4].tolist() == [3, 5, 1, 7] and nbr[:, 0].tolist() == [-1, 1, -1, 3]
    iy, ix = (a.reshape(-1) for a in np.meshgrid(np.arange(3), np.arange(3), indexing="ij"))
    spec = TubeSpec(8, 4, need=None)

    def hist(scales, lon0=1.0):
        r = np.zeros((9, len(scales), 8))
        for i, (sx, sy) in enumerate(scales):
            r[:, i, 0] = lon0 + 0.0625 * sx * (ix - 1)
            r[:, i, 1] = 0.03125 * sy * (iy - 1)
        return r

    got = reference_tube(hist([(1, 1), (2, 1), (2, -1), (2, -1), (-2, -1)]), nbr, None, spec)
    assert got["nrow"].tolist() == [5] * 9 and got["close_row"].tolist() == [-1] * 9
    # (wrap adds and subtracts pi: a longitude difference carries that rounding, a latitude difference none)
    assert got["mu"][4] == 2 and got["first"][4] == 2 and abs(got["dlast"][4] - 2.0) < 1e-13 and got["dmin"][4] == 1.0
    assert got["code"][:, 4].tolist() == [1, 1] and got["code"][:, 0].tolist() == [2, 2]
    assert got["code"][:, 8].tolist() == [3, 3]
    assert np.allclose(got["f0"][:, 4], [0.125, 0.0, 0.0, 0.0625], rtol=1e-13, atol=0.0)
    assert np.allclose(got["flast"][:, 4], [-0.25, 0.0, 0.0, -0.0625], rtol=1e-13, atol=0.0)
    assert got["cnt"].sum() == 45 and got["ncaus"].sum() == 18 and got["dropped"] == 0
    # log 1 + log 2 + log 2 + log 2 + log 2 in the centre ray's box (the equator rays share it)
    assert abs(got["slog"].sum() - 9 * 4 * math.log(2.0)) < 1e-9
    # across 0 degrees: the same tubes
    wrapped = hist([(1, 1), (2, 1), (2, -1)], lon0=0.0)
    wrapped[..., 0] %= 2 * PI
    assert wrapped[..., 0].max() > 6.0
    a, b = reference_tube(wrapped, nbr, None, spec), reference_tube(hist([(1, 1), (2, 1), (2, -1)]), nbr, None, spec)
    assert np.array_equal(a["mu"], b["mu"]) and np.allclose(a["dlast"], b["dlast"], rtol=1e-13)
    assert a["mu"].tolist() == [1] * 9
    # jac_0 == 0: no tube; jac == 0 later: dropped, non-negative
    flat = reference_tube(hist([(1, 0), (1, 1)]), nbr, None, spec)
    assert flat["nrow"].tolist() == [0] * 9 and flat["close_row"].tolist() == [-1] * 9 and flat["cnt"].sum() == 0
    zero = reference_tube(hist([(1, 1), (1, 0), (1, 1), (1, -1)]), nbr, None, spec)
    assert zero["dropped"] == 9 and zero["mu"].tolist() == [1] * 9 and zero["first"].tolist() == [3] * 9
    assert zero["dmin"].tolist() == [0.0] * 9 and zero["cnt"].sum() == 27
    # max_sep: the stretch to 0.25 rad between W and E closes the centred tubes at row 1
    tight = reference_tube(hist([(1, 1), (2, 1), (1, 1)]), nbr, None, TubeSpec(8, 4, need=None, max_sep=0.2))
    assert tight["close_row"][4] == 1 and tight["nrow"][4] == 1 and tight["close_row"][0] == -1
    with pytest.raises(ValueError):
        reference_tube(hist([(1, 1)]), nbr[:, :8], None, spec)
    with pytest.raises(ValueError):
        reference_tube(hist([(1, 1)]), np.full((4, 9), 9), None, spec)
    with pytest.raises(ValueError):
        reference_tube(hist([(1, 1)]), nbr, [0, 1], spec)


def test_sigma_max_is_the_largest_singular_value():
    rng = np.random.default_rng(5)
    f0, f1 = rng.normal(size=(4, 50)), rng.normal(size=(4, 50))
    got = T.sigma_max(f0, f1)
    for j in range(50):
        F0 = np.array([[f0[0, j], f0[2, j]], [f0[1, j], f0[3, j]]])
        F1 = np.array([[f1[0, j], f1[2, j]], [f1[1, j], f1[3, j]]])
        want = np.linalg.svd(F1 @ np.linalg.inv(F0), compute_uv=False)[0]
        assert abs(got[j] - want) <= 1e-9 * want


# ------------------------------------------------------ lattice_neighbours
def test_lattice_neighbours_edges_and_cyclic_x():
    nbr = lattice_neighbours(4, 3, 2, nlead=3)
    assert nbr.shape == (4, 72) and nbr.dtype == np.int32
    idx = lambda lead, jy, jx, z: ((lead * 3 + jy) * 4 + jx) * 2 + z      # noqa: E731
    j = idx(1, 1, 2, 1)
    assert nbr[:, j].tolist() == [idx(1, 1, 1, 1), idx(1, 1, 3, 1), idx(1, 0, 2, 1), idx(1, 2, 2, 1)]
    assert nbr[:, idx(2, 0, 0, 0)].tolist() == [-1, idx(2, 0, 1, 0), -1, idx(2, 1, 0, 0)]
    assert nbr[:, idx(0, 2, 3, 1)].tolist() == [idx(0, 2, 2, 1), -1, idx(0, 1, 3, 1), -1]
    # a neighbour has the same lead and zwn, and the relation is mutual
    for d, back in ((0, 1), (1, 0), (2, 3), (3, 2)):
        has = nbr[d] >= 0
        assert np.array_equal(nbr[back][nbr[d][has]], np.where(has)[0])
        assert np.array_equal(nbr[d][has] % 2, np.where(has)[0] % 2)
        assert np.array_equal(nbr[d][has] // 24, np.where(has)[0] // 24)
    assert (nbr[0] < 0).sum() == 3 * 3 * 2 and (nbr[2] < 0).sum() == 3 * 4 * 2
    cyc = lattice_neighbours(4, 3, 2, nlead=3, cyclic_x=True)
    assert (cyc[:2] >= 0).all() and np.array_equal(cyc[2:], nbr[2:])
    assert cyc[0, idx(2, 0, 0, 0)] == idx(2, 0, 3, 0) and cyc[1, idx(0, 2, 3, 1)] == idx(0, 2, 0, 1)
    one = lattice_neighbours(1, 1, 1, nlead=1)
    assert one.tolist() == [[-1]] * 4
    for bad in (dict(nnx=0), dict(nny=0), dict(nzwn=0), dict(nlead=0), dict(nnx=1 << 16, nny=1 << 16)):
        with pytest.raises(ValueError):
            lattice_neighbours(**{**dict(nnx=2, nny=2, nzwn=1), **bad})


# ---------------------------------------------------------------- the spec
def test_spec():
    assert ctypes.sizeof(H.TubeMapC) == 48
    s = TubeSpec(36, 18)
    assert (s.nchan, s.lat_range, s.need, s.max_sep) == (1, (-90, 90), "amp", 0.5)
    assert s.shape == (1, 18, 36) and (s.ncol, s.wcol) == (4, -1)
    u = TubeSpec(1440, 720, nchan=3, lat_range=(-60, 60), need=None, max_sep=INF)
    c = u.c_struct()
    assert (c.nx, c.ny, c.nchan, c.need) == (1440, 720, 3, -1)
    assert (c.lat0, c.inv_dlat, c.inv_dlon, c.max_sep) == (-PI / 3, 720 / (PI / 3 - -PI / 3), 1440 / (2 * PI), INF)
    from raymap import with_channels
    assert with_channels(u, 7).nchan == 7 and with_channels(u, 7).max_sep == INF
    with pytest.raises(Exception):
        u.nx = 3                                         # frozen
    for bad in (dict(nx=0), dict(ny=-1), dict(nchan=0), dict(nx=2 ** 16, ny=2 ** 15), dict(lat_range=(10.0, 10.0)),
                dict(need="lon"), dict(max_sep=0.0), dict(max_sep=-1.0), dict(max_sep=NAN)):
        with pytest.raises(ValueError):
            TubeSpec(**{**dict(nx=7, ny=5), **bad})


# -------------------------------------------- csrc/tube_rows.h on the host
host_program = hostprog.fixture("tube_rows")
SPLITS = {"one": [(1, 24)], "three": [(1, 9), (9, 10), (10, 24)], "five": [(1, 4), (4, 8), (8, 9), (9, 17), (17, 24)]}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_rows_host_program_under_sanitizers(host_program, name):
    """csrc/tube_rows.h (what the kernel calls) in a stand-alone program built
    with ASan + UBSan and run directly: row 0, then the launch [1, 24) with
    tail_from below, at, inside, at the end of and above it, different among
    the rays of a stencil, and rays without a row block, in all three row
    layouts and in three splits: the integers equal reference_tube, the
    per-ray floats within 1e-12, slog within the bound; every split and layout
    gives the same per-ray floats bit for bit."""
    spec = crafted_spec(name)
    h = crafted_history(24, seed=3)
    nbr = crafted_nbr()
    assert {-1, 1, 2, 23, 24, 27} <= set(h["tf"].tolist())
    want = reference_tube(h["rows"], nbr, h["chan"], spec)
    first = None
    for layout in LAYOUTS:
        for split, bounds in SPLITS.items():
            got = run_host_program(host_program, spec, nbr, launches_of(h, bounds, layout))
            assert got["bad"] == 0
            assert_tube(got, want, (name, layout, split))
            first = first or got
            assert_same_run(first, got, want, (name, layout, split))


def test_rows_host_program_whole_history_and_bad_neighbours(host_program):
    """One dense launch [0, 24) fixes the stencil itself; a neighbour index
    out of range is not followed: the error flag is set and the ray has no
    tube, the rays that do not point at it are as before."""
    spec = crafted_spec("7x5")
    h = crafted_history(24, seed=4)
    nbr = crafted_nbr()
    want = reference_tube(h["rows"], nbr, h["chan"], spec)
    whole = [(dict(i0=0, i1=24, rows=h["rows"], tail=h["tail"], tf=np.full(NRAY, 24), chan=h["chan"]), "dense")]
    got = run_host_program(host_program, spec, nbr, whole)
    assert got["bad"] == 0
    assert_tube(got, want, "one launch from row 0")
    bad = nbr.copy()
    j = (1 * NNX + 2) * NZ                               # an interior ray with a channel in range
    assert 0 <= h["chan"][j] < 3 and want["nrow"][j] > 0
    bad[1, j] = NRAY
    bad[2, j + 1] = -2
    got = run_host_program(host_program, spec, bad, launches_of(h, [(1, 24)], "slots"))
    assert got["bad"] == 1
    # an index out of range counts as no neighbour: the stencil is one-sided there
    fixed = bad.copy()
    fixed[1, j] = fixed[2, j + 1] = -1
    assert_tube(got, reference_tube(h["rows"], fixed, h["chan"], spec), "out of range as none")


# ----------------------------------------------------------- C entry point
def _call(lib, m, nray=16, i0=1, i1=5, rows=64, slot=None, tfrom=None, trow=None, chan=None, nbr=64, si=64, sf=64,
          cnt=64, slog=64, ncaus=64, dropped=64, err=64):
    """rwrt_ray_tube with fake (never dereferenced) device pointers."""
    return lib.rwrt_ray_tube(None if m is None else ctypes.byref(m), nray, i0, i1, rows, slot, tfrom, trow, chan,
                             nbr, si, sf, cnt, slog, ncaus, dropped, err, None)


def test_tube_argument_errors_without_a_gpu():
    """Every check happens before any HIP call and names the argument."""
    lib = H.load()
    assert "rwrt_ray_tube" in H.ABI_SYMBOLS and hasattr(lib, "rwrt_ray_tube")
    assert "abi 5" in H.version()                      # an additive member: the version stays
    spec = TubeSpec(7, 5, nchan=2, lat_range=(-60.0, 60.0))
    good = spec.c_struct()

    def m(**kw):
        c = spec.c_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    cases = [
        (dict(m=None), b"map"),
        (dict(m=m(nx=0)), b"nx"), (dict(m=m(ny=-1)), b"ny"), (dict(m=m(nchan=0)), b"nchan"),
        (dict(m=m(nx=1 << 16, ny=1 << 15)), b"2^31"), (dict(m=m(nx=1 << 15, ny=1 << 10, nchan=1 << 6)), b"2^31"),
        (dict(m=m(need=0)), b"need"), (dict(m=m(need=1)), b"need"), (dict(m=m(need=7)), b"need"),
        (dict(m=m(need=-2)), b"need"),
        (dict(m=m(inv_dlon=0.0)), b"inv_dlon"), (dict(m=m(inv_dlon=NAN)), b"inv_dlon"),
        (dict(m=m(inv_dlon=INF)), b"inv_dlon"), (dict(m=m(inv_dlat=-1.0)), b"inv_dlat"),
        (dict(m=m(inv_dlat=INF)), b"inv_dlat"), (dict(m=m(lat0=NAN)), b"lat0"), (dict(m=m(lat0=-INF)), b"lat0"),
        (dict(m=m(max_sep=0.0)), b"max_sep"), (dict(m=m(max_sep=-0.5)), b"max_sep"), (dict(m=m(max_sep=NAN)), b"max_sep"),
        (dict(m=good, i0=5, i1=5), b"it_begin"), (dict(m=good, i0=6, i1=5), b"it_begin"),
        (dict(m=good, i0=-1, i1=3), b"it_begin"),
        (dict(m=good, slot=64), b"d_row_slot"),
        (dict(m=good, tfrom=64), b"d_tail_row"), (dict(m=good, trow=64), b"d_tail_from"),
        (dict(m=good, rows=None), b"d_rows"),
        (dict(m=good, nray=-1), b"nray"), (dict(m=good, nray=1 << 31), b"nray"),
        (dict(m=good, rows=72), b"16-byte"), (dict(m=good, tfrom=64, trow=72), b"16-byte"),
        (dict(m=good, nbr=None), b"d_nbr"), (dict(m=good, si=None), b"d_state_i"), (dict(m=good, sf=None), b"d_state_f"),
        (dict(m=good, cnt=None), b"d_cnt"), (dict(m=good, slog=None), b"d_slog"), (dict(m=good, ncaus=None), b"d_ncaus"),
        (dict(m=good, dropped=None), b"d_dropped"), (dict(m=good, err=None), b"d_err"),
    ]
    for kw, word in cases:
        refused(lib, _call, kw, word, b"rwrt_ray_tube: ")
    # the output pointers are checked with no rays too
    assert _call(lib, good, nray=0, rows=None, cnt=None) == H.RWRT_ERR_ARG
    # no rays: a no-op (no device is touched; there is none on the build host)
    assert _call(lib, good, nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, good, nray=0, rows=None, i0=0, i1=1) == H.RWRT_OK
    assert _call(lib, m(need=-1, max_sep=INF), nray=0, rows=None, i0=100, i1=200) == H.RWRT_OK
    assert _call(lib, TubeSpec(1440, 720, nchan=12).c_struct(), nray=0, rows=None) == H.RWRT_OK


# ------------------------------------------------------------ WR.ray_tube
def test_ray_tube_refusals_before_any_work():
    """A process group, and sources without a lattice and without nbr, are
    refused before ray_initial (which would need the basic state): row 0 of
    the history stays untouched."""
    from wr import WR
    w = WR(2, 6, 7200.0, 86400.0, 0.0, nx=144, ny=73)
    w.set_zwn([2.0, 4.0])
    spec = TubeSpec(36, 18)
    w.set_source_array([10.0, 12.0, 14.0, 10.0, 12.0, 14.0], [20.0, 20.0, 20.0, 22.0, 22.0, 22.0])
    with pytest.raises(ValueError, match="nbr"):
        w.ray_tube(spec)
    w.set_source_matrix(10.0, 20.0, 2.0, 2.0, 3, 2)
    assert (w.source_nnx, w.source_nny, w.source_dlon, w.source_cyclic_x) == (3, 2, 2.0, False)
    with pytest.raises(NotImplementedError, match="neighbours"):
        w.ray_tube(spec, group=object())
    with pytest.raises(ValueError):
        w.ray_tube(spec, nbr=np.zeros((4, 5), np.int32))
    with pytest.raises(ValueError):
        w.ray_tube(spec, by="source")
    assert np.isnan(w.rlon).all()
    # sources all around a latitude circle are cyclic in x
    c = WR(1, 8, 7200.0, 86400.0, 0.0, nx=144, ny=73)
    c.set_source_matrix(0.0, 20.0, 90.0, 2.0, 4, 2)
    assert c.source_cyclic_x is True
    c.set_source_array(list(range(8)), [0.0] * 8)
    assert c.source_nnx is None
