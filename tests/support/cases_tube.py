"""The lattices, the crafted history and the comparisons of the ray-tube tests."""
import math

import numpy as np

import synthetic as S
import tube as T
from support import hostprog
from support.cases_track import device_layouts, launches_of, sum_bound  # noqa: F401
from support.rows import layout_text

NAN, INF = math.nan, math.inf
REL = 1e-12      # of a per-ray float: the bar summary's path has; only cos differs
TSTEP, NT = 7200.0, 121

# The two lattices on real rays: 7 x 6 sources x 2 wavenumbers x 3 roots = 252 slots, 121 rows of 2 h.
# (A) straddles 0 degrees east (raw longitude differences of -358 degrees must wrap) on the non-zonal
# state, where stencil separations reach 2.6 rad; (B) is the quiet one on the zonal state.
LATTICES = {
    "A": dict(kind="nonzonal", SW_lon=355.0, SW_lat=15.0, dlon=2, dlat=2, nnx=7, nny=6, zwn=[2.0, 4.0]),
    "B": dict(kind="zonal", SW_lon=100.0, SW_lat=15.0, dlon=1, dlat=1, nnx=7, nny=6, zwn=[2.0, 4.0]),
}


def lattice_cfg(name):
    kw = dict(LATTICES[name])
    kind = kw.pop("kind")
    return kind, S.config("C2", **kw)


def lattice_nbr(name, nlead=3):
    _, c = lattice_cfg(name)
    return T.lattice_neighbours(c.nnx, c.nny, c.nzwn, nlead=nlead)


# ------------------------------------------------------------ crafted history
NNX, NNY, NZ, NLEAD = 5, 4, 2, 1
NRAY = NLEAD * NNX * NNY * NZ          # 40: a partial wave
SPECS = {
    "7x5": dict(nx=7, ny=5, nchan=3),
    "36x18-inf-no-need": dict(nx=36, ny=18, nchan=3, max_sep=INF, need=None),
    "36x18-band-tight": dict(nx=36, ny=18, nchan=3, max_sep=0.2, lat_range=(-20.0, 40.0), need="ug"),
}


def crafted_spec(name):
    return T.TubeSpec(**SPECS[name])


def crafted_nbr():
    return T.lattice_neighbours(NNX, NNY, NZ, nlead=NLEAD)


def crafted_history(nt, seed, i0=1):
    """A logical history ``[40, nt, 8]`` of a 5 x 4 lattice x 2 wavenumbers
    around 0 degrees east (a third of the rays carry their longitude plus a
    multiple of 2 pi: the differences must wrap) that every row layout can hold
    in launches starting at ``i0`` or later.  The lattice is carried by a linear
    map that shears, and whose meridional scale ``1 - i / 8`` (wavenumber 0)
    passes through exactly 0 at row 8: ``jac == 0`` there, a caustic right
    after; wavenumber 1 folds in longitude later.  A small per-ray wobble makes
    the tubes differ.  Ray j's rows from ``tf[j]`` on repeat one row, with
    ``tf`` below, at, inside, at the end of and above a launch and different
    among the rays of a stencil; the j % 3 == 0 rays (no row block in the slots
    layout) are at rest from row ``i0`` on.  NaN ``need`` (amp) at row 0 of two
    rays -- their neighbours' stencils become one-sided like those on the
    lattice's edges -- and in mid-run of two others, which closes the tubes
    around them; an infinite latitude; ``ug`` NaN on one ray; channels -1 and
    3 among 0..2."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-3.0, 3.0, (NRAY, nt, 8))
    iy, ix, z = (a.reshape(-1) for a in np.meshgrid(np.arange(NNY), np.arange(NNX), np.arange(NZ), indexing="ij"))
    x0, y0 = 0.04 * (ix - 2.0), 0.03 * (iy - 1.5)
    i = np.arange(nt)[None, :]
    sy = np.where(z[:, None] == 0, 1.0 - i / 8.0, 1.0 + 0.02 * i)
    sx = np.where(z[:, None] == 0, 1.0 + 0.03 * i, 1.0 - i / 13.5)
    lon = 0.01 * i + sx * x0[:, None] + 0.5 * (i / nt) * y0[:, None]
    lat = 0.3 + 0.004 * i + sy * y0[:, None]
    lon = lon + 0.002 * np.cumsum(rng.uniform(-1.0, 1.0, (NRAY, nt)), axis=1) * (i > 9)
    lat = lat + 0.002 * np.cumsum(rng.uniform(-1.0, 1.0, (NRAY, nt)), axis=1) * (i > 9)
    lon = lon + 2.0 * math.pi * np.where(np.arange(NRAY) % 3 == 1, rng.integers(-2, 3, NRAY), 0)[:, None]
    rows[..., 0], rows[..., 1] = lon, lat
    rows[..., 4] = 1.0
    rows[13, 0, 4] = NAN                      # invalid at row 0: no tube, its neighbours one-sided
    rows[26, 0, 4] = NAN
    rows[17, min(12, nt - 1):, 4] = NAN       # dies in mid-run
    rows[31, min(5, nt - 1), 4] = NAN         # one bad row closes for good
    rows[22, min(15, nt - 1), 1] = INF
    rows[8, min(3, nt - 1), 5] = NAN          # (matters with need = 'ug' only)
    choice = sorted({i0 - 2, i0, i0 + 1, i0 + 3, i0 + 4, i0 + 5, nt - 1, nt, nt + 3})
    j = np.arange(NRAY)
    q = np.cumsum(j % 3 != 0)                 # (the rays with a block take every value)
    late = np.array([nt - 1, nt, nt + 3])     # (three block rays in four move to the end: whole stencils that do)
    tf = np.where(j % 3 == 0, np.array([i0 - 2, i0])[(j // 3) % 2],
                  np.where(q % 4 == 0, np.array(choice)[(q // 4) % len(choice)], late[q % 3])).astype(np.int32)
    cut = np.clip(tf, i0, nt)
    tail = rows[:, -1].copy()
    for r in range(NRAY):
        if cut[r] < nt:
            tail[r] = rows[r, cut[r]]
            rows[r, cut[r]:] = tail[r]
    chan = rng.integers(0, 3, NRAY).astype(np.int32)
    chan[[6, 33]] = [-1, 3]
    return dict(rows=rows, tail=tail, tf=tf, chan=chan)


# ------------------------------------------------------------- comparisons
INTS = ("cnt", "ncaus", "mu", "first", "nrow", "close_row")
FLOATS = ("dmin", "dlast", "f0", "flast")


def assert_tube(got, want, what=""):
    """The integers exactly; the per-ray floats within 1e-12 relative (NaN
    where the reference has NaN); slog per box within the bound of a sum taken
    in any order, on the summed magnitudes of its terms."""
    for k in INTS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    assert int(got["dropped"]) == int(want["dropped"]), (what, "dropped", got["dropped"], want["dropped"])
    has = want["nrow"] > 0
    assert np.array_equal(got["code"][:, has], want["code"][:, has]), (what, "code")
    worst = 0.0
    for k in FLOATS:
        g, w = got[k], want[k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k, "NaN")
        fin = ~np.isnan(w)
        err = np.abs(g[fin] - w[fin])
        if err.size:
            worst = max(worst, float((err / np.maximum(np.abs(w[fin]), 1e-300)).max()))
        assert np.all(err <= REL * np.abs(w[fin])), (what, k)
    bound = sum_bound(want["cnt"], want["sabs"])
    err = np.abs(got["slog"] - want["slog"])
    hit = want["cnt"] > 0
    ratio = float((err[hit] / np.maximum(bound[hit], 1e-300)).max()) if hit.any() else 0.0
    print(f"{what}: per-ray floats max rel err {worst:.3g}; slog max err / bound {ratio:.3g}, "
          f"max |err| {float(err.max()):.3g}")
    assert np.all(np.isfinite(got["slog"])), (what, "slog")
    assert np.all(err <= bound), (what, "slog", ratio)


def assert_same_run(a, b, want, what=""):
    """Two deliveries of the same rows in different launches or layouts: the
    integers equal, the per-ray floats bit for bit, slog within the bound."""
    for k in INTS + ("code",):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["dropped"] == b["dropped"], what
    for k in FLOATS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert np.all(np.abs(a["slog"] - b["slog"]) <= sum_bound(want["cnt"], want["sabs"])), (what, "slog")


def start(m, rows0):
    """Row 0 of a history ``[nray, 8]`` into the map."""
    s = m.spec
    return m.start(rows0[:, 0], rows0[:, 1], None if s.ncol < 0 else rows0[:, s.ncol])


# -------------------------------------------- csrc/tube_rows.h on the host
def run_host_program(exe, spec, nbr, launches, nray=NRAY):
    """tests/host/tube_rows_main.cpp over ``launches`` (``launches_of``)."""
    c = spec.c_struct()
    lines = [f"{c.nx} {c.ny} {c.nchan} {c.need} {nray}",
             " ".join(float(x).hex() for x in (c.lat0, c.inv_dlat, c.inv_dlon, c.max_sep))]
    lines += [" ".join(str(int(v)) for v in row) for row in np.asarray(nbr)]
    lines.append(str(len(launches)))
    for L, layout in launches:
        lines += layout_text(L, layout)
    out = hostprog.run(exe, lines)
    floats = lambda s: np.array([float.fromhex(x) if "nan" not in x else NAN for x in s.split()])   # noqa: E731
    st = np.array(out[4].split(), np.int32).reshape(T.NSTATE_I, nray)
    pv = floats(out[5]).reshape(T.NSTATE_F, nray)
    return {"cnt": np.array(out[0].split(), np.int64).reshape(spec.shape),
            "ncaus": np.array(out[1].split(), np.int64).reshape(spec.shape),
            "slog": floats(out[2]).reshape(spec.shape), "dropped": int(out[3].split()[1]),
            "bad": int(out[3].split()[3]), "mu": st[1], "first": st[2], "nrow": st[3], "close_row": st[4],
            "dmin": pv[3], "dlast": pv[4], "f0": pv[5:9], "flast": pv[9:13],
            "code": np.stack([st[0] & 3, (st[0] >> 2) & 3]).astype(np.int32)}
