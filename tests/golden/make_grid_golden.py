"""Generate ``tests/golden/grid_<name>.npz`` from the reference itself: its
records on the grids of ``tests/support/cases_grids.py`` (181 x 360, 19 x 36,
33 x 127, the non-cyclic 73 x 144 and 721 x 1440).

Run where the reference is present (``refharness.py`` imports it), like ``make_golden.py``:

    python tests/golden/make_grid_golden.py [name ...]

Every file is DATA: inputs and the reference's outputs on them, float64 arrays
only.  The reference's own functions produce every expected value:

* ``sha256, shape, sample``  ``BS.fields`` after ``BS.ready(xcyclic=...)``
* ``merc_*``   ``cal_bs_mercator_point(mode='numpy')[:12]`` on random points and
               the edge longitudes x latitudes below
* ``rhs_*``    ``WR.diffun_numpy`` on random states and ``make_golden.edge_states``
               rebuilt on this grid's axes
* ``step_*``   ``rk_step`` and the error norm on 256 ``(y, f, h)``
* ``row0``     the rows of ``ray_initial_numpy`` for the seed set
* ``track, hist, nacc, attempts``  ``ray_run(mode='numpy', inte_method='rk45')``,
               41 rows: ``track`` is lon, lat at every row, ``hist`` all seven
               columns at the rows ``rows``
* ``rk4``      ``ray_run(mode='numpy', inte_method='')`` at the rows ``rk4_rows``
  (``rows``, ``rk4_rows``: every row if the file then stays below the largest
  golden, else every 2nd, 3rd or 4th row and the last -- see ``write``)

The conditions of ``cases_grids.check_events`` are asserted before a file is
written.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))            # tests/: the support package
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import make_golden as G                              # noqa: E402  (loads the reference)
from support import cases_grids as CG                # noqa: E402

R, H, PI = G.R, G.H, G.PI
MAX_BYTES = os.path.getsize(os.path.join(HERE, "roots_C3.npz"))


def make_wr(name):
    """A reference WR on grid ``name`` with the seed set (main_wr.py:66-86)."""
    bg = CG.state(name)
    nc = f"grid_{name}.nc"
    H.put_nc(nc, **bg)
    s = CG.SEEDS
    ns = s["nnx"] * s["nny"]
    wr = R.wr.WR(len(CG.ZWN), ns, CG.TSTEP, (CG.NT - 1) * CG.TSTEP, CG.FREQ,
                 nx=len(bg["lon"]), ny=len(bg["lat"]), rtol=1e-6, atol=1e-6, ncfile=nc,
                 MinStepFactor=1e-3)
    wr.bs.loadbs_ncfile(nc)
    wr.bs.ready(xcyclic=CG.xcyclic(name))
    wr.set_zwn(CG.ZWN)
    wr.set_source_matrix(s["SW_lon"], s["SW_lat"], s["dlon"], s["dlat"], s["nnx"], s["nny"])
    return wr


def edge_lons(lon):
    dlon = lon[1] - lon[0]
    return np.array([0.0, -0.0, 2 * PI, np.nextafter(2 * PI, 0), 2 * PI - 1e-9,
                     lon[-1], lon[-1] + 0.5 * dlon, 4 * PI, -1e-300] + list(lon[::7]))


def edge_lats(lat):
    a = np.arccos(0.0175)                            # |cos| = 0.0175: the Mercator mask
    lo, hi = a - 1e-7, a + 1e-7
    assert np.cos(lo) > 0.0175 > np.cos(hi)
    return np.array([0.5 * PI, -0.5 * PI, np.nextafter(0.5 * PI, 0), -np.nextafter(0.5 * PI, 0),
                     lat[0], lat[1], lat[-2], lat[-1], lo, hi, -lo, -hi])


def merc_points(bs, rng, n=256):
    elon, elat = edge_lons(bs.lon), edge_lats(bs.lat)
    special = elon[:9]
    lon = np.concatenate([elon, np.resize(special, len(elat)), np.repeat(special, len(elat))])
    lat = np.concatenate([np.resize(elat, len(elon)), elat, np.tile(elat, len(special))])
    m = max(n - len(lon), 64)
    lon = np.concatenate([lon, rng.uniform(-2 * PI, 4 * PI, m)])
    lat = np.concatenate([lat, rng.uniform(-1.575, 1.575, m)])
    return lon, lat


def edge_states(bs):
    """``make_golden.edge_states`` on this grid's axes."""
    rows = []
    base = [2.0, 0.6, 5.0, 3.0, 1.0]

    def add(**kw):
        r = list(base)
        for k, v in kw.items():
            r["lon lat k l amp".split().index(k)] = v
        rows.append(r)
    nlat, nlon = len(bs.lat), len(bs.lon)
    for lat in [0.5 * PI, -0.5 * PI, np.nextafter(0.5 * PI, 0), -np.nextafter(0.5 * PI, 0),
                1.5533, -1.5533, 1.56, -1.565, 0.0, -0.0]:
        add(lat=lat)
    for lon in [0.0, -0.0, 2 * PI, -1e-300, 2 * PI - 1e-15, np.nextafter(2 * PI, 0), 4 * PI, -2 * PI,
                1e3, -1e3, 3649 * PI / 180]:
        add(lon=lon)
    for j in [0, 1, nlat // 2 - 1, nlat // 2, nlat - 2, nlat - 1]:
        add(lat=bs.lat[j])
    for i in [0, 1, nlon // 2, nlon - 1]:
        add(lon=bs.lon[i])
    add(lon=bs.lon[-1] + 0.5 * (bs.lon[1] - bs.lon[0]))
    add(lon=bs.lon[-1] + 0.5 * (bs.lon[1] - bs.lon[0]), lat=bs.lat[-2] + 0.25 * (bs.lat[1] - bs.lat[0]))
    add(lon=np.nextafter(2 * PI, 0), lat=np.nextafter(0.5 * PI, 0))
    for l in [100.0, -100.0, np.nextafter(100.0, 0), 99.99]:
        add(l=l)
    for k in [0.0, -3.0, 1e-8]:
        add(k=k)
    for v in range(5):
        r = list(base)
        r[v] = np.nan
        rows.append(r)
    add(amp=np.inf)
    add(lon=np.inf)
    return np.array(rows).T


def history(wr):
    return np.array([wr.rlon, wr.rlat, wr.rzwn, wr.rmwn, wr.ramp, wr.rug, wr.rvg]).reshape(7, CG.NT, -1)


def records(name, rng):
    wr = make_wr(name)
    bs = wr.bs
    F = bs.fields
    out = dict(sha256=np.array(G.hash_fields(F)), shape=np.array(F.shape),
               sample=F[::-(-F.shape[0] // 8), ::-(-F.shape[1] // 8), :].astype(np.float64),
               lat=bs.lat, lon=bs.lon)
    lon, lat = merc_points(bs, rng)
    with np.errstate(all="ignore"):
        out["merc_lon"], out["merc_lat"] = lon, lat
        out["merc_out"] = bs.cal_bs_mercator_point(lon.copy(), lat.copy(), mode="numpy")[:12]
        es = edge_states(bs)
        y = np.concatenate([G.random_states(rng, 512 - es.shape[1]), es], axis=1)
        d, bad = wr.diffun_numpy(y.reshape((5, -1, 1, 1)).copy())
        out["rhs_y"], out["rhs_dydt"], out["rhs_bad"] = y, d[0:5].reshape(5, -1), bad.reshape(-1)
        fun = G.fun_of(wr)
        m = 256
        ys = G.random_states(rng, m)
        ys[1] = rng.uniform(-1.3, 1.3, m)
        ys[3] = rng.uniform(-20, 20, m)
        f = fun(0, ys)
        h = 10 ** rng.uniform(0.0, 4.5, m)
        K = np.empty((7, 5, m))
        yn, _ = R.rkf45.rk_step(fun, np.zeros(m), ys, f, h, R.rkf45.RK45.A, R.rkf45.RK45.B, R.rkf45.RK45.C, K)
        scale = 1e-6 + np.maximum(np.abs(ys), np.abs(yn)) * 1e-6
        en = R.rkf45.norm(h[None, :] * np.einsum("snf,s->nf", K, R.rkf45.RK45.E) / scale)
        out.update(step_y=ys, step_f=f, step_h=h, step_K=K, step_y_new=yn, step_err=en)
        with G.StepCounter() as sc:
            G.quiet(wr.ray_run, mode="numpy", inte_method="rk45", root_method="numpy")
        hist = history(wr)
        out.update(row0=hist[:, 0].copy(), hist=hist, nacc=sc.nacc, attempts=np.array(sc.attempts))
        w4 = make_wr(name)
        G.quiet(w4.ray_run, mode="numpy", inte_method="", root_method="numpy")
        out["rk4"] = history(w4)
    return out


def kept(stride):
    return np.unique(np.concatenate([np.arange(0, CG.NT, stride), [CG.NT - 1]]))


def write(name, out):
    """The histories' live values do not compress, so a file with every row of
    both outgrows the largest golden: ``track`` (lon, lat) keeps every RK45 row,
    the seven-column histories keep every ``stride``-th row and the last, with
    the first pair of strides at which the file fits."""
    path = os.path.join(HERE, f"grid_{name}.npz")
    for s45, s4 in [(1, 1), (1, 2), (2, 2), (2, 4), (3, 4), (4, 4)]:
        rows, rk4_rows = kept(s45), kept(s4)
        thin = dict(out, track=out["hist"][:2], hist=out["hist"][:, rows], rows=rows,
                    rk4=out["rk4"][:, rk4_rows], rk4_rows=rk4_rows)
        np.savez_compressed(path, **thin)
        if os.path.getsize(path) < MAX_BYTES:
            return path, thin
    raise AssertionError((name, os.path.getsize(path)))


def main(names):
    for name in names:
        rng = np.random.default_rng([20261020, list(CG.GRIDS).index(name)])
        out = records(name, rng)
        CG.check_events(name, dict(out, track=out["hist"][:2]))     # (before anything is written)
        path, out = write(name, out)
        e = CG.check_events(name, np.load(path))
        print(name, os.path.getsize(path), "bytes, rows kept", len(out["rows"]), len(out["rk4_rows"]), e)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CG.GRIDS))
