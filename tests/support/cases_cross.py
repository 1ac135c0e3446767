"""Gates, spec variants and comparisons of the cross tests."""
import numpy as np

import cross as X
from cross import CrossSpec, Gate, reference_cross
from support.cases_track import sum_bound


# ---------------------------------------------------- the reference's C1 history
C1_GATES = (Gate.lat(30.0), Gate.lat(0.0), Gate.lon(180.0))
C1_NORTH, C1_SOUTH = [0, 77, 55], [0, 78, 56]
C1_WINDOWS = [23, 28, 27, 31, 31, 32, 33, 31, 30]
C1_EAST = [0, 10, 8]


def c1_spec(**kw):
    return CrossSpec(C1_GATES, 36, window_rows=120, nt=1081, **kw)


def assert_c1(r, what=""):
    """The literals of the definition on the C1 history (3 roots, 1081 rows, by root)."""
    cnt = r["cnt"]
    assert cnt.shape == (9, 3, 2, 3, 36), what
    g30 = cnt[:, 0]
    assert g30.sum(axis=(0, 2, 3)).tolist() == [132, 134], what
    assert g30.sum(axis=(0, 3)).tolist() == [C1_NORTH, C1_SOUTH], what
    assert np.count_nonzero(g30.sum(axis=(0, 1, 2))) == 36, what
    assert g30.sum(axis=(1, 2, 3)).tolist() == C1_WINDOWS, what
    assert r["ncross"][0].tolist() == [C1_NORTH, C1_SOUTH], what
    assert r["tfirst"][0, 1, 1] == 0.0 and np.isnan(r["tfirst"][0, :, 0]).all(), what   # the source lies on the gate
    assert cnt[:, 1].sum() == 0 and r["ncross"][1].sum() == 0 and np.isnan(r["tfirst"][1]).all(), what
    m180 = cnt[:, 2]
    assert m180.sum(axis=(0, 3)).tolist() == [C1_EAST, [0, 0, 0]], what
    assert np.count_nonzero(m180.sum(axis=(0, 1, 2))) == 4 and r["dropped"] == 0, what
    assert r["ncross"][2].tolist() == [C1_EAST, [0, 0, 0]], what


# ------------------------------------------------------------- crafted launches
GATES8 = (Gate.lat(0.0), Gate.lon(0.0), Gate.lat(30.0), Gate.lon(90.0), Gate.lat(-20.0), Gate.lon(180.0),
          Gate.lat(72.0), Gate.lon(270.0))
VARIANTS = {
    "8-gates-weight-windows": dict(gates=GATES8, weight="ug", window_rows=3),
    "8-gates": dict(gates=GATES8),
    "1-gate-weight": dict(gates=GATES8[:1], weight="vg", need=None),
    "1-meridian-windows": dict(gates=GATES8[1:2], window_rows=3),
    "3-gates-weight": dict(gates=GATES8[2:5], weight="k"),
}


def crafted_spec(name, nt, **kw):
    v = dict(VARIANTS[name])
    if v.get("window_rows"):
        v["nt"] = nt
    return CrossSpec(nbin=7, nchan=3, lat_range=(-60.0, 60.0), **{**v, **kw})


def reference_and_abs(rows, chan, spec):
    """``reference_cross`` and the per-bin sums of |tc| and |wv| (the sum|v| of
    the rounding bound) in one pass over the crossings."""
    rows = np.asarray(rows, np.float64)
    want = reference_cross(rows, chan, spec)
    a = np.zeros((2,) + spec.shape)
    for x in X.crossings(rows, chan, spec):
        if x is not None and x[5] >= 0:
            g, d, j, c, w, b, t, tc, wv = x
            a[0, w, g, d, c, b] += abs(tc)
            a[1, w, g, d, c, b] += abs(wv)
    return want, a


def assert_cross(got, want, a=None, what="", per_ray=True):
    """cnt, dropped and ncross exactly, tfirst bit for bit; tsum and wsum
    exactly (``a`` None) or to the bound."""
    assert got["cnt"].dtype == np.int64 and np.array_equal(got["cnt"], want["cnt"]), (what, "cnt")
    assert int(got["dropped"]) == int(want["dropped"]), (what, "dropped", got["dropped"], want["dropped"])
    if per_ray:
        assert got["ncross"].dtype == np.int32 and np.array_equal(got["ncross"], want["ncross"]), (what, "ncross")
        same = got["tfirst"].view(np.int64) == want["tfirst"].view(np.int64)
        assert np.all(same | (np.isnan(got["tfirst"]) & np.isnan(want["tfirst"]))), (what, "tfirst")
    for q, name in enumerate(("tsum", "wsum")):
        if want[name] is None:
            assert got[name] is None, (what, name)
            continue
        assert np.all(np.isfinite(got[name])), (what, name)
        if a is None:
            assert np.array_equal(got[name], want[name]), (what, name)
        else:
            err = np.abs(got[name] - want[name])
            assert np.all(err <= sum_bound(want["cnt"], a[q])), (what, name, float(err.max()))


def assert_crafted_is_rich(rows, chan, spec):
    """More than 50 crossings, both directions on both kinds, a drop and a
    meridian crossing outside lat_range: checked on the definition's side."""
    xs = list(X.crossings(rows, chan, spec))
    hits = [x for x in xs if x is not None]
    kinds = {(spec.gates[x[0]].kind, x[1]) for x in hits}
    assert len(hits) > 50 and xs.count(None) >= 1, (len(hits), xs.count(None))
    assert kinds == {(k, d) for k in {g.kind for g in spec.gates} for d in (0, 1)}, kinds
    if any(g.kind == 1 for g in spec.gates):
        assert any(x[5] < 0 for x in hits if spec.gates[x[0]].kind == 1)
