"""The crafted history, spec variants and comparisons of the phase tests."""
import math

import numpy as np

import phase as P
from support import cases_track as CT
from support import hostprog
from support.cases_track import NRAY, device_layouts, launches_of, sum_bound  # noqa: F401
from support.rows import layout_text

NAN = math.nan
REL = 1e-12     # of S = sum(|dk| + |dl|): the bar summary's path has, a per-ray sequential sum too

# (nx, ny, weight): a coarse and a finer map, with and without a weight; three channels (-1 and 3 among the rays')
VARIANTS = {
    "7x5-amp": dict(nx=7, ny=5, weight="amp"),
    "7x5-unweighted": dict(nx=7, ny=5, weight=None),
    "36x18-ug-no-need": dict(nx=36, ny=18, weight="ug", need=None),
    "36x18-unweighted-omega": dict(nx=36, ny=18, weight=None, omega_dt=0.375),
}


def crafted_spec(name, nchan=3):
    return P.PhaseSpec(nchan=nchan, **VARIANTS[name])


def crafted_history(nt, seed, nray=NRAY, tf=None, i0=1):
    """``cases_track.crafted_history`` (41 rays, all three layouts, tails
    below, at, inside and above a launch, NaN and inf holes, channels -1 and
    3) on a copy in which no finite longitude exceeds 1e3: its two 1e300
    entries would make S, and with it every bar, meaningless.  The k and l
    columns are its uniform values in (-3, 3); latitudes pass +-pi/2."""
    h = {k: np.array(v, copy=True) for k, v in CT.crafted_history(nt, seed, nray, tf, i0).items()}
    for a in (h["rows"], h["tail"]):
        lon = a[..., 0]
        lon[np.isfinite(lon) & (np.abs(lon) > 1e3)] = 2.5
    cut = np.clip(h["tf"], i0, nt)
    for j in range(nray):                               # (the tails still repeat their row)
        assert np.array_equal(h["rows"][j, cut[j]:], np.broadcast_to(h["tail"][j], (nt - cut[j], 8)), equal_nan=True)
    return h


def wabs_ref(want):
    """Per box the sum of |w| of its deposits: ``wabs``, or ``cnt`` without a weight."""
    return want["cnt"].astype(np.float64) if want["wabs"] is None else want["wabs"]


def assert_phase(got, want, what="", factor=1):
    """cnt, nseg and dropped exactly; theta within 1e-12 max(S, 1) (where it
    is not finite: the same value); per box re and im within (1e-12 max(S_max,
    1) + 2 (n + 1) 2^-53) wabs_ref and wabs within the bound of a sum taken in
    any order.  ``want``: ``reference_phase``'s dict; ``factor``: ``got`` holds
    that many identical deliveries of the maps (the per-ray arrays of one)."""
    cnt = want["cnt"] * factor
    assert got["cnt"].dtype == np.int64 and np.array_equal(got["cnt"], cnt), (what, "cnt")
    assert int(got["dropped"]) == int(want["dropped"]) * factor, (what, "dropped", got["dropped"], want["dropped"])
    assert got["nseg"].dtype == np.int32 and np.array_equal(got["nseg"], want["nseg"]), (what, "nseg")
    S = want["S"]
    fin = np.isfinite(want["theta"])
    assert np.array_equal(got["theta"][~fin], want["theta"][~fin], equal_nan=True), (what, "theta, not finite")
    err = np.abs(got["theta"][fin] - want["theta"][fin])
    rel = err / np.maximum(S[fin], 1.0)
    print(f"{what}: max |theta err| / max(S, 1) = {rel.max() if rel.size else 0.0:.3g}")
    assert np.all(err <= REL * np.maximum(S[fin], 1.0)), (what, "theta", float(rel.max()))
    a = wabs_ref(want) * factor
    s_max = max(float(S[np.isfinite(S)].max()) if np.isfinite(S).any() else 0.0, 1.0)
    bar = (REL * s_max + 2.0 * (cnt + 1) * 2.0 ** -53) * a
    for name in ("re", "im"):
        assert np.all(np.isfinite(got[name])), (what, name)
        e = np.abs(got[name] - want[name] * factor)
        assert np.all(e <= bar), (what, name, float((e - bar).max()))
    if want["wabs"] is None:
        assert got["wabs"] is None, (what, "wabs")
    else:
        e = np.abs(got["wabs"] - want["wabs"] * factor)
        assert np.all(e <= sum_bound(cnt, a)), (what, "wabs", float(e.max()))


def assert_same_run(a, b, want, what=""):
    """Two deliveries of the same rows in different launches: theta, nseg, the
    carried rows and cnt bit for bit, dropped equal, the sums within the bound
    of a sum of the same terms taken in any order."""
    for name in ("theta", "carry"):
        x, y = a[name], b[name]
        assert np.array_equal(x, y, equal_nan=True), (what, name)
        assert np.array_equal(np.signbit(x[x == x]), np.signbit(y[y == y])), (what, name, "the sign of a zero")
    assert np.array_equal(a["nseg"], b["nseg"]) and np.array_equal(a["cnt"], b["cnt"]), what
    assert a["dropped"] == b["dropped"], what
    bound = sum_bound(want["cnt"], wabs_ref(want))
    for name in ("re", "im", "wabs"):
        if a[name] is None:
            assert b[name] is None
            continue
        assert np.all(np.abs(a[name] - b[name]) <= bound), (what, name)


def start(m, rows0):
    """Row 0 of a history ``[nray, 8]`` into the map."""
    s = m.spec
    return m.start(rows0[:, 0], rows0[:, 1], None if s.ncol < 0 else rows0[:, s.ncol],
                   None if s.wcol < 0 else rows0[:, s.wcol], k=rows0[:, 2], l=rows0[:, 3])


def numpy_with_carry(m):
    return dict(m.numpy(), carry=m.prev.cpu().numpy())


# ------------------------------------------- csrc/phase_rows.h on the host
def run_host_program(exe, spec, launches, nray=NRAY, theta0=None):
    """tests/host/phase_rows_main.cpp over ``launches`` (``launches_of``)."""
    c = spec.c_struct()
    theta0 = np.zeros(nray) if theta0 is None else np.asarray(theta0, np.float64)
    lines = [f"{c.nx} {c.ny} {c.nchan} {c.need} {c.wcol} {nray}",
             " ".join(float(x).hex() for x in (c.lat0, c.inv_dlat, c.inv_dlon, c.omega_dt)),
             " ".join(float(x).hex() for x in theta0), str(len(launches))]
    for L, layout in launches:
        lines += layout_text(L, layout)
    out = hostprog.run(exe, lines)
    floats = lambda s: np.array([float.fromhex(x) if "nan" not in x else NAN for x in s.split()])   # noqa: E731
    return {"cnt": np.array(out[0].split(), np.int64).reshape(spec.shape), "re": floats(out[1]).reshape(spec.shape),
            "im": floats(out[2]).reshape(spec.shape),
            "wabs": floats(out[3]).reshape(spec.shape) if spec.wcol >= 0 else None,
            "dropped": int(out[4].split()[1]), "theta": floats(out[5]), "nseg": np.array(out[6].split(), np.int32),
            "carry": floats(out[7]).reshape(4, nray)}
