"""The specs, the per-deposit record and the comparisons of the wave-map tests
(the crafted history and the lattices are ``cases_tube``'s)."""
import math

import numpy as np

import phase as P
import tube as T
import wave as W
from support import cases_phase, cases_tube, hostprog
from support.cases_tube import (NRAY, SPECS, crafted_history, crafted_nbr, device_layouts, launches_of,  # noqa: F401
                                sum_bound)
from support.rows import layout_text

NAN = math.nan
REL_THETA = cases_phase.REL      # of S = sum(|dk| + |dl|)
REL_TUBE = cases_tube.REL        # of a per-ray float of the tube, and of w = wv / sqrt(|D|)
NT_CRAFTED = 24
SEEDS = (0, 1, 2, 3)
# the launch splits of tests/test_gpu_tube.py
SPLITS = {"one": [(1, 24)], "three": [(1, 9), (9, 10), (10, 24)], "five": [(1, 4), (4, 8), (8, 9), (9, 17), (17, 24)]}
INTS = ("cnt", "nseg", "mu", "first", "nrow", "close_row")


def crafted_spec(name, **kw):
    """The grid of ``cases_tube.SPECS[name]`` with the weight ``amp``."""
    return W.WaveSpec(**{**SPECS[name], "weight": "amp", **kw})


def deposits(rows, nbr, chan, spec):
    """What ``reference_wave`` is asked to deposit, from the two definitions it
    composes alone: per depositing row (phase-valid, tube open, in the map)
    ``mu``, ``|D|`` and whether ``jac == 0``, and the number of rows that are
    tube-open and not phase-valid."""
    _, _, _, ok = P.phase_along(rows, chan, spec.phase_spec())
    mu, absd, zero, open_not_valid = [], [], [], 0
    with np.errstate(all="ignore"):
        for r in T.tube_along(rows, nbr, chan, spec.tube_spec(), {}):
            put = ok[:, r.i] & r.open & (r.idx >= 0)
            mu.append(r.mu[put].copy())
            absd.append(np.abs(r.D[put]))
            zero.append(r.jac[put] == 0.0)
            open_not_valid += int((r.open & ~ok[:, r.i]).sum())
    return dict(mu=np.concatenate(mu), absd=np.concatenate(absd), zero=np.concatenate(zero),
                open_not_valid=open_not_valid)


def _ratio(err, bar):
    hit = bar > 0
    assert np.all(err[~hit] == 0.0)
    return float((err[hit] / bar[hit]).max()) if hit.any() else 0.0


def assert_wave(got, want, what=""):
    """The integers, ``dropped`` and ``clipped`` exactly; ``theta`` within
    1e-12 max(S, 1) (phase's bar) and ``dlast`` within 1e-12 relative (tube's);
    per box ``re`` and ``im`` within (1e-12 s_max + 1e-12 + 2 (cnt + 1) 2^-53)
    wabs_ref -- phase's bar plus tube's relative bar on ``w``, which covers cos
    and sqrt -- and ``wabs`` within the bound of a sum taken in any order plus
    1e-12 wabs_ref.  Returns the worst ratio to each bar (printed)."""
    for k in INTS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    for k in ("dropped", "clipped"):
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
    has = want["nrow"] > 0
    assert np.array_equal(got["code"][:, has], want["code"][:, has]), (what, "code")
    S = want["S"]
    fin = np.isfinite(want["theta"])
    assert np.array_equal(got["theta"][~fin], want["theta"][~fin], equal_nan=True), (what, "theta, not finite")
    bar_theta = REL_THETA * np.maximum(S[fin], 1.0)
    err_theta = np.abs(got["theta"][fin] - want["theta"][fin])
    worst = {"theta": _ratio(err_theta, bar_theta)}
    assert np.array_equal(np.isnan(got["dlast"]), np.isnan(want["dlast"])), (what, "dlast, NaN")
    d = ~np.isnan(want["dlast"])
    err_d, bar_d = np.abs(got["dlast"][d] - want["dlast"][d]), REL_TUBE * np.abs(want["dlast"][d])
    worst["dlast"] = _ratio(err_d, bar_d) if d.any() else 0.0
    a, cnt = want["wabs"], want["cnt"]
    s_max = max(float(S[np.isfinite(S)].max()) if np.isfinite(S).any() else 0.0, 1.0)
    bar = (REL_THETA * s_max + REL_TUBE + 2.0 * (cnt + 1) * 2.0 ** -53) * a
    errs = {}
    for name in ("re", "im"):
        assert np.all(np.isfinite(got[name])), (what, name)
        errs[name] = np.abs(got[name] - want[name])
        worst[name] = _ratio(errs[name], bar)
    bar_w = sum_bound(cnt, a) + REL_TUBE * a
    err_w = np.abs(got["wabs"] - want["wabs"])
    worst["wabs"] = _ratio(err_w, bar_w)
    print(f"{what}: worst error / bar " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert np.all(err_theta <= bar_theta), (what, "theta", worst["theta"])
    assert np.all(err_d <= bar_d), (what, "dlast", worst["dlast"])
    for name in ("re", "im"):
        assert np.all(errs[name] <= bar), (what, name, worst[name])
    assert np.all(err_w <= bar_w), (what, "wabs", worst["wabs"])
    return worst


def assert_same_run(a, b, want, what=""):
    """Two deliveries of the same rows in different launches or layouts: the
    integers equal, the per-ray state bit for bit, the sums within the bound
    of a sum of the same terms taken in any order."""
    for k in INTS + ("code",):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["dropped"] == b["dropped"] and a["clipped"] == b["clipped"], what
    for k in ("theta", "dlast", "state_f"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    bound = sum_bound(want["cnt"], want["wabs"])
    for name in ("re", "im", "wabs"):
        assert np.all(np.abs(a[name] - b[name]) <= bound), (what, name)


def start(m, rows0):
    """Row 0 of a history ``[nray, 8]`` into the map."""
    s = m.spec
    return m.start(rows0[:, 0], rows0[:, 1], None if s.ncol < 0 else rows0[:, s.ncol],
                   None if s.wcol < 0 else rows0[:, s.wcol], k=rows0[:, 2], l=rows0[:, 3])


def numpy_with_state(m):
    return dict(m.numpy(), state_f=m.prev.cpu().numpy())


# -------------------------------------------- csrc/wave_rows.h on the host
def run_host_program(exe, spec, nbr, launches, nray=NRAY, theta0=None):
    """tests/host/wave_rows_main.cpp over ``launches`` (``launches_of``)."""
    c = spec.c_struct()
    theta0 = np.zeros(nray) if theta0 is None else np.asarray(theta0, np.float64)
    lines = [f"{c.nx} {c.ny} {c.nchan} {c.need} {c.wcol} {c.spread} {nray}",
             " ".join(float(x).hex() for x in (c.lat0, c.inv_dlat, c.inv_dlon, c.max_sep, c.omega_dt, c.d_floor)),
             " ".join(float(x).hex() for x in theta0)]
    lines += [" ".join(str(int(v)) for v in row) for row in np.asarray(nbr)]
    lines.append(str(len(launches)))
    for L, layout in launches:
        lines += layout_text(L, layout)
    out = hostprog.run(exe, lines)
    floats = lambda s: np.array([float.fromhex(x) if "nan" not in x else NAN for x in s.split()])   # noqa: E731
    st = np.array(out[5].split(), np.int32).reshape(W.NSTATE_I, nray)
    pv = floats(out[6]).reshape(W.NSTATE_F, nray)
    tally = out[4].split()
    return {"cnt": np.array(out[0].split(), np.int64).reshape(spec.shape), "re": floats(out[1]).reshape(spec.shape),
            "im": floats(out[2]).reshape(spec.shape), "wabs": floats(out[3]).reshape(spec.shape),
            "dropped": int(tally[1]), "clipped": int(tally[3]), "bad": int(tally[5]),
            "mu": st[1], "first": st[2], "nrow": st[3], "close_row": st[4], "nseg": st[5],
            "theta": pv[4], "dlast": pv[8], "state_f": pv,
            "code": np.stack([st[0] & 3, (st[0] >> 2) & 3]).astype(np.int32)}
