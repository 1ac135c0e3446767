"""The lean RHS tail (rhs_tail_lean, csrc/rwrt.hip) against the oracle, bit for bit.

``rwrt_rhs`` takes the lean tier when the launch's background is inside its
exponent window (bg_lean) and a lane's six leaves are inside theirs (leaf_ok);
every other evaluation takes the guarded or the IEEE tail.  All three must
give the oracle's ``rhs`` to the last bit -- int64 views, NaN canonicalised,
the sign of zero included -- on

* the states of tests/golden/rhs_<kind>.npz on their own backgrounds,
* adversarial states: one leaf at a time 0, -0, 5e-324, +-inf, NaN or on either
  side of each edge of its window, the others physical,
* backgrounds that turn the launch's verdict off (u, v scaled by 2^-300 and by
  2^250; a single value of 1e-250) and one of exact zeros and negative zeros,
  which leaves it on.

Selftest kind 40 is the leaf guard's verdict for one value as one leaf, kind 43
the background window's for one packed value; 41/42 hold the literal 1 / R to
rcp2(R).  The oracle runs here with the kernels' own sin/cos/tan
(``O.device_math``), so the comparison does not depend on this host's libm.
"""
import math

import numpy as np
import pytest

import rwrt_oracle as O
import synthetic as S
from conftest import golden

pytestmark = pytest.mark.gpu

HOT = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]
LEAVES = ("dx", "dy", "lat", "k", "l", "amp")
# the windows of csrc/rwrt.hip (tests/test_divguard_bounds.py holds them to the source)
LO, AMP_HI, K_WIN, BG_WIN = -100, 100, (-7, 19), (-250, 200)
_CACHE = {}


def bitwise(a, b):
    a = np.where(np.isnan(a), np.nan, np.asarray(a, np.float64))
    b = np.where(np.isnan(b), np.nan, np.asarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def fexp(v):
    """frexp exponent as v_frexp_exp_i32_f64 gives it: 0 for 0, inf and NaN"""
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        return np.where((v == 0) | ~np.isfinite(v), 0, np.frexp(v)[1])


def model_verdict(leaf, v):
    """leaf_ok for value(s) v as leaf ``leaf``, the others physical"""
    v = np.asarray(v, np.float64)
    e = fexp(v)
    with np.errstate(invalid="ignore"):
        if leaf == "k":
            return (e >= K_WIN[0]) & (e <= K_WIN[1])
        if leaf == "amp":
            return (e >= LO) & (e <= AMP_HI)
        if leaf == "lat":   # masked from pi/2 on: l is NaN there and every leaf passes
            return (np.abs(v) >= 0.5 * np.pi) | (e >= LO)
        if leaf == "l":
            return (np.abs(v) >= 100.0) | (e >= LO)
    return e >= LO


def base(kind):
    """(oracle background, golden states, golden dydt) of one kind, once"""
    if kind not in _CACHE:
        g = golden(f"rhs_{kind}.npz")
        _CACHE[kind] = (O.Background(**S.background(kind)), g["y"], g["dydt"])
    return _CACHE[kind]


def leaves_of(ob, y):
    with np.errstate(all="ignore"):
        lons = (y[0] % (2 * np.pi)) % (2 * np.pi)
    return {"dx": lons - ob.lon[0], "dy": y[1] - ob.lat[0], "lat": y[1], "k": y[2], "l": y[3], "amp": y[4]}


def edge_values(leaf):
    sp = [0.0, -0.0, 5e-324, np.inf, -np.inf, np.nan]
    lo = K_WIN[0] if leaf == "k" else LO
    inside = math.ldexp(1.0, lo - 1)                       # the smallest magnitude with exponent lo
    sp += [inside, -inside, np.nextafter(inside, 0.0), -np.nextafter(inside, 0.0)]
    if leaf in ("k", "amp"):
        hi = K_WIN[1] if leaf == "k" else AMP_HI
        out = math.ldexp(1.0, hi)                          # the smallest magnitude with exponent hi + 1
        sp += [np.nextafter(out, 0.0), -np.nextafter(out, 0.0), out, -out]
    if leaf == "lat":                                      # the mask's edge
        sp += [np.nextafter(0.5 * np.pi, 0.0), 0.5 * np.pi, -0.5 * np.pi]
    if leaf == "l":
        sp += [np.nextafter(100.0, 0.0), 100.0, -100.0]
    return np.array(sp)


def adversarial(ob, y, nbase=6):
    """states that differ from a physical one in a single leaf"""
    with np.errstate(all="ignore"):
        ref = O.rhs(ob, y)[0]
    phys = np.where(np.isfinite(ref).all(axis=0) & np.isfinite(y).all(axis=0) & (np.abs(y[2]) > 0.5))[0]
    pick = phys[np.linspace(0, len(phys) - 1, nbase).astype(int)]
    cols, tags = [], []
    for leaf in LEAVES:
        for v in edge_values(leaf):
            for j in pick:
                s = y[:, j].copy()
                if leaf == "dx":
                    s[0] = ob.lon[0] + v
                elif leaf == "dy":
                    s[1] = ob.lat[0] + v
                else:
                    s[{"lat": 1, "k": 2, "l": 3, "amp": 4}[leaf]] = v
                cols.append(s)
                tags.append(leaf)
    return np.array(cols).T.copy(), tags


def states(kind):
    key = ("states", kind)
    if key not in _CACHE:
        ob, y, _ = base(kind)
        adv, _ = adversarial(ob, y)
        _CACHE[key] = np.concatenate([y, adv], axis=1)
    return _CACHE[key]


def gpu_and_oracle(fields, ob, y):
    from engine import RayEngine
    eng = RayEngine(fields, ob.lon, ob.lat)
    got = eng.rhs(y).cpu().numpy()
    keep = ob.fields
    ob.fields = fields
    try:
        with np.errstate(all="ignore"), O.device_math():
            want = O.rhs(ob, y)[0]
    finally:
        ob.fields = keep
    return got, want


def bg_inside(fields):
    from engine import selftest_math
    return selftest_math("bg_window", fields[..., HOT].ravel()) == 1.0


def variant(fields, name):
    f = fields.copy()
    if name == "uv_2^-300":
        f[..., :2] *= 2.0 ** -300
    elif name == "uv_2^250":
        f[..., :2] *= 2.0 ** 250
    elif name == "one_1e-250":
        f[7, 31, 0] = 1e-250
    elif name == "zeros":
        f[...] = 0.0
        f[::2] = -0.0
    return f


# -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nonzonal", "zonal"])
def test_fixture_states_take_the_lean_tail_and_match(kind):
    from engine import selftest_math
    ob, y, dydt = base(kind)
    assert bg_inside(ob.fields).all()            # the launch's verdict: lean
    lv = leaves_of(ob, y)
    refused = np.zeros(y.shape[1], bool)
    for i, leaf in enumerate(LEAVES):
        got = selftest_math("leaf_guard", lv[leaf], np.full(y.shape[1], float(i))) == 1.0
        assert np.array_equal(got, model_verdict(leaf, lv[leaf])), leaf
        refused |= ~got
    # every state is admitted, so the lean tail is what is compared -- but the
    # fixture's one k = 1e-8, which no window that keeps k^2 (1 + (l/k)^2)^2
    # inside [2^-99, 2^100] can hold (tests/test_divguard_bounds.py)
    assert np.array_equal(np.where(refused)[0], np.where(np.abs(y[2]) == 1e-8)[0]) and refused.sum() == 1
    got, want = gpu_and_oracle(ob.fields, ob, states(kind))
    assert bitwise(got, want)
    assert bitwise(got[:, :y.shape[1]], dydt)    # and the reference's own values


def test_leaf_guard_verdicts_at_the_edges():
    from engine import selftest_math
    for i, leaf in enumerate(LEAVES):
        v = edge_values(leaf)
        got = selftest_math("leaf_guard", v, np.full(v.shape, float(i))) == 1.0
        want = model_verdict(leaf, v)
        assert np.array_equal(got, want), (leaf, v[got != want])
        # 0, -0, inf and NaN are admitted (v_div_fixup's cases), 5e-324 is not; below
        # the window's lower edge and above its upper one (k, amp) a value is refused
        assert want[[0, 1, 5]].all() and not want[2]
        assert want[[6, 7]].all() and not want[[8, 9]].any()
        if leaf in ("k", "amp"):
            assert want[[3, 4]].all() and want[[10, 11]].all() and not want[[12, 13]].any()


@pytest.mark.parametrize("name", ["uv_2^-300", "uv_2^250", "one_1e-250", "zeros"])
def test_backgrounds_off_and_on_the_window(name):
    ob, _, _ = base("nonzonal")
    f = variant(ob.fields, name)
    inside = bg_inside(f)
    assert inside.all() == (name == "zeros")     # the verdict: guarded tier, but for the zeros
    got, want = gpu_and_oracle(f, ob, states("nonzonal"))
    assert bitwise(got, want)


def test_background_window_edges():
    from engine import selftest_math
    lo, hi = math.ldexp(1.0, BG_WIN[0] - 1), math.ldexp(1.0, BG_WIN[1])
    v = np.array([0.0, -0.0, lo, -lo, np.nextafter(hi, 0.0), np.nextafter(lo, 0.0), hi, -hi, np.inf, -np.inf, np.nan,
                  5e-324])
    assert np.array_equal(selftest_math("bg_window", v) == 1.0, [True] * 5 + [False] * 7)


def test_rcp_rearth_literal_is_rcp2():
    from engine import selftest_math
    r = selftest_math("rcp2", np.array([6.3712e6]))
    lit = selftest_math("rcp_rearth_literal", np.array([0.0]))
    print("rcp2(R) =", float(r[0]).hex(), " literal =", float(lit[0]).hex())
    assert r.view(np.int64)[0] == lit.view(np.int64)[0]
