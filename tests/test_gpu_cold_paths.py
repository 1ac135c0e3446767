"""The ray loop's rarely taken branches, driven on purpose, bit for bit against
the oracle.

The bodies of the run kernel's rare branches (RARE in csrc/rwrt.hip) lie
behind the loop, out of its common path; the common workloads hardly take
them.  This launch does: 256 slots -- four waves, each mixing common-path
lanes with lanes that take a cold body -- for 41 rows on the zonal and the
non-zonal 144 x 73 backgrounds, with, by the oracle's own states, at least
one ray each that

* is evaluated in the Mercator pole band (|cos lat| <= 0.0175),
* is refused by the lean tail's guard and takes the IEEE tail: amp above
  2^100, and k outside [2^-7, 2^19),
* takes a row-to-row step with a half-difference above 1/16 between two
  stored rows: the exact sines of the jump mask,
* has a longitude of at least 2^40: the library fmod,
* freezes in the middle of the launch: the frozen-row loop.

All eight row columns, nacc, nrej and nanrow equal oracle/rwrt_oracle.py bit
for bit (the oracle computes with the kernel's own sin/cos/tan/pow,
``O.device_math``: no dependence on this host's libm).  The common-path lanes
are rays of tests/golden/init_C2_<kind>.npz; the others are states written
down here.  No new reference data.
"""
import numpy as np
import pytest
import torch

import rwrt_oracle as O
import synthetic as S
from conftest import golden
from support.backward import first_nan_row

pytestmark = pytest.mark.gpu

NT, TSTEP, NRAY = 41, 7200.0, 256
KINDS = ("zonal", "nonzonal")
_REF = {}


def seeds(kind):
    """``y0[5, 256]``: 160 slots of the C2 golden (live and dead mixed), 48 long
    waves at high latitudes (fast in longitude: large row-to-row steps, jump-mask
    and pole freezes), 8 rays in the pole band, 8 with amp = 2^101, 8 with k
    outside the lean window, 8 with a longitude of 2^40 and more, 16 dead slots;
    dealt over the four waves by a fixed stride."""
    rows = golden(f"init_C2_{kind}.npz")["rows"][:5].reshape(5, -1)
    live = np.flatnonzero(~np.isnan(rows.sum(0)))
    dead = np.flatnonzero(np.isnan(rows.sum(0)))
    common = rows[:, np.concatenate([live[:: len(live) // 128][:128], dead[:: len(dead) // 32][:32]])]
    base = rows[:, live[:: len(live) // 8][:8]]
    lw = np.empty((5, 48))
    j = np.arange(48)
    lw[0] = (0.13 + 0.131 * j) % (2 * np.pi)
    lw[1] = np.deg2rad(np.array([60.0, 70.0, 75.0, 80.0, 86.0, 88.0, -75.0, -82.0])[j % 8])
    lw[2] = np.array([0.1, 0.2, 0.3, 0.5, 0.05, 1.0])[(j // 8) % 6]
    lw[3] = -1.4 + 0.06 * j
    lw[4] = 1.0
    pole = base.copy()
    pole[1] = np.deg2rad([89.2, 89.5, -89.3, 89.9, -89.6, 89.1, 89.4, -89.2])
    amp = base.copy()
    amp[4] = 2.0 ** 101
    kout = base.copy()
    kout[2] = [2.0 ** -8, 2.0 ** 19, 2.0 ** -9, 2.0 ** 20, 2.0 ** -8, 2.0 ** 19, 2.0 ** -12, 2.0 ** 21]
    far = base.copy()
    far[0] = 2.0 ** 40 + base[0] + np.arange(8) * 2.0 ** 37
    nan = np.full((5, 16), np.nan)
    nan[:2] = common[:2, :16]          # dead root slots: finite position, NaN wavenumbers
    y0 = np.concatenate([common, lw, pole, amp, kout, far, nan], axis=1)
    assert y0.shape == (5, NRAY)
    tag = np.repeat(np.arange(7), [160, 48, 8, 8, 8, 8, 16])
    deal = (np.arange(NRAY) * 37) % NRAY   # (37 is coprime to 256: a permutation)
    return np.ascontiguousarray(y0[:, deal]), tag[deal]


def reference(kind):
    """The oracle's ``(y0, tag, hist[7, NT, nray], nacc_rows[NT - 1, nray], nacc, nrej)``, once per kind."""
    if kind not in _REF:
        y0, tag = seeds(kind)
        per_row = []
        stepper = O.DP54

        class Kept(stepper):   # (the accepted steps after every interval: the rows' eighth column)
            def advance_to(self, t_bound):
                super().advance_to(t_bound)
                per_row.append(self.nacc.copy())

        O.DP54 = Kept
        try:
            with np.errstate(all="ignore"), O.device_math():
                hist, nacc, nrej, status = O.ray_run(O.Background(**S.background(kind)), y0.copy(), NT, TSTEP)
        finally:
            O.DP54 = stepper
        assert status == 0 and len(per_row) == NT - 1
        for a in (y0, hist, nacc, nrej):
            a.setflags(write=False)
        _REF[kind] = (y0, tag, hist, np.array(per_row), nacc, nrej)
    return _REF[kind]


def same(a, b):
    a = np.where(np.isnan(a), np.nan, np.asarray(a, np.float64))
    b = np.where(np.isnan(b), np.nan, np.asarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("kind", KINDS)
def test_cold_paths_bitwise(kind):
    y0, tag, hist, nacc_rows, nacc, nrej = reference(kind)
    lon, lat = hist[0], hist[1]
    live0 = ~np.isnan(y0.sum(0))
    stored = np.isfinite(lon) & np.isfinite(lat)
    stored[0] = live0

    # ---- the oracle's states meet every condition
    # (a live ray's first evaluation is at its row 0; a stored row is the last evaluation's position)
    band = stored & (np.abs(np.cos(lat)) <= 0.0175)
    assert band.any(axis=0).sum() >= 1
    assert band[0].any() and band[1:].any()
    # a live ray with amp above 2^100 / k outside [2^-7, 2^19) at a stored row: its next attempt's
    # evaluations take the IEEE tail
    big_amp = stored & (np.abs(hist[4]) > 2.0 ** 100)
    k_out = stored & ((np.abs(hist[2]) < 2.0 ** -7) | (np.abs(hist[2]) >= 2.0 ** 19))
    assert big_amp[:-1].any() and k_out[:-1].any()
    assert (nacc[big_amp[0]] > 0).any() and (nacc[k_out[0]] > 0).any()       # ... and they are integrated
    # a step between two stored rows with a half-difference above 1/16: neither masked, so the
    # jump mask's polynomial verdict was refused and the exact sines decided
    both = stored[1:] & stored[:-1]
    with np.errstate(invalid="ignore"):
        half = np.maximum(np.abs(lon[1:] - lon[:-1]), np.abs(lat[1:] - lat[:-1])) / 2.0
    assert (both & (half > 0.0625)).any(axis=0).sum() >= 1
    # a longitude of 2^40 and more at a stored row of a ray that goes on
    far = stored & (np.abs(lon) >= 2.0 ** 40)
    assert far[:-1].any() and (nacc[far[0]] > 0).any()
    # a ray stored at row r - 1 and frozen from row r on, with rows left in the launch behind r
    froze = first_nan_row(lon, NT)
    mid = live0 & (froze >= 2) & (froze <= NT - 2)
    assert mid.sum() >= 1
    # every wave (64 consecutive slots) mixes common-path lanes with the others
    for w in range(4):
        t = tag[64 * w:64 * (w + 1)]
        assert (t == 0).sum() >= 32 and len(set(t.tolist())) == 7

    # ---- the launch (one call: 40 rows) equals the oracle bit for bit
    from support.cases import engine
    got = {}
    res = engine(kind).integrate(torch.as_tensor(y0), NT, TSTEP, ttotal=(NT - 1) * TSTEP,
                                 sink=lambda a, b, o: got.__setitem__((a, b), o.cpu().numpy().copy()))
    rows = np.full((NRAY, NT, 8), np.nan)
    for (i0, i1), r in got.items():
        rows[:, i0:i1] = r
    assert sorted(got) == [(1, NT)]                                           # one launch: freezes are mid-launch
    assert same(np.transpose(rows[:, 1:, :7], (2, 1, 0)), hist[:, 1:])
    assert np.array_equal(rows[:, 1:, 7], nacc_rows.T.astype(np.float64))
    assert np.array_equal(res.nacc.cpu().numpy(), nacc)
    assert np.array_equal(res.nrej.cpu().numpy(), nrej)
    assert np.array_equal(res.nanrow.cpu().numpy(), froze)
