"""Release stacks on the host (no GPU): ``release.reference_state_at`` -- the
NumPy definition of ``Levels.state_at`` -- on a 3-level toy stack, the
release -> level-origin conversion, and the per-release outcomes through
``ensemble.member_outcomes``."""
import numpy as np

import release as R
from levels import level_origin, time_index

DT = 21600.0


def _stack():
    rng = np.random.default_rng(7)
    return rng.standard_normal((3, 4, 5, 12))


def test_a_level_time_returns_the_levels_own_array():
    p = _stack()
    for j in range(3):
        got = R.reference_state_at(p, j * DT, DT)
        assert np.shares_memory(got, p[j]) and np.array_equal(got, p[j]), j
    # w == 1 is reached only by the clamp above the last level: the last level itself
    got = R.reference_state_at(p, 2 * DT, DT)
    assert np.shares_memory(got, p[2])


def test_clamps_below_the_first_and_above_the_last_level():
    p = _stack()
    for r in (-1.0, -5 * DT, -1e30):
        assert np.shares_memory(R.reference_state_at(p, r, DT), p[0]), r
    for r in (2 * DT + 1e-3, 7 * DT, 1e6 * DT):
        assert np.shares_memory(R.reference_state_at(p, r, DT), p[2]), r
    # (a level index past int32 wraps as the kernels' floor_i32 does: index 0, weight 1)
    assert time_index(0.0, -1e30, DT, 3) == (0, 1.0)
    assert time_index(0.0, 5 * DT, DT, 3) == (0, 0.0)          # s = -5
    assert time_index(0.0, -7 * DT, DT, 3) == (1, 1.0)         # s = 7: the last pair, weight 1
    assert time_index(0.0, -1.25 * DT, DT, 3) == (1, 0.25)
    assert time_index(0.0, -0.5 * DT, DT, 1) == (0, 0.5)       # one level: index 0, the weight clamped alone
    assert time_index(0.0, -3.0 * DT, DT, 1) == (0, 1.0)


def test_a_midpoint_is_the_three_operations():
    p = _stack()
    got = R.reference_state_at(p, 0.5 * DT, DT)
    assert np.array_equal(got, p[0] * 0.5 + p[1] * 0.5)
    got = R.reference_state_at(p, 1.25 * DT, DT)
    a = p[1] * (1.0 - 0.25)
    b = p[2] * 0.25
    assert np.array_equal(got, a + b)
    # one level is blended with itself, as the kernels do
    one = p[:1]
    assert np.array_equal(R.reference_state_at(one, 0.3 * DT, DT), one[0] * (1.0 - 0.3) + one[0] * 0.3)
    assert np.shares_memory(R.reference_state_at(one, 0.0, DT), one[0])


def test_release_to_level_origin():
    """A release r seconds after the first level: t0_ray = levels.t0 - r, fp64."""
    r = np.array([0.0, DT, 1.5 * DT, 3 * DT + 1234.5])
    assert np.array_equal(level_origin(0.0, r), -r)
    t0 = level_origin(864000.25, r)
    assert t0.dtype == np.float64 and np.array_equal(t0, np.float64(864000.25) - r)
    assert R.level_origin is level_origin
    # the kernels' s at ray time 0 with that origin: the release in levels
    for ri, want in zip(r, ((0, 0.0), (1, 0.0), (1, 0.5), (3, 1234.5 / DT))):
        j, w = time_index(0.0, level_origin(0.0, ri), DT, 5)
        assert j == want[0] and abs(w - want[1]) < 1e-15, (ri, j, w)
    # (levels.t0 is the first level's ray time in a plain run; the origin moves with it)
    assert level_origin(3 * DT, 3 * DT + 1.5 * DT) == -1.5 * DT
    # the state's index uses the same conversion
    p = _stack()
    assert np.shares_memory(R.reference_state_at(p, DT, DT, t0=0.0), p[1])


def test_outcomes_per_release():
    """``member_outcomes`` with the release index: a release whose live rays all
    have a NaN first step fails (break row 1) alone; the others report their
    largest nanrow below nt, or None."""
    nt = 37
    rel = np.repeat(np.arange(4), 3)
    live = np.array([1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0])
    nan = float("nan")
    h = np.array([1.0, nan, 1.0, nan, nan, 1.0, 2.0, nan, nan, nan, nan, nan])
    nanrow = np.array([nt, 5, 0, 9, 9, 0, 7, 0, 0, 0, 0, 0])
    failed, brk = R.member_outcomes(rel, live, h, nanrow, 4, nt)
    assert failed == [False, True, False, False]
    assert brk == [None, 1, 7, 0]
    failed, brk = R.member_outcomes(rel[:6], live[:6], h[:6], nanrow[:6], 4, nt)
    assert failed == [False, True, False, False] and brk == [None, 1, None, None]


def test_releasewr_layout_and_checks_need_no_gpu():
    class L:   # (the attributes ReleaseWR's constructor reads)
        nlev, fp32, t0, dt = 5, False, 0.0, DT

    import pytest
    rw = R.ReleaseWR(L(), [0.0, DT, 1.5 * DT], 4, 16, 7200.0, 72 * 3600.0)
    assert rw.nrelease == 3 and rw.slot_shape == (3, 3, 16, 4) and rw.nray == 576 and rw.nt == 37
    chan, n = rw.channels("release")
    assert n == 3 and np.array_equal(chan, np.repeat(np.arange(3), 192))
    assert np.array_equal(rw.members(), chan)
    assert rw.channels("zwn")[1] == 4 and rw.channels("root")[1] == 3 and rw.channels(None) == (None, 1)
    with pytest.raises(ValueError, match="'release'"):
        rw.channels("member")
    with pytest.raises(ValueError, match="finite"):
        R.ReleaseWR(L(), [0.0, float("nan")], 4, 16)
    with pytest.raises(ValueError, match="at least one"):
        R.ReleaseWR(L(), [], 4, 16)
    L.fp32 = True
    with pytest.raises(NotImplementedError, match="fp64"):
        R.ReleaseWR(L(), [0.0], 4, 16)
