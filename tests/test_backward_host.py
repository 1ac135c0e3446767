"""Backward ray tracing without a GPU: the premise of its test-side definition
(tests/support/backward.py), a round trip with the oracle, the C ABI's flag
checks (include/rwrt.h ``rwrt_params.flags``) and what ``WR`` refuses.

Fixture (tests/support/backward.py): the zonal and the non-zonal state at 2.5
degrees, 4 x 4 sources x 4 wavenumbers x 3 roots = 192 slots, 2-hour rows.
"""
import ctypes

import numpy as np
import pytest

import _hip as H
import rwrt_oracle as O
from support.abi import A, ENTRIES, N, params
from support.backward import KINDS, TSTEP, background, cfg, oracle_backward, row0
from support.bits import bitwise


def _live(kind):
    r = row0(kind)
    return ~np.isnan(r[:5].mean(axis=0))


def test_fixture_has_live_and_dead_slots():
    for kind in KINDS:
        live = _live(kind)
        assert live.size == 192 and live.sum() >= 30 and (~live).sum() >= 1, (kind, int(live.sum()))


def test_a_negative_step_is_the_positive_step_of_the_negated_rhs():
    """``oracle_backward``'s premise, one DP5(4) attempt: the reference's
    attempt with ``direction = -1`` -- ``dp54_attempt(fun, t, y, f, -h)`` --
    and the attempt of the negated problem at the mirrored time --
    ``dp54_attempt(-fun, -t, y, -f, h)`` -- give the same ``y_new`` bit for bit
    and the stages ``K`` negated.  (The issue writes both calls with ``h``; a
    forward and a backward step from one state cannot agree, the first call's
    step is the signed one.)  All live states of row 0 on both backgrounds,
    three step sizes each."""
    total = 0
    for kind in KINDS:
        ob = background(kind)
        y = np.array(row0(kind)[:5][:, _live(kind)])
        n = y.shape[1]
        total += n

        def fun(t, yy):
            return O.rhs(ob, yy, t)[0]

        def neg(t, yy):
            return -O.rhs(ob, yy, t)[0]

        with np.errstate(all="ignore"):
            f = fun(np.zeros(n), y)
            for step in (7.2, 900.0, 7200.0):
                h = np.full(n, step) * (1.0 + 0.01 * np.arange(n))
                t = np.full(n, -3.0 * TSTEP)
                y1, K1 = O.dp54_attempt(fun, t, y, f, -h)
                y2, K2 = O.dp54_attempt(neg, -t, y, -f, h)
                assert np.isfinite(y1).all(), (kind, step)
                assert bitwise(y1, y2), (kind, step)
                assert np.array_equal(K1, -K2), (kind, step)
                assert not np.array_equal(y1, y), (kind, step)
                # and the error norm is even in the sign
                e1 = O.error_norm(K1, -h, y, y1, 1e-6, 1e-6)
                e2 = O.error_norm(K2, h, y, y2, 1e-6, 1e-6)
                assert bitwise(e1, e2), (kind, step)
    assert total >= 64, total


def test_oracle_round_trip_on_the_zonal_state():
    """Forward rows 0..20, then 20 rows backward from row 20's state: every
    live ray returns to its start within 1e-4 rad (measured 2.3e-5 in
    longitude and 1.6e-5 in latitude where the bound was set: rtol = 1e-6 over
    20 intervals, times four).  (Not on the non-zonal state: its rays diverge,
    up to 1.3e-3 rad there.)"""
    ob = background("zonal")
    r0 = np.array(row0("zonal"))
    live = _live("zonal")
    assert live.sum() == 40
    with np.errstate(all="ignore"):
        fwd, _, _, st = O.ray_run(ob, r0[:5].copy(), 21, TSTEP, row0=r0)
        assert st == 0 and not np.isnan(fwd[0, 20, live]).any()
        back, nacc, _, st = oracle_backward(ob, fwd[:5, 20].copy(), 21, TSTEP)
    assert st == 0
    assert not np.isnan(back[:2, 20][:, live]).any(), "a live ray did not return"
    assert (nacc[live] > 0).all()
    dlon = np.abs(back[0, 20, live] - r0[0, live]).max()
    dlat = np.abs(back[1, 20, live] - r0[1, live]).max()
    print(f"round trip, 20 rows: max |dlon| {dlon:.3g} rad, max |dlat| {dlat:.3g} rad")
    assert dlon <= 1e-4 and dlat <= 1e-4, (dlon, dlat)
    # half way back the rays are where they were half way out (backward row 10 is forward row 20 - 10)
    assert np.abs(back[:2, 10][:, live] - fwd[:2, 10][:, live]).max() <= 1e-4


# ---------------------------------------------------------------------------------------------- C ABI
def _grid():
    return H.Grid(145, 73, 0.0, 0.04363323, -1.5707964, 0.04363323)


def _params(flags):
    return H.Params(1e-6, 1e-6, 7.2, 0.2, 181, flags, 7200.0)


def _calls(lib, flags):
    """Every entry that takes ``rwrt_params``, with valid-looking arguments and ``flags``."""
    g, p = _grid(), _params(flags)
    gr, pr = ctypes.byref(g), ctypes.byref(p)
    calls = {name: (lambda e=e: e(lib, p=params(flags=flags))) for name, e in ENTRIES.items()}
    calls["rwrt_rk4_run"] = lambda: lib.rwrt_rk4_run(A, gr, A, N, pr, 1, 5, None, A, A, A, A, A, None)
    return calls


HONOUR = ("rwrt_rk45_init", "rwrt_rk45_run", "rwrt_rk45_run_tails", "rwrt_rk45_run_slots")


def test_params_keep_their_layout_and_carry_the_flag():
    from engine import RayEngine
    assert ctypes.sizeof(H.Params) == 48
    assert H.Params.flags.offset == 36 and H.Params.flags.size == 4 and H.Params.tstep.offset == 40
    assert H.PARAMS_BACKWARD == 1
    assert RayEngine.params(10, 7200.).flags == 0
    assert RayEngine.params(10, 7200., backward=True).flags == 1
    fwd, back = RayEngine.params(10, 7200.), RayEngine.params(10, 7200., backward=True)
    for name in ("rtol", "atol", "min_step", "cut_off", "nt", "tstep"):
        assert getattr(fwd, name) == getattr(back, name), name
    assert back.min_step > 0


def test_flag_argument_errors_without_a_gpu():
    """Any bit beyond RWRT_PARAMS_BACKWARD is refused by every entry that takes
    rwrt_params; RWRT_PARAMS_BACKWARD by every entry but the static DP5(4)
    ones.  Before any HIP call (this host has no device; the pointers are
    never read), with the entry point's name in front of the message.
    (rwrt_kat_rk45, which the issue lists too, takes no rwrt_params: there is
    no argument through which the flag could reach it.)"""
    lib = H.load()
    for flags in (2, 4, 3, 1 << 30, -2147483648):
        for name, call in _calls(lib, flags).items():
            assert call() == H.RWRT_ERR_ARG, (name, flags)
            msg = lib.rwrt_last_error()
            assert msg.startswith(name.encode() + b":") and b"flags" in msg, (name, flags, msg)
    for name, call in _calls(lib, H.PARAMS_BACKWARD).items():
        if name in HONOUR:
            continue
        assert call() == H.RWRT_ERR_ARG, name
        msg = lib.rwrt_last_error()
        assert msg.startswith(name.encode() + b":") and b"RWRT_PARAMS_BACKWARD" in msg, (name, msg)
    # the entries that honour the flag go on to their own checks with it
    g, p = _grid(), _params(H.PARAMS_BACKWARD)
    assert lib.rwrt_rk45_init(ctypes.byref(g), A, N, None, ctypes.byref(p), A, A, A, A, A, None) == H.RWRT_ERR_ARG
    assert b"NULL buffer" in lib.rwrt_last_error()
    for fn, tail in ((lib.rwrt_rk45_run, (A,)), (lib.rwrt_rk45_run_tails, (A, A, A)),
                     (lib.rwrt_rk45_run_slots, (A, A, A, A))):
        st = fn(None, ctypes.byref(g), A, N, ctypes.byref(p), A, 1, 5, None, 0, A, A, A, A, *tail, None)
        assert st == H.RWRT_ERR_ARG and b"rwrt_ctx is NULL" in lib.rwrt_last_error()
    # an empty backward batch is the forward no-op
    assert lib.rwrt_rk45_run(A, ctypes.byref(g), A, 0, ctypes.byref(p), A, 1, 5, None, 0, None, None, None, None, A,
                             None) == H.RWRT_OK


def test_kat_entry_has_no_params():
    """(why the flag check above has no rwrt_kat_rk45 case)"""
    lib = H.load()
    assert ctypes.POINTER(H.Params) not in lib.rwrt_kat_rk45.argtypes


# ---------------------------------------------------------------------------------------------- WR
def _wr(**kw):
    from wr import WR
    c = cfg()
    w = WR(c.nzwn, c.nsource, TSTEP, 20 * TSTEP, 0.0, nx=144, ny=73, **kw)
    w.set_zwn(c.zwn)
    w.set_source_matrix(c.SW_lon, c.SW_lat, c.dlon, c.dlat, c.nnx, c.nny)
    return w


def test_wr_refuses_backward_rk4_before_any_work(monkeypatch):
    assert _wr().backward is False
    w = _wr(backward=True)
    assert w.backward is True

    def touched(*a, **k):
        raise AssertionError("ray_initial ran")

    monkeypatch.setattr(w, "ray_initial", touched)
    with pytest.raises(NotImplementedError, match="rk45"):
        w.ray_run(mode="hip", inte_method="")
    from density import DensitySpec
    with pytest.raises(NotImplementedError, match="rk45"):
        w.ray_density(DensitySpec(72, 36), inte_method="")


def test_main_wr_takes_an_optional_backward_key():
    import inspect
    import main_wr
    assert "backward" not in main_wr.parameters          # (the reference's keys)
    sig = inspect.signature(main_wr.real2d_hnf)
    assert sig.parameters["backward"].default is False
    assert set(main_wr.parameters) | {"backward"} == set(sig.parameters)


def test_ensemble_wr_has_no_backward():
    import inspect
    from ensemble import EnsembleWR
    assert "backward" not in inspect.signature(EnsembleWR.__init__).parameters
