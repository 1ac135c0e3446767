"""rwrt_rk45_init_rel / rwrt_rk45_run_rel (release stacks, include/rwrt.h)
validate their arguments before the first HIP call (no GPU needed):
RWRT_ERR_ARG with a message -- the entry's own checks with its name in front --
and an empty batch is a no-op."""
import ctypes

import _hip as H
from support.abi import A, ENTRIES, NROW, background, grid, params

run, init = ENTRIES["rwrt_rk45_run_rel"], ENTRIES["rwrt_rk45_init_rel"]   # (keyword callers, valid-looking defaults)
NAMES = {run: b"rwrt_rk45_run_rel", init: b"rwrt_rk45_init_rel"}


def refused(lib, st, word, name=None):
    assert st == H.RWRT_ERR_ARG, st
    msg = lib.rwrt_last_error()
    assert word in msg, msg
    if name is not None:
        assert msg.startswith(name), msg


def test_both_symbols_are_exported_and_bound():
    lib = H.load()
    for name in ("rwrt_rk45_init_rel", "rwrt_rk45_run_rel"):
        assert name in H.ABI_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert len(lib.rwrt_rk45_init_rel.argtypes) == 12 and len(lib.rwrt_rk45_run_rel.argtypes) == 19


def test_the_entries_own_refusals_start_with_their_name():
    lib = H.load()
    for call, name in NAMES.items():
        refused(lib, call(lib, g=None), b"grid is NULL", name)
        refused(lib, call(lib, b=None), b"background is NULL", name)
        for n in (0, -3):
            refused(lib, call(lib, b=background(nlev=n)), b"nlev >= 1", name)
        for dt in (0.0, -1.0, float("nan")):
            refused(lib, call(lib, b=background(dt=dt)), b"dt must be > 0", name)
        for f in (1, 2):
            refused(lib, call(lib, b=background(fp32=f)), b"fp64 levels only", name)
        refused(lib, call(lib, t0=None), b"d_t0 is NULL", name)


def test_flag_refusals_the_backward_flag_included():
    lib = H.load()
    for call, name in NAMES.items():
        refused(lib, call(lib, p=params(flags=H.PARAMS_BACKWARD)), b"RWRT_PARAMS_BACKWARD", name)
        refused(lib, call(lib, p=params(flags=2)), b"not defined", name)
        refused(lib, call(lib, p=params(flags=H.PARAMS_BACKWARD | 4)), b"not defined", name)
        # (the flags speak before the background's checks)
        refused(lib, call(lib, p=params(flags=H.PARAMS_BACKWARD), b=None), b"RWRT_PARAMS_BACKWARD", name)


def test_run_keeps_every_check_of_the_time_varying_slots_entry():
    lib = H.load()
    refused(lib, run(lib, b=background(levels=None)), b"packed fields pointer is NULL")
    refused(lib, run(lib, b=background(levels=A + 8)), b"16-byte aligned")
    refused(lib, run(lib, g=grid(1, NROW)), b"at least 2x2")
    refused(lib, run(lib, ctx=None), b"rwrt_ctx is NULL")
    refused(lib, run(lib, p=None), b"params is NULL")
    for nray in (-1, 1 << 31):
        refused(lib, run(lib, nray=nray), b"nray out of range")
    for i0, i1 in ((0, 5), (5, 5), (1, 182)):
        refused(lib, run(lib, i0=i0, i1=i1), b"it_begin")
    for name in ("tbound", "work", "state", "count", "nanrow", "out"):
        refused(lib, run(lib, **{name: None}), b"NULL buffer")
    refused(lib, run(lib, out=A + 8), b"16-byte aligned")
    refused(lib, run(lib, tail_from=A), b"tails need both")
    refused(lib, run(lib, tail_row=A), b"tails need both")
    refused(lib, run(lib, tail_from=A, tail_row=A + 8), b"16-byte aligned")
    refused(lib, run(lib, slot=A), b"row slots need tails")


def test_init_keeps_every_check_of_the_time_varying_entry():
    lib = H.load()
    refused(lib, init(lib, b=background(levels=None)), b"packed fields pointer is NULL")
    refused(lib, init(lib, p=None), b"params is NULL")
    refused(lib, init(lib, nray=-1), b"nray out of range")
    for name in ("y0", "state", "count", "nanrow", "live", "summary"):
        refused(lib, init(lib, **{name: None}), b"NULL buffer")


def test_empty_batch_is_a_noop():
    """nray == 0: nothing is launched and no per-ray buffer is needed, d_t0
    included; b->t0 is ignored whatever it holds."""
    lib = H.load()
    b = background(t0=float("nan"))
    assert run(lib, nray=0, b=b, t0=None, state=None, count=None, nanrow=None, out=None) == H.RWRT_OK
    assert run(lib, nray=0, t0=None, tail_from=A, tail_row=A, slot=A, state=None, count=None, nanrow=None,
               out=None) == H.RWRT_OK
    # (the checks that need no ray still speak)
    refused(lib, run(lib, nray=0, b=background(nlev=0)), b"nlev >= 1", NAMES[run])
    refused(lib, run(lib, nray=0, ctx=None), b"rwrt_ctx is NULL")
    refused(lib, init(lib, nray=0, t0=None, b=background(fp32=1)), b"fp64 levels only", NAMES[init])


def test_last_grid_validates_without_a_device():
    """rwrt_ctx_last_grid is host bookkeeping: a NULL context is refused, like every context call."""
    lib = H.load()
    b, r = ctypes.c_int32(-1), ctypes.c_int32(-1)
    refused(lib, lib.rwrt_ctx_last_grid(None, ctypes.byref(b), ctypes.byref(r)), b"rwrt_ctx is NULL")
    assert (b.value, r.value) == (-1, -1)
    assert "rwrt_ctx_last_grid" in H.ABI_SYMBOLS
