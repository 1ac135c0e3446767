"""The twelve ``rwrt_rk45_*`` entries refuse the same calls with the same words
as the library of the commit before their host code was gathered into one call
record and one background dispatch (no GPU needed: every case returns before
the first HIP call and before the context is read).

One table of single-argument mutations (``MUTATIONS``) is applied to every
entry that has the argument (``support.abi.ENTRIES``), the time-varying entries
once per level storage kind (``fp32`` 0, 1, 2); status and the exact bytes of
``rwrt_last_error`` are compared with ``tests/golden/ray_loop_entry_errors.json``,
as is every bound symbol's ``argtypes``.

The golden file was recorded once, by this module's ``__main__``, from a second
checkout of that earlier commit and is never re-recorded from a later library:

    PYTHONPATH=<checkout>/rossby-wave-ray-tracing_amd RWRT_LIB=<checkout>/rossby-wave-ray-tracing_amd/librwrt.so \\
        python tests/test_ray_loop_entries_host.py

That library's fp64 time-varying run entries read the context ahead of their
checks, so their cases are recorded with ``ctx=None`` only (the background's
checks, then "rwrt_ctx is NULL"); ``test_fp64_time_varying_runs_check_before_the_context``
asserts for this library that they give the words of the ``fp32 = 1`` cases.
"""
import json
import os
import sys

import pytest

if __name__ == "__main__":   # (a PYTHONPATH entry, the earlier checkout's package, comes first)
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(_root, "tests"))
    sys.path.append(os.path.join(_root, "rossby-wave-ray-tracing_amd"))

import _hip as H
from support.abi import A, ENTRIES, N, NPTS, NROW, background, grid, params, stack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_loop_entry_errors.json")

# (id, the arguments it replaces -- a callable is given the case's fp32 --, where it applies beyond "the entry has
# these arguments": a predicate of (entry, fp32); fp32 is None for the entries without rwrt_background)
_run_only = lambda e, f: "ctx" in e                      # noqa: E731
_static = lambda e, f: "packed" in e                     # noqa: E731
_tv = lambda e, f: "b" in e and "t0" not in e            # noqa: E731
_levels = lambda **kw: (lambda f: background(fp32=f or 0, **kw))   # noqa: E731

BACKGROUND = [
    ("grid_null", dict(g=None), None),
    ("packed_null", dict(packed=None), None),
    ("background_null", dict(b=None), lambda e, f: not f),
    ("stack_null", dict(s=None), None),
    ("packed_misaligned", dict(packed=A + 8), None),
    ("levels_null", dict(b=_levels(levels=None)), None),
    ("levels_misaligned", dict(b=_levels(levels=A + 8)), None),
    ("stack_packed_null", dict(s=stack(packed=None)), None),
    ("stack_packed_misaligned", dict(s=stack(packed=A + 8)), None),
    ("grid_1x73", dict(g=grid(1, NROW)), None),
    ("nlev_0", dict(b=_levels(nlev=0)), None),
    ("dt_0", dict(b=_levels(dt=0.0)), None),
    ("dt_negative", dict(b=_levels(dt=-1.0)), None),
    ("dt_nan", dict(b=_levels(dt=float("nan"))), None),
    ("release_fp32_1", dict(b=background(fp32=1)), lambda e, f: "t0" in e),
    ("release_fp32_2", dict(b=background(fp32=2)), lambda e, f: "t0" in e),
    ("nmember_0", dict(s=stack(nmember=0)), None),
    ("member_stride_odd", dict(s=stack(stride=NPTS * 12 + 1)), None),
    ("member_stride_small", dict(s=stack(stride=NPTS * 12 - 2)), None),
    ("member_null", dict(s=stack(member=None)), None),
    ("t0_null", dict(t0=None), None),
    ("flags_1", dict(p=params(flags=1)), lambda e, f: not _static(e, f)),
    # (the static entries honour the flag and go on to their own checks with it)
    ("flags_1_ctx_null", dict(p=params(flags=1), ctx=None), _static),
    ("flags_1_y0_null", dict(p=params(flags=1), y0=None), _static),
    ("flags_2", dict(p=params(flags=2)), None),
    ("flags_3", dict(p=params(flags=3)), None),
    ("ctx_null", dict(ctx=None), None),
]
CALL = [
    ("params_null", dict(p=None), None),
    ("nray_negative", dict(nray=-1), None),
    ("nray_2_31", dict(nray=1 << 31), None),
    ("rows_0_5", dict(i0=0, i1=5), None),
    ("rows_5_5", dict(i0=5, i1=5), None),
    ("rows_1_nt_plus_1", dict(i0=1, i1=182), None),
] + [(f"{k}_null", {k: None}, None) for k in ("tbound", "work", "state", "count", "nanrow", "out", "y0", "live",
                                              "summary")] + [
    ("out_misaligned", dict(out=A + 8), None),
    ("tail_row_misaligned", dict(tail_from=A, tail_row=A + 8), None),
    ("tail_from_alone", dict(tail_from=A, tail_row=None), None),
    ("tail_row_alone", dict(tail_from=None, tail_row=A), None),
    ("slot_without_tails", dict(slot=A, tail_from=None, tail_row=None), None),
    ("slots_entry_without_slot", dict(slot=None), lambda e, f: e.name.endswith("_slots")),
    ("n_heavy_negative", dict(heavy=-1), None),
    ("n_heavy_above_nray", dict(heavy=N + 1), None),
    ("n_heavy_without_order", dict(heavy=4, order=None), None),
    ("n_heavy_on_fp32_arithmetic", dict(heavy=4, order=A), lambda e, f: f == 2),
    ("nray_0", dict(nray=0, state=None, count=None, nanrow=None, out=None), _run_only),
]
MUTATIONS = BACKGROUND + CALL
NOOPS = ("nray_0",)   # RWRT_OK; every other case is an argument error
CALL_IDS = {m[0] for m in CALL}


def _fp64_tv_run(e, f):
    return _tv(e, f) and "ctx" in e and f == 0


def _call(lib, e, f, kw, **more):
    v = {k: x(f) if callable(x) else x for k, x in kw.items()}
    if f is not None and "b" not in v:
        v["b"] = background(fp32=f)
    v = {**more, **v}
    st = e(lib, **v)
    return [st, None if st == H.RWRT_OK else lib.rwrt_last_error().decode("latin-1")]


def cases(muts=MUTATIONS):
    """``(id, entry, fp32, kw)`` of every recorded case.  An fp64 time-varying
    run is recorded without a context, and then only where that still says
    something: the background's checks, the flags, the empty batch."""
    for e in ENTRIES.values():
        for f in ((0, 1, 2) if _tv(e, None) else (0,) if "b" in e else (None,)):
            for mid, kw, when in muts:
                if not all(k in e for k in kw) or (when is not None and not when(e, f)):
                    continue
                if _fp64_tv_run(e, f) and mid in CALL_IDS and mid not in NOOPS:
                    continue
                yield f"{e.name}{'' if f is None else f'[fp32={f}]'}/{mid}", e, f, kw


def record_errors(lib):
    return {cid: _call(lib, e, f, kw, **(dict(ctx=None) if _fp64_tv_run(e, f) else {}))
            for cid, e, f, kw in cases()}


def record_argtypes(lib):
    return {name: [t.__name__ for t in getattr(lib, name).argtypes] for name in H.ABI_SYMBOLS
            if getattr(lib, name).argtypes is not None}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_every_case_gives_the_recorded_status_and_words(golden):
    got = record_errors(H.load())
    want = golden["errors"]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))     # no case left out, none unrecorded
    diff = {c: (got[c], want[c]) for c in want if got[c] != want[c]}
    assert not diff, diff
    print(f"{len(want)} cases, {len(ENTRIES)} entries")


def test_the_recording_is_of_refusals_before_any_hip_call(golden):
    """Argument errors all, but the empty batches of the run entries (RWRT_OK:
    nothing launched); every entry has cases, the time-varying ones per storage kind."""
    for cid, (st, msg) in golden["errors"].items():
        if cid.rsplit("/", 1)[1] in NOOPS and msg is None:
            assert st == H.RWRT_OK, cid
        else:
            assert st == H.RWRT_ERR_ARG and msg, (cid, st, msg)
    heads = {cid.split("/")[0] for cid in golden["errors"]}
    for e in ENTRIES.values():
        want = [f"{e.name}[fp32={f}]" for f in (0, 1, 2)] if _tv(e, None) else \
            [e.name + ("[fp32=0]" if "b" in e else "")]
        assert set(want) <= heads, e.name


OWN_LIBRARY = "RWRT_LIB" not in os.environ


@pytest.mark.skipif(not OWN_LIBRARY, reason="RWRT_LIB selects another build, which may read the context first")
def test_fp64_time_varying_runs_check_before_the_context(golden):
    """With fp64 levels and a (dummy) context, the time-varying run entries give
    every call check's status and words as with fp32 = 1 levels: they no longer
    touch the context ahead of their checks."""
    lib = H.load()
    n = 0
    for cid, e, f, kw in cases(CALL):
        if _tv(e, f) and "ctx" in e and f == 1 and "b" not in kw:
            assert _call(lib, e, 0, kw) == golden["errors"][cid], cid
            n += 1
    assert n == 17 + 20 + 22, n   # dense; + the three tail cases; + the two slot cases


def test_bound_signatures_are_the_recorded_ones(golden):
    got = record_argtypes(H.load())
    assert got == golden["argtypes"]
    assert set(ENTRIES) <= set(got)


if __name__ == "__main__":
    lib = H.load()
    print("recording from", H.LIB_PATH, "bound by", H.__file__)
    rec = {"errors": record_errors(lib), "argtypes": record_argtypes(lib)}
    with open(GOLDEN, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(len(rec["errors"]), "cases,", len(rec["argtypes"]), "signatures")
