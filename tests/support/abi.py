"""What the C entry points' argument-check tests share: the tail of their
loops (``refused``) and keyword callers of the twelve ``rwrt_rk45_*`` entries
with valid-looking dummy arguments (``ENTRIES``)."""
import ctypes

import _hip as H

A = 4096          # an aligned, non-NULL "device pointer": never dereferenced by a refused call
N = 16
NCOL, NROW = 145, 73
NPTS = NCOL * NROW


def refused(lib, call, kw, word, prefix):
    """``call(lib, **kw)`` is refused as an argument error whose message names
    ``word`` and starts with the entry point's name ``prefix``."""
    assert call(lib, **kw) == H.RWRT_ERR_ARG, kw
    assert word in lib.rwrt_last_error(), (kw, lib.rwrt_last_error())
    assert lib.rwrt_last_error().startswith(prefix)


def grid(ncol=NCOL, nrow=NROW):
    return H.Grid(ncol, nrow, 0.0, 0.04363323, -1.5707964, 0.04363323)


def params(nt=181, flags=0):
    return H.Params(1e-6, 1e-6, 7.2, 0.2, nt, flags, 7200.0)


def background(levels=A, nlev=5, fp32=0, t0=0.0, dt=21600.0):
    return H.Background(levels, nlev, fp32, t0, dt)


def stack(packed=A, nmember=3, stride=NPTS * 12, member=A):
    return H.Stack(packed, nmember, 0, stride, member)


_STRUCTS = {"g": grid, "b": background, "s": stack, "p": params}


class Entry:
    """``entry(lib, **kw)`` calls one ``rwrt_rk45_*`` entry on the NULL stream:
    ``names`` gives its arguments in the ABI's order, ``defaults`` gives each a
    valid-looking value (``True`` for a struct: the one of the function above),
    ``kw`` replaces some.  The call the defaults alone make passes every check
    and goes on to the dummy context or the device: only mutated calls are made."""

    def __init__(self, name, names, **defaults):
        self.name, self.names = name, names
        self.defaults = {k: A for k in names}
        self.defaults.update(g=True, p=True, nray=N, **defaults)
        assert set(self.defaults) == set(names), name

    def __contains__(self, key):
        return key in self.defaults

    def __call__(self, lib, **kw):
        unknown = set(kw) - set(self.defaults)
        if unknown:
            raise TypeError(f"{self.name} takes no {sorted(unknown)}")
        v = {**self.defaults, **kw}
        args = []
        for k in self.names:
            x = v[k]
            if k in _STRUCTS:
                x = _STRUCTS[k]() if x is True else x
                x = ctypes.byref(x) if x is not None else None
            args.append(x)
        return getattr(lib, self.name)(*args, None)


# the arguments between grid and nray, per background kind
_BG = {"": ("packed",), "_tv": ("b",), "_stack": ("s",), "_rel": ("b", "t0")}
_ROWS = {"": (), "_tails": ("tail_from", "tail_row"), "_slots": ("slot", "tail_from", "tail_row")}


def _init(kind):
    order = ("g",) + _BG[kind] + ("nray", "y0", "p", "state", "count", "nanrow", "live", "summary")
    return Entry("rwrt_rk45_init" + kind, order, **{k: True for k in _BG[kind] if k in _STRUCTS})


def _run(kind, rows):
    """The static and the time-varying trio take ``heavy`` and their own row
    arguments (given by default); the stack and release entries take all three
    row arguments, NULL by default."""
    trio = kind in ("", "_tv")
    order = (("ctx", "g") + _BG[kind] + ("nray", "p", "tbound", "i0", "i1", "order") + (("heavy",) if trio else ()) +
             ("state", "count", "nanrow", "out") + _ROWS[rows if trio else "_slots"] + ("work",))
    d = {k: True for k in _BG[kind] if k in _STRUCTS}
    d.update(i0=1, i1=5, order=None)
    if trio:
        d.update(heavy=0)
    else:
        d.update(slot=None, tail_from=None, tail_row=None)
    return Entry("rwrt_rk45_run" + kind + rows, order, **d)


ENTRIES = {e.name: e for e in
           [_init(k) for k in _BG] + [_run(k, r) for k in ("", "_tv") for r in _ROWS] +
           [_run("_stack", ""), _run("_rel", "")]}
assert len(ENTRIES) == 12
