"""The shared tail of the C entry points' argument-check loops."""
import _hip as H


def refused(lib, call, kw, word, prefix):
    """``call(lib, **kw)`` is refused as an argument error whose message names
    ``word`` and starts with the entry point's name ``prefix``."""
    assert call(lib, **kw) == H.RWRT_ERR_ARG, kw
    assert word in lib.rwrt_last_error(), (kw, lib.rwrt_last_error())
    assert lib.rwrt_last_error().startswith(prefix)
