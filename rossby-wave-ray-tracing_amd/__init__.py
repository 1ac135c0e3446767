"""rwrt -- MI355X-native batched Rossby-wave ray integrator.

The modules of this directory mirror the reference's flat layout (``main_wr``,
``wr``, ``bs``, ``wn``, ``constants``) and are imported the same way: put
this directory on ``sys.path`` and ``from wr import WR``.  ``engine`` and
``_hip`` are the device layer (librwrt.so through ctypes).  ``density`` bins
ray points into lon-lat maps on the GPU and ``summary`` reduces every ray's
rows to a path summary there; ``wn.WN`` maps the admissible meridional
wavenumbers of every grid node there; their names are exported here too.
"""
import os
import sys

_here = os.path.dirname(os.path.abspath(__file__))
if _here not in sys.path:
    sys.path.insert(0, _here)

_DENSITY = ["DensitySpec", "DensityMap", "DensitySink", "reference_bins"]
_SUMMARY = ["RaySummary", "SummarySink", "Tee", "reference_summary"]
_WN = ["WN", "reference_wn_map", "reference_fill"]
__all__ = _DENSITY + _SUMMARY + _WN


def __getattr__(name):
    # (resolved on first use: importing the package does not load the device layer)
    if name in _DENSITY:
        import density
        return getattr(density, name)
    if name in _SUMMARY:
        import summary
        return getattr(summary, name)
    if name in _WN:
        import wn
        return getattr(wn, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
