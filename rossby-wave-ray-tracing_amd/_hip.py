"""ctypes binding of librwrt.so (the C ABI declared in include/rwrt.h).

PyTorch-ROCm owns every device buffer: callers pass tensors, this module
passes ``data_ptr()`` and the current HIP stream.  There is no CPU fallback:
if the library is missing or no GPU is visible, every entry point raises.
"""
import ctypes
import os

import torch  # noqa: F401  -- load torch's HIP runtime first (same SONAME as ours)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RWRT_LIB", os.path.join(_HERE, "librwrt.so"))

NFIELD_REF, NFIELD_PACK, NVAR, NMERC, NOUT, NSTATE = 18, 12, 5, 12, 8, 12
ABI_SYMBOLS = ("rwrt_version", "rwrt_last_error", "rwrt_ctx_create", "rwrt_ctx_destroy",
               "rwrt_ctx_set_latency_density", "rwrt_ctx_set_tv_lanes", "rwrt_ctx_set_handoff",
               "rwrt_ctx_set_trace", "rwrt_ctx_last_grid",
               "rwrt_pack_fields",
               "rwrt_mercator_point", "rwrt_rhs", "rwrt_dp54_attempt",
               "rwrt_ray_initial", "rwrt_rk45_init", "rwrt_rk45_run", "rwrt_rk45_run_tails",
               "rwrt_expand_tails", "rwrt_row_slots", "rwrt_rk45_run_slots", "rwrt_expand_slots",
               "rwrt_launch_plan_bytes", "rwrt_launch_plan",
               "rwrt_rk4_run", "rwrt_ray_density", "rwrt_ray_summary", "rwrt_ray_arrival", "rwrt_ray_flux",
               "rwrt_ray_track", "rwrt_ray_cross", "rwrt_ray_phase", "rwrt_ray_tube", "rwrt_ray_wave",
               "rwrt_wn_map", "rwrt_wn_fill",
               "rwrt_sh_filter", "rwrt_sh_helmholtz", "rwrt_sh_rws",
               "rwrt_bs_ready", "rwrt_bs_diag", "rwrt_rk45_init_tv", "rwrt_rk45_run_tv", "rwrt_rk45_run_tv_tails",
               "rwrt_rk45_run_tv_slots", "rwrt_rhs_tv",
               "rwrt_rk45_init_stack", "rwrt_rk45_run_stack",
               "rwrt_rk45_init_rel", "rwrt_rk45_run_rel",
               "rwrt_kat_rk45", "rwrt_selftest_math", "rwrt_host_fill_rows")

RWRT_OK, RWRT_ERR_ARG, RWRT_ERR_HIP, RWRT_SOLVER_FAILED = 0, 1, 2, 3
PLAN_SINCE, PLAN_TOTAL = 0, 1   # RWRT_PLAN_SINCE, RWRT_PLAN_TOTAL


class RwrtError(RuntimeError):
    pass


class SolverFailed(RwrtError):
    """rkf45.py:423-425: every retrying column has a NaN step (status -1)."""


class Grid(ctypes.Structure):
    _fields_ = [("ncol", ctypes.c_int32), ("nrow", ctypes.c_int32),
                ("lon0", ctypes.c_double), ("dlon", ctypes.c_double),
                ("lat0", ctypes.c_double), ("dlat", ctypes.c_double)]


class Params(ctypes.Structure):
    _fields_ = [("rtol", ctypes.c_double), ("atol", ctypes.c_double),
                ("min_step", ctypes.c_double), ("cut_off", ctypes.c_double),
                ("nt", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("tstep", ctypes.c_double)]


PARAMS_BACKWARD = 1   # RWRT_PARAMS_BACKWARD (rwrt_params.flags): the DP5(4) loop's direction is -1


class Background(ctypes.Structure):
    _fields_ = [("d_levels", ctypes.c_void_p), ("nlev", ctypes.c_int32), ("fp32", ctypes.c_int32),
                ("t0", ctypes.c_double), ("dt", ctypes.c_double)]


class Stack(ctypes.Structure):
    """``rwrt_stack``: ``nmember`` static basic states ``[nmember][ncol][nrow][12]``
    (fp64, ``member_stride`` doubles apart) and each ray's member (int32, device)."""
    _fields_ = [("d_packed", ctypes.c_void_p), ("nmember", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("member_stride", ctypes.c_int64), ("d_member", ctypes.c_void_p)]


assert ctypes.sizeof(Stack) == 32


class DensityMap(ctypes.Structure):
    """``rwrt_density_map`` (ABI 5): the map a ``rwrt_ray_density`` call bins into."""
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nchan", ctypes.c_int32),
                ("wcol", ctypes.c_int32), ("inv_dlon", ctypes.c_double),
                ("lat0", ctypes.c_double), ("inv_dlat", ctypes.c_double)]


class ArrivalMap(ctypes.Structure):
    """``rwrt_arrival_map``: the map a ``rwrt_ray_arrival`` call reduces into
    (``bins.wcol``: the row column that must be finite)."""
    _fields_ = [("bins", DensityMap), ("window_rows", ctypes.c_int32), ("nwin", ctypes.c_int32)]


class FluxMapC(ctypes.Structure):
    """``rwrt_flux_map``: the map a ``rwrt_ray_flux`` call reduces into (``mode``
    bit 0: unit vectors, bit 1: unwrapped longitude window)."""
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nchan", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("lon0", ctypes.c_double), ("inv_dlon", ctypes.c_double),
                ("lat0", ctypes.c_double), ("inv_dlat", ctypes.c_double),
                ("s2_min", ctypes.c_double), ("s2_max", ctypes.c_double), ("wn_max", ctypes.c_double)]


assert ctypes.sizeof(FluxMapC) == 72


class TrackMapC(ctypes.Structure):
    """``rwrt_track_map``: the map a ``rwrt_ray_track`` call deposits into
    (``mode`` bit 1: unwrapped longitude window; ``need`` / ``wcol``: row
    columns, -1 for none)."""
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nchan", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("need", ctypes.c_int32), ("wcol", ctypes.c_int32),
                ("max_cells", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("lon0", ctypes.c_double), ("inv_dlon", ctypes.c_double),
                ("lat0", ctypes.c_double), ("inv_dlat", ctypes.c_double)]


assert ctypes.sizeof(TrackMapC) == 64

CROSS_MAXGATE = 8    # RWRT_CROSS_MAXGATE


class CrossGateC(ctypes.Structure):
    """``rwrt_cross_gate``: a latitude circle (``kind`` 0) or a meridian
    (``kind`` 1) at ``pos`` (radians) and the bins along it."""
    _fields_ = [("kind", ctypes.c_int32), ("reserved", ctypes.c_int32), ("pos", ctypes.c_double),
                ("org", ctypes.c_double), ("inv_d", ctypes.c_double)]


class CrossMapC(ctypes.Structure):
    """``rwrt_cross_map``: the gates a ``rwrt_ray_cross`` call tests and the
    maps it accumulates into (``need`` / ``wcol``: row columns, -1 for none)."""
    _fields_ = [("ngate", ctypes.c_int32), ("nbin", ctypes.c_int32), ("nchan", ctypes.c_int32),
                ("need", ctypes.c_int32), ("wcol", ctypes.c_int32), ("window_rows", ctypes.c_int32),
                ("nwin", ctypes.c_int32), ("reserved", ctypes.c_int32), ("gate", CrossGateC * CROSS_MAXGATE)]


assert ctypes.sizeof(CrossGateC) == 32 and ctypes.sizeof(CrossMapC) == 288


class PhaseMapC(ctypes.Structure):
    """``rwrt_phase_map``: the map a ``rwrt_ray_phase`` call deposits into
    (``need`` / ``wcol``: row columns, -1 for none; ``omega_dt``: radians per
    row)."""
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nchan", ctypes.c_int32),
                ("need", ctypes.c_int32), ("wcol", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("lat0", ctypes.c_double), ("inv_dlat", ctypes.c_double), ("inv_dlon", ctypes.c_double),
                ("omega_dt", ctypes.c_double)]


assert ctypes.sizeof(PhaseMapC) == 56


class TubeMapC(ctypes.Structure):
    """``rwrt_tube_map``: the map a ``rwrt_ray_tube`` call deposits into
    (``need``: a row column, -1 for none; ``max_sep``: radians)."""
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nchan", ctypes.c_int32),
                ("need", ctypes.c_int32), ("lat0", ctypes.c_double), ("inv_dlat", ctypes.c_double),
                ("inv_dlon", ctypes.c_double), ("max_sep", ctypes.c_double)]


assert ctypes.sizeof(TubeMapC) == 48


class WaveMapC(ctypes.Structure):
    """``rwrt_wave_map``: the map a ``rwrt_ray_wave`` call deposits into
    (``need`` / ``wcol``: row columns, -1 for none; ``spread``: 0 or 1;
    ``max_sep``: radians; ``omega_dt``: radians per row)."""
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nchan", ctypes.c_int32),
                ("need", ctypes.c_int32), ("wcol", ctypes.c_int32), ("spread", ctypes.c_int32),
                ("lat0", ctypes.c_double), ("inv_dlat", ctypes.c_double), ("inv_dlon", ctypes.c_double),
                ("max_sep", ctypes.c_double), ("omega_dt", ctypes.c_double), ("d_floor", ctypes.c_double)]


assert ctypes.sizeof(WaveMapC) == 72

SUMMARY_MAXREG, SUMMARY_NF64, SUMMARY_NI32 = 8, 9, 4
NDIAG = 23     # RWRT_NDIAG: the planes of rwrt_bs_diag
# RWRT_SHV_*: the planes of rwrt_sh_helmholtz, in bit (and output) order
SHV_PLANES = ("vrt", "div", "psi", "chi", "u_rot", "v_rot", "u_div", "v_div", "vrt_x", "vrt_y")


class SummaryRegions(ctypes.Structure):
    """``rwrt_summary_regions``: the lon-lat boxes of a ``rwrt_ray_summary`` call
    (radians: lon_w, lon_e, lat_s, lat_n)."""
    _fields_ = [("nreg", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("box", (ctypes.c_double * 4) * SUMMARY_MAXREG)]


_lib = None
_P = ctypes.c_void_p
_I64 = ctypes.c_int64
_I32 = ctypes.c_int32
_D = ctypes.c_double


def load():
    """Load librwrt.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RwrtError(f"HIP library not found at {LIB_PATH}: build it with "
                        f"`make -C rossby-wave-ray-tracing_amd/csrc` (hipcc, gfx950)")
    lib = ctypes.CDLL(LIB_PATH)
    lib.rwrt_version.restype = ctypes.c_char_p
    lib.rwrt_last_error.restype = ctypes.c_char_p
    G, Pr, B = ctypes.POINTER(Grid), ctypes.POINTER(Params), ctypes.POINTER(Background)
    M = ctypes.POINTER(DensityMap)
    R = ctypes.POINTER(SummaryRegions)
    A = ctypes.POINTER(ArrivalMap)
    F = ctypes.POINTER(FluxMapC)
    T = ctypes.POINTER(TrackMapC)
    X = ctypes.POINTER(CrossMapC)
    Ph = ctypes.POINTER(PhaseMapC)
    Tu = ctypes.POINTER(TubeMapC)
    sig = {
        "rwrt_pack_fields": [G, _P, _P, _P],
        "rwrt_mercator_point": [G, _P, _I64, _P, _P, _P, _P],
        "rwrt_rhs": [G, _P, _I64, _P, _P, _P],
        "rwrt_dp54_attempt": [G, _P, _I64, _P, _P, _P, _D, _D, _P, _P, _P, _P],
        "rwrt_ray_initial": [G, _P, _I64, _P, _P, _P, _I32, _P, _P, _P, _P],
        "rwrt_expand_tails": [_I64, _I32, _I32, _P, _P, _P, _P],
        "rwrt_row_slots": [_I64, _P, _P, _P, _P],
        "rwrt_expand_slots": [_I64, _I32, _I32, _P, _P, _P, _P, _P, _P],
        "rwrt_launch_plan_bytes": [_I64, ctypes.POINTER(_I64)],
        "rwrt_launch_plan": [_I64, _I32, _P, _P, _P, _P, _P, _P, _P, ctypes.POINTER(_I64), _P, _I64, _P],
        "rwrt_rk4_run": [_P, G, _P, _I64, Pr, _I32, _I32, _P, _P, _P, _P, _P, _P, _P],
        "rwrt_ray_density": [M, _I64, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P],
        "rwrt_ray_arrival": [A, _I64, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P],
        "rwrt_ray_flux": [F, _I64, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P],
        "rwrt_ray_track": [T, _I64, _I32, _I32, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _P],
        "rwrt_ray_cross": [X, _I64, _I32, _I32, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P],
        "rwrt_ray_phase": [Ph, _I64, _I32, _I32, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
        "rwrt_ray_tube": [Tu, _I64, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
        "rwrt_ray_summary": [_I64, _I32, _I32, _P, _P, _P, _P, _P, _I64, R, _P, _P, _P],
        "rwrt_wn_map": [G, _P, _I32, _I64, _I32, _P, _P, _P, _I32, _P, _P, _P, _P, _P, _P, _P],
        "rwrt_wn_fill": [_I32, _I32, _I32, _I32, _P, _P, _P],
        "rwrt_sh_filter": [_I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P],
        "rwrt_bs_ready": [_I32, _I32, _P, _P, _P, _D, _D, _P, _P, _I32, _P],
        "rwrt_bs_diag": [_I32, _I32, _I32, _P, _P, _P, _D, _D, ctypes.c_uint32, _P, _P, _I32, _P],
        "rwrt_ctx_create": [_I32, ctypes.POINTER(_P)],
        "rwrt_ctx_destroy": [_P],
        "rwrt_ctx_set_latency_density": [_P, _I32],
        "rwrt_ctx_set_tv_lanes": [_P, _I32],
        "rwrt_ctx_set_handoff": [_P, _I32],
        "rwrt_ctx_set_trace": [_P, _P, _I64],
        "rwrt_ctx_last_grid": [_P, ctypes.POINTER(_I32), ctypes.POINTER(_I32)],
        "rwrt_rhs_tv": [G, B, _I64, _P, _P, _P, _P],
        "rwrt_kat_rk45": [_I32, _I64, _P, _I32, _P, _D, _D, _D, _P, _P],
        "rwrt_selftest_math": [_I32, _I64, _P, _P, _P, _P],
        "rwrt_host_fill_rows": [_P, _I64, _I64, _I64, _P, _P, _I64, _I64, _P],
    }
    # The twelve rwrt_rk45_* entries, from their pieces: what lies between grid and nray per background kind;
    # n_heavy and the layout's own row arguments for the static and the time-varying trio, all three row
    # arguments and no n_heavy for the stack and release entries.
    rows = {"": [], "_tails": [_P, _P], "_slots": [_P, _P, _P]}
    for kind, bg in {"": [_P], "_tv": [B], "_stack": [ctypes.POINTER(Stack)], "_rel": [B, _P]}.items():
        trio = kind in ("", "_tv")
        sig["rwrt_rk45_init" + kind] = [G] + bg + [_I64, _P, Pr] + [_P] * 6
        for layout in (rows if trio else ["_slots"]):
            sig["rwrt_rk45_run" + kind + (layout if trio else "")] = (
                [_P, G] + bg + [_I64, Pr, _P, _I32, _I32, _P] + ([_I64] if trio else []) + [_P] * 4 + rows[layout] +
                [_P, _P])
    for name, args in sig.items():
        fn = getattr(lib, name, None)
        if fn is None:     # (an older A/B build: bench.py --lib; tests/test_abi.py checks ours)
            continue
        fn.argtypes = args
        fn.restype = ctypes.c_int
    _lib = lib
    return lib


# Entry points bound apart from load()'s table.  The argtypes set on the
# library's attributes are pinned, all of them, by a record that is not taken
# again (tests/test_ray_loop_entries_host.py), so an entry added after it keeps
# its typed binding in a function object of its own: entry(name).
LATER_SIGNATURES = {
    "rwrt_sh_helmholtz": [_I32, _I32, _I32, _I32, ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "rwrt_sh_rws": [_I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "rwrt_ray_wave": [ctypes.POINTER(WaveMapC), _I64, _I32, _I32] + [_P] * 16,
}
_entries = {}


def entry(name):
    """The typed binding of an entry point of ``LATER_SIGNATURES`` (raises if
    the library was not built or lacks the symbol)."""
    if name not in _entries:
        fn = load()[name]           # (a function object of its own, not the attribute's)
        fn.argtypes = LATER_SIGNATURES[name]
        fn.restype = ctypes.c_int
        _entries[name] = fn
    return _entries[name]


def version():
    return load().rwrt_version().decode()


def check(status):
    if status != RWRT_OK:
        msg = load().rwrt_last_error().decode()
        raise RwrtError(f"rwrt status {status}: {msg}")


def require_gpu():
    if not torch.cuda.is_available():
        raise RwrtError("no HIP device visible: the ray integrator runs only on the GPU "
                        "(there is no CPU fallback)")


def dptr(t, dtype=None, what="tensor"):
    """Device pointer of a contiguous tensor (checked)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RwrtError(f"{what} must be a device tensor")
    if dtype is not None and t.dtype != dtype:
        raise RwrtError(f"{what} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RwrtError(f"{what} must be contiguous")
    return t.data_ptr()


def stream(device=None):
    """The current HIP stream of ``device`` (default: torch's current device)."""
    return torch.cuda.current_stream(device).cuda_stream


class Context:
    """An ``rwrt_ctx`` (include/rwrt.h): the scratch of the ray-loop entry points
    on one device.  Engines own one each; distinct contexts are independent."""

    def __init__(self, device):
        require_gpu()
        self.device = torch.device(device)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        h = _P()
        check(load().rwrt_ctx_create(int(idx), ctypes.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def set_latency_density(self, rays_per_wave):
        """Rays per wave in the latency mode (1..16): rwrt_ctx_set_latency_density."""
        if getattr(self, "_qpw", 16) != int(rays_per_wave):
            check(load().rwrt_ctx_set_latency_density(self._h, int(rays_per_wave)))
            self._qpw = int(rays_per_wave)

    def set_tv_lanes(self, lanes):
        """Rays per wave of the fp64 time-varying loops, 64 or 32 (rwrt_ctx_set_tv_lanes)."""
        if getattr(self, "_tvl", 64) != int(lanes):
            check(load().rwrt_ctx_set_tv_lanes(self._h, int(lanes)))
            self._tvl = int(lanes)

    def set_handoff(self, max_rays):
        """Drain-time hand-off threshold, 0..16 rays per wave (rwrt_ctx_set_handoff)."""
        if getattr(self, "_hof", 16) != int(max_rays):
            check(load().rwrt_ctx_set_handoff(self._h, int(max_rays)))
            self._hof = int(max_rays)

    def last_grid(self):
        """``(blocks, rays_per_block)`` of the last ray-loop launch's work-queue
        grid (rwrt_ctx_last_grid): ``blocks * rays_per_block`` rays are in flight
        at once, any further live ray is some lane's second."""
        b, r = _I32(), _I32()
        check(load().rwrt_ctx_last_grid(self._h, ctypes.byref(b), ctypes.byref(r)))
        return int(b.value), int(r.value)

    def set_trace(self, trace=None):
        """Diagnostic ray trace (rwrt_ctx_set_trace): ``trace`` an int64 device
        tensor ``[cap, 10]`` (None: off)."""
        if trace is None:
            check(load().rwrt_ctx_set_trace(self._h, None, 0))
        else:
            check(load().rwrt_ctx_set_trace(self._h, ctypes.c_void_p(trace.data_ptr()), int(trace.shape[0])))
        self._trace = trace

    _plan_scratch = None   # launch_plan's device scratch (uint8) for _plan_rays rays, grown on demand
    _plan_rays = 0

    def launch_plan(self, nray, total, state, count, prev_work, work, order, row_slot, nslot):
        """``rwrt_launch_plan`` on this context's scratch and the device's
        current stream: fills ``work``, ``order``, ``row_slot``, ``nslot`` and
        updates ``prev_work`` (device tensors); returns the number of live rays
        (waits for the stream once)."""
        lib = load()
        if self._plan_scratch is None or self._plan_rays < nray:   # (asked once per size, not per launch)
            need = _I64()
            check(lib.rwrt_launch_plan_bytes(int(nray), ctypes.byref(need)))
            self._plan_scratch = torch.empty(need.value, dtype=torch.uint8, device=self.device)
            self._plan_rays = int(nray)
        n_live = _I64()
        i64 = torch.int64
        check(lib.rwrt_launch_plan(int(nray), PLAN_TOTAL if total else PLAN_SINCE, dptr(state), dptr(count, i64),
                                   dptr(prev_work, i64), dptr(work, i64), dptr(order, i64),
                                   dptr(row_slot, torch.int32), dptr(nslot, i64), ctypes.byref(n_live),
                                   dptr(self._plan_scratch), self._plan_scratch.numel(), stream(self.device)))
        return int(n_live.value)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value and _lib is not None:
            _lib.rwrt_ctx_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass
