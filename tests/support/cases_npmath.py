"""What the host and the GPU tests of csrc/np_math.h share."""
import numpy as np


def svml_host():
    try:
        from numpy._core._multiarray_umath import __cpu_features__ as cf
    except ImportError:
        return False
    return bool(cf.get("AVX512_SKX"))


def trig_args(rng, n):
    half_pi = np.pi / 2
    k = np.arange(-500, 501, dtype=np.float64)
    edges = np.concatenate([k / 128.0, k * np.pi / 16.0, [0.126, 0.855469, 2.426265, half_pi, np.pi]])
    edges = np.concatenate([edges, -edges])
    near = np.concatenate([np.nextafter(edges, np.inf), np.nextafter(edges, -np.inf), edges])
    return np.concatenate([
        rng.uniform(-half_pi, half_pi, n),                        # latitudes
        rng.uniform(-0.2, 0.2, n // 4),                           # half position steps
        rng.standard_normal(n // 4) * 10.0 ** rng.uniform(-30, 0, n // 4),
        rng.uniform(-200.0, 200.0, n // 4),                       # unwrapped longitudes
        rng.uniform(-6.5e4, 6.5e4, n // 8),
        near, [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-300, np.nan, np.inf, -np.inf]])
