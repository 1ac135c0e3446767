// density_bins.h -- the bin index of a ray-density map (rwrt_ray_density,
// include/rwrt.h), shared by the device kernel (csrc/density.hip) and by host
// programs (tests/host/density_bins_main.cpp runs it under the sanitizers).
//
// The definition is density.reference_bins (NumPy); this restates it operation
// for operation -- one multiply for the longitude, one subtract and one
// multiply for the latitude, no fused multiply-add (build with
// -ffp-contract=off) -- so that every index equals NumPy's bit for bit.
//
// A wrong index is an out-of-bounds atomic, so the order is part of the
// specification: finite -> range check in fp64 -> conversion to integer.
#ifndef RWRT_DENSITY_BINS_H
#define RWRT_DENSITY_BINS_H

#include <cmath>
#include <cstdint>

#include "rwrt.h"

#if defined(__HIPCC__)
#define RWRT_HD __host__ __device__
#else
#define RWRT_HD
#endif

namespace rwrt {

// (lon % (2 pi)) % (2 pi) with Python's float % -- the longitude every lookup
// of the ray loops uses (py_mod_2pi_again(py_mod_2pi(lon)) in csrc/rwrt.hip,
// the same steps): fmod is exact; for |lon| < 2^40 the quotient
// trunc(|lon| / 2 pi) from one multiply is off by at most one, which shows as
// a remainder outside [0, 2 pi) and is corrected exactly with one more FMA.
// NaN and +-inf give NaN.
RWRT_HD inline double density_wrap_2pi(double lon) {
  constexpr double b = 2.0 * 3.14159265358979323846, binv = 1.0 / b;
  const double x = fabs(lon);
  double r;
  if (x < 0x1p40) {
    const double n = trunc(x * binv);
    r = fma(-n, b, x);
    const double lo = r + b, hi = fma(-(n + 1.0), b, x);
    r = (r < 0.0) ? lo : ((r >= b) ? hi : r);
  } else {
    r = fabs(fmod(lon, b));   // huge, infinite or NaN (rare)
  }
  double m = copysign(r, lon);
  // Python's %: a remainder of the other sign moves into [0, b); zero is +0
  if (m != 0.0) {
    if (m < 0.0) m += b;
  } else {
    m = 0.0;
  }
  // the second %: only a remainder that rounded up to 2 pi itself changes
  return (m >= b) ? 0.0 : m;
}

// Flat index (c * ny + iy) * nx + ix of the point (lam, lat) of a ray with
// channel c, lam = density_wrap_2pi(lon); -1 when the point is not binned
// (non-finite lon / lat, latitude outside [lat0, lat1), channel outside
// [0, nchan), or a non-finite weight when the map sums one).
RWRT_HD inline int32_t density_bin(double lam, double lat, double w, int32_t c, const rwrt_density_map& m) {
  if (!(c >= 0 && c < m.nchan)) return -1;
  if (!(fabs(lam) <= 1.7976931348623157e308) || !(fabs(lat) <= 1.7976931348623157e308)) return -1;
  if (m.wcol >= 0 && !(fabs(w) <= 1.7976931348623157e308)) return -1;
  const double fx = floor(lam * m.inv_dlon);
  const double fy = floor((lat - m.lat0) * m.inv_dlat);
  // the range checks are made on the fp64 values: only a value known to lie in
  // [0, n) is converted (NaN and +-inf fail the comparisons)
  if (!(fy >= 0.0 && fy < (double)m.ny)) return -1;
  if (!(fx >= 0.0)) return -1;   // (never for a wrapped longitude)
  // min(floor(lam * inv_dlon), nx - 1): lam just below 2 pi can round up to nx
  const int32_t ix = (fx < (double)m.nx) ? (int32_t)fx : m.nx - 1;
  const int32_t iy = (int32_t)fy;
  return (c * m.ny + iy) * m.nx + ix;
}

}  // namespace rwrt

#endif  // RWRT_DENSITY_BINS_H
