// phase_rows.h -- one ray's rows of a launch integrated into the WKB phase
// theta = int k dlon + l dY, dY = dlat / cos(lat), and deposited as waves
// w exp(i psi) into a lon-lat map (rwrt_ray_phase, include/rwrt.h).  Shared by
// the device kernel (csrc/phase.hip, whose emitter issues atomics) and by host
// programs (tests/host/phase_rows_main.cpp updates plain arrays under the
// sanitizers).
//
// The definition is phase.reference_phase (NumPy); this restates it operation
// for operation -- every sum, difference, product and quotient rounded on its
// own, no fused multiply-add (build with -ffp-contract=off) -- so that theta
// differs from the definition's only through cos, and every count and every
// bin equals it.
//
// What is carried from a row to the next: lon, lat, k and a = l / cos(lat)
// (lon NaN: no valid previous row), so that a row costs one cos.
//
// The bin is density_bins.h's, on a rwrt_density_map made of the phase map's
// grid (phase_bins): a wrong index is an out-of-bounds atomic, and that code
// converts only a value known to lie in [0, n).
//
// An emitter E has
//   void add(int32_t bin, int32_t n, double re, double im, double wabs);
//   void drop(int32_t n);
// with `n` the deposits (rows) the sums stand for.
#ifndef RWRT_PHASE_ROWS_H
#define RWRT_PHASE_ROWS_H

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "density_bins.h"   // RWRT_HD, density_wrap_2pi, density_bin
#include "launch_rows.h"

namespace rwrt {

constexpr double kPhaseHalfPi = 1.5707963267948966;   // the double nearest pi / 2
constexpr int32_t kPhaseInvalid = -2;                 // phase_row: the row was not valid (-1: valid, not binned)

struct PhaseRow {   // what the lane needs of a row
  double lon, lat, k, l, need, w;
};

// lon lat and k l in one 16-byte load each on the device (rows are 16-byte
// aligned there); the two named columns (none: 0.0 and the weight 1.0, finite)
RWRT_HD inline PhaseRow phase_load(const double* r, const rwrt_phase_map& m) {
#if defined(__HIPCC__)
  const double2 p = *reinterpret_cast<const double2*>(r);
  const double2 q = *reinterpret_cast<const double2*>(r + 2);
  return {p.x, p.y, q.x, q.y, m.need >= 0 ? r[m.need] : 0.0, m.wcol >= 0 ? r[m.wcol] : 1.0};
#else
  return {r[0], r[1], r[2], r[3], m.need >= 0 ? r[m.need] : 0.0, m.wcol >= 0 ? r[m.wcol] : 1.0};
#endif
}

RWRT_HD inline bool phase_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

RWRT_HD inline bool phase_valid(const PhaseRow& v) {
  return phase_finite(v.lon) && phase_finite(v.lat) && phase_finite(v.k) && phase_finite(v.l) &&
         phase_finite(v.need) && phase_finite(v.w) && fabs(v.lat) < kPhaseHalfPi;
}

// a of a valid row: cos(lat) > 0 there
RWRT_HD inline double phase_a(double l, double lat) { return l / cos(lat); }

// what segment (lon0, lat0, k0, a0) -> (lon1, lat1, k1, a1) adds to theta
RWRT_HD inline double phase_segment(double lon0, double lat0, double k0, double a0, double lon1, double lat1,
                                    double k1, double a1) {
  const double dk = (0.5 * (k0 + k1)) * (lon1 - lon0);
  const double dl = (0.5 * (a0 + a1)) * (lat1 - lat0);
  return dk + dl;
}

// the map's grid as density_bin takes it
RWRT_HD inline rwrt_density_map phase_bins(const rwrt_phase_map& m) {
  return {m.nx, m.ny, m.nchan, m.wcol, m.inv_dlon, m.lat0, m.inv_dlat};
}

RWRT_HD inline void phase_sincos(double x, double* s, double* c) {
#if defined(__HIP_DEVICE_COMPILE__)
  sincos(x, s, c);
#else
  *s = sin(x);
  *c = cos(x);
#endif
}

// `n` equal deposits of w exp(i psi) into `bin` (-1: none): for n > 1 one
// product (double)n * term per sum.  A psi that is not finite drops them.
template <class E>
RWRT_HD inline void phase_deposit(int32_t bin, double psi, double w, int32_t n, E& e) {
  if (bin < 0) return;
  if (!phase_finite(psi)) {
    e.drop(n);
    return;
  }
  double s, c;
  phase_sincos(psi, &s, &c);
  double re = w * c, im = w * s, wabs = fabs(w);
  if (n > 1) {
    const double f = (double)n;
    re = f * re;
    im = f * im;
    wabs = f * wabs;
  }
  e.add(bin, n, re, im, wabs);
}

// The lane's state: the carried previous row (lon NaN: none) and the ray's sums.
struct PhaseState {
  double lon, lat, k, a, theta;
  int32_t nseg;
};

// Row i of a ray with channel `chan` in [0, nchan): the segment from the
// carried row into it, and its deposit.  Returns its bin (-1: valid and not
// binned), kPhaseInvalid for a row that is not valid.
template <class E>
RWRT_HD inline int32_t phase_row(PhaseState& s, int32_t i, const PhaseRow& r, const rwrt_phase_map& m,
                                 const rwrt_density_map& bins, int32_t chan, E& e) {
  if (!phase_valid(r)) {
    s.lon = NAN;   // the segments on both sides vanish
    return kPhaseInvalid;
  }
  const double a = phase_a(r.l, r.lat);
  if (s.lon == s.lon) {   // a valid previous row
    s.theta = s.theta + phase_segment(s.lon, s.lat, s.k, s.a, r.lon, r.lat, r.k, a);
    s.nseg += 1;
  }
  s.lon = r.lon;
  s.lat = r.lat;
  s.k = r.k;
  s.a = a;
  const int32_t bin = density_bin(density_wrap_2pi(r.lon), r.lat, r.w, chan, bins);
  phase_deposit(bin, s.theta - m.omega_dt * (double)i, r.w, 1, e);
  return bin;
}

// Rows [i, i + n) all equal to r, n >= 1: a constant tail.  The first is an
// ordinary row against the carried row; each of the other n - 1 joins the row
// to itself: one more segment, whose sum is +0 (NaN where an average
// overflows) -- added once, which leaves theta as adding it n - 1 times does --
// and one more deposit into the same bin, with the same psi when omega_dt == 0
// (one product for all of them) and row by row otherwise.
template <class E>
RWRT_HD inline void phase_tail(PhaseState& s, int32_t i, int32_t n, const PhaseRow& r, const rwrt_phase_map& m,
                               const rwrt_density_map& bins, int32_t chan, E& e) {
  const int32_t bin = phase_row(s, i, r, m, bins, chan, e);
  if (n <= 1 || bin == kPhaseInvalid) return;
  s.theta = s.theta + phase_segment(s.lon, s.lat, s.k, s.a, s.lon, s.lat, s.k, s.a);
  s.nseg += n - 1;
  if (bin < 0) return;
  if (m.omega_dt == 0.0) {
    phase_deposit(bin, s.theta, r.w, n - 1, e);
  } else {
    for (int32_t q = 1; q < n; ++q) phase_deposit(bin, s.theta - m.omega_dt * (double)(i + q), r.w, 1, e);
  }
}

// Ray j of the launch L, its state in `s` on entry and on return: BATCH rows
// loaded ahead.  A launch that starts at row 0 has no previous row.
template <int BATCH, class E>
RWRT_HD inline void phase_ray(const LaunchRows& L, int64_t j, const rwrt_phase_map& m, const rwrt_density_map& bins,
                              int32_t chan, PhaseState& s, E& e) {
  if (L.it_begin == 0) s.lon = NAN;
  launch_rows_walk<BATCH, PhaseRow>(
      L, j, [&](const double* r) { return phase_load(r, m); },
      [&](int32_t i, const PhaseRow& v) { phase_row(s, i, v, m, bins, chan, e); },
      [&](int32_t i, int32_t n, const PhaseRow& v) { phase_tail(s, i, n, v, m, bins, chan, e); });
}

}  // namespace rwrt

#endif  // RWRT_PHASE_ROWS_H
