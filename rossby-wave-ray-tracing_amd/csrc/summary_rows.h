// summary_rows.h -- the per-row update of one ray's path summary
// (rwrt_ray_summary, include/rwrt.h), shared by the device kernel
// (csrc/summary.hip) and by host programs (tests/host/summary_rows_main.cpp
// runs it under the sanitizers).
//
// The definition is summary.reference_summary (NumPy).  Everything but `path`
// is a count or a selection and equals NumPy's bit for bit; `path` adds the
// same non-negative haversine angles in the same (row) order with this
// platform's sin / cos / atan2 / sqrt, no fused multiply-add (build with
// -ffp-contract=off), and is compared by tolerance.
//
// A row is valid iff its lon and lat are finite.  A segment (and a sign change
// of l) is counted for row i iff rows i-1 and i are both valid, so the
// accumulator carries the previous row: its validity in `prev_valid`, its lon,
// lat and l in `lon_last, lat_last, l_last` (a valid previous row IS the last
// valid row).  That is what lets a ray's rows arrive in several calls.
#ifndef RWRT_SUMMARY_ROWS_H
#define RWRT_SUMMARY_ROWS_H

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "density_bins.h"   // RWRT_HD, density_wrap_2pi

namespace rwrt {

// One ray's accumulator; NR: the regions it has room for (0 .. RWRT_SUMMARY_MAXREG).
// The initial values are those of a ray with no row yet (summary.RaySummary
// writes the same into the device arrays).
template <int NR>
struct SummaryAcc {
  double lon_first = NAN, lat_first = NAN, lon_last = NAN, lat_last = NAN, l_last = NAN;
  double lat_min = INFINITY, lat_max = -INFINITY, amp_max = -INFINITY, path = 0.0;
  int32_t n_valid = 0, last_row = -1, n_turn = 0, prev_valid = 0;
  int32_t first_row[NR > 0 ? NR : 1];
  int32_t rows_inside[NR > 0 ? NR : 1];
  RWRT_HD SummaryAcc() {
    for (int r = 0; r < (NR > 0 ? NR : 1); ++r) {
      first_row[r] = -1;
      rows_inside[r] = 0;
    }
  }
};

RWRT_HD inline bool summary_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// The haversine angle between (lon_p, lat_p) and (lon_c, lat_c): the
// reference's cal_dis, operation for operation.
RWRT_HD inline double summary_segment(double lon_c, double lat_c, double lon_p, double lat_p) {
  const double dlon = lon_c - lon_p, dlat = lat_c - lat_p;
  const double sa = sin(dlat / 2.0), sb = sin(dlon / 2.0);
  const double a = sa * sa + (cos(lat_p) * cos(lat_c)) * (sb * sb);
  return fabs(2.0 * atan2(sqrt(a), sqrt(1.0 - a)));
}

// Bit r set: the valid point (lon, lat) lies in box r -- lat_s <= lat < lat_n
// and, with lam = (lon % 2 pi) % 2 pi, lon_w <= lam < lon_e, or
// lam >= lon_w or lam < lon_e for a box across 0 (lon_w >= lon_e).
template <int NR>
RWRT_HD inline uint32_t summary_inside(const rwrt_summary_regions& reg, double lon, double lat) {
  uint32_t in = 0;
  if (NR == 0 || reg.nreg <= 0) return in;
  const double lam = density_wrap_2pi(lon);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < NR; ++r) {
    if (r >= reg.nreg) continue;
    const double w = reg.box[r][0], e = reg.box[r][1], s = reg.box[r][2], n = reg.box[r][3];
    const bool in_lat = lat >= s && lat < n;
    const bool in_lon = (w < e) ? (lam >= w && lam < e) : (lam >= w || lam < e);
    if (in_lat && in_lon) in |= 1u << r;
  }
  return in;
}

// Row i = (lon, lat, l, amp) of the ray.  Returns the regions it lies in
// (0 for a row that is not valid).
template <int NR>
RWRT_HD inline uint32_t summary_row(SummaryAcc<NR>& a, const rwrt_summary_regions& reg, int32_t i, double lon,
                                    double lat, double l, double amp) {
  const bool valid = summary_finite(lon) && summary_finite(lat);
  if (!valid) {
    a.prev_valid = 0;
    return 0;
  }
  if (a.prev_valid) {
    if ((a.l_last > 0.0 && l < 0.0) || (a.l_last < 0.0 && l > 0.0)) a.n_turn += 1;
    // (equal points: a == 0 and atan2(0, 1) == 0, the sum does not change)
    if (!(lon == a.lon_last && lat == a.lat_last)) a.path = a.path + summary_segment(lon, lat, a.lon_last, a.lat_last);
  }
  if (a.n_valid == 0) {
    a.lon_first = lon;
    a.lat_first = lat;
  }
  a.n_valid += 1;
  a.last_row = i;
  a.lon_last = lon;
  a.lat_last = lat;
  a.l_last = l;
  a.prev_valid = 1;
  if (lat < a.lat_min) a.lat_min = lat;
  if (lat > a.lat_max) a.lat_max = lat;
  if (summary_finite(amp)) {
    const double v = fabs(amp);
    if (v > a.amp_max) a.amp_max = v;
  }
  const uint32_t in = summary_inside<NR>(reg, lon, lat);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < NR; ++r) {
    if (in & (1u << r)) {
      if (a.first_row[r] < 0) a.first_row[r] = i;
      a.rows_inside[r] += 1;
    }
  }
  return in;
}

// Rows [i, i + m) all equal to (lon, lat, l, amp), m >= 1: a constant tail in
// closed form.  The first is an ordinary row against the carried previous
// row; the other m - 1 repeat it -- a zero segment each, no sign change, the
// same extrema -- so they only count: m - 1 more valid rows, m - 1 more rows
// in every region the point lies in, and the last of them is the last row.
template <int NR>
RWRT_HD inline void summary_tail(SummaryAcc<NR>& a, const rwrt_summary_regions& reg, int32_t i, int32_t m, double lon,
                                 double lat, double l, double amp) {
  const uint32_t in = summary_row<NR>(a, reg, i, lon, lat, l, amp);
  if (m <= 1 || !a.prev_valid) return;
  a.n_valid += m - 1;
  a.last_row = i + m - 1;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < NR; ++r) {
    if (in & (1u << r)) a.rows_inside[r] += m - 1;
  }
}

}  // namespace rwrt

#endif  // RWRT_SUMMARY_ROWS_H
