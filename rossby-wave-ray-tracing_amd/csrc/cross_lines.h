// cross_lines.h -- one ray's rows of a launch tested against up to
// RWRT_CROSS_MAXGATE gates (rwrt_ray_cross, include/rwrt.h): latitude circles
// and meridians, each crossing of a segment between two consecutive valid rows
// reported with its direction, its place along the gate and its time.  Shared
// by the device kernel (csrc/cross.hip, whose emitter issues atomics) and by
// host programs (tests/host/cross_lines_main.cpp updates plain arrays under
// the sanitizers).
//
// The definition is cross.reference_cross (Python); this restates it operation
// for operation -- every difference, product and quotient rounded on its own,
// IEEE division, no fused multiply-add (build with -ffp-contract=off) -- so
// that every side, every bin and every crossing time equals the definition's.
//
// A row's SIDE of a gate is one number, computed once per row and carried to
// the next row:
//   latitude circle   (lat >= pos) as 0.0 / 1.0
//   meridian          floor((lon - pos) * (1 / 2 pi)), the circle the ray is on
// and a segment crosses the gate iff the sides of its ends differ, in
// direction 0 (northward, eastward) iff the side grew.  Everything else -- the
// drop rule, the division, the interpolation, the bin -- is cross_hit, which
// runs only for a crossing.
//
// A wrong bin is an out-of-bounds atomic, so the order is part of the
// specification: the drop rule and every range check are made on the fp64
// values, and only a value known to lie in [0, nbin) is converted.
//
// An emitter E has
//   void hit(int32_t g, int32_t d, int32_t w, int32_t bin, double tc, double wv);
//   void drop();
// with `bin` -1 for a crossing outside the map (per-ray counts only) and `w`
// the time window.
#ifndef RWRT_CROSS_LINES_H
#define RWRT_CROSS_LINES_H

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "density_bins.h"   // RWRT_HD, density_wrap_2pi
#include "launch_rows.h"

namespace rwrt {

constexpr double kCrossTwoPi = 2.0 * 3.14159265358979323846;
constexpr double kCrossInvTwoPi = 1.0 / kCrossTwoPi;   // (one IEEE division, as the caller of the definition takes it)
constexpr double kCrossMaxCircle = 1073741824.0;       // 2^30

struct CrossRow {   // what the lane needs of a row
  double lon, lat, need, v;
};

// lon lat in one 16-byte load on the device (rows are 16-byte aligned there);
// the two named columns (0.0 for none: finite)
RWRT_HD inline CrossRow cross_load(const double* r, const rwrt_cross_map& m) {
#if defined(__HIPCC__)
  const double2 p = *reinterpret_cast<const double2*>(r);
  return {p.x, p.y, m.need >= 0 ? r[m.need] : 0.0, m.wcol >= 0 ? r[m.wcol] : 0.0};
#else
  return {r[0], r[1], m.need >= 0 ? r[m.need] : 0.0, m.wcol >= 0 ? r[m.wcol] : 0.0};
#endif
}

RWRT_HD inline bool cross_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

RWRT_HD inline bool cross_valid(const CrossRow& v) {
  return cross_finite(v.lon) && cross_finite(v.lat) && cross_finite(v.need) && cross_finite(v.v);
}

// the side of gate g a valid row lies on (finite: lon and lat are)
RWRT_HD inline double cross_side(const rwrt_cross_gate& g, double lon, double lat) {
  if (g.kind == 0) return lat >= g.pos ? 1.0 : 0.0;
  return floor((lon - g.pos) * kCrossInvTwoPi);
}

struct CrossHit {
  int32_t dir;   // 0 northward / eastward, 1 southward / westward; -1: the segment is dropped
  int32_t bin;   // -1: outside the map
  double t;      // where on the segment, 0..1
};

// The crossing of gate g by the segment (lon0, lat0) -> (lon1, lat1) whose
// ends lie on the sides s0 != s1.
RWRT_HD inline CrossHit cross_hit(const rwrt_cross_gate& g, int32_t nbin, double s0, double s1, double lon0,
                                  double lat0, double lon1, double lat1) {
  CrossHit h;
  h.dir = s1 > s0 ? 0 : 1;
  h.bin = -1;
  if (g.kind == 0) {
    h.t = (g.pos - lat0) / (lat1 - lat0);
    const double lon_c = lon0 + h.t * (lon1 - lon0);
    // (lon1 - lon0 may overflow for |lon| near the largest double: NaN then, and no bin)
    const double fx = floor(density_wrap_2pi(lon_c) * g.inv_d);
    if (fx >= 0.0) h.bin = fx < (double)nbin ? (int32_t)fx : nbin - 1;   // (lam just below 2 pi can round up to nbin)
    return h;
  }
  if (!(fabs(s0) <= kCrossMaxCircle) || !(fabs(s1) <= kCrossMaxCircle) || fabs(s1 - s0) > 1.0) {
    h.dir = -1;
    h.t = 0.0;
    return h;
  }
  const double u0 = lon0 - g.pos, u1 = lon1 - g.pos;
  const double G = (s1 > s0 ? s1 : s0) * kCrossTwoPi;
  double t = (G - u0) / (u1 - u0);
  t = t < 0.0 ? 0.0 : t;   // (-0.0 stays)
  t = t > 1.0 ? 1.0 : t;
  h.t = t;
  const double lat_c = lat0 + t * (lat1 - lat0);
  const double fb = floor((lat_c - g.org) * g.inv_d);
  if (fb >= 0.0 && fb < (double)nbin) h.bin = (int32_t)fb;
  return h;
}

// The lane's state: the carried previous row (lon NaN: none) and its sides.
template <int NG>
struct CrossState {
  double lon, lat, v;
  double side[NG];
};

template <int NG>
RWRT_HD inline void cross_sides(const rwrt_cross_map& m, double lon, double lat, double* side) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int g = 0; g < NG; ++g) side[g] = cross_side(m.gate[g], lon, lat);
}

// the sides of the row a call starts from (d_prev holds no sides)
template <int NG>
RWRT_HD inline void cross_begin(const rwrt_cross_map& m, CrossState<NG>& s) {
  if (s.lon == s.lon) cross_sides<NG>(m, s.lon, s.lat, s.side);
}

// Row i of a ray: the segment from the carried row into it.
template <int NG, class E>
RWRT_HD inline void cross_row(CrossState<NG>& s, int32_t i, const CrossRow& r, const rwrt_cross_map& m, E& e) {
  if (!cross_valid(r)) {
    s.lon = NAN;   // the segments on both sides vanish
    return;
  }
  double side[NG];
  cross_sides<NG>(m, r.lon, r.lat, side);
  if (s.lon == s.lon) {   // a valid previous row
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int g = 0; g < NG; ++g) {
      if (side[g] == s.side[g]) continue;
      const CrossHit h = cross_hit(m.gate[g], m.nbin, s.side[g], side[g], s.lon, s.lat, r.lon, r.lat);
      if (h.dir < 0) {
        e.drop();
        continue;
      }
      const int32_t w = m.window_rows > 0 ? (i - 1) / m.window_rows : 0;
      e.hit(g, h.dir, w, h.bin, (double)(i - 1) + h.t, s.v + h.t * (r.v - s.v));
    }
  }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int g = 0; g < NG; ++g) s.side[g] = side[g];
  s.lon = r.lon;
  s.lat = r.lat;
  s.v = r.v;
}

// Ray j of the launch L, its carried row in `s` on entry and on return: BATCH
// rows loaded ahead.  A constant tail is its first row: the segments of length
// zero that follow cross nothing.
template <int NG, int BATCH, class E>
RWRT_HD inline void cross_ray(const LaunchRows& L, int64_t j, const rwrt_cross_map& m, CrossState<NG>& s, E& e) {
  cross_begin<NG>(m, s);
  launch_rows_walk<BATCH, CrossRow>(
      L, j, [&](const double* r) { return cross_load(r, m); },
      [&](int32_t i, const CrossRow& v) { cross_row<NG>(s, i, v, m, e); },
      [&](int32_t i, int32_t, const CrossRow& v) { cross_row<NG>(s, i, v, m, e); });
}

// the flat index of a map bin: [nwin][ngate][2][nchan][nbin]
RWRT_HD inline int64_t cross_index(const rwrt_cross_map& m, int32_t w, int32_t g, int32_t d, int32_t c, int32_t bin) {
  return ((((int64_t)w * m.ngate + g) * 2 + d) * m.nchan + c) * m.nbin + bin;
}

}  // namespace rwrt

#endif  // RWRT_CROSS_LINES_H
