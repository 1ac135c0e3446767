// flux_rows.h -- one ray's rows of a launch reduced into a wave-ray flux map
// (rwrt_ray_flux, include/rwrt.h), shared by the device kernel (csrc/flux.hip,
// whose emitter issues atomics) and by host programs
// (tests/host/flux_rows_main.cpp updates plain arrays under the sanitizers).
//
// The definition is flux.reference_flux (NumPy); this restates its accept rule
// and its index arithmetic operation for operation -- products and sums
// rounded one by one, no fused multiply-add (build with -ffp-contract=off) --
// so that every accept decision and every index equals NumPy's.
//
// A wrong index is an out-of-bounds atomic, so the order is part of the
// specification: finite -> range check in fp64 -> conversion to integer.
//
// The lane keeps the current bin's run: its points, the sum of their row
// indices and the three sums, added in row order.
//   bin change      add_cnt(bin, n, rowsum), add_sum(bin, fx, fy, fs)
//   constant tail   one run of it_end - tf rows: n, n tf + n (n - 1) / 2, v * n
// so a frozen ray costs one emit pair, not one per row.
//
// An emitter E has
//   void add_cnt(int64_t index, unsigned long long n, long long rowsum);
//   void add_sum(int64_t index, double fx, double fy, double fs);
// with `index` the bin (c * ny + iy) * nx + ix: the integers of the bin are at
// cnt[2 * index], its sums at sum[3 * index].
#ifndef RWRT_FLUX_ROWS_H
#define RWRT_FLUX_ROWS_H

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "density_bins.h"
#include "launch_rows.h"

namespace rwrt {

constexpr int32_t kFluxUnit = 1;        // rwrt_flux_map.mode bit 0
constexpr int32_t kFluxUnwrapped = 2;   // bit 1

struct FluxRow {   // what the lane needs of a row
  double lon, lat, k, l, ug, vg;
};

#if defined(__HIPCC__)
// (ug vg are columns 5 and 6: 8-byte aligned only)
typedef double flux_double2_a8 __attribute__((ext_vector_type(2), aligned(8)));
#endif

// three 16-byte loads on the device: lon lat, k l, ug vg (rows are 16-byte aligned there)
RWRT_HD inline FluxRow flux_load(const double* r) {
#if defined(__HIPCC__)
  const double2 p = *reinterpret_cast<const double2*>(r);
  const double2 w = *reinterpret_cast<const double2*>(r + 2);
  const flux_double2_a8 g = *reinterpret_cast<const flux_double2_a8*>(r + 5);
  return {p.x, p.y, w.x, w.y, g.x, g.y};
#else
  return {r[0], r[1], r[2], r[3], r[5], r[6]};
#endif
}

struct FluxPoint {
  int32_t bin;          // -1: not accepted
  double vx, vy, sp;    // (set only with bin >= 0)
};

RWRT_HD inline bool flux_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// The accept rule and the bin of one row of a ray with channel c.
RWRT_HD inline FluxPoint flux_point(const FluxRow& v, int32_t c, const rwrt_flux_map& m) {
  const FluxPoint none{-1, 0.0, 0.0, 0.0};
  if (!(c >= 0 && c < m.nchan)) return none;
  if (!flux_finite(v.lon) || !flux_finite(v.lat) || !flux_finite(v.ug) || !flux_finite(v.vg)) return none;
  if (!(fabs(v.k) <= m.wn_max) || !(fabs(v.l) <= m.wn_max)) return none;   // (false for NaN)
  const double uu = v.ug * v.ug, vv = v.vg * v.vg;
  const double s2 = uu + vv;
  if (!flux_finite(s2) || !(s2 >= m.s2_min && s2 <= m.s2_max)) return none;
  const bool unit = (m.mode & kFluxUnit) != 0;
  if (unit && !(s2 > 0.0)) return none;
  // only a value known to lie in [0, n) is converted (NaN and +-inf fail the comparisons)
  const double fy = floor((v.lat - m.lat0) * m.inv_dlat);
  if (!(fy >= 0.0 && fy < (double)m.ny)) return none;
  int32_t ix;
  if (m.mode & kFluxUnwrapped) {
    const double fx = floor((v.lon - m.lon0) * m.inv_dlon);
    if (!(fx >= 0.0 && fx < (double)m.nx)) return none;   // outside the window
    ix = (int32_t)fx;
  } else {
    const double fx = floor(density_wrap_2pi(v.lon) * m.inv_dlon);
    if (!(fx >= 0.0)) return none;   // (never for a wrapped longitude)
    // min(floor(lam * inv_dlon), nx - 1): lam just below 2 pi can round up to nx
    ix = (fx < (double)m.nx) ? (int32_t)fx : m.nx - 1;
  }
  const int32_t bin = (c * m.ny + (int32_t)fy) * m.nx + ix;
  const double sp = sqrt(s2);
  return unit ? FluxPoint{bin, v.ug / sp, v.vg / sp, sp} : FluxPoint{bin, v.ug, v.vg, sp};
}

struct FluxRun {
  int32_t bin = -1;            // -1: no run
  unsigned long long n = 0;
  long long rowsum = 0;
  double fx = 0.0, fy = 0.0, fs = 0.0;
};

template <class E>
RWRT_HD inline void flux_flush(FluxRun& r, E& e) {
  if (r.bin >= 0) {
    e.add_cnt((int64_t)r.bin, r.n, r.rowsum);
    e.add_sum((int64_t)r.bin, r.fx, r.fy, r.fs);
  }
  r.bin = -1;
}

// `rows` >= 1 equal points from row i on; rows must be fed in order
template <class E>
RWRT_HD inline void flux_points(FluxRun& r, int32_t i, int32_t rows, const FluxPoint& p, E& e) {
  if (p.bin != r.bin) {
    flux_flush(r, e);
    r.bin = p.bin;
    r.n = 0;
    r.rowsum = 0;
    r.fx = r.fy = r.fs = 0.0;
  }
  if (p.bin < 0) return;
  const long long n = rows;
  const double dn = (double)rows;   // (rows = 1: the value itself)
  r.n += (unsigned long long)n;
  r.rowsum += n * (long long)i + n * (n - 1) / 2;   // i + (i + 1) + .. + (i + n - 1); below 2^63 for n, |i| < 2^31
  r.fx = r.fx + p.vx * dn;
  r.fy = r.fy + p.vy * dn;
  r.fs = r.fs + p.sp * dn;
}

// Ray j (channel c) of the launch L: BATCH rows loaded ahead, as the density
// kernel walks them.
template <int BATCH, class E>
RWRT_HD inline void flux_ray(const LaunchRows& L, int64_t j, int32_t c, const rwrt_flux_map& m, E& e) {
  if (c < 0 || c >= m.nchan) return;
  FluxRun run;
  launch_rows_walk<BATCH, FluxRow>(
      L, j, [](const double* r) { return flux_load(r); },
      [&](int32_t i, const FluxRow& v) { flux_points(run, i, 1, flux_point(v, c, m), e); },
      [&](int32_t tf, int32_t n, const FluxRow& v) { flux_points(run, tf, n, flux_point(v, c, m), e); });
  flux_flush(run, e);
}

}  // namespace rwrt

#endif  // RWRT_FLUX_ROWS_H
