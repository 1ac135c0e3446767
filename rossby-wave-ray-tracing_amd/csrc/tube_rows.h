// tube_rows.h -- one ray's tube over the rows of a launch: the cross-section
// spanned by its neighbours in the source lattice, its sign changes (caustics)
// and its deposits into a lon-lat map (rwrt_ray_tube, include/rwrt.h).  Shared
// by the device kernel (csrc/tube.hip, whose emitter issues atomics) and by
// host programs (tests/host/tube_rows_main.cpp updates plain arrays under the
// sanitizers).
//
// The definition is tube.reference_tube (NumPy); this restates it operation
// for operation -- every difference, product and quotient rounded on its own,
// no fused multiply-add (build with -ffp-contract=off).  Every integer output
// rests on the sign of jac = dla * dpb - dlb * dpa, which holds no
// transcendental, so it equals the definition's bit for bit; D and the tube's
// columns differ only through cos, slog through log too.
//
// The first consumer that reads other rays' rows: a stencil ray's row i is row
// i of its block while i < its tail_from, else its tail row (tube_row_ptr).
// Nothing but the lane's own state is written, so the lanes do not depend on
// one another.
//
// The bin is density_bins.h's, on a rwrt_density_map made of the tube map's
// grid (tube_bins): a wrong index is an out-of-bounds atomic, and that code
// converts only a value known to lie in [0, n).
//
// An emitter E has
//   void add(int32_t bin, int32_t n, double slog);   n open rows, their summed log|D|
//   void caustic(int32_t bin);
//   void drop(int32_t n);                            n open rows with jac == 0
//   void bad_index();                                a neighbour outside [-1, nray)
#ifndef RWRT_TUBE_ROWS_H
#define RWRT_TUBE_ROWS_H

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "density_bins.h"   // RWRT_HD, density_wrap_2pi, density_bin
#include "launch_rows.h"

namespace rwrt {

constexpr double kTubeHalfPi = 1.5707963267948966;   // the double nearest pi / 2
constexpr double kTubePi = 3.141592653589793;        // the double nearest pi
constexpr int32_t kTubeOpen = 16;                    // flags: the tube is open
constexpr int kTubeNI = RWRT_TUBE_NI, kTubeNF = RWRT_TUBE_NF;

struct TubePoint {   // what the lane needs of a row
  double lon, lat, need;
};

// lon lat in one 16-byte load on the device (rows are 16-byte aligned there)
// and the need column (none: 0.0, finite)
RWRT_HD inline TubePoint tube_load(const double* r, const rwrt_tube_map& m) {
#if defined(__HIPCC__)
  const double2 p = *reinterpret_cast<const double2*>(r);
  return {p.x, p.y, m.need >= 0 ? r[m.need] : 0.0};
#else
  return {r[0], r[1], m.need >= 0 ? r[m.need] : 0.0};
#endif
}

RWRT_HD inline bool tube_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

RWRT_HD inline bool tube_valid(const TubePoint& v) {
  return tube_finite(v.lon) && tube_finite(v.lat) && tube_finite(v.need) && fabs(v.lat) < kTubeHalfPi;
}

// ((d + pi) % 2 pi) % 2 pi - pi with Python's %: a longitude difference in [-pi, pi)
RWRT_HD inline double tube_wrap(double d) { return density_wrap_2pi(d + kTubePi) - kTubePi; }

// the map's grid as density_bin takes it (no weight)
RWRT_HD inline rwrt_density_map tube_bins(const rwrt_tube_map& m) {
  return {m.nx, m.ny, m.nchan, -1, m.inv_dlon, m.lat0, m.inv_dlat};
}

// The lane's state: what is carried from a launch to the next and the ray's results.
struct TubeState {
  int32_t flags, mu, first, nrow, close_row;
  double jac_prev, jac0, cos0, dmin, dlast;
  double f0[4], flast[4];
};

// state_i[kTubeNI][nray], state_f[kTubeNF][nray]: ray j is column j
RWRT_HD inline TubeState tube_state_load(const int32_t* si, const double* sf, int64_t nray, int64_t j) {
  TubeState s;
  s.flags = si[j];
  s.mu = si[nray + j];
  s.first = si[2 * nray + j];
  s.nrow = si[3 * nray + j];
  s.close_row = si[4 * nray + j];
  s.jac_prev = sf[j];
  s.jac0 = sf[nray + j];
  s.cos0 = sf[2 * nray + j];
  s.dmin = sf[3 * nray + j];
  s.dlast = sf[4 * nray + j];
  for (int k = 0; k < 4; ++k) {
    s.f0[k] = sf[(5 + k) * nray + j];
    s.flast[k] = sf[(9 + k) * nray + j];
  }
  return s;
}

RWRT_HD inline void tube_state_store(const TubeState& s, int32_t* si, double* sf, int64_t nray, int64_t j) {
  si[j] = s.flags;
  si[nray + j] = s.mu;
  si[2 * nray + j] = s.first;
  si[3 * nray + j] = s.nrow;
  si[4 * nray + j] = s.close_row;
  sf[j] = s.jac_prev;
  sf[nray + j] = s.jac0;
  sf[2 * nray + j] = s.cos0;
  sf[3 * nray + j] = s.dmin;
  sf[4 * nray + j] = s.dlast;
  for (int k = 0; k < 4; ++k) {
    sf[(5 + k) * nray + j] = s.f0[k];
    sf[(9 + k) * nray + j] = s.flast[k];
  }
}

// Row i (it_begin <= i < it_end) of ray p, whose span is s: in its block
// before its tail, its tail row from there on (tf == it_end without tails).
RWRT_HD inline const double* tube_row_ptr(const LaunchRows& L, const LaunchRowsSpan& s, int64_t p, int32_t i) {
  return i < s.tf ? s.block + (int64_t)(i - L.it_begin) * RWRT_NOUT : L.tail_row + p * RWRT_NOUT;
}

// The four stencil rays p_a q_a p_b q_b of ray j (j itself on the short side
// of a one-sided pair) and their spans, resolved once per launch.
struct TubeStencil {
  int64_t ray[4];
  LaunchRowsSpan span[4];
  bool ok;   // every ray in [0, nray)
};

RWRT_HD inline TubeStencil tube_stencil(const LaunchRows& L, int64_t j, int64_t nray, const int32_t* nbr,
                                        int32_t flags) {
  TubeStencil st;
  st.ok = true;
  for (int d = 0; d < 2; ++d) {
    const int32_t code = (flags >> (2 * d)) & 3;   // 1 (lo, hi), 2 (j, hi), 3 (lo, j)
    st.ray[2 * d] = (code == 1 || code == 3) ? (int64_t)nbr[(2 * d) * nray + j] : j;
    st.ray[2 * d + 1] = (code == 1 || code == 2) ? (int64_t)nbr[(2 * d + 1) * nray + j] : j;
  }
  for (int k = 0; k < 4; ++k) {
    if (st.ray[k] < 0 || st.ray[k] >= nray) {
      st.ok = false;
      st.ray[k] = j;
    }
    st.span[k] = launch_rows_span(L, st.ray[k]);
  }
  return st;
}

// Row 0 (the launch's first row, it_begin == 0): the stencil of ray j from the
// validity of j and of its four neighbours there, and the per-ray results
// started over.
template <class E>
RWRT_HD inline void tube_fix(const LaunchRows& L, int64_t j, int64_t nray, const int32_t* nbr, const rwrt_tube_map& m,
                             const TubePoint& own, TubeState& s, E& e) {
  bool v[4];
  for (int k = 0; k < 4; ++k) {
    const int64_t p = nbr[k * nray + j];
    v[k] = false;
    if (p < -1 || p >= nray) {
      e.bad_index();
    } else if (p >= 0) {
      v[k] = tube_valid(tube_load(tube_row_ptr(L, launch_rows_span(L, p), p, 0), m));
    }
  }
  const int32_t a = (v[0] && v[1]) ? 1 : (v[1] ? 2 : (v[0] ? 3 : 0));
  const int32_t b = (v[2] && v[3]) ? 1 : (v[3] ? 2 : (v[2] ? 3 : 0));
  s.flags = (tube_valid(own) && a && b) ? (a | (b << 2) | kTubeOpen) : 0;
  s.mu = 0;
  s.first = -1;
  s.nrow = 0;
  s.close_row = -1;
  s.jac_prev = s.jac0 = s.cos0 = s.dmin = s.dlast = NAN;
  for (int k = 0; k < 4; ++k) s.f0[k] = s.flast[k] = NAN;
}

struct TubeRowOut {   // what a constant tail repeats
  bool open, zero;
  int32_t bin;
  double logd;
};

// Row i of an open tube: `own` ray j's point, P the stencil rays' points.
template <class E>
RWRT_HD inline TubeRowOut tube_row(TubeState& s, int32_t i, const TubePoint& own, const TubePoint* P,
                                   const rwrt_tube_map& m, const rwrt_density_map& bins, int32_t chan, E& e) {
  const double dla = tube_wrap(P[1].lon - P[0].lon), dpa = P[1].lat - P[0].lat;
  const double dlb = tube_wrap(P[3].lon - P[2].lon), dpb = P[3].lat - P[2].lat;
  const double sa = fabs(dla) > fabs(dpa) ? fabs(dla) : fabs(dpa);
  const double sb = fabs(dlb) > fabs(dpb) ? fabs(dlb) : fabs(dpb);
  const bool open = tube_valid(own) && tube_valid(P[0]) && tube_valid(P[1]) && tube_valid(P[2]) && tube_valid(P[3]) &&
                    (sa > sb ? sa : sb) <= m.max_sep;
  if (!open) {
    s.flags &= ~kTubeOpen;
    s.close_row = i;
    return {false, false, -1, 0.0};
  }
  const double jac = dla * dpb - dlb * dpa;
  const double c = cos(own.lat);
  bool caustic = false;
  if (i == 0) {
    if (jac == 0.0) {   // no tube
      s.flags = 0;
      return {false, false, -1, 0.0};
    }
    s.jac0 = jac;
    s.cos0 = c;
  } else if ((jac < 0.0) != (s.jac_prev < 0.0)) {
    caustic = true;
    s.mu += 1;
    if (s.first < 0) s.first = i;
  }
  s.jac_prev = jac;
  const double D = (jac * c) / (s.jac0 * s.cos0);
  const double aD = fabs(D);
  s.nrow += 1;
  if (!(s.dmin <= aD)) s.dmin = aD;   // (NaN: none yet)
  s.dlast = D;
  s.flast[0] = dla * c;
  s.flast[1] = dpa;
  s.flast[2] = dlb * c;
  s.flast[3] = dpb;
  if (i == 0) {
    for (int k = 0; k < 4; ++k) s.f0[k] = s.flast[k];
  }
  const int32_t bin = density_bin(density_wrap_2pi(own.lon), own.lat, 1.0, chan, bins);
  if (bin < 0) return {true, false, -1, 0.0};
  if (caustic) e.caustic(bin);
  if (jac == 0.0) {
    e.drop(1);
    return {true, true, bin, 0.0};
  }
  const double logd = log(aD);
  e.add(bin, 1, logd);
  return {true, false, bin, logd};
}

// n more rows equal to the row that gave r (a constant tail of the ray and of
// its whole stencil): the same jac, so no caustic, and one product for slog.
template <class E>
RWRT_HD inline void tube_repeat(TubeState& s, int32_t n, const TubeRowOut& r, E& e) {
  if (n <= 0 || !r.open) return;
  s.nrow += n;
  if (r.bin < 0) return;
  if (r.zero) {
    e.drop(n);
  } else {
    e.add(r.bin, n, (double)n * r.logd);
  }
}

// Ray j of the launch L over all nray rays, its state in `s` on entry and on
// return: BATCH of its own rows loaded ahead, the stencil rays' rows gathered
// per row.  A launch that starts at row 0 fixes the stencil.
template <int BATCH, class E>
RWRT_HD inline void tube_ray(const LaunchRows& L, int64_t j, int64_t nray, const int32_t* nbr, const rwrt_tube_map& m,
                             const rwrt_density_map& bins, int32_t chan, TubeState& s, E& e) {
  if (L.it_begin == 0) {
    const TubePoint own = tube_load(tube_row_ptr(L, launch_rows_span(L, j), j, 0), m);
    tube_fix(L, j, nray, nbr, m, own, s, e);
  }
  if (!(s.flags & kTubeOpen)) return;
  const TubeStencil st = tube_stencil(L, j, nray, nbr, s.flags);
  if (!st.ok) {   // (a neighbour array changed under a run: never followed)
    e.bad_index();
    s.flags &= ~kTubeOpen;
    s.close_row = L.it_begin;
    return;
  }
  auto at = [&](int32_t i, const TubePoint& own) {
    TubePoint P[4];
    for (int k = 0; k < 4; ++k)
      P[k] = st.ray[k] == j ? own : tube_load(tube_row_ptr(L, st.span[k], st.ray[k], i), m);
    return tube_row(s, i, own, P, m, bins, chan, e);
  };
  launch_rows_walk<BATCH, TubePoint>(
      L, j, [&](const double* r) { return (s.flags & kTubeOpen) ? tube_load(r, m) : TubePoint{0.0, 0.0, 0.0}; },
      [&](int32_t i, const TubePoint& v) {
        if (s.flags & kTubeOpen) at(i, v);
      },
      [&](int32_t i, int32_t n, const TubePoint& v) {
        // rows [i, T) while a stencil ray still moves, then row T and the rest as one
        int32_t T = i;
        for (int k = 0; k < 4; ++k) T = st.span[k].tf > T ? st.span[k].tf : T;
        for (int32_t r = i; r < T && (s.flags & kTubeOpen); ++r) at(r, v);
        if (T < L.it_end && (s.flags & kTubeOpen)) {
          const TubeRowOut out = at(T, v);
          tube_repeat(s, L.it_end - T - 1, out, e);
        }
      });
}

}  // namespace rwrt

#endif  // RWRT_TUBE_ROWS_H
