// wave_rows.h -- one ray's tube and one ray's WKB phase walked together over
// the rows of a launch, and the caustic-aware deposit
//   w |D|^(-1/2) exp(i (theta - omega_dt i - mu pi / 2))
// into a lon-lat map (rwrt_ray_wave, include/rwrt.h).  Shared by the device
// kernel (csrc/wave.hip, whose emitter issues atomics) and by host programs
// (tests/host/wave_rows_main.cpp updates plain arrays under the sanitizers).
//
// The definition is wave.reference_wave (NumPy), a composition of
// tube.reference_tube's per-row quantities and phase.phase_along's; this
// composes the two headers that restate those, tube_rows.h (tube_load,
// tube_fix, tube_stencil, tube_row, tube_repeat) and phase_rows.h (phase_load,
// phase_valid, phase_a, phase_segment, phase_sincos), and states only the
// deposit rule itself -- every operation rounded on its own, no fused
// multiply-add (build with -ffp-contract=off).  tube_row is called with an
// emitter whose deposits are empty: what it leaves in the state (jac in
// jac_prev, D in dlast, mu) and its TubeRowOut (open, jac == 0, the bin by
// position alone) are what the deposit needs, and its log|D| has no use and no
// side effect.
//
// theta runs over every phase-valid row whether the tube is open or not, so a
// lane walks all of its ray's rows; a closed tube costs it no gathers.
//
// An emitter E has
//   void add(int32_t bin, int32_t n, double re, double im, double wabs);
//   void drop(int32_t n);      n deposits with jac == 0, or a psi or w that is not finite
//   void clip(int32_t n);      n deposits with |jac| < d_floor |jac_0|
//   void bad_index();          a neighbour outside [-1, nray)
// with `n` the deposits (rows) the sums stand for.
#ifndef RWRT_WAVE_ROWS_H
#define RWRT_WAVE_ROWS_H

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "phase_rows.h"
#include "tube_rows.h"

namespace rwrt {

constexpr int kWaveNI = RWRT_WAVE_NI, kWaveNF = RWRT_WAVE_NF;

// the two maps the composed headers read their columns and limits from
RWRT_HD inline rwrt_tube_map wave_tube_map(const rwrt_wave_map& m) {
  return {m.nx, m.ny, m.nchan, m.need, m.lat0, m.inv_dlat, m.inv_dlon, m.max_sep};
}

RWRT_HD inline rwrt_phase_map wave_phase_map(const rwrt_wave_map& m) {
  return {m.nx, m.ny, m.nchan, m.need, m.wcol, 0, m.lat0, m.inv_dlat, m.inv_dlon, m.omega_dt};
}

struct WaveMaps {
  rwrt_tube_map tube;
  rwrt_phase_map phase;
  rwrt_density_map bins;   // tube_bins: position only, no weight enters the bin
  double omega_dt, d_floor;
  bool spread;
};

RWRT_HD inline WaveMaps wave_maps(const rwrt_wave_map& m) {
  const rwrt_tube_map t = wave_tube_map(m);
  return {t, wave_phase_map(m), tube_bins(t), m.omega_dt, m.d_floor, m.spread != 0};
}

// The lane's state: both walks'.  Of TubeState only flags, mu, first, nrow,
// close_row, jac_prev, jac0, cos0 and dlast are carried (dmin, f0 and flast
// are the tube product's own and are dead here).
struct WaveState {
  TubeState t;
  PhaseState p;
};

// state_i[kWaveNI][nray], state_f[kWaveNF][nray]: ray j is column j
RWRT_HD inline WaveState wave_state_load(const int32_t* si, const double* sf, int64_t nray, int64_t j) {
  WaveState s;
  s.t.flags = si[j];
  s.t.mu = si[nray + j];
  s.t.first = si[2 * nray + j];
  s.t.nrow = si[3 * nray + j];
  s.t.close_row = si[4 * nray + j];
  s.p.nseg = si[5 * nray + j];
  s.p.lon = sf[j];
  s.p.lat = sf[nray + j];
  s.p.k = sf[2 * nray + j];
  s.p.a = sf[3 * nray + j];
  s.p.theta = sf[4 * nray + j];
  s.t.jac_prev = sf[5 * nray + j];
  s.t.jac0 = sf[6 * nray + j];
  s.t.cos0 = sf[7 * nray + j];
  s.t.dlast = sf[8 * nray + j];
  s.t.dmin = NAN;
  for (int k = 0; k < 4; ++k) s.t.f0[k] = s.t.flast[k] = NAN;
  return s;
}

RWRT_HD inline void wave_state_store(const WaveState& s, int32_t* si, double* sf, int64_t nray, int64_t j) {
  si[j] = s.t.flags;
  si[nray + j] = s.t.mu;
  si[2 * nray + j] = s.t.first;
  si[3 * nray + j] = s.t.nrow;
  si[4 * nray + j] = s.t.close_row;
  si[5 * nray + j] = s.p.nseg;
  sf[j] = s.p.lon;
  sf[nray + j] = s.p.lat;
  sf[2 * nray + j] = s.p.k;
  sf[3 * nray + j] = s.p.a;
  sf[4 * nray + j] = s.p.theta;
  sf[5 * nray + j] = s.t.jac_prev;
  sf[6 * nray + j] = s.t.jac0;
  sf[7 * nray + j] = s.t.cos0;
  sf[8 * nray + j] = s.t.dlast;
}

// tube_row's emitter here: its deposits are empty, a bad index is E's
template <class E>
struct WaveTubeEmitter {
  E& e;
  RWRT_HD void add(int32_t, int32_t, double) {}
  RWRT_HD void caustic(int32_t) {}
  RWRT_HD void drop(int32_t) {}
  RWRT_HD void bad_index() { e.bad_index(); }
};

// `n` equal deposits of row i into `bin` >= 0 -- an open, phase-valid row of a
// tube whose jac, jac_0, D and mu the state holds, with the weight column's
// value wv and the phase theta: the definition's steps 1 to 6 in order.  For
// n > 1 one product (double)n * term per sum.
template <class E>
RWRT_HD inline void wave_deposit(const TubeState& t, int32_t bin, int32_t i, double theta, double wv, int32_t n,
                                 const WaveMaps& m, E& e) {
  const double jac = t.jac_prev;   // (tube_row leaves the row's jac there)
  if (jac == 0.0) {
    e.drop(n);
    return;
  }
  if (fabs(jac) < m.d_floor * fabs(t.jac0)) {
    e.clip(n);
    return;
  }
  double w = wv;
  if (m.spread) w = wv / sqrt(fabs(t.dlast));
  const double psi = (theta - m.omega_dt * (double)i) - (double)t.mu * kTubeHalfPi;
  if (!phase_finite(psi) || !phase_finite(w)) {
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

// The phase's part of row i: the segment from the carried row into r, and the
// carry.  Returns whether the row is phase-valid (phase_row without its deposit).
RWRT_HD inline bool wave_phase_step(PhaseState& p, const PhaseRow& r) {
  if (!phase_valid(r)) {
    p.lon = NAN;   // the segments on both sides vanish
    return false;
  }
  const double a = phase_a(r.l, r.lat);
  if (p.lon == p.lon) {   // a valid previous row
    p.theta = p.theta + phase_segment(p.lon, p.lat, p.k, p.a, r.lon, r.lat, r.k, a);
    p.nseg += 1;
  }
  p.lon = r.lon;
  p.lat = r.lat;
  p.k = r.k;
  p.a = a;
  return true;
}

struct WaveRowOut {   // what a constant tail repeats
  bool valid;         // phase-valid
  TubeRowOut tube;    // (open false: the tube was closed before the row or by it)
};

// What a launch begins with for ray j: a launch that starts at row 0 has no
// previous row and fixes the stencil; then the stencil rays and their spans,
// resolved once per launch while the tube is open.
template <class E>
RWRT_HD inline TubeStencil wave_begin(const LaunchRows& L, int64_t j, int64_t nray, const int32_t* nbr,
                                      const WaveMaps& m, WaveState& s, E& e) {
  WaveTubeEmitter<E> te{e};
  if (L.it_begin == 0) {
    s.p.lon = NAN;
    const TubePoint own = tube_load(tube_row_ptr(L, launch_rows_span(L, j), j, 0), m.tube);
    tube_fix(L, j, nray, nbr, m.tube, own, s.t, te);
  }
  TubeStencil st = {};
  if (s.t.flags & kTubeOpen) {
    st = tube_stencil(L, j, nray, nbr, s.t.flags);
    if (!st.ok) {   // (a neighbour array changed under a run: never followed)
      e.bad_index();
      s.t.flags &= ~kTubeOpen;
      s.t.close_row = L.it_begin;
    }
  }
  return st;
}

// Row i of ray j, r its own row: the phase's step, then, while the tube is
// open, the stencil rays' points gathered, the tube's row and the deposit.
template <class E>
RWRT_HD inline WaveRowOut wave_row(WaveState& s, const LaunchRows& L, const TubeStencil& st, int64_t j, int32_t i,
                                   const PhaseRow& r, const WaveMaps& m, int32_t chan, E& e) {
  WaveRowOut out = {wave_phase_step(s.p, r), {false, false, -1, 0.0}};
  if (!(s.t.flags & kTubeOpen)) return out;
  WaveTubeEmitter<E> te{e};
  const TubePoint own = {r.lon, r.lat, r.need};
  TubePoint P[4];
  for (int k = 0; k < 4; ++k)
    P[k] = st.ray[k] == j ? own : tube_load(tube_row_ptr(L, st.span[k], st.ray[k], i), m.tube);
  out.tube = tube_row(s.t, i, own, P, m.tube, m.bins, chan, te);
  if (out.valid && out.tube.open && out.tube.bin >= 0) wave_deposit(s.t, out.tube.bin, i, s.p.theta, r.w, 1, m, e);
  return out;
}

// Ray j of the launch L over all nray rays, its state in `s` on entry and on
// return: BATCH of its own rows loaded ahead, the stencil rays' rows gathered
// per row while the tube is open.
template <int BATCH, class E>
RWRT_HD inline void wave_ray(const LaunchRows& L, int64_t j, int64_t nray, const int32_t* nbr, const WaveMaps& m,
                             int32_t chan, WaveState& s, E& e) {
  WaveTubeEmitter<E> te{e};
  const TubeStencil st = wave_begin(L, j, nray, nbr, m, s, e);
  auto at = [&](int32_t i, const PhaseRow& r) { return wave_row(s, L, st, j, i, r, m, chan, e); };
  launch_rows_walk<BATCH, PhaseRow>(
      L, j, [&](const double* r) { return phase_load(r, m.phase); },
      [&](int32_t i, const PhaseRow& v) { at(i, v); },
      [&](int32_t i, int32_t, const PhaseRow& v) {
        // rows [i, T) while the tube is open and a stencil ray still moves: ordinary rows, in which the
        // own row joins itself; then row r, and the n rows after it, all equal to it, as one
        int32_t T = i;
        if (s.t.flags & kTubeOpen) {
          for (int k = 0; k < 4; ++k) T = st.span[k].tf > T ? st.span[k].tf : T;
        }
        int32_t r = i;
        for (; r < T && (s.t.flags & kTubeOpen); ++r) at(r, v);
        if (r >= L.it_end) return;
        const WaveRowOut out = at(r, v);
        const int32_t n = L.it_end - r - 1;
        if (n <= 0) return;
        tube_repeat(s.t, n, out.tube, te);   // (nrow; a tube stays open over rows that only the phase rejects)
        if (!out.valid) return;
        s.p.theta = s.p.theta + phase_segment(s.p.lon, s.p.lat, s.p.k, s.p.a, s.p.lon, s.p.lat, s.p.k, s.p.a);
        s.p.nseg += n;
        if (!out.tube.open || out.tube.bin < 0) return;
        if (m.omega_dt == 0.0 || out.tube.zero) {
          wave_deposit(s.t, out.tube.bin, r, s.p.theta, v.w, n, m, e);
        } else {
          for (int32_t q = 1; q <= n; ++q) wave_deposit(s.t, out.tube.bin, r + q, s.p.theta, v.w, 1, m, e);
        }
      });
}

}  // namespace rwrt

#endif  // RWRT_WAVE_ROWS_H
