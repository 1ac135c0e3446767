// track_cells.h -- one ray's rows of a launch deposited along their segments
// into a residence-time map (rwrt_ray_track, include/rwrt.h), shared by the
// device kernel (csrc/track.hip, whose emitter issues atomics) and by host
// programs (tests/host/track_cells_main.cpp updates plain arrays under the
// sanitizers).
//
// The definition is track.reference_track (Python); this restates its walk
// operation for operation -- differences, products and quotients rounded one
// by one, IEEE division, no fused multiply-add (build with -ffp-contract=off)
// -- so that every `tx <= ty` decision, and with it every cell sequence, equals
// the definition's.
//
// A wrong cell is an out-of-bounds atomic and an unbounded segment is a lane
// that never ends, so the order is part of the specification: finite rows ->
// floors compared with 2^30 and the cell count compared with max_cells, both
// in fp64 -> conversion to integers -> the walk, at most max_cells cells.
//
// A ray ends each segment in the cell in which it starts the next, so the lane
// keeps the current cell's run (visits, sum of weights, sum of weighted
// values) in registers across segments and emits it only when the cell
// changes: a ray at rest costs nothing per row, a crossed cell one emit.
//   constant tail of n rows   the segment into the tail row is walked, the
//                             n - 1 segments of length zero are one update of
//                             the run: n - 1, (double)(n - 1), 0.5 (v + v) (n - 1)
//
// An emitter E has
//   void add(int64_t index, unsigned long long n, double w, double wv);
// with `index` the cell (c * ny + iy) * nx + col.
#ifndef RWRT_TRACK_CELLS_H
#define RWRT_TRACK_CELLS_H

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "density_bins.h"   // RWRT_HD
#include "launch_rows.h"

namespace rwrt {

constexpr int32_t kTrackUnwrapped = 2;      // rwrt_track_map.mode bit 1
constexpr double kTrackMaxFloor = 1073741824.0;   // 2^30

struct TrackRow {   // what the lane needs of a row
  double lon, lat, need, v;
};

// lon lat in one 16-byte load on the device (rows are 16-byte aligned there);
// the two named columns (0.0 for none: finite)
RWRT_HD inline TrackRow track_load(const double* r, const rwrt_track_map& m) {
#if defined(__HIPCC__)
  const double2 p = *reinterpret_cast<const double2*>(r);
  return {p.x, p.y, m.need >= 0 ? r[m.need] : 0.0, m.wcol >= 0 ? r[m.wcol] : 0.0};
#else
  return {r[0], r[1], m.need >= 0 ? r[m.need] : 0.0, m.wcol >= 0 ? r[m.wcol] : 0.0};
#endif
}

RWRT_HD inline bool track_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

RWRT_HD inline bool track_valid(const TrackRow& v) {
  return track_finite(v.lon) && track_finite(v.lat) && track_finite(v.need) && track_finite(v.v);
}

// The lane's state: the carried previous row (lon NaN: none), the run of the
// current cell and the dropped segments.
struct TrackState {
  double lon, lat, v;          // the previous row as it is carried from call to call
  int32_t bin = -1;            // -1: no run
  unsigned long long n = 0;
  double w = 0.0, wv = 0.0;
  unsigned long long dropped = 0;
};

template <class E>
RWRT_HD inline void track_flush(TrackState& s, E& e) {
  if (s.bin >= 0) e.add((int64_t)s.bin, s.n, s.w, s.wv);
  s.bin = -1;
}

// `n` visits of the cell `bin` (-1: outside the map) with weights summing to w
template <class E>
RWRT_HD inline void track_emit(TrackState& s, int32_t bin, unsigned long long n, double w, double wv, E& e) {
  if (bin != s.bin) {
    track_flush(s, e);
    s.bin = bin;
    s.n = 0;
    s.w = s.wv = 0.0;
  }
  if (bin < 0) return;
  s.n += n;
  s.w = s.w + w;
  s.wv = s.wv + wv;
}

// the column of cell ix: ix mod nx (Python's %) on the wrapped axis
RWRT_HD inline int32_t track_column(int32_t ix, const rwrt_track_map& m) {
  if (m.mode & kTrackUnwrapped) return ix;
  const int32_t r = ix % m.nx;
  return r < 0 ? r + m.nx : r;
}

// the cell (col, iy) of channel c, -1 outside the map
RWRT_HD inline int32_t track_bin(int32_t col, int32_t iy, int32_t c, const rwrt_track_map& m) {
  if (!(iy >= 0 && iy < m.ny && col >= 0 && col < m.nx)) return -1;
  return (c * m.ny + iy) * m.nx + col;
}

RWRT_HD inline bool track_floors_ok(double fx, double fy) {
  return fabs(fx) <= kTrackMaxFloor && fabs(fy) <= kTrackMaxFloor;   // (false for NaN and inf)
}

// The segment (X0, Y0) -> (X1, Y1) of a ray with channel c, weight values v0, v1.
template <class E>
RWRT_HD inline void track_segment(TrackState& s, double X0, double Y0, double v0, double X1, double Y1, double v1,
                                  int32_t c, const rwrt_track_map& m, E& e) {
  const double fx0 = floor(X0), fy0 = floor(Y0), fx1 = floor(X1), fy1 = floor(Y1);
  if (!track_floors_ok(fx0, fy0) || !track_floors_ok(fx1, fy1)) {
    ++s.dropped;
    return;
  }
  const double dcx = fabs(fx1 - fx0), dcy = fabs(fy1 - fy0);
  if (dcx + dcy + 1.0 > (double)m.max_cells) {   // (in fp64: the counts are below 2^31 past this line)
    ++s.dropped;
    return;
  }
  int32_t ncx = (int32_t)dcx, ncy = (int32_t)dcy;
  int32_t iy = (int32_t)fy0;
  int32_t col = track_column((int32_t)fx0, m);
  const double vm = 0.5 * (v0 + v1);
  if ((ncx | ncy) == 0) {   // inside one cell: exactly 1.0, nothing divided
    track_emit(s, track_bin(col, iy, c, m), 1ull, 1.0, vm, e);
    return;
  }
  const bool wrapped = !(m.mode & kTrackUnwrapped);
  const double DX = X1 - X0, DY = Y1 - Y0;
  const int32_t sx = fx1 > fx0 ? 1 : -1, sy = fy1 > fy0 ? 1 : -1;
  double gx = sx > 0 ? fx0 + 1.0 : fx0;   // the next lines: integers, exact in fp64
  double gy = sy > 0 ? fy0 + 1.0 : fy0;
  const double inf = HUGE_VAL;
  double tx = ncx > 0 ? (gx - X0) / DX : inf;
  double ty = ncy > 0 ? (gy - Y0) / DY : inf;
  double t = 0.0;
  while ((ncx | ncy) != 0) {   // at most max_cells - 1 times
    const int32_t bin = track_bin(col, iy, c, m);
    if (tx <= ty) {   // (a tie goes to x)
      const double w = tx - t;
      track_emit(s, bin, 1ull, w, w * vm, e);
      t = tx;
      col += sx;
      if (wrapped) col = col == m.nx ? 0 : (col < 0 ? m.nx - 1 : col);
      gx += (double)sx;
      --ncx;
      tx = ncx > 0 ? (gx - X0) / DX : inf;
    } else {
      const double w = ty - t;
      track_emit(s, bin, 1ull, w, w * vm, e);
      t = ty;
      iy += sy;
      gy += (double)sy;
      --ncy;
      ty = ncy > 0 ? (gy - Y0) / DY : inf;
    }
  }
  const double w = 1.0 - t;
  track_emit(s, track_bin(col, iy, c, m), 1ull, w, w * vm, e);
}

// `rows` >= 1 equal rows: the segment from the carried row into the first of
// them, then rows - 1 segments of length zero in one update.
template <class E>
RWRT_HD inline void track_rows(TrackState& s, const TrackRow& r, int32_t rows, int32_t c, const rwrt_track_map& m,
                               E& e) {
  if (!track_valid(r)) {
    s.lon = NAN;   // the segments on both sides vanish
    return;
  }
  const double X1 = (r.lon - m.lon0) * m.inv_dlon, Y1 = (r.lat - m.lat0) * m.inv_dlat;
  if (s.lon == s.lon)   // a valid previous row
    track_segment(s, (s.lon - m.lon0) * m.inv_dlon, (s.lat - m.lat0) * m.inv_dlat, s.v, X1, Y1, r.v, c, m, e);
  s.lon = r.lon;
  s.lat = r.lat;
  s.v = r.v;
  if (rows > 1) {
    const unsigned long long n = (unsigned long long)(rows - 1);
    const double fx = floor(X1), fy = floor(Y1);
    if (!track_floors_ok(fx, fy)) {
      s.dropped += n;
      return;
    }
    const double dn = (double)(rows - 1);
    // (each of the n segments adds 1.0 and 0.5 * (v + v))
    track_emit(s, track_bin(track_column((int32_t)fx, m), (int32_t)fy, c, m), n, dn, (0.5 * (r.v + r.v)) * dn, e);
  }
}

// Ray j (channel c) of the launch L, its carried row in `s` on entry and on
// return: BATCH rows loaded ahead, as the density kernel walks them.  The run
// is flushed before returning.
template <int BATCH, class E>
RWRT_HD inline void track_ray(const LaunchRows& L, int64_t j, int32_t c, const rwrt_track_map& m, TrackState& s,
                              E& e) {
  if (c < 0 || c >= m.nchan) return;   // (no segment of such a ray is considered)
  launch_rows_walk<BATCH, TrackRow>(
      L, j, [&](const double* r) { return track_load(r, m); },
      [&](int32_t, const TrackRow& v) { track_rows(s, v, 1, c, m, e); },
      [&](int32_t, int32_t n, const TrackRow& v) { track_rows(s, v, n, c, m, e); });
  track_flush(s, e);
}

}  // namespace rwrt

#endif  // RWRT_TRACK_CELLS_H
