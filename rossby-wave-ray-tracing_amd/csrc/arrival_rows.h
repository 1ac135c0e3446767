// arrival_rows.h -- one ray's rows of a launch reduced into an arrival-time map
// (rwrt_ray_arrival, include/rwrt.h), shared by the device kernel
// (csrc/arrival.hip, whose emitter issues atomics) and by host programs
// (tests/host/arrival_rows_main.cpp updates plain arrays under the sanitizers).
//
// The definition is arrival.reference_arrival (NumPy): per bin the smallest
// and the largest row index of a counted point, and per window w = row / W the
// number of counted points.  Every output is an integer, so the order of the
// updates does not matter; what this header fixes is how few there are.
//
// The lane keeps the current bin's run: its first row, its last row and the
// points it has inside the current window.
//   bin change      first(bin, first row), last(bin, last row), count(window, bin, n)
//   window change   count(window, bin, n) only -- the run goes on
//   constant tail   one run of it_end - tf rows: one count per window it touches
// so a frozen ray costs O(windows of the launch), not O(rows).
//
// An emitter E has
//   void first(int32_t bin, int32_t row);            // min into first[bin]
//   void last(int32_t bin, int32_t row);             // max into last[bin]
//   void count(int64_t index, unsigned long long n); // add into count[index]
#ifndef RWRT_ARRIVAL_ROWS_H
#define RWRT_ARRIVAL_ROWS_H

#include <cstdint>

#include "rwrt.h"
#include "density_bins.h"
#include "launch_rows.h"

namespace rwrt {

struct ArrivalRow {   // what the lane needs of a row: lon lat, and the required column
  double lon, lat, req;
};

// (16 B for lon lat, 8 B for the column; rows are 16-byte aligned on the device)
RWRT_HD inline ArrivalRow arrival_load(const double* r, int col) {
#if defined(__HIPCC__)
  const double2 p = *reinterpret_cast<const double2*>(r);
  return {p.x, p.y, r[col]};
#else
  return {r[0], r[1], r[col]};
#endif
}

struct ArrivalRun {
  int32_t bin = -1;            // -1: no run
  int32_t first = 0, last = 0;
  unsigned long long n = 0;    // points of the run inside window `win`
  int32_t win = 0;             // the window of the next row
  int32_t left = 0;            // rows of that window still to come, the next row included
};

// The walk starts at row it_begin.  window_rows 0: one window that never ends
// (a launch has fewer than 2^31 rows) and no counts.
RWRT_HD inline ArrivalRun arrival_begin(const rwrt_arrival_map& m, int32_t it_begin) {
  ArrivalRun r;
  const int32_t W = m.window_rows;
  r.win = W > 0 ? it_begin / W : 0;
  r.left = W > 0 ? W - it_begin % W : 0x7fffffff;
  return r;
}

// flat index into count[nwin][nchan][ny][nx], in 64 bits
RWRT_HD inline int64_t arrival_count_index(const rwrt_arrival_map& m, int32_t win, int32_t bin) {
  return (int64_t)win * ((int64_t)m.bins.nchan * m.bins.ny * m.bins.nx) + bin;
}

template <class E>
RWRT_HD inline void arrival_flush_count(ArrivalRun& r, const rwrt_arrival_map& m, E& e) {
  if (m.window_rows > 0 && r.bin >= 0 && r.n > 0) e.count(arrival_count_index(m, r.win, r.bin), r.n);
  r.n = 0;
}

// the run ends: count first, then the two bounds
template <class E>
RWRT_HD inline void arrival_flush(ArrivalRun& r, const rwrt_arrival_map& m, E& e) {
  arrival_flush_count(r, m, e);
  if (r.bin >= 0) {
    e.first(r.bin, r.first);
    e.last(r.bin, r.last);
  }
  r.bin = -1;
}

// the next row starts a new window
template <class E>
RWRT_HD inline void arrival_next_window(ArrivalRun& r, const rwrt_arrival_map& m, E& e) {
  arrival_flush_count(r, m, e);
  r.win += 1;
  r.left = m.window_rows;
}

// `rows` >= 1 equal points from row i on, bin b (-1: not counted); rows must be
// fed in order and without a gap from it_begin on
template <class E>
RWRT_HD inline void arrival_points(ArrivalRun& r, const rwrt_arrival_map& m, int32_t i, int32_t rows, int32_t b,
                                   E& e) {
  if (r.left == 0) arrival_next_window(r, m, e);
  if (b != r.bin) {
    arrival_flush(r, m, e);
    r.bin = b;
    r.first = i;
  }
  if (b >= 0) r.last = i + rows - 1;
  // the window split: bounded by the windows [i, i + rows) touches
  for (;;) {
    const int32_t take = rows < r.left ? rows : r.left;
    if (b >= 0) r.n += (unsigned long long)take;
    r.left -= take;
    rows -= take;
    if (rows == 0) break;
    arrival_next_window(r, m, e);
  }
}

// Ray j (channel c) of the launch L: BATCH rows loaded ahead, as the density
// kernel walks them.
template <int BATCH, class E>
RWRT_HD inline void arrival_ray(const LaunchRows& L, int64_t j, int32_t c, const rwrt_arrival_map& m, E& e) {
  if (c < 0 || c >= m.bins.nchan) return;
  const int col = (m.bins.wcol >= 0) ? m.bins.wcol : 0;   // (a column that exists: unused without a requirement)
  ArrivalRun run = arrival_begin(m, L.it_begin);
  launch_rows_walk<BATCH, ArrivalRow>(
      L, j, [col](const double* r) { return arrival_load(r, col); },
      [&](int32_t i, const ArrivalRow& v) {
        arrival_points(run, m, i, 1, density_bin(density_wrap_2pi(v.lon), v.lat, v.req, c, m.bins), e);
      },
      [&](int32_t tf, int32_t n, const ArrivalRow& v) {
        arrival_points(run, m, tf, n, density_bin(density_wrap_2pi(v.lon), v.lat, v.req, c, m.bins), e);
      });
  arrival_flush(run, m, e);
}

}  // namespace rwrt

#endif  // RWRT_ARRIVAL_ROWS_H
