// track.hip -- rwrt_ray_track (ABI 5, additive): residence-time maps along ray
// segments, reduced on the device from the row blocks and constant tails a
// ray-loop call has left: the straight segment between two consecutive valid
// rows of a ray is deposited into every map box it passes through, each box
// receiving the fraction of the segment inside it.
//
// A translation unit of its own, linked into librwrt.so next to the others, so
// that no other code object is touched by it.
//
// One lane walks one ray's rows of the call in order (csrc/track_cells.h: the
// drop rule that bounds the lane's loop, the walk with IEEE divisions, the run
// of the current cell kept in registers across segments).  The ray's carried
// previous row is loaded from its column of d_prev before the first row and
// stored after the last -- neighbouring lanes, neighbouring columns.  The
// emitter here turns a run's end into global atomics: one 64-bit integer add
// and one or two hardware fp64 adds, all native (no compare-exchange loop).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "abi_host.h"
#include "map_host.h"
#include "track_cells.h"

// -DRWRT_TRACK_COUNT_FLUSHES=1 (make variant NAME=trackcount DEFS=...): an A/B
// build for tools/track_rate.py in which d_dropped receives the number of
// flushes (calls of add) instead of the dropped segments.
#ifndef RWRT_TRACK_COUNT_FLUSHES
#define RWRT_TRACK_COUNT_FLUSHES 0
#endif

namespace rwrt {
namespace {

struct TrackAtomics {
  unsigned long long* __restrict__ cnt_;
  double* __restrict__ time_;
  double* __restrict__ wsum_;   // NULL without a weight

#if RWRT_TRACK_COUNT_FLUSHES
  unsigned long long flushes_ = 0;
#endif

  __device__ __forceinline__ void add(int64_t index, unsigned long long n, double w, double wv) {
#if RWRT_TRACK_COUNT_FLUSHES
    ++flushes_;
#endif
    atomicAdd(cnt_ + index, n);
    unsafeAtomicAdd(time_ + index, w);   // (global_atomic_add_f64, no compare-exchange loop)
    if (wsum_) unsafeAtomicAdd(wsum_ + index, wv);
  }
};

constexpr int kTrackBatch = 4;   // rows loaded ahead per lane

__global__ void __launch_bounds__(256)
ray_track_kernel(const rwrt_track_map m, int64_t nray, int32_t it_begin, int32_t it_end,
                 const double* __restrict__ rows, const int32_t* __restrict__ row_slot,
                 const int32_t* __restrict__ tail_from, const double* __restrict__ tail_row,
                 const int64_t* __restrict__ ray, int64_t ncol, const int32_t* __restrict__ chan,
                 double* __restrict__ prev, unsigned long long* __restrict__ cnt, double* __restrict__ time,
                 double* __restrict__ wsum, unsigned long long* __restrict__ dropped) {
  const LaunchRows L{rows, row_slot, tail_from, tail_row, it_begin, it_end};
  TrackAtomics e{cnt, time, wsum};
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nray; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = ray ? ray[j] : j;
    if (c < 0 || c >= ncol) continue;
    const int32_t ch = chan ? chan[c] : 0;
    if (ch < 0 || ch >= m.nchan) continue;
    TrackState s;
    s.lon = prev[c];
    s.lat = prev[ncol + c];
    s.v = prev[2 * ncol + c];
    track_ray<kTrackBatch>(L, j, ch, m, s, e);
    prev[c] = s.lon;
    prev[ncol + c] = s.lat;
    prev[2 * ncol + c] = s.v;
#if RWRT_TRACK_COUNT_FLUSHES
    if (e.flushes_) atomicAdd(dropped, e.flushes_);
    e.flushes_ = 0;
#else
    if (s.dropped) atomicAdd(dropped, s.dropped);
#endif
  }
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_ray_track(const rwrt_track_map* m, int64_t nray, int32_t it_begin, int32_t it_end,
                                      const double* d_rows, const int32_t* d_row_slot,
                                      const int32_t* d_tail_from, const double* d_tail_row, const int64_t* d_ray,
                                      int64_t nacc_cols, const int32_t* d_chan, double* d_prev, int64_t* d_cnt,
                                      double* d_time, double* d_wsum, int64_t* d_dropped, void* stream) {
  // (every check before the first HIP call)
  if (!m) return fail(RWRT_ERR_ARG, "rwrt_ray_track: map is NULL%s", "");
  if (const rwrt_status st = check_map_shape("rwrt_ray_track", m->nx, m->ny, m->nchan)) return st;
  if (m->mode != 0 && m->mode != kTrackUnwrapped)
    return fail(RWRT_ERR_ARG, "rwrt_ray_track: mode has bits other than 1 (unwrapped)%s", "");
  if (m->max_cells < 1) return fail(RWRT_ERR_ARG, "rwrt_ray_track: max_cells must be at least 1%s", "");
  if (!map_column_ok(m->need)) return fail(RWRT_ERR_ARG, "rwrt_ray_track: need must be -1 or a column 2..6%s", "");
  if (!map_column_ok(m->wcol)) return fail(RWRT_ERR_ARG, "rwrt_ray_track: wcol must be -1 or a column 2..6%s", "");
  if (const rwrt_status st = check_map_axes("rwrt_ray_track", m->inv_dlon, m->inv_dlat, m->lat0, m->lon0,
                                            m->mode & kTrackUnwrapped))
    return st;
  if (const rwrt_status st = check_launch_rows("rwrt_ray_track", nray, it_begin, it_end, d_rows, d_row_slot,
                                               d_tail_from, d_tail_row))
    return st;
  if (it_begin < 0) return fail(RWRT_ERR_ARG, "rwrt_ray_track: it_begin must not be negative%s", "");
  if (nacc_cols < 0 || nacc_cols > 0x7fffffffLL || (!d_ray && nacc_cols < nray))
    return fail(RWRT_ERR_ARG, "rwrt_ray_track: nacc_cols must cover every ray's column%s", "");
  if (!d_prev) return fail(RWRT_ERR_ARG, "rwrt_ray_track: d_prev is NULL%s", "");
  if (!d_cnt) return fail(RWRT_ERR_ARG, "rwrt_ray_track: d_cnt is NULL%s", "");
  if (!d_time) return fail(RWRT_ERR_ARG, "rwrt_ray_track: d_time is NULL%s", "");
  if (m->wcol >= 0 && !d_wsum) return fail(RWRT_ERR_ARG, "rwrt_ray_track: d_wsum is NULL with a weight column%s", "");
  if (m->wcol < 0 && d_wsum) return fail(RWRT_ERR_ARG, "rwrt_ray_track: d_wsum needs a weight column (wcol)%s", "");
  if (!d_dropped) return fail(RWRT_ERR_ARG, "rwrt_ray_track: d_dropped is NULL%s", "");
  if (nray == 0) return RWRT_OK;
  return launch_per_ray("ray_track_kernel", ray_track_kernel, nray, stream, *m, nray, it_begin, it_end, d_rows,
                        d_row_slot, d_tail_from, d_tail_row, d_ray, nacc_cols, d_chan, d_prev,
                        reinterpret_cast<unsigned long long*>(d_cnt), d_time, d_wsum,
                        reinterpret_cast<unsigned long long*>(d_dropped));
}
