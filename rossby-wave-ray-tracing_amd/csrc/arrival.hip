// arrival.hip -- rwrt_ray_arrival (ABI 5, additive): arrival-time maps reduced
// on the device from the row blocks and constant tails a ray-loop call has
// left: per bin the first and the last row with a ray point in it, and per
// time window the number of points.
//
// A translation unit of its own, linked into librwrt.so next to the others, so
// that no other code object is touched by it.
//
// One lane walks one ray's rows of the call in order (csrc/arrival_rows.h: the
// run kept in registers, the window split of a tail, the flush order); the
// emitter here turns a run's end into global atomics: a 32-bit integer min, a
// 32-bit integer max and a 64-bit integer add, all native (no compare-exchange
// loop).
//
// RWRT_ARRIVAL_SKIP (0 / 1): first[] only ever decreases and last[] only ever
// increases, so a relaxed agent-scope load that already shows a value at least
// as good lets the lane leave the atomic out; a stale value costs an atomic
// that was not needed and never loses one.  The results are identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "abi_host.h"
#include "arrival_rows.h"
#include "map_host.h"

#ifndef RWRT_ARRIVAL_SKIP
#define RWRT_ARRIVAL_SKIP 1
#endif

namespace rwrt {
namespace {

struct ArrivalAtomics {
  int32_t* __restrict__ first_;
  int32_t* __restrict__ last_;
  unsigned long long* __restrict__ count_;

  __device__ __forceinline__ void first(int32_t bin, int32_t row) {
#if RWRT_ARRIVAL_SKIP
    if (__hip_atomic_load(first_ + bin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= row) return;
#endif
    atomicMin(first_ + bin, row);
  }
  __device__ __forceinline__ void last(int32_t bin, int32_t row) {
#if RWRT_ARRIVAL_SKIP
    if (__hip_atomic_load(last_ + bin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= row) return;
#endif
    atomicMax(last_ + bin, row);
  }
  __device__ __forceinline__ void count(int64_t index, unsigned long long n) { atomicAdd(count_ + index, n); }
};

constexpr int kArrivalBatch = 4;   // rows loaded ahead per lane

__global__ void __launch_bounds__(256)
ray_arrival_kernel(const rwrt_arrival_map m, int64_t nray, int32_t it_begin, int32_t it_end,
                   const double* __restrict__ rows, const int32_t* __restrict__ row_slot,
                   const int32_t* __restrict__ tail_from, const double* __restrict__ tail_row,
                   const int32_t* __restrict__ chan, int32_t* __restrict__ first, int32_t* __restrict__ last,
                   unsigned long long* __restrict__ count) {
  const LaunchRows L{rows, row_slot, tail_from, tail_row, it_begin, it_end};
  ArrivalAtomics e{first, last, count};
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nray; j += (int64_t)gridDim.x * blockDim.x)
    arrival_ray<kArrivalBatch>(L, j, chan ? chan[j] : 0, m, e);
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_ray_arrival(const rwrt_arrival_map* m, int64_t nray, int32_t it_begin, int32_t it_end,
                                        const double* d_rows, const int32_t* d_row_slot,
                                        const int32_t* d_tail_from, const double* d_tail_row,
                                        const int32_t* d_chan, int32_t* d_first, int32_t* d_last,
                                        int64_t* d_count, void* stream) {
  // (every check before the first HIP call)
  if (!m) return fail(RWRT_ERR_ARG, "rwrt_ray_arrival: map is NULL%s", "");
  const rwrt_density_map& b = m->bins;
  if (const rwrt_status st = check_map_shape("rwrt_ray_arrival", b.nx, b.ny, b.nchan)) return st;
  if (!map_column_ok(b.wcol))
    return fail(RWRT_ERR_ARG, "rwrt_ray_arrival: wcol must be -1 or 2..6 (k l amp ug vg)%s", "");
  if (const rwrt_status st = check_map_axes("rwrt_ray_arrival", b.inv_dlon, b.inv_dlat, b.lat0)) return st;
  if (const rwrt_status st = check_launch_rows("rwrt_ray_arrival", nray, it_begin, it_end, d_rows, d_row_slot,
                                               d_tail_from, d_tail_row))
    return st;
  // (a negative row index would stand for "none" in d_last and index in front of d_count)
  if (it_begin < 0) return fail(RWRT_ERR_ARG, "rwrt_ray_arrival: it_begin must not be negative%s", "");
  if (!d_first) return fail(RWRT_ERR_ARG, "rwrt_ray_arrival: d_first is NULL%s", "");
  if (!d_last) return fail(RWRT_ERR_ARG, "rwrt_ray_arrival: d_last is NULL%s", "");
  if (m->window_rows < 0) return fail(RWRT_ERR_ARG, "rwrt_ray_arrival: window_rows must not be negative%s", "");
  if (m->window_rows > 0) {
    if (!d_count) return fail(RWRT_ERR_ARG, "rwrt_ray_arrival: window_rows > 0 needs d_count%s", "");
    if (m->nwin <= 0) return fail(RWRT_ERR_ARG, "rwrt_ray_arrival: window_rows > 0 needs nwin > 0%s", "");
    // (the product of three factors each below 2^31 and a fourth: divide, do not multiply)
    if ((int64_t)m->nwin > ((1LL << 31) - 1) / ((int64_t)b.nx * b.ny * b.nchan))
      return fail(RWRT_ERR_ARG, "rwrt_ray_arrival: nwin*nchan*ny*nx must be below 2^31%s", "");
    if ((int64_t)it_end > (int64_t)m->nwin * m->window_rows)
      return fail(RWRT_ERR_ARG, "rwrt_ray_arrival: it_end is past nwin*window_rows, the last row of d_count%s", "");
  }
  if (nray == 0) return RWRT_OK;
  return launch_per_ray("ray_arrival_kernel", ray_arrival_kernel, nray, stream, *m, nray, it_begin, it_end, d_rows,
                        d_row_slot, d_tail_from, d_tail_row, d_chan, d_first, d_last,
                        reinterpret_cast<unsigned long long*>(d_count));
}
