// flux.hip -- rwrt_ray_flux (ABI 5, additive): wave-ray flux maps reduced on
// the device from the row blocks and constant tails a ray-loop call has left:
// per bin the number of accepted ray points, the sum of their row indices and
// the sums of their group-velocity vectors (or unit vectors) and speeds.
//
// A translation unit of its own, linked into librwrt.so next to the others, so
// that no other code object is touched by it.
//
// One lane walks one ray's rows of the call in order (csrc/flux_rows.h: the
// accept rule, the bin, the run kept in registers and summed in row order);
// the emitter here turns a run's end into global atomics: two 64-bit integer
// adds and three hardware fp64 adds, all native (no compare-exchange loop).
// A bin's accumulators are interleaved -- (count, rowsum) in one 16-byte pair,
// (fx, fy, fs) in 24 consecutive bytes -- so that the five atomics of a run go
// to two places of a map that does not fit L2, not to five planes.
//
// Lane pairing: when two neighbouring lanes (lane, lane ^ 1) end a run in the
// same instruction they share the work -- first both add to the even lane's
// bin, then both to the odd lane's -- so that the two lanes of an atomic
// instruction address neighbouring words of one bin instead of two bins (a
// scattered atomic costs one memory request whatever lies next to it; two
// lanes on adjacent words share one: 0.70 x the kernel time).
// Every addend reaches the same address as without it; only the lane that
// issues it changes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "abi_host.h"
#include "flux_rows.h"
#include "map_host.h"

namespace rwrt {
namespace {

struct FluxAtomics {
  unsigned long long* __restrict__ cnt_;
  double* __restrict__ sum_;

  // whether the neighbouring lane (lane ^ 1) ends a run in this very instruction
  static __device__ __forceinline__ bool with_neighbour(unsigned lane) {
    return (__ballot(1) >> (lane ^ 1u)) & 1ull;
  }

  __device__ __forceinline__ void add_cnt(int64_t index, unsigned long long n, long long rowsum) {
    const unsigned lane = __lane_id();
    if (with_neighbour(lane)) {
      // even lane E, odd lane O: first E's pair (E adds E.n, O adds E.rowsum), then O's pair
      const bool odd = lane & 1u;
      const int64_t other = __shfl_xor(index, 1);
      const unsigned long long got = __shfl_xor(odd ? n : (unsigned long long)rowsum, 1);
      atomicAdd(cnt_ + 2 * (odd ? other : index) + odd, odd ? got : n);
      atomicAdd(cnt_ + 2 * (odd ? index : other) + odd, odd ? (unsigned long long)rowsum : got);
      return;
    }
    atomicAdd(cnt_ + 2 * index, n);
    atomicAdd(cnt_ + 2 * index + 1, (unsigned long long)rowsum);   // (two's complement: a signed add)
  }
  __device__ __forceinline__ void add_sum(int64_t index, double fx, double fy, double fs) {
    const unsigned lane = __lane_id();
    if (with_neighbour(lane)) {
      // E.fx E.fy | E.fs O.fx | O.fy O.fs: the first and the last instruction put two lanes on one triple
      const bool odd = lane & 1u;
      const int64_t other = __shfl_xor(index, 1);
      const double got = __shfl_xor(fy, 1);
      unsafeAtomicAdd(sum_ + 3 * (odd ? other : index) + odd, odd ? got : fx);
      unsafeAtomicAdd(sum_ + 3 * index + (odd ? 0 : 2), odd ? fx : fs);
      unsafeAtomicAdd(sum_ + 3 * (odd ? index : other) + 1 + odd, odd ? fs : got);
      return;
    }
    unsafeAtomicAdd(sum_ + 3 * index, fx);   // (global_atomic_add_f64, no compare-exchange loop)
    unsafeAtomicAdd(sum_ + 3 * index + 1, fy);
    unsafeAtomicAdd(sum_ + 3 * index + 2, fs);
  }
};

constexpr int kFluxBatch = 4;   // rows loaded ahead per lane

__global__ void __launch_bounds__(256)
ray_flux_kernel(const rwrt_flux_map m, int64_t nray, int32_t it_begin, int32_t it_end,
                const double* __restrict__ rows, const int32_t* __restrict__ row_slot,
                const int32_t* __restrict__ tail_from, const double* __restrict__ tail_row,
                const int32_t* __restrict__ chan, unsigned long long* __restrict__ cnt, double* __restrict__ sum) {
  const LaunchRows L{rows, row_slot, tail_from, tail_row, it_begin, it_end};
  FluxAtomics e{cnt, sum};
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nray; j += (int64_t)gridDim.x * blockDim.x)
    flux_ray<kFluxBatch>(L, j, chan ? chan[j] : 0, m, e);
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_ray_flux(const rwrt_flux_map* m, int64_t nray, int32_t it_begin, int32_t it_end,
                                     const double* d_rows, const int32_t* d_row_slot,
                                     const int32_t* d_tail_from, const double* d_tail_row,
                                     const int32_t* d_chan, int64_t* d_cnt, double* d_sum, void* stream) {
  // (every check before the first HIP call)
  if (!m) return fail(RWRT_ERR_ARG, "rwrt_ray_flux: map is NULL%s", "");
  if (const rwrt_status st = check_map_shape("rwrt_ray_flux", m->nx, m->ny, m->nchan)) return st;
  if (m->mode < 0 || m->mode >= 4)
    return fail(RWRT_ERR_ARG, "rwrt_ray_flux: mode has bits other than 0 (unit vectors) and 1 (unwrapped)%s", "");
  if (const rwrt_status st = check_map_axes("rwrt_ray_flux", m->inv_dlon, m->inv_dlat, m->lat0, m->lon0,
                                            m->mode & kFluxUnwrapped))
    return st;
  if (!(m->s2_min >= 0.0)) return fail(RWRT_ERR_ARG, "rwrt_ray_flux: s2_min must not be NaN or negative%s", "");
  if (!(m->s2_max >= m->s2_min))
    return fail(RWRT_ERR_ARG, "rwrt_ray_flux: s2_max must not be NaN or below s2_min%s", "");
  if (!(m->wn_max >= 0.0)) return fail(RWRT_ERR_ARG, "rwrt_ray_flux: wn_max must not be NaN or negative%s", "");
  if (const rwrt_status st = check_launch_rows("rwrt_ray_flux", nray, it_begin, it_end, d_rows, d_row_slot,
                                               d_tail_from, d_tail_row))
    return st;
  if (!d_cnt) return fail(RWRT_ERR_ARG, "rwrt_ray_flux: d_cnt is NULL%s", "");
  if (!d_sum) return fail(RWRT_ERR_ARG, "rwrt_ray_flux: d_sum is NULL%s", "");
  if (nray == 0) return RWRT_OK;
  return launch_per_ray("ray_flux_kernel", ray_flux_kernel, nray, stream, *m, nray, it_begin, it_end, d_rows,
                        d_row_slot, d_tail_from, d_tail_row, d_chan, reinterpret_cast<unsigned long long*>(d_cnt), d_sum);
}
