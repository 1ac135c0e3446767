// tube.hip -- rwrt_ray_tube (ABI 5, additive): the ray tube spanned by every
// ray's neighbours in the source lattice -- its cross-section relative to the
// sources' (the geometric spreading D), its sign changes (caustics, the Maslov
// index) -- reduced on the device from the row blocks and constant tails a
// ray-loop call has left.
//
// A translation unit of its own, linked into librwrt.so next to the others, so
// that no other code object is touched by it.  It uses the device library's
// cos and log, not the ray loops' np_math.h.
//
// One lane walks one ray's rows of the call in order (csrc/tube_rows.h) and
// gathers its stencil rays' (lon, lat) and need column per row: up to four
// 16-byte and four 8-byte loads.  Lanes adjacent in ray index are adjacent in
// zwn and share their sources, and the W/E neighbours lie nzwn rays away, so a
// wave's gathers at one row fall into the row blocks of rays the wave, or the
// one next to it, walks itself.  A tube that has closed costs its ray one
// 4-byte load per launch.  The ray's state is loaded from its column before
// the first row and stored after the last: plain loads and stores, and no lane
// reads another's state.  The emitter turns a deposit into one 64-bit integer
// add and one hardware fp64 add (no compare-exchange loop); the drops and a
// bad neighbour index are kept in registers and added once per ray.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "abi_host.h"
#include "map_host.h"
#include "tube_rows.h"

namespace rwrt {
namespace {

struct TubeAtomics {
  unsigned long long* __restrict__ cnt_;
  double* __restrict__ slog_;
  unsigned long long* __restrict__ ncaus_;
  unsigned long long dropped_ = 0;
  int32_t bad_ = 0;

  __device__ __forceinline__ void drop(int32_t n) { dropped_ += (unsigned long long)n; }
  __device__ __forceinline__ void bad_index() { bad_ = 1; }
  __device__ __forceinline__ void caustic(int32_t bin) { atomicAdd(ncaus_ + bin, 1ULL); }

  __device__ __forceinline__ void add(int32_t bin, int32_t n, double slog) {
    atomicAdd(cnt_ + bin, (unsigned long long)n);
    unsafeAtomicAdd(slog_ + bin, slog);   // (global_atomic_add_f64, no compare-exchange loop)
  }
};

constexpr int kTubeBatch = 2;   // own rows loaded ahead per lane (each row gathers up to four more)

__global__ void __launch_bounds__(256)
ray_tube_kernel(const rwrt_tube_map m, int64_t nray, int32_t it_begin, int32_t it_end,
                const double* __restrict__ rows, const int32_t* __restrict__ row_slot,
                const int32_t* __restrict__ tail_from, const double* __restrict__ tail_row,
                const int32_t* __restrict__ chan, const int32_t* __restrict__ nbr, int32_t* __restrict__ state_i,
                double* __restrict__ state_f, unsigned long long* __restrict__ cnt, double* __restrict__ slog,
                unsigned long long* __restrict__ ncaus, unsigned long long* __restrict__ dropped,
                int32_t* __restrict__ err) {
  const LaunchRows L{rows, row_slot, tail_from, tail_row, it_begin, it_end};
  const rwrt_density_map bins = tube_bins(m);
  TubeAtomics e{cnt, slog, ncaus};
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nray; j += (int64_t)gridDim.x * blockDim.x) {
    const int32_t ch = chan ? chan[j] : 0;
    if (ch < 0 || ch >= m.nchan) continue;                        // (not walked: its columns stay)
    if (it_begin != 0 && !(state_i[j] & kTubeOpen)) continue;     // closed, or no tube
    TubeState s = tube_state_load(state_i, state_f, nray, j);
    tube_ray<kTubeBatch>(L, j, nray, nbr, m, bins, ch, s, e);
    tube_state_store(s, state_i, state_f, nray, j);
    if (e.dropped_) atomicAdd(dropped, e.dropped_);
    if (e.bad_) atomicOr(err, 1);
    e.dropped_ = 0;
    e.bad_ = 0;
  }
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_ray_tube(const rwrt_tube_map* m, int64_t nray, int32_t it_begin, int32_t it_end,
                                     const double* d_rows, const int32_t* d_row_slot, const int32_t* d_tail_from,
                                     const double* d_tail_row, const int32_t* d_chan, const int32_t* d_nbr,
                                     int32_t* d_state_i, double* d_state_f, int64_t* d_cnt, double* d_slog,
                                     int64_t* d_ncaus, int64_t* d_dropped, int32_t* d_err, void* stream) {
  // (every check before the first HIP call)
  if (!m) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: map is NULL%s", "");
  if (const rwrt_status st = check_map_shape("rwrt_ray_tube", m->nx, m->ny, m->nchan)) return st;
  if (!map_column_ok(m->need)) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: need must be -1 or a column 2..6%s", "");
  if (const rwrt_status st = check_map_axes("rwrt_ray_tube", m->inv_dlon, m->inv_dlat, m->lat0)) return st;
  if (!(m->max_sep > 0.0)) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: max_sep must be positive%s", "");
  if (const rwrt_status st = check_launch_rows("rwrt_ray_tube", nray, it_begin, it_end, d_rows, d_row_slot,
                                               d_tail_from, d_tail_row))
    return st;
  if (it_begin < 0) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: it_begin must not be negative%s", "");
  if (!d_nbr) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: d_nbr is NULL%s", "");
  if (!d_state_i) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: d_state_i is NULL%s", "");
  if (!d_state_f) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: d_state_f is NULL%s", "");
  if (!d_cnt) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: d_cnt is NULL%s", "");
  if (!d_slog) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: d_slog is NULL%s", "");
  if (!d_ncaus) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: d_ncaus is NULL%s", "");
  if (!d_dropped) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: d_dropped is NULL%s", "");
  if (!d_err) return fail(RWRT_ERR_ARG, "rwrt_ray_tube: d_err is NULL%s", "");
  if (nray == 0) return RWRT_OK;
  return launch_per_ray("ray_tube_kernel", ray_tube_kernel, nray, stream, *m, nray, it_begin, it_end, d_rows,
                        d_row_slot, d_tail_from, d_tail_row, d_chan, d_nbr, d_state_i, d_state_f,
                        reinterpret_cast<unsigned long long*>(d_cnt), d_slog,
                        reinterpret_cast<unsigned long long*>(d_ncaus),
                        reinterpret_cast<unsigned long long*>(d_dropped), d_err);
}
