// wave.hip -- rwrt_ray_wave (ABI 5, additive): the caustic-aware WKB wave
// field.  Every ray point of an open tube deposits w |D|^(-1/2) exp(i (theta -
// omega_dt i - mu pi / 2)) into its box of a lon-lat map: the phase of
// rwrt_ray_phase, the geometric spreading D and the running Maslov index mu of
// rwrt_ray_tube, which is known at every row only where both walks share a
// lane.  Reduced on the device from the row blocks and constant tails a
// ray-loop call has left.
//
// A translation unit of its own, linked into librwrt.so next to the others, so
// that no other code object is touched by it.  It uses the device library's
// cos, sincos and sqrt, not the ray loops' np_math.h.
//
// One lane walks one ray's rows of the call in order (csrc/wave_rows.h, which
// composes tube_rows.h and phase_rows.h) and, while its tube is open, gathers
// its stencil rays' (lon, lat) and need column per row as the tube kernel
// does.  A ray whose tube has closed goes on integrating its phase and gathers
// nothing.  The ray's state -- both walks' -- is loaded from its column before
// the first row and stored after the last: plain loads and stores, and no lane
// reads another's state.  The emitter turns a deposit into one 64-bit integer
// add and three hardware fp64 adds (no compare-exchange loop); the drops, the
// clipped deposits and a bad neighbour index are kept in registers and added
// once per ray.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "abi_host.h"
#include "map_host.h"
#include "wave_rows.h"

namespace rwrt {
namespace {

struct WaveAtomics {
  unsigned long long* __restrict__ cnt_;
  double* __restrict__ re_;
  double* __restrict__ im_;
  double* __restrict__ wabs_;
  unsigned long long dropped_ = 0;
  unsigned long long clipped_ = 0;
  int32_t bad_ = 0;

  __device__ __forceinline__ void drop(int32_t n) { dropped_ += (unsigned long long)n; }
  __device__ __forceinline__ void clip(int32_t n) { clipped_ += (unsigned long long)n; }
  __device__ __forceinline__ void bad_index() { bad_ = 1; }

  __device__ __forceinline__ void add(int32_t bin, int32_t n, double re, double im, double wabs) {
    atomicAdd(cnt_ + bin, (unsigned long long)n);
    unsafeAtomicAdd(re_ + bin, re);   // (global_atomic_add_f64, no compare-exchange loop)
    unsafeAtomicAdd(im_ + bin, im);
    unsafeAtomicAdd(wabs_ + bin, wabs);
  }
};

// Own rows loaded ahead per lane.  A row here holds six doubles (phase_load),
// each row gathers up to four more points, and both walks' states stay live
// across them: 2, as the tube kernel has it, keeps the kernel clear of scratch.
constexpr int kWaveBatch = 2;

__global__ void __launch_bounds__(256)
ray_wave_kernel(const rwrt_wave_map wm, int64_t nray, int32_t it_begin, int32_t it_end,
                const double* __restrict__ rows, const int32_t* __restrict__ row_slot,
                const int32_t* __restrict__ tail_from, const double* __restrict__ tail_row,
                const int32_t* __restrict__ chan, const int32_t* __restrict__ nbr, int32_t* __restrict__ state_i,
                double* __restrict__ state_f, unsigned long long* __restrict__ cnt, double* __restrict__ re,
                double* __restrict__ im, double* __restrict__ wabs, unsigned long long* __restrict__ dropped,
                unsigned long long* __restrict__ clipped, int32_t* __restrict__ err) {
  const LaunchRows L{rows, row_slot, tail_from, tail_row, it_begin, it_end};
  const WaveMaps m = wave_maps(wm);
  WaveAtomics e{cnt, re, im, wabs};
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nray; j += (int64_t)gridDim.x * blockDim.x) {
    const int32_t ch = chan ? chan[j] : 0;
    if (ch < 0 || ch >= wm.nchan) continue;   // (not walked: its columns stay)
    WaveState s = wave_state_load(state_i, state_f, nray, j);
    wave_ray<kWaveBatch>(L, j, nray, nbr, m, ch, s, e);
    wave_state_store(s, state_i, state_f, nray, j);
    if (e.dropped_) atomicAdd(dropped, e.dropped_);
    if (e.clipped_) atomicAdd(clipped, e.clipped_);
    if (e.bad_) atomicOr(err, 1);
    e.dropped_ = 0;
    e.clipped_ = 0;
    e.bad_ = 0;
  }
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_ray_wave(const rwrt_wave_map* m, int64_t nray, int32_t it_begin, int32_t it_end,
                                     const double* d_rows, const int32_t* d_row_slot, const int32_t* d_tail_from,
                                     const double* d_tail_row, const int32_t* d_chan, const int32_t* d_nbr,
                                     int32_t* d_state_i, double* d_state_f, int64_t* d_cnt, double* d_re,
                                     double* d_im, double* d_wabs, int64_t* d_dropped, int64_t* d_clipped,
                                     int32_t* d_err, void* stream) {
  // (every check before the first HIP call)
  if (!m) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: map is NULL%s", "");
  if (const rwrt_status st = check_map_shape("rwrt_ray_wave", m->nx, m->ny, m->nchan)) return st;
  if (!map_column_ok(m->need)) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: need must be -1 or a column 2..6%s", "");
  if (!map_column_ok(m->wcol)) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: wcol must be -1 or a column 2..6%s", "");
  if (m->spread != 0 && m->spread != 1) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: spread must be 0 or 1%s", "");
  if (const rwrt_status st = check_map_axes("rwrt_ray_wave", m->inv_dlon, m->inv_dlat, m->lat0)) return st;
  if (!(m->max_sep > 0.0)) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: max_sep must be positive%s", "");
  if (!std::isfinite(m->omega_dt)) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: omega_dt must be finite%s", "");
  if (!(m->d_floor >= 0.0) || !std::isfinite(m->d_floor))
    return fail(RWRT_ERR_ARG, "rwrt_ray_wave: d_floor must be finite and not negative%s", "");
  if (const rwrt_status st = check_launch_rows("rwrt_ray_wave", nray, it_begin, it_end, d_rows, d_row_slot,
                                               d_tail_from, d_tail_row))
    return st;
  if (it_begin < 0) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: it_begin must not be negative%s", "");
  if (!d_nbr) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: d_nbr is NULL%s", "");
  if (!d_state_i) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: d_state_i is NULL%s", "");
  if (!d_state_f) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: d_state_f is NULL%s", "");
  if (!d_cnt) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: d_cnt is NULL%s", "");
  if (!d_re) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: d_re is NULL%s", "");
  if (!d_im) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: d_im is NULL%s", "");
  if (!d_wabs) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: d_wabs is NULL%s", "");
  if (!d_dropped) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: d_dropped is NULL%s", "");
  if (!d_clipped) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: d_clipped is NULL%s", "");
  if (!d_err) return fail(RWRT_ERR_ARG, "rwrt_ray_wave: d_err is NULL%s", "");
  if (nray == 0) return RWRT_OK;
  return launch_per_ray("ray_wave_kernel", ray_wave_kernel, nray, stream, *m, nray, it_begin, it_end, d_rows,
                        d_row_slot, d_tail_from, d_tail_row, d_chan, d_nbr, d_state_i, d_state_f,
                        reinterpret_cast<unsigned long long*>(d_cnt), d_re, d_im, d_wabs,
                        reinterpret_cast<unsigned long long*>(d_dropped),
                        reinterpret_cast<unsigned long long*>(d_clipped), d_err);
}
