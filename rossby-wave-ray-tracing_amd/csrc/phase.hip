// phase.hip -- rwrt_ray_phase (ABI 5, additive): the WKB phase theta = int k
// dlon + l dY along every ray, and the rays' waves w exp(i psi) superposed per
// box of a lon-lat map, reduced on the device from the row blocks and constant
// tails a ray-loop call has left.
//
// A translation unit of its own, linked into librwrt.so next to the others, so
// that no other code object is touched by it.  It uses the device library's
// cos and sincos, not the ray loops' np_math.h.
//
// One lane walks one ray's rows of the call in order (csrc/phase_rows.h: one
// cos per valid row, a = l / cos(lat) carried to the next row).  The ray's
// carried previous row, its theta and its nseg are loaded from its column
// before the first row and stored after the last -- neighbouring lanes,
// neighbouring columns, plain loads and stores.  The emitter here turns a
// deposit into one 64-bit integer add and two or three hardware fp64 adds, all
// native (no compare-exchange loop); the drops are counted in a register and
// added once per ray.  The map does not fit LDS (1440 x 720 x 8 B = 8 MB per
// sum and channel), and consecutive rows of a ray carry different phases, so
// every deposit goes straight to global atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "abi_host.h"
#include "map_host.h"
#include "phase_rows.h"

namespace rwrt {
namespace {

struct PhaseAtomics {
  unsigned long long* __restrict__ cnt_;
  double* __restrict__ re_;
  double* __restrict__ im_;
  double* __restrict__ wabs_;   // NULL without a weight
  unsigned long long dropped_ = 0;

  __device__ __forceinline__ void drop(int32_t n) { dropped_ += (unsigned long long)n; }

  __device__ __forceinline__ void add(int32_t bin, int32_t n, double re, double im, double wabs) {
    atomicAdd(cnt_ + bin, (unsigned long long)n);
    unsafeAtomicAdd(re_ + bin, re);   // (global_atomic_add_f64, no compare-exchange loop)
    unsafeAtomicAdd(im_ + bin, im);
    if (wabs_) unsafeAtomicAdd(wabs_ + bin, wabs);
  }
};

constexpr int kPhaseBatch = 4;   // rows loaded ahead per lane

__global__ void __launch_bounds__(256)
ray_phase_kernel(const rwrt_phase_map m, int64_t nray, int32_t it_begin, int32_t it_end,
                 const double* __restrict__ rows, const int32_t* __restrict__ row_slot,
                 const int32_t* __restrict__ tail_from, const double* __restrict__ tail_row,
                 const int64_t* __restrict__ ray, int64_t ncol, const int32_t* __restrict__ chan,
                 double* __restrict__ carry, double* __restrict__ theta, int32_t* __restrict__ nseg,
                 unsigned long long* __restrict__ cnt, double* __restrict__ re, double* __restrict__ im,
                 double* __restrict__ wabs, unsigned long long* __restrict__ dropped) {
  const LaunchRows L{rows, row_slot, tail_from, tail_row, it_begin, it_end};
  const rwrt_density_map bins = phase_bins(m);
  PhaseAtomics e{cnt, re, im, wabs};
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nray; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = ray ? ray[j] : j;
    if (c < 0 || c >= ncol) continue;
    const int32_t ch = chan ? chan[c] : 0;
    if (ch < 0 || ch >= m.nchan) continue;   // (not walked: its columns stay)
    PhaseState s;
    s.lon = carry[c];
    s.lat = carry[ncol + c];
    s.k = carry[2 * ncol + c];
    s.a = carry[3 * ncol + c];
    s.theta = theta[c];
    s.nseg = nseg[c];
    phase_ray<kPhaseBatch>(L, j, m, bins, ch, s, e);
    carry[c] = s.lon;
    carry[ncol + c] = s.lat;
    carry[2 * ncol + c] = s.k;
    carry[3 * ncol + c] = s.a;
    theta[c] = s.theta;
    nseg[c] = s.nseg;
    if (e.dropped_) atomicAdd(dropped, e.dropped_);
    e.dropped_ = 0;
  }
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_ray_phase(const rwrt_phase_map* m, int64_t nray, int32_t it_begin, int32_t it_end,
                                      const double* d_rows, const int32_t* d_row_slot,
                                      const int32_t* d_tail_from, const double* d_tail_row, const int64_t* d_ray,
                                      int64_t nacc_cols, const int32_t* d_chan, double* d_carry, double* d_theta,
                                      int32_t* d_nseg, int64_t* d_cnt, double* d_re, double* d_im, double* d_wabs,
                                      int64_t* d_dropped, void* stream) {
  // (every check before the first HIP call)
  if (!m) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: map is NULL%s", "");
  if (const rwrt_status st = check_map_shape("rwrt_ray_phase", m->nx, m->ny, m->nchan)) return st;
  if (!map_column_ok(m->need)) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: need must be -1 or a column 2..6%s", "");
  if (!map_column_ok(m->wcol)) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: wcol must be -1 or a column 2..6%s", "");
  if (const rwrt_status st = check_map_axes("rwrt_ray_phase", m->inv_dlon, m->inv_dlat, m->lat0)) return st;
  if (!std::isfinite(m->omega_dt)) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: omega_dt must be finite%s", "");
  if (const rwrt_status st = check_launch_rows("rwrt_ray_phase", nray, it_begin, it_end, d_rows, d_row_slot,
                                               d_tail_from, d_tail_row))
    return st;
  if (it_begin < 0) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: it_begin must not be negative%s", "");
  if (nacc_cols < 0 || nacc_cols > 0x7fffffffLL || (!d_ray && nacc_cols < nray))
    return fail(RWRT_ERR_ARG, "rwrt_ray_phase: nacc_cols must cover every ray's column%s", "");
  if (!d_carry) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: d_carry is NULL%s", "");
  if (!d_theta) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: d_theta is NULL%s", "");
  if (!d_nseg) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: d_nseg is NULL%s", "");
  if (!d_cnt) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: d_cnt is NULL%s", "");
  if (!d_re) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: d_re is NULL%s", "");
  if (!d_im) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: d_im is NULL%s", "");
  if (m->wcol >= 0 && !d_wabs) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: d_wabs is NULL with a weight column%s", "");
  if (m->wcol < 0 && d_wabs) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: d_wabs needs a weight column (wcol)%s", "");
  if (!d_dropped) return fail(RWRT_ERR_ARG, "rwrt_ray_phase: d_dropped is NULL%s", "");
  if (nray == 0) return RWRT_OK;
  return launch_per_ray("ray_phase_kernel", ray_phase_kernel, nray, stream, *m, nray, it_begin, it_end, d_rows,
                        d_row_slot, d_tail_from, d_tail_row, d_ray, nacc_cols, d_chan, d_carry, d_theta, d_nseg,
                        reinterpret_cast<unsigned long long*>(d_cnt), d_re, d_im, d_wabs,
                        reinterpret_cast<unsigned long long*>(d_dropped));
}
