// cross.hip -- rwrt_ray_cross (ABI 5, additive): gate-crossing maps, reduced on
// the device from the row blocks and constant tails a ray-loop call has left:
// every passage of a ray's segment through a latitude circle or a meridian is
// counted by direction, binned along the gate and timed, per map bin and per
// ray.
//
// A translation unit of its own, linked into librwrt.so next to the others, so
// that no other code object is touched by it.
//
// One lane walks one ray's rows of the call in order (csrc/cross_lines.h: a
// row's side of every gate computed once and carried, the crossing worked out
// only where two sides differ).  The ray's carried previous row is loaded from
// its column of d_prev before the first row and stored after the last --
// neighbouring lanes, neighbouring columns.  The emitter here turns a crossing
// into one 64-bit integer add and one or two hardware fp64 adds, all native
// (no compare-exchange loop), and into plain loads and stores of the ray's own
// column of d_ncross / d_tfirst; the drops are counted in a register and added
// once per ray.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "abi_host.h"
#include "cross_lines.h"
#include "map_host.h"

namespace rwrt {
namespace {

struct CrossAtomics {
  const rwrt_cross_map& m_;
  unsigned long long* __restrict__ cnt_;
  double* __restrict__ tsum_;
  double* __restrict__ wsum_;     // NULL without a weight
  int32_t* __restrict__ ncross_;  // NULL (with tfirst_): maps only
  double* __restrict__ tfirst_;
  int64_t ncol_;
  int64_t col_ = 0;               // the ray's column
  int32_t chan_ = 0;
  unsigned long long dropped_ = 0;

  __device__ __forceinline__ void drop() { ++dropped_; }

  __device__ __forceinline__ void hit(int32_t g, int32_t d, int32_t w, int32_t bin, double tc, double wv) {
    if (ncross_) {   // (the lane owns its column)
      const int64_t k = (int64_t)(g * 2 + d) * ncol_ + col_;
      ncross_[k] += 1;
      if (tfirst_[k] != tfirst_[k]) tfirst_[k] = tc;
    }
    if (bin < 0) return;
    const int64_t index = cross_index(m_, w, g, d, chan_, bin);
    atomicAdd(cnt_ + index, 1ull);
    unsafeAtomicAdd(tsum_ + index, tc);   // (global_atomic_add_f64, no compare-exchange loop)
    if (wsum_) unsafeAtomicAdd(wsum_ + index, wv);
  }
};

constexpr int kCrossBatch = 4;   // rows loaded ahead per lane

template <int NG>
__global__ void __launch_bounds__(256)
ray_cross_kernel(const rwrt_cross_map m, int64_t nray, int32_t it_begin, int32_t it_end,
                 const double* __restrict__ rows, const int32_t* __restrict__ row_slot,
                 const int32_t* __restrict__ tail_from, const double* __restrict__ tail_row,
                 const int64_t* __restrict__ ray, int64_t ncol, const int32_t* __restrict__ chan,
                 double* __restrict__ prev, unsigned long long* __restrict__ cnt, double* __restrict__ tsum,
                 double* __restrict__ wsum, unsigned long long* __restrict__ dropped, int32_t* __restrict__ ncross,
                 double* __restrict__ tfirst) {
  const LaunchRows L{rows, row_slot, tail_from, tail_row, it_begin, it_end};
  CrossAtomics e{m, cnt, tsum, wsum, ncross, tfirst, ncol};
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nray; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = ray ? ray[j] : j;
    if (c < 0 || c >= ncol) continue;
    const int32_t ch = chan ? chan[c] : 0;
    if (ch < 0 || ch >= m.nchan) continue;   // (not walked: its column stays)
    e.col_ = c;
    e.chan_ = ch;
    CrossState<NG> s;
    s.lon = prev[c];
    s.lat = prev[ncol + c];
    s.v = prev[2 * ncol + c];
    cross_ray<NG, kCrossBatch>(L, j, m, s, e);
    prev[c] = s.lon;
    prev[ncol + c] = s.lat;
    prev[2 * ncol + c] = s.v;
    if (e.dropped_) atomicAdd(dropped, e.dropped_);
    e.dropped_ = 0;
  }
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_ray_cross(const rwrt_cross_map* m, int64_t nray, int32_t it_begin, int32_t it_end,
                                      const double* d_rows, const int32_t* d_row_slot,
                                      const int32_t* d_tail_from, const double* d_tail_row, const int64_t* d_ray,
                                      int64_t nacc_cols, const int32_t* d_chan, double* d_prev, int64_t* d_cnt,
                                      double* d_tsum, double* d_wsum, int64_t* d_dropped, int32_t* d_ncross,
                                      double* d_tfirst, void* stream) {
  // (every check before the first HIP call)
  if (!m) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: map is NULL%s", "");
  if (m->ngate < 1 || m->ngate > RWRT_CROSS_MAXGATE)
    return fail(RWRT_ERR_ARG, "rwrt_ray_cross: ngate must be 1..8 (RWRT_CROSS_MAXGATE)%s", "");
  if (m->nbin <= 0 || m->nchan <= 0) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: nbin and nchan must be positive%s", "");
  if (m->window_rows < 0) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: window_rows must not be negative%s", "");
  if (m->nwin < 1) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: nwin must be at least 1%s", "");
  if (m->window_rows == 0 && m->nwin != 1)
    return fail(RWRT_ERR_ARG, "rwrt_ray_cross: nwin must be 1 without windows (window_rows == 0)%s", "");
  {
    // (each product is of a value below 2^31 and a factor below 2^31: no overflow of int64)
    const int64_t lim = 1LL << 31, planes = (int64_t)m->nwin * m->ngate * 2;
    if (planes >= lim || planes * m->nchan >= lim || planes * m->nchan * m->nbin >= lim)
      return fail(RWRT_ERR_ARG, "rwrt_ray_cross: nwin*ngate*2*nchan*nbin must be below 2^31%s", "");
  }
  static const char* const kGate[RWRT_CROSS_MAXGATE] = {"0", "1", "2", "3", "4", "5", "6", "7"};
  for (int g = 0; g < m->ngate; ++g) {
    const rwrt_cross_gate& q = m->gate[g];
    if (q.kind != 0 && q.kind != 1)
      return fail(RWRT_ERR_ARG, "rwrt_ray_cross: gate %s: kind must be 0 (latitude circle) or 1 (meridian)", kGate[g]);
    if (!std::isfinite(q.pos)) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: gate %s: pos must be finite", kGate[g]);
    if (!std::isfinite(q.org)) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: gate %s: org must be finite", kGate[g]);
    if (!(q.inv_d > 0.0) || !std::isfinite(q.inv_d))
      return fail(RWRT_ERR_ARG, "rwrt_ray_cross: gate %s: inv_d must be finite and positive", kGate[g]);
    if (q.kind == 0 && q.org != 0.0)
      return fail(RWRT_ERR_ARG, "rwrt_ray_cross: gate %s: org must be 0 for a latitude circle (bins over longitude)",
                  kGate[g]);
    if (q.kind == 1 && !(q.pos >= 0.0 && q.pos < kCrossTwoPi))
      return fail(RWRT_ERR_ARG, "rwrt_ray_cross: gate %s: pos of a meridian must lie in [0, 2 pi)", kGate[g]);
  }
  if (!map_column_ok(m->need)) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: need must be -1 or a column 2..6%s", "");
  if (!map_column_ok(m->wcol)) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: wcol must be -1 or a column 2..6%s", "");
  if (const rwrt_status st = check_launch_rows("rwrt_ray_cross", nray, it_begin, it_end, d_rows, d_row_slot,
                                               d_tail_from, d_tail_row))
    return st;
  if (it_begin < 0) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: it_begin must not be negative%s", "");
  if (m->window_rows > 0 && (int64_t)it_end - 1 > (int64_t)m->nwin * m->window_rows)
    return fail(RWRT_ERR_ARG, "rwrt_ray_cross: it_end - 1 exceeds nwin * window_rows%s", "");
  if (nacc_cols < 0 || nacc_cols > 0x7fffffffLL || (!d_ray && nacc_cols < nray))
    return fail(RWRT_ERR_ARG, "rwrt_ray_cross: nacc_cols must cover every ray's column%s", "");
  if (!d_prev) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: d_prev is NULL%s", "");
  if (!d_cnt) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: d_cnt is NULL%s", "");
  if (!d_tsum) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: d_tsum is NULL%s", "");
  if (m->wcol >= 0 && !d_wsum) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: d_wsum is NULL with a weight column%s", "");
  if (m->wcol < 0 && d_wsum) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: d_wsum needs a weight column (wcol)%s", "");
  if (!d_dropped) return fail(RWRT_ERR_ARG, "rwrt_ray_cross: d_dropped is NULL%s", "");
  if (!d_ncross != !d_tfirst)
    return fail(RWRT_ERR_ARG, "rwrt_ray_cross: the per-ray arrays need both d_ncross and d_tfirst%s", "");
  if (nray == 0) return RWRT_OK;
#define RWRT_CROSS_CASE(NG)                                                                                      \
  case NG:                                                                                                       \
    return launch_per_ray("ray_cross_kernel", ray_cross_kernel<NG>, nray, stream, *m, nray, it_begin, it_end,    \
                          d_rows, d_row_slot, d_tail_from, d_tail_row, d_ray, nacc_cols, d_chan, d_prev,         \
                          reinterpret_cast<unsigned long long*>(d_cnt), d_tsum, d_wsum,                          \
                          reinterpret_cast<unsigned long long*>(d_dropped), d_ncross, d_tfirst);
  switch (m->ngate) {
    RWRT_CROSS_CASE(1)
    RWRT_CROSS_CASE(2)
    RWRT_CROSS_CASE(3)
    RWRT_CROSS_CASE(4)
    RWRT_CROSS_CASE(5)
    RWRT_CROSS_CASE(6)
    RWRT_CROSS_CASE(7)
    RWRT_CROSS_CASE(8)
  }
#undef RWRT_CROSS_CASE
  return RWRT_OK;   // (not reached: ngate was checked above)
}
