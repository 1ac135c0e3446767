// summary.hip -- rwrt_ray_summary (ABI 5, additive): per-ray path summaries
// reduced on the device from the row blocks and constant tails a ray-loop call
// has left.
//
// A third translation unit, linked into librwrt.so next to rwrt.hip and
// density.hip, so that neither code object is touched by it.  It uses the
// device library's sin / cos / atan2 / sqrt, not the ray loops' np_math.h.
//
// One lane walks one ray's rows of the call in order and keeps the ray's
// accumulator (csrc/summary_rows.h) in registers: its column of the
// struct-of-arrays accumulators is loaded once before the first row and stored
// once after the last -- neighbouring lanes, neighbouring columns -- so there
// are no atomics and no LDS.  Of a 64-byte row the lane needs columns 0..4
// (lon lat | k l | amp ug): three 16-byte loads, issued for a few rows ahead.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "abi_host.h"
#include "launch_rows.h"
#include "summary_rows.h"

namespace rwrt {
namespace {

constexpr int kSummaryBatch = 4;   // rows loaded ahead per lane

struct SummaryRow {   // what the lane needs of a row: three 16-byte loads
  double2 p, q, s;    // lon lat | k l | amp ug
};

enum { F_LON_FIRST, F_LAT_FIRST, F_LON_LAST, F_LAT_LAST, F_L_LAST, F_LAT_MIN, F_LAT_MAX, F_AMP_MAX, F_PATH };
enum { I_N_VALID, I_LAST_ROW, I_N_TURN, I_PREV_VALID };
static_assert(F_PATH + 1 == RWRT_SUMMARY_NF64 && I_PREV_VALID + 1 == RWRT_SUMMARY_NI32, "accumulator layout");

template <int NR>
__global__ void __launch_bounds__(256)
ray_summary_kernel(const rwrt_summary_regions reg, int64_t nray, int32_t it_begin, int32_t it_end,
                   const double* __restrict__ rows, const int32_t* __restrict__ row_slot,
                   const int32_t* __restrict__ tail_from, const double* __restrict__ tail_row,
                   const int64_t* __restrict__ ray, int64_t ncol, double* __restrict__ f64,
                   int32_t* __restrict__ i32) {
  const LaunchRows L{rows, row_slot, tail_from, tail_row, it_begin, it_end};
  const int nreg = (NR > 0) ? reg.nreg : 0;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nray; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = ray ? ray[j] : j;
    if (c < 0 || c >= ncol) continue;
    SummaryAcc<NR> a;
    a.lon_first = f64[F_LON_FIRST * ncol + c];
    a.lat_first = f64[F_LAT_FIRST * ncol + c];
    a.lon_last = f64[F_LON_LAST * ncol + c];
    a.lat_last = f64[F_LAT_LAST * ncol + c];
    a.l_last = f64[F_L_LAST * ncol + c];
    a.lat_min = f64[F_LAT_MIN * ncol + c];
    a.lat_max = f64[F_LAT_MAX * ncol + c];
    a.amp_max = f64[F_AMP_MAX * ncol + c];
    a.path = f64[F_PATH * ncol + c];
    a.n_valid = i32[I_N_VALID * ncol + c];
    a.last_row = i32[I_LAST_ROW * ncol + c];
    a.n_turn = i32[I_N_TURN * ncol + c];
    a.prev_valid = i32[I_PREV_VALID * ncol + c];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (r < nreg) {
        a.first_row[r] = i32[(RWRT_SUMMARY_NI32 + r) * ncol + c];
        a.rows_inside[r] = i32[(RWRT_SUMMARY_NI32 + nreg + r) * ncol + c];
      }
    }
    launch_rows_walk<kSummaryBatch, SummaryRow>(
        L, j,
        [](const double* r) {
          const double2* __restrict__ v = reinterpret_cast<const double2*>(r);
          return SummaryRow{v[0], v[1], v[2]};
        },
        [&](int32_t i, const SummaryRow& v) { summary_row<NR>(a, reg, i, v.p.x, v.p.y, v.q.y, v.s.x); },
        [&](int32_t tf, int32_t n, const SummaryRow& v) {
          summary_tail<NR>(a, reg, tf, n, v.p.x, v.p.y, v.q.y, v.s.x);
        });
    f64[F_LON_FIRST * ncol + c] = a.lon_first;
    f64[F_LAT_FIRST * ncol + c] = a.lat_first;
    f64[F_LON_LAST * ncol + c] = a.lon_last;
    f64[F_LAT_LAST * ncol + c] = a.lat_last;
    f64[F_L_LAST * ncol + c] = a.l_last;
    f64[F_LAT_MIN * ncol + c] = a.lat_min;
    f64[F_LAT_MAX * ncol + c] = a.lat_max;
    f64[F_AMP_MAX * ncol + c] = a.amp_max;
    f64[F_PATH * ncol + c] = a.path;
    i32[I_N_VALID * ncol + c] = a.n_valid;
    i32[I_LAST_ROW * ncol + c] = a.last_row;
    i32[I_N_TURN * ncol + c] = a.n_turn;
    i32[I_PREV_VALID * ncol + c] = a.prev_valid;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (r < nreg) {
        i32[(RWRT_SUMMARY_NI32 + r) * ncol + c] = a.first_row[r];
        i32[(RWRT_SUMMARY_NI32 + nreg + r) * ncol + c] = a.rows_inside[r];
      }
    }
  }
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_ray_summary(int64_t nray, int32_t it_begin, int32_t it_end, const double* d_rows,
                                        const int32_t* d_row_slot, const int32_t* d_tail_from,
                                        const double* d_tail_row, const int64_t* d_ray, int64_t nacc_cols,
                                        const rwrt_summary_regions* reg, double* d_f64, int32_t* d_i32,
                                        void* stream) {
  // (every check before the first HIP call)
  rwrt_summary_regions none = {};
  if (reg) {
    if (reg->nreg < 0 || reg->nreg > RWRT_SUMMARY_MAXREG)
      return fail(RWRT_ERR_ARG, "rwrt_ray_summary: nreg must be 0..8%s", "");
    for (int r = 0; r < reg->nreg; ++r)
      for (int k = 0; k < 4; ++k)
        if (!std::isfinite(reg->box[r][k]))
          return fail(RWRT_ERR_ARG, "rwrt_ray_summary: every box edge must be finite%s", "");
  }
  if (const rwrt_status st = check_launch_rows("rwrt_ray_summary", nray, it_begin, it_end, d_rows, d_row_slot,
                                               d_tail_from, d_tail_row))
    return st;
  if (it_begin < 0) return fail(RWRT_ERR_ARG, "rwrt_ray_summary: it_begin must not be negative%s", "");
  if (!d_f64) return fail(RWRT_ERR_ARG, "rwrt_ray_summary: d_f64 is NULL%s", "");
  if (!d_i32) return fail(RWRT_ERR_ARG, "rwrt_ray_summary: d_i32 is NULL%s", "");
  if (nacc_cols < 0 || nacc_cols > 0x7fffffffLL || (!d_ray && nacc_cols < nray))
    return fail(RWRT_ERR_ARG, "rwrt_ray_summary: nacc_cols must cover every ray's column%s", "");
  if (nray == 0) return RWRT_OK;
  const rwrt_summary_regions& rg = reg ? *reg : none;
  const unsigned blocks = (unsigned)((nray + 255) / 256);
#define RWRT_SUMMARY_LAUNCH(NR)                                                                              \
  hipLaunchKernelGGL(ray_summary_kernel<NR>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rg, nray,     \
                     it_begin, it_end, d_rows, d_row_slot, d_tail_from, d_tail_row, d_ray, nacc_cols, d_f64, \
                     d_i32)
  // (the accumulator's region registers: none, two, or all eight)
  if (rg.nreg == 0) {
    RWRT_SUMMARY_LAUNCH(0);
  } else if (rg.nreg <= 2) {
    RWRT_SUMMARY_LAUNCH(2);
  } else {
    RWRT_SUMMARY_LAUNCH(8);
  }
#undef RWRT_SUMMARY_LAUNCH
  return check_launch("ray_summary_kernel");
}
