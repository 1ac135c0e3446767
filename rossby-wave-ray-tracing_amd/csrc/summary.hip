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
#include "summary_rows.h"

namespace rwrt {

// (defined in rwrt.hip: the calling thread's last error, rwrt_last_error)
rwrt_status fail(rwrt_status s, const char* fmt, const char* detail);
rwrt_status check_launch(const char* what);

namespace {

constexpr int kSummaryBatch = 4;   // rows loaded ahead per lane

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
  const int32_t nrows = it_end - it_begin;
  const int nreg = (NR > 0) ? reg.nreg : 0;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nray; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = ray ? ray[j] : j;
    if (c < 0 || c >= ncol) continue;
    // rows [it_begin, tf) are read from the ray's block, rows [tf, it_end) are its tail
    int32_t tf = it_end;
    if (tail_from) tf = min(max(tail_from[j], it_begin), it_end);
    int64_t blk = j;
    if (row_slot) {
      blk = row_slot[j];
      if (blk < 0) tf = it_begin;   // no block: every row is the tail
    }
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
    const int32_t nread = tf - it_begin;
    if (nread > 0) {
      const double* __restrict__ r = rows + blk * (int64_t)nrows * RWRT_NOUT;
      int32_t i = 0;
      for (; i + kSummaryBatch <= nread; i += kSummaryBatch) {
        double2 p[kSummaryBatch], q[kSummaryBatch], s[kSummaryBatch];
#pragma unroll
        for (int k = 0; k < kSummaryBatch; ++k) {
          const double2* __restrict__ v = reinterpret_cast<const double2*>(r + (int64_t)(i + k) * RWRT_NOUT);
          p[k] = v[0];   // lon lat
          q[k] = v[1];   // k l
          s[k] = v[2];   // amp ug
        }
#pragma unroll
        for (int k = 0; k < kSummaryBatch; ++k)
          summary_row<NR>(a, reg, it_begin + i + k, p[k].x, p[k].y, q[k].y, s[k].x);
      }
      for (; i < nread; ++i) {
        const double2* __restrict__ v = reinterpret_cast<const double2*>(r + (int64_t)i * RWRT_NOUT);
        const double2 p = v[0], q = v[1], s = v[2];
        summary_row<NR>(a, reg, it_begin + i, p.x, p.y, q.y, s.x);
      }
    }
    if (tf < it_end) {
      const double2* __restrict__ v = reinterpret_cast<const double2*>(tail_row + j * RWRT_NOUT);
      const double2 p = v[0], q = v[1], s = v[2];
      summary_tail<NR>(a, reg, tf, it_end - tf, p.x, p.y, q.y, s.x);
    }
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
  if (it_end <= it_begin) return fail(RWRT_ERR_ARG, "rwrt_ray_summary: need it_begin < it_end%s", "");
  if (it_begin < 0) return fail(RWRT_ERR_ARG, "rwrt_ray_summary: it_begin must not be negative%s", "");
  if (nray < 0 || nray > 0x7fffffffLL) return fail(RWRT_ERR_ARG, "rwrt_ray_summary: nray out of range%s", "");
  if (!d_tail_from != !d_tail_row)
    return fail(RWRT_ERR_ARG, "rwrt_ray_summary: tails need both d_tail_from and d_tail_row%s", "");
  if (d_row_slot && !d_tail_from)
    return fail(RWRT_ERR_ARG, "rwrt_ray_summary: d_row_slot needs tails (d_tail_from, d_tail_row)%s", "");
  if (!d_f64) return fail(RWRT_ERR_ARG, "rwrt_ray_summary: d_f64 is NULL%s", "");
  if (!d_i32) return fail(RWRT_ERR_ARG, "rwrt_ray_summary: d_i32 is NULL%s", "");
  if (nacc_cols < 0 || nacc_cols > 0x7fffffffLL || (!d_ray && nacc_cols < nray))
    return fail(RWRT_ERR_ARG, "rwrt_ray_summary: nacc_cols must cover every ray's column%s", "");
  if (nray == 0) return RWRT_OK;
  if (!d_rows) return fail(RWRT_ERR_ARG, "rwrt_ray_summary: d_rows is NULL%s", "");
  if (reinterpret_cast<uintptr_t>(d_rows) % 16 != 0 || reinterpret_cast<uintptr_t>(d_tail_row) % 16 != 0)
    return fail(RWRT_ERR_ARG, "rwrt_ray_summary: d_rows and d_tail_row must be 16-byte aligned%s", "");
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
