// density.hip -- rwrt_ray_density (ABI 5): ray-density maps binned on the
// device from the row blocks and constant tails a ray-loop call has left.
//
// A translation unit of its own, linked into librwrt.so next to rwrt.hip, so
// that the ray loops' code object is not touched by it.
//
// One lane walks one ray's rows of the call in order.  Consecutive rows of a
// ray mostly fall into the same or a neighbouring bin, so the lane keeps the
// current bin's run (rows, weight sum) in registers and issues one atomic per
// run, not per row; a constant tail is one more run (rows x weight).  The map
// does not fit LDS (1440 x 720 x 8 B = 8 MB per channel), so runs go straight
// to global atomics: 64-bit integer adds for the counts (C5: 4.03 M rays x
// 1 080 rows in one bin exceed 2^32) and the hardware fp64 add for the sums.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "rwrt.h"
#include "abi_host.h"
#include "density_bins.h"
#include "launch_rows.h"
#include "map_host.h"

namespace rwrt {
namespace {

struct DensityRun {
  int32_t bin = -1;
  unsigned long long n = 0;
  double w = 0.0;
};

__device__ __forceinline__ void density_flush(const DensityRun& r, bool weighted,
                                              unsigned long long* __restrict__ count,
                                              double* __restrict__ wsum) {
  if (r.bin < 0) return;
  atomicAdd(count + r.bin, r.n);
  if (weighted) unsafeAtomicAdd(wsum + r.bin, r.w);   // (global_atomic_add_f64, no compare-exchange loop)
}

// one more point (or `rows` equal points) of the lane's ray
__device__ __forceinline__ void density_point(DensityRun& r, const rwrt_density_map& m, double lon, double lat,
                                              double w, int32_t c, unsigned long long rows,
                                              unsigned long long* __restrict__ count,
                                              double* __restrict__ wsum) {
  const int32_t b = density_bin(density_wrap_2pi(lon), lat, w, c, m);
  if (b != r.bin) {
    density_flush(r, m.wcol >= 0, count, wsum);
    r.bin = b;
    r.n = 0;
    r.w = 0.0;
  }
  if (b < 0) return;   // (w may be NaN here: never summed)
  r.n += rows;
  r.w = r.w + w * (double)rows;   // (rows = 1: w itself)
}

constexpr int kDensityBatch = 4;   // rows loaded ahead per lane

struct DensityRow {   // what the lane needs of a row: lon lat, and the weight column
  double2 p;
  double w;
};

__global__ void __launch_bounds__(256)
ray_density_kernel(const rwrt_density_map m, int64_t nray, int32_t it_begin, int32_t it_end,
                   const double* __restrict__ rows, const int32_t* __restrict__ row_slot,
                   const int32_t* __restrict__ tail_from, const double* __restrict__ tail_row,
                   const int32_t* __restrict__ chan, unsigned long long* __restrict__ count,
                   double* __restrict__ wsum) {
  const LaunchRows L{rows, row_slot, tail_from, tail_row, it_begin, it_end};
  const int wc = (m.wcol >= 0) ? m.wcol : 0;   // (a column that exists: its value is unused without a weight)
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nray; j += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = chan ? chan[j] : 0;
    if (c < 0 || c >= m.nchan) continue;
    DensityRun run;
    launch_rows_walk<kDensityBatch, DensityRow>(
        L, j, [wc](const double* r) { return DensityRow{*reinterpret_cast<const double2*>(r), r[wc]}; },
        [&](int32_t, const DensityRow& v) { density_point(run, m, v.p.x, v.p.y, v.w, c, 1, count, wsum); },
        [&](int32_t, int32_t n, const DensityRow& v) {
          density_point(run, m, v.p.x, v.p.y, v.w, c, (unsigned long long)n, count, wsum);
        });
    density_flush(run, m.wcol >= 0, count, wsum);
  }
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_ray_density(const rwrt_density_map* m, int64_t nray, int32_t it_begin, int32_t it_end,
                                        const double* d_rows, const int32_t* d_row_slot,
                                        const int32_t* d_tail_from, const double* d_tail_row,
                                        const int32_t* d_chan, int64_t* d_count, double* d_wsum, void* stream) {
  // (every check before the first HIP call)
  if (!m) return fail(RWRT_ERR_ARG, "rwrt_ray_density: map is NULL%s", "");
  if (const rwrt_status st = check_map_shape("rwrt_ray_density", m->nx, m->ny, m->nchan)) return st;
  if (!map_column_ok(m->wcol))
    return fail(RWRT_ERR_ARG, "rwrt_ray_density: wcol must be -1 or 2..6 (k l amp ug vg)%s", "");
  if (const rwrt_status st = check_map_axes("rwrt_ray_density", m->inv_dlon, m->inv_dlat, m->lat0)) return st;
  if (m->wcol >= 0 && !d_wsum) return fail(RWRT_ERR_ARG, "rwrt_ray_density: wcol >= 0 needs d_wsum%s", "");
  if (const rwrt_status st = check_launch_rows("rwrt_ray_density", nray, it_begin, it_end, d_rows, d_row_slot,
                                               d_tail_from, d_tail_row))
    return st;
  if (!d_count) return fail(RWRT_ERR_ARG, "rwrt_ray_density: d_count is NULL%s", "");
  if (nray == 0) return RWRT_OK;
  return launch_per_ray("ray_density_kernel", ray_density_kernel, nray, stream, *m, nray, it_begin, it_end, d_rows,
                        d_row_slot, d_tail_from, d_tail_row, d_chan, reinterpret_cast<unsigned long long*>(d_count),
                        d_wsum);
}
