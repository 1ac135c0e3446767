// wn_map.hip -- rwrt_wn_map and rwrt_wn_fill (ABI 5, additive): the wavenumber
// map, the reference's class WN (wn.py:21-135) on the device.
//
// A fourth translation unit, linked into librwrt.so next to rwrt.hip,
// density.hip and summary.hip, so that no other code object is touched by it.
// It shares csrc/ray_point.h with rwrt.hip: the bilinear lookup, the Mercator
// factors, np.roots (csrc/nproots.h) and the root ordering are the ones the
// initial rays use.
//
// wn_map_kernel: one thread per (level, node, zonal wavenumber), k fastest; a
// thread stores its three slots of mwn, ug, vg as 24 consecutive bytes.
// wn_fill_kernel: one thread per entry of [nlon][nlat][nplane], the plane
// fastest: a wave reads and writes consecutive doubles, and the eight
// neighbour reads of a NaN entry are consecutive across the wave as well.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rwrt.h"
#include "abi_host.h"
#include "ray_point.h"
#include "wn_fill.h"

namespace rwrt {

// (defined in rwrt.hip: the conditions of a packed level)
rwrt_status make_field(const rwrt_grid* g, const double* packed, Field& F);

namespace {

// initial_point at every grid node of every level.  mwn, ug, vg
// [nlev][nlon][nrow][nzwn][3], rootnum [nlev][nlon][nrow][nzwn]: the count of
// non-NaN slots, -1 where the polynomial was counted in info.
__global__ void __launch_bounds__(256)
wn_map_kernel(Field F, int32_t nlev, int64_t level_stride, int32_t nlon, const double* __restrict__ glon,
              const double* __restrict__ glat, const double* __restrict__ gcos, int32_t nzwn,
              const double* __restrict__ zc, double* __restrict__ mwn, double* __restrict__ ugo,
              double* __restrict__ vgo, int32_t* __restrict__ rootnum, int32_t* __restrict__ info) {
  const int64_t per_col = (int64_t)F.H * nzwn;
  const int64_t per_lev = (int64_t)nlon * per_col;
  const int64_t n = (int64_t)nlev * per_lev;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lev = i / per_lev;
    const int64_t r = i - lev * per_lev;
    const int ix = (int)(r / per_col);
    const int64_t q = r - ix * per_col;
    const int jy = (int)(q / nzwn);
    const int iz = (int)(q - (int64_t)jy * nzwn);
    Field L = F;
    L.P = F.P + lev * level_stride;
    double mr[3], ug[3], vg[3];
    const bool raised = initial_point(L, glon[ix], glat[jy], gcos[jy], zc[iz], zc[nzwn + iz], zc[2 * nzwn + iz],
                                      zc[3 * nzwn + iz], mr, ug, vg);
    int nroot = 0;
    for (int slot = 0; slot < 3; ++slot) {
      nroot += isnan(mr[slot]) ? 0 : 1;
      mwn[3 * i + slot] = mr[slot];
      ugo[3 * i + slot] = ug[slot];
      vgo[3 * i + slot] = vg[slot];
    }
    if (raised) atomicAdd(info, 1);
    rootnum[i] = raised ? -1 : nroot;
  }
}

__global__ void __launch_bounds__(256)
wn_fill_kernel(int32_t nlon, int32_t nlat, int32_t nplane, int32_t cyclic, const double* __restrict__ in,
               double* __restrict__ out) {
  const int64_t per_col = (int64_t)nlat * nplane;
  const int64_t n = (int64_t)nlon * per_col;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)(e / per_col);
    const int64_t r = e - i * per_col;
    const int32_t j = (int32_t)(r / nplane);
    const int32_t p = (int32_t)(r - (int64_t)j * nplane);
    out[e] = wn_fill_entry(in, nlon, nlat, nplane, cyclic != 0, i, j, p);
  }
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_wn_map(const rwrt_grid* g, const double* d_packed, int32_t nlev, int64_t level_stride,
                                   int32_t nlon, const double* d_lon, const double* d_lat, const double* d_cos,
                                   int32_t nzwn, const double* d_zwn, double* d_mwn, double* d_ug, double* d_vg,
                                   int32_t* d_rootnum, int32_t* d_info, void* stream) {
  // (every check before the first HIP call)
  Field F;
  if (rwrt_status s = make_field(g, d_packed, F)) return s;
  if (nlev < 1 || nzwn < 1) return fail(RWRT_ERR_ARG, "rwrt_wn_map: nlev and nzwn must be at least 1%s", "");
  if (nlon < 1 || nlon > g->ncol) return fail(RWRT_ERR_ARG, "rwrt_wn_map: nlon must be 1..ncol%s", "");
  if (nlev > 1 && level_stride < (int64_t)g->ncol * g->nrow * kNF)
    return fail(RWRT_ERR_ARG, "rwrt_wn_map: level_stride is shorter than one packed level%s", "");
  if (nlev > 1 && level_stride % 2 != 0)
    return fail(RWRT_ERR_ARG, "rwrt_wn_map: level_stride must keep every level 16-byte aligned%s", "");
  if (!d_lon || !d_lat || !d_cos || !d_zwn || !d_mwn || !d_ug || !d_vg || !d_rootnum || !d_info)
    return fail(RWRT_ERR_ARG, "rwrt_wn_map: NULL buffer%s", "");
  if (hipMemsetAsync(d_info, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess)
    return check_launch("hipMemsetAsync(info)");
  const int64_t n = (int64_t)nlev * nlon * g->nrow * nzwn;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 65535LL * 32) blocks = 65535LL * 32;
  hipLaunchKernelGGL(wn_map_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, F, nlev,
                     nlev > 1 ? level_stride : 0, nlon, d_lon, d_lat, d_cos, nzwn, d_zwn, d_mwn, d_ug, d_vg,
                     d_rootnum, d_info);
  return check_launch("wn_map_kernel");
}

extern "C" rwrt_status rwrt_wn_fill(int32_t nlon, int32_t nlat, int32_t nplane, int32_t cyclic, const double* d_in,
                                    double* d_out, void* stream) {
  // (every check before the first HIP call)
  if (nlon < 1 || nlat < 1 || nplane < 1)
    return fail(RWRT_ERR_ARG, "rwrt_wn_fill: nlon, nlat and nplane must be at least 1%s", "");
  if (!d_in) return fail(RWRT_ERR_ARG, "rwrt_wn_fill: d_in is NULL%s", "");
  if (!d_out) return fail(RWRT_ERR_ARG, "rwrt_wn_fill: d_out is NULL%s", "");
  if (d_in == d_out)
    return fail(RWRT_ERR_ARG, "rwrt_wn_fill: d_out must not be d_in (neighbours are read from the input)%s", "");
  const int64_t n = (int64_t)nlon * nlat * nplane;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 65535LL * 32) blocks = 65535LL * 32;
  hipLaunchKernelGGL(wn_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, nlon, nlat, nplane,
                     cyclic, d_in, d_out);
  return check_launch("wn_fill_kernel");
}
