// bs_diag.hip -- rwrt_bs_diag (ABI 5, additive): the 23 planes of the
// reference's BS.output (bs.py:461-511) for a batch of levels, on the device.
//
// A seventh translation unit, linked into librwrt.so next to the other six, so
// that no other code object is touched by it.  The per-node arithmetic is
// csrc/bs_diag.h, shared with the host program tests/host/bs_diag_main.cpp; it
// restates the vorticity, the stencils and smth9 of rwrt_bs_ready (rwrt.hip),
// and tests/test_gpu_bsdiag.py pins the two copies to each other.
//
// Input u, v is [nlat][nlon] (file layout), output [nlon][nlat]: a transposing
// stencil.  A block stages a 32 x 32 tile of u, v with its halo (one column,
// two rows: the edge rows' stencils reach two rows in) in shared memory,
// loading along longitude, and then computes and stores along latitude.  (The
// variant without a tile -- one thread per node, latitude fastest, u, v read
// from global memory with a stride of a whole latitude row, as rwrt_bs_ready's
// kernels do -- measured slower at 0.25 degrees and is gone: DESIGN.md
// section 16.)  The scratch planes q, qxx, qyy, qxy are [nlon][nlat] like the
// output, so their loads run along latitude already and go through no tile.
// No atomics; a node's planes depend on its level's u, v alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rwrt.h"
#include "abi_host.h"
#include "bs_diag.h"

namespace rwrt {
namespace {

constexpr int kThreads = 256;
constexpr int kTI = 32, kTJ = 32;        // tile: longitudes x latitudes
constexpr int kHaloJ = 2;                // rows below and above the tile
constexpr int kTileW = 35;               // floats per tile row: kTI + 2 halo columns, padded to an odd stride
constexpr int kTileH = kTJ + 2 * kHaloJ;

struct DiagArgs {
  BsdGeom g;
  int32_t nlev;          // levels of this launch
  uint32_t select;
  int32_t nsel;          // popcount(select)
  const float* u;        // [nlev][nlat][nlon]
  const float* v;
  const double* trig;    // [3][nlat]
  double* scratch;       // [nlev][4][nlon][nlat]: q, qxx, qyy, qxy (NULL without a q plane)
  double* out;           // [nlev][nsel][nlon][nlat]
};

// u or v of one level in global memory, file layout
struct GlobalUV {
  const float* p;
  int32_t nlon;
  __device__ __forceinline__ double operator()(int i, int j) const {
    return (double)p[(int64_t)j * nlon + bsd_wrap(i, nlon)];
  }
};

// a [nlon][nlat] plane of one level in global memory
struct GlobalQ {
  const double* p;
  int32_t nlon, nlat;
  __device__ __forceinline__ double operator()(int i, int j) const {
    return p[(int64_t)bsd_wrap(i, nlon) * nlat + j];
  }
};

// the selected planes of one node
template <class FU, class FV>
__device__ __forceinline__ void store_node(const DiagArgs& a, uint32_t select, const FU& u, const FV& v, int64_t lev,
                                           int i, int j) {
  const int64_t n = (int64_t)a.g.nlon * a.g.nlat;
  const double* sq = a.scratch ? a.scratch + lev * 4 * n : nullptr;
  const GlobalQ q{sq, a.g.nlon, a.g.nlat}, qxx{sq + n, a.g.nlon, a.g.nlat}, qyy{sq + 2 * n, a.g.nlon, a.g.nlat},
      qxy{sq + 3 * n, a.g.nlon, a.g.nlat};
  double* o = a.out + lev * a.nsel * n + (int64_t)i * a.g.nlat + j;
#pragma unroll
  for (int p = 0; p < BSD_NDIAG; ++p) {
    if (select & (1u << p)) {
      *o = bsd_plane(p, u, v, q, qxx, qyy, qxy, a.trig, a.g, i, j);
      o += n;
    }
  }
}

// u or v of one tile in shared memory: columns i0-1 .. i0+kTI, rows j0-2 .. j0+kTJ+1
struct TileUV {
  const float* s;
  int32_t i0, j0;
  __device__ __forceinline__ double operator()(int i, int j) const {
    return (double)s[(j - j0 + kHaloJ) * kTileW + (i - i0 + 1)];
  }
};

// Stage the tile at (i0, j0) of one level's field: only the columns and rows a
// node of the grid can reach (columns up to min(i0 + kTI, nlon), which wraps to
// 0; rows inside [0, nlat)), a wave loading along longitude.
__device__ __forceinline__ void load_tile(float* s, const float* __restrict__ f, const BsdGeom& g, int i0, int j0) {
  const int ncol = (g.nlon - i0 < kTI ? g.nlon - i0 : kTI) + 2;
  for (int e = threadIdx.x; e < kTileH * kTileW; e += kThreads) {
    const int r = e / kTileW, c = e - r * kTileW;
    const int j = j0 - kHaloJ + r;
    if (c < ncol && j >= 0 && j < g.nlat) s[e] = f[(int64_t)j * g.nlon + bsd_wrap(i0 - 1 + c, g.nlon)];
  }
}

// A block per 32 x 32 tile of one level (tiles: latitude fastest, then
// longitude, then level).  VORT: the vorticity q of every node into the scratch;
// otherwise the selected planes (SEL: the mask at compile time, 0: a.select).
template <bool VORT, uint32_t SEL>
__global__ void __launch_bounds__(kThreads) diag_tiled_kernel(DiagArgs a) {
  __shared__ float su[kTileH * kTileW];
  __shared__ float sv[kTileH * kTileW];
  const uint32_t select = SEL ? SEL : a.select;
  const bool need_v = VORT || (select & kBsdReadsV) != 0;   // (the q planes come from the scratch)
  const int64_t n = (int64_t)a.g.nlon * a.g.nlat;
  const int64_t tj = (a.g.nlat + kTJ - 1) / kTJ, ti = (a.g.nlon + kTI - 1) / kTI;
  const int64_t ntile = tj * ti * a.nlev;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t lev = t / (tj * ti), r = t - lev * (tj * ti);
    const int i0 = (int)(r / tj) * kTI, j0 = (int)(r % tj) * kTJ;
    load_tile(su, a.u + lev * n, a.g, i0, j0);
    if (need_v) load_tile(sv, a.v + lev * n, a.g, i0, j0);
    __syncthreads();
    const TileUV u{su, i0, j0}, v{sv, i0, j0};
#pragma unroll 1   // (one node's planes at a time: unrolled, the 23-plane kernel spills)
    for (int k = 0; k < kTI * kTJ / kThreads; ++k) {
      const int e = threadIdx.x + k * kThreads;
      const int i = i0 + e / kTJ, j = j0 + e % kTJ;
      if (i < a.g.nlon && j < a.g.nlat) {
        if (VORT)
          a.scratch[lev * 4 * n + (int64_t)i * a.g.nlat + j] = bsd_vorticity(u, v, a.trig, a.g, i, j);
        else
          store_node(a, select, u, v, lev, i, j);
      }
    }
    __syncthreads();
  }
}

// unsmoothed qxx, qyy, qxy of every node from q ([nlon][nlat] throughout)
__global__ void __launch_bounds__(kThreads) diag_q2_kernel(DiagArgs a) {
  const int64_t n = (int64_t)a.g.nlon * a.g.nlat, total = n * a.nlev;
  for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lev = id / n, r = id - lev * n;
    const int i = (int)(r / a.g.nlat), j = (int)(r - (int64_t)i * a.g.nlat);
    double* s = a.scratch + lev * 4 * n;
    const GlobalQ q{s, a.g.nlon, a.g.nlat};
    s[n + r] = bsd_grad_xx(q, a.g, i, j);
    s[2 * n + r] = bsd_grad_yy(q, a.g, i, j);
    s[3 * n + r] = bsd_grad_xy(q, a.g, i, j);
  }
}

unsigned blocks_for(int64_t work) {
  int64_t b = work < 1 ? 1 : work;
  if (b > 65535LL * 32) b = 65535LL * 32;
  return (unsigned)b;
}

int64_t tiles_of(const DiagArgs& a) {
  return (int64_t)((a.g.nlat + kTJ - 1) / kTJ) * ((a.g.nlon + kTI - 1) / kTI) * a.nlev;
}

template <uint32_t SEL>
void launch_out(const DiagArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((diag_tiled_kernel<false, SEL>), dim3(blocks_for(tiles_of(a))), dim3(kThreads), 0, st, a);
}

void launch_group(const DiagArgs& a, hipStream_t st) {
  const int64_t n = (int64_t)a.g.nlon * a.g.nlat;
  const unsigned nodes = blocks_for((n * a.nlev + kThreads - 1) / kThreads);
  if (a.select & kBsdNeedsQ) {
    hipLaunchKernelGGL((diag_tiled_kernel<true, 0u>), dim3(blocks_for(tiles_of(a))), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(diag_q2_kernel, dim3(nodes), dim3(kThreads), 0, st, a);
  }
  // select is uniform: the kernel is specialised for {betam, KS}, and any other
  // mask branches on it.  (Specialised for all 23 planes the kernel needs 126
  // VGPRs and spills 120 B a lane; branching, it needs 99 and spills nothing.)
  if (a.select == kBsdBetaKs)
    launch_out<kBsdBetaKs>(a, st);
  else
    launch_out<0u>(a, st);
}

bool overlap(const void* p, int64_t pbytes, const void* q, int64_t qbytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)qbytes && b < a + (uintptr_t)pbytes;
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_bs_diag(int32_t nlon, int32_t nlat, int32_t nlev, const float* d_u, const float* d_v,
                                    const double* d_trig, double dx, double dy, uint32_t select, double* d_out,
                                    double* d_scratch, int32_t scratch_levels, void* stream) {
  // (every check before the first HIP call)
  if (nlon < 3 || nlat < 4) return fail(RWRT_ERR_ARG, "rwrt_bs_diag: needs nlon >= 3 and nlat >= 4%s", "");
  if (nlev < 0) return fail(RWRT_ERR_ARG, "rwrt_bs_diag: nlev must not be negative%s", "");
  if (select == 0) return fail(RWRT_ERR_ARG, "rwrt_bs_diag: select names no plane%s", "");
  if (select & ~kBsdAll) return fail(RWRT_ERR_ARG, "rwrt_bs_diag: select has bits at or above RWRT_NDIAG%s", "");
  if (!d_u) return fail(RWRT_ERR_ARG, "rwrt_bs_diag: d_u is NULL%s", "");
  if (!d_v) return fail(RWRT_ERR_ARG, "rwrt_bs_diag: d_v is NULL%s", "");
  if (!d_trig) return fail(RWRT_ERR_ARG, "rwrt_bs_diag: d_trig is NULL%s", "");
  if (!d_out) return fail(RWRT_ERR_ARG, "rwrt_bs_diag: d_out is NULL%s", "");
  const bool needs_q = (select & kBsdNeedsQ) != 0;
  if (needs_q && !d_scratch)
    return fail(RWRT_ERR_ARG, "rwrt_bs_diag: d_scratch is NULL and a plane derived from q is selected%s", "");
  if (needs_q && scratch_levels < 1) return fail(RWRT_ERR_ARG, "rwrt_bs_diag: scratch_levels must be at least 1%s", "");
  const int nsel = __builtin_popcount(select);
  const int64_t n = (int64_t)nlon * nlat;
  const int64_t in_bytes = n * nlev * (int64_t)sizeof(float), out_bytes = n * nlev * nsel * (int64_t)sizeof(double);
  if (nlev > 0 && (overlap(d_out, out_bytes, d_u, in_bytes) || overlap(d_out, out_bytes, d_v, in_bytes) ||
                   overlap(d_out, out_bytes, d_trig, 3 * (int64_t)nlat * (int64_t)sizeof(double))))
    return fail(RWRT_ERR_ARG, "rwrt_bs_diag: d_out overlaps an input%s", "");
  if (nlev > 0 && needs_q) {
    const int64_t sl = scratch_levels < nlev ? scratch_levels : nlev;
    const int64_t sbytes = 4 * n * sl * (int64_t)sizeof(double);
    if (overlap(d_scratch, sbytes, d_out, out_bytes) || overlap(d_scratch, sbytes, d_u, in_bytes) ||
        overlap(d_scratch, sbytes, d_v, in_bytes) ||
        overlap(d_scratch, sbytes, d_trig, 3 * (int64_t)nlat * (int64_t)sizeof(double)))
      return fail(RWRT_ERR_ARG, "rwrt_bs_diag: d_scratch overlaps d_out or an input%s", "");
  }
  if (nlev == 0) return RWRT_OK;
  hipStream_t st = (hipStream_t)stream;
  DiagArgs a{bsd_geom(nlon, nlat, dx, dy), nlev, select, nsel, d_u, d_v, d_trig, needs_q ? d_scratch : nullptr, d_out};
  if (!needs_q) {
    launch_group(a, st);                       // no scratch: every level in one launch
    return check_launch("bs_diag kernel");
  }
  for (int64_t lev0 = 0; lev0 < nlev; lev0 += scratch_levels) {
    DiagArgs b = a;
    b.nlev = (int32_t)(nlev - lev0 < scratch_levels ? nlev - lev0 : scratch_levels);
    b.u = d_u + lev0 * n;
    b.v = d_v + lev0 * n;
    b.out = d_out + lev0 * nsel * n;
    launch_group(b, st);
    if (rwrt_status s = check_launch("bs_diag kernels")) return s;
  }
  return RWRT_OK;
}
