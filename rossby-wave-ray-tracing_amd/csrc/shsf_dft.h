// shsf_dft.h -- the inverse longitude transform of the spherical-harmonic
// kernels and what their launches share, included by csrc/shsf.hip
// (rwrt_sh_filter) and csrc/helmholtz.hip (rwrt_sh_helmholtz): each
// translation unit gets a kernel of its own from it, in its own code object.
//   sh_inverse_dft_kernel   f(j, i) = (G_0 + 2 sum_{m>=1} Re(G_m exp(2 pi i m i / nlon))) / nlon;
//                           a block builds the twiddles once in LDS and walks rows
// and the twiddles, the recurrence's latitude-independent factors in LDS, the
// wave sum, the alias check and the LDS attribute of a launch.
#ifndef RWRT_SHSF_DFT_H
#define RWRT_SHSF_DFT_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rwrt.h"
#include "abi_host.h"
#include "shsf_legendre.h"

namespace rwrt {
namespace {

constexpr int kShThreads = 256;
constexpr int kShWaves = kShThreads / 64;
constexpr size_t kShLdsDefault = 64 * 1024;   // a launch may ask for this much without an attribute
constexpr size_t kShLdsMax = 160 * 1024;      // LDS of a gfx950 compute unit

// cos and sin of 2 pi i / nlon, i < nlon, into LDS (the caller synchronises).
__device__ inline void sh_twiddles(int32_t nlon, double* twc, double* tws) {
  for (int32_t i = threadIdx.x; i < nlon; i += kShThreads) {
    double s, c;
    sincospi((2.0 * i) / nlon, &s, &c);
    twc[i] = c;
    tws[i] = s;
  }
}

// The factors of the recurrence of order m that do not depend on latitude,
// into LDS: diag[k - 1], k = 1..m; ra, rb[l - m], l = m + 2..T.
__device__ inline void sh_factors(int32_t m, int32_t T, double* diag, double* ra, double* rb) {
  for (int32_t k = 1 + threadIdx.x; k <= m; k += kShThreads) diag[k - 1] = sh_diag_factor(k);
  for (int32_t l = m + 2 + threadIdx.x; l <= T; l += kShThreads) {
    ra[l - m] = sh_rec_a(l, m);
    rb[l - m] = sh_rec_b(l, m);
  }
}

__device__ inline double sh_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
  return v;   // (lane 0 holds the wave's sum)
}

// G [nfield][M][nlat][2] -> out32 and/or out64 [nfield][nlat][nlon].
__global__ void __launch_bounds__(kShThreads)
sh_inverse_dft_kernel(int32_t nlon, int32_t nlat, int32_t M, const double* __restrict__ G, float* __restrict__ out32,
                      double* __restrict__ out64) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* twc = reinterpret_cast<double*>(smem);
  double* tws = twc + nlon;
  double* g = tws + nlon;   // [M][2]
  const int64_t field = blockIdx.y;
  sh_twiddles(nlon, twc, tws);
  for (int32_t r = blockIdx.x; r < nlat; r += gridDim.x) {
    __syncthreads();   // the twiddles are there; the last row's orders were read
    for (int32_t m = threadIdx.x; m < M; m += kShThreads) {
      const double* src = G + ((field * M + m) * nlat + r) * 2;
      g[2 * m] = src[0];
      g[2 * m + 1] = src[1];
    }
    __syncthreads();
    const int64_t base = (field * nlat + r) * nlon;
    for (int32_t i = threadIdx.x; i < nlon; i += kShThreads) {
      double acc = 0.0;
      int32_t k = 0;
      for (int32_t m = 1; m < M; ++m) {
        k += i;
        if (k >= nlon) k -= nlon;
        acc = acc + (g[2 * m] * twc[k] - g[2 * m + 1] * tws[k]);
      }
      const double v = (g[0] + 2.0 * acc) / nlon;
      if (out64) out64[base + i] = v;
      if (out32) out32[base + i] = (float)v;
    }
  }
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || na == 0 || nb == 0) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

// A launch's dynamic LDS: above the default limit the kernel is told so first.
template <typename K>
rwrt_status allow_lds(K kernel, size_t bytes, const char* what) {
  if (bytes <= kShLdsDefault) return RWRT_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)bytes) != hipSuccess)
    return check_launch(what);
  return RWRT_OK;
}
}  // namespace
}  // namespace rwrt

#endif
