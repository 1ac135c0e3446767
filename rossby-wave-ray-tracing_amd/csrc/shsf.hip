// shsf.hip -- rwrt_sh_filter (ABI 5, additive): triangular spherical-harmonic
// truncation of u, v on the device, the reference's SHSF.py (NCL's
// shaec -> tri_trunc -> shsec) on the project's own pole-to-pole grid.
//
// A fifth translation unit, linked into librwrt.so next to rwrt.hip,
// density.hip, summary.hip and wn_map.hip, so that no other code object is
// touched by it.  The definition is shsf.reference_filter (NumPy); the weights
// and the Legendre recurrence are csrc/shsf_legendre.h.
//
// Four kernels, all fp64, the batch of fields a grid dimension:
//   sh_forward_dft_kernel   F_m(j) = sum_i f(j, i) exp(-2 pi i m i / nlon), m < M = min(T, nlon/2 - 1) + 1;
//                           a block builds the twiddles once in LDS and walks rows
//   sh_analysis_kernel      one block per (field, m): a_lm = sum_j w_j p_lm(x_j) F_m(j); a thread per latitude
//                           runs the recurrence, each degree is reduced across the wave by shuffles and
//                           accumulated per wave in LDS, the four waves are added in a fixed order
//   sh_synthesis_kernel     one block per (field, m, 256 latitudes): G_m(j) = sum_l a_lm p_lm(x_j), l ascending
//   sh_inverse_dft_kernel   f(j, i) = (G_0 + 2 sum_{m>=1} Re(G_m exp(2 pi i m i / nlon))) / nlon
// No atomics: every sum has one order, so a call's output is the same bits
// every time, and a field's result does not depend on the batch it is in.
// The inverse transform, sh_twiddles, sh_factors, sh_wave_sum, overlap and
// allow_lds are csrc/shsf_dft.h, shared with csrc/helmholtz.hip.
#include "shsf_dft.h"

namespace rwrt {
namespace {

// in [nfield][nlat][nlon] float32 -> F [nfield][M][nlat][2].  A row's sum over
// longitude is split into S segments of len points, each summed in order, and
// the segments are added in order.
__global__ void __launch_bounds__(kShThreads)
sh_forward_dft_kernel(int32_t nlon, int32_t nlat, int32_t M, int32_t S, int32_t len, const float* __restrict__ in,
                      double* __restrict__ F) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* twc = reinterpret_cast<double*>(smem);
  double* tws = twc + nlon;
  double* row = tws + nlon;
  double* part = row + nlon;
  const int64_t field = blockIdx.y;
  sh_twiddles(nlon, twc, tws);
  for (int32_t r = blockIdx.x; r < nlat; r += gridDim.x) {
    __syncthreads();   // the twiddles are there; the last row's segments were read
    const float* src = in + (field * nlat + r) * nlon;
    for (int32_t i = threadIdx.x; i < nlon; i += kShThreads) row[i] = (double)src[i];
    __syncthreads();
    for (int32_t item = threadIdx.x; item < M * S; item += kShThreads) {
      const int32_t m = item % M, s = item / M;
      const int32_t i0 = s * len, i1 = (i0 + len < nlon) ? i0 + len : nlon;
      int32_t k = (int32_t)(((int64_t)m * i0) % nlon);
      double re = 0.0, im = 0.0;
      for (int32_t i = i0; i < i1; ++i) {
        const double v = row[i];
        re = re + v * twc[k];
        im = im - v * tws[k];
        k += m;
        if (k >= nlon) k -= nlon;
      }
      part[2 * item] = re;
      part[2 * item + 1] = im;
    }
    __syncthreads();
    for (int32_t m = threadIdx.x; m < M; m += kShThreads) {
      double re = part[2 * m], im = part[2 * m + 1];
      for (int32_t s = 1; s < S; ++s) {
        re = re + part[2 * (s * M + m)];
        im = im + part[2 * (s * M + m) + 1];
      }
      double* dst = F + ((field * M + m) * nlat + r) * 2;
      dst[0] = re;
      dst[1] = im;
    }
  }
}

// F [nfield][M][nlat][2] -> spec [nfield][T+1][T+1][2] (a_lm at [l][m], zero
// for l < m and for m >= M).  One block per (m, field).
__global__ void __launch_bounds__(kShThreads)
sh_analysis_kernel(int32_t nlat, int32_t T, int32_t M, const double* __restrict__ w, const double* __restrict__ xc,
                   const double* __restrict__ F, double* __restrict__ spec) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int32_t m = blockIdx.x;
  const int64_t field = blockIdx.y;
  const int32_t n1 = T + 1;
  double* out = spec + field * n1 * n1 * 2;
  if (m >= M) {   // (an order the longitude grid cannot carry: dropped)
    for (int32_t l = threadIdx.x; l <= T; l += kShThreads) {
      out[((int64_t)l * n1 + m) * 2] = 0.0;
      out[((int64_t)l * n1 + m) * 2 + 1] = 0.0;
    }
    return;
  }
  double* diag = reinterpret_cast<double*>(smem);
  double* ra = diag + n1;
  double* rb = ra + n1;
  double* acc = rb + n1;   // [T - m + 1][kShWaves][2]
  const int32_t L = T - m + 1;
  sh_factors(m, T, diag, ra, rb);
  for (int32_t e = threadIdx.x; e < L * kShWaves * 2; e += kShThreads) acc[e] = 0.0;
  __syncthreads();
  const int32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double* Fm = F + (field * M + m) * nlat * 2;
  for (int32_t j0 = 0; j0 < nlat; j0 += kShThreads) {
    const int32_t j = j0 + threadIdx.x;
    const bool in = j < nlat;
    // (a lane past the last latitude adds +0.0 to every sum)
    const double x = in ? xc[j] : 0.0, c = in ? xc[nlat + j] : 0.0, wj = in ? w[j] : 0.0;
    const double wre = wj * (in ? Fm[2 * j] : 0.0), wim = wj * (in ? Fm[2 * j + 1] : 0.0);
    const ShNode nd = sh_make_node(x, c);
    double p2 = sqrt(0.5);
    for (int32_t k = 0; k < m; ++k) p2 = sh_diag_step(diag[k], c, p2);
    double p1 = 0.0;
    for (int32_t d = 0; d < L; ++d) {
      double p;
      if (d == 0) {
        p = p2;
      } else if (d == 1) {
        p = p1 = sh_first_step(sh_first_factor(m), nd, p2);
      } else {
        p = sh_rec_step(ra[d], rb[d], nd, p1, p2);
        p2 = p1;
        p1 = p;
      }
      const double re = sh_wave_sum(p * wre), im = sh_wave_sum(p * wim);
      if (lane == 0) {   // (this lane alone owns the wave's accumulators)
        double* a = acc + (d * kShWaves + wave) * 2;
        a[0] = a[0] + re;
        a[1] = a[1] + im;
      }
    }
  }
  __syncthreads();
  for (int32_t l = threadIdx.x; l <= T; l += kShThreads) {
    double re = 0.0, im = 0.0;
    if (l >= m) {
      const double* a = acc + (l - m) * kShWaves * 2;
      re = ((a[0] + a[2]) + a[4]) + a[6];
      im = ((a[1] + a[3]) + a[5]) + a[7];
    }
    out[((int64_t)l * n1 + m) * 2] = re;
    out[((int64_t)l * n1 + m) * 2 + 1] = im;
  }
}

// spec -> G [nfield][M][nlat][2].  One block per (m, field, 256 latitudes).
__global__ void __launch_bounds__(kShThreads)
sh_synthesis_kernel(int32_t nlat, int32_t T, int32_t M, const double* __restrict__ xc,
                    const double* __restrict__ spec, double* __restrict__ G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int32_t m = blockIdx.x;
  const int64_t field = blockIdx.y;
  const int32_t n1 = T + 1, L = T - m + 1;
  double* diag = reinterpret_cast<double*>(smem);
  double* ra = diag + n1;
  double* rb = ra + n1;
  double* a = rb + n1;   // [L][2]
  sh_factors(m, T, diag, ra, rb);
  const double* src = spec + field * n1 * n1 * 2;
  for (int32_t d = threadIdx.x; d < L; d += kShThreads) {
    a[2 * d] = src[((int64_t)(m + d) * n1 + m) * 2];
    a[2 * d + 1] = src[((int64_t)(m + d) * n1 + m) * 2 + 1];
  }
  __syncthreads();
  const int32_t j = blockIdx.z * kShThreads + threadIdx.x;
  if (j >= nlat) return;
  const double x = xc[j], c = xc[nlat + j];
  const ShNode nd = sh_make_node(x, c);
  double p2 = sqrt(0.5);
  for (int32_t k = 0; k < m; ++k) p2 = sh_diag_step(diag[k], c, p2);
  double re = a[0] * p2, im = a[1] * p2;
  if (L > 1) {
    double p1 = sh_first_step(sh_first_factor(m), nd, p2);
    re = re + a[2] * p1;
    im = im + a[3] * p1;
    for (int32_t d = 2; d < L; ++d) {
      const double p = sh_rec_step(ra[d], rb[d], nd, p1, p2);
      re = re + a[2 * d] * p;
      im = im + a[2 * d + 1] * p;
      p2 = p1;
      p1 = p;
    }
  }
  double* dst = G + ((field * M + m) * nlat + j) * 2;
  dst[0] = re;
  dst[1] = im;
}


}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_sh_filter(int32_t nlon, int32_t nlat, int32_t nfield, int32_t trunc, const float* d_in,
                                      const double* d_w, const double* d_x, double* d_spec, float* d_out32,
                                      double* d_out64, double* d_scratch, void* stream) {
  // (every check before the first HIP call)
  if (nlat < 3 || nlat % 2 == 0)
    return fail(RWRT_ERR_ARG, "rwrt_sh_filter: nlat must be odd and at least 3 (both poles are nodes)%s", "");
  if (nlon < 2 || nlon % 2 != 0) return fail(RWRT_ERR_ARG, "rwrt_sh_filter: nlon must be even and at least 2%s", "");
  if (trunc < 0 || trunc > (nlat - 1) / 2)
    return fail(RWRT_ERR_ARG, "rwrt_sh_filter: trunc must be 0..(nlat-1)/2 (the quadrature's exact range)%s", "");
  if (nfield < 0 || nfield > 65535) return fail(RWRT_ERR_ARG, "rwrt_sh_filter: nfield must be 0..65535%s", "");
  const size_t npoint = (size_t)nfield * nlat * nlon;
  if (overlap(d_in, npoint * 4, d_out32, npoint * 4) || overlap(d_in, npoint * 4, d_out64, npoint * 8) ||
      overlap(d_out32, npoint * 4, d_out64, npoint * 8))
    return fail(RWRT_ERR_ARG, "rwrt_sh_filter: d_in, d_out32 and d_out64 must not alias each other%s", "");
  if (nfield == 0) return RWRT_OK;
  if (!d_in || !d_w || !d_x || !d_spec || !d_scratch)
    return fail(RWRT_ERR_ARG, "rwrt_sh_filter: NULL buffer (d_in, d_w, d_x, d_spec, d_scratch)%s", "");
  const int32_t T = trunc, n1 = T + 1;
  const int32_t M = (T < nlon / 2 - 1 ? T : nlon / 2 - 1) + 1;   // orders 0..min(T, nlon/2 - 1); nlon == 2: order 0
  // the forward sum of a row: S segments per order, at least 16 points each
  int32_t S = kShThreads / M < 1 ? 1 : kShThreads / M;
  if (S > nlon / 16) S = nlon / 16 < 1 ? 1 : nlon / 16;
  const int32_t len = (nlon + S - 1) / S;
  const size_t lds_fwd = ((size_t)3 * nlon + (size_t)2 * M * S) * sizeof(double);
  const size_t lds_inv = ((size_t)2 * nlon + (size_t)2 * M) * sizeof(double);
  const size_t lds_ana = ((size_t)3 * n1 + (size_t)n1 * kShWaves * 2) * sizeof(double);
  const size_t lds_syn = (size_t)5 * n1 * sizeof(double);
  if (lds_fwd > kShLdsMax || lds_inv > kShLdsMax)
    return fail(RWRT_ERR_ARG, "rwrt_sh_filter: nlon is too large for a row and its twiddles in LDS%s", "");
  if (lds_ana > kShLdsDefault || lds_syn > kShLdsDefault)
    return fail(RWRT_ERR_ARG, "rwrt_sh_filter: trunc is too large for one order's sums in LDS%s", "");
  hipStream_t st = (hipStream_t)stream;
  if (rwrt_status s = allow_lds(sh_forward_dft_kernel, lds_fwd, "hipFuncSetAttribute(sh_forward_dft_kernel)")) return s;
  if (rwrt_status s = allow_lds(sh_inverse_dft_kernel, lds_inv, "hipFuncSetAttribute(sh_inverse_dft_kernel)")) return s;
  double* d_F = d_scratch;
  double* d_G = d_scratch + (size_t)nfield * n1 * nlat * 2;
  // a block of the two transforms walks several rows, so that its twiddles are built once for all of them
  int32_t rows = (2048 + nfield - 1) / nfield;
  if (rows > nlat) rows = nlat;
  hipLaunchKernelGGL(sh_forward_dft_kernel, dim3(rows, nfield), dim3(kShThreads), lds_fwd, st, nlon, nlat, M, S, len,
                     d_in, d_F);
  if (rwrt_status s = check_launch("sh_forward_dft_kernel")) return s;
  hipLaunchKernelGGL(sh_analysis_kernel, dim3(n1, nfield), dim3(kShThreads), lds_ana, st, nlat, T, M, d_w, d_x, d_F,
                     d_spec);
  if (rwrt_status s = check_launch("sh_analysis_kernel")) return s;
  if (!d_out32 && !d_out64) return RWRT_OK;   // coefficients only
  hipLaunchKernelGGL(sh_synthesis_kernel, dim3(M, nfield, (nlat + kShThreads - 1) / kShThreads), dim3(kShThreads),
                     lds_syn, st, nlat, T, M, d_x, d_spec, d_G);
  if (rwrt_status s = check_launch("sh_synthesis_kernel")) return s;
  hipLaunchKernelGGL(sh_inverse_dft_kernel, dim3(rows, nfield), dim3(kShThreads), lds_inv, st, nlon, nlat, M, d_G,
                     d_out32, d_out64);
  return check_launch("sh_inverse_dft_kernel");
}
