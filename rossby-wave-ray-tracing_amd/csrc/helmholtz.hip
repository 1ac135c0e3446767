// helmholtz.hip -- rwrt_sh_helmholtz and rwrt_sh_rws (ABI 5, additive): the
// Helmholtz decomposition of a wind (u, v) on the filter's pole-to-pole grid
// -- vorticity and divergence, streamfunction and velocity potential,
// rotational and divergent wind, the vorticity gradient -- and the pointwise
// Rossby-wave source of Sardeshmukh & Hoskins (1988) from such planes.
//
// A fourteenth translation unit with a code object of its own.  The
// definition is helmholtz.reference_helmholtz / reference_rws (NumPy); the
// vector basis q_lm, b_lm, d_lm is csrc/sh_vector.h, the weights and p_lm are
// csrc/shsf_legendre.h, the inverse longitude transform is csrc/shsf_dft.h
// (the filter's).
//
// Kernels, all fp64, a pair (u, v) a grid dimension:
//   shv_forward_dft_kernel  the filter's forward transform on the 2 npair fields u and v in one launch, with
//                           the twiddles as the definition rounds them
//   shv_analysis_kernel     one block per (pair, m), a thread per latitude: runs the q recurrence to T + 1,
//                           forms b_lm, d_lm on the fly; the four real sums of a degree (vrt, div, each
//                           complex) are reduced across the wave by shuffles, accumulated per wave in LDS,
//                           and the four waves are added in a fixed order
//   shv_synthesis_kernel    one block per (pair, m, 256 latitudes): the coefficients of order m in LDS (psi,
//                           chi formed on load), p and q recurrences, l ascending, the planes asked for only
//   sh_inverse_dft_kernel   (shsf_dft.h) on the npair * nplane spectra
//   sh_rws_kernel           pointwise S(A, B; planetary)
// No atomics: every sum has one order, so a call's output is the same bits
// every time, and a pair's result does not depend on the batch it is in.
#include "shsf_dft.h"
#include "sh_vector.h"

namespace rwrt {
namespace {

constexpr uint32_t kShvAll = (1u << RWRT_SHV_NPLANE) - 1u;

// The latitude-independent factors of one block, in LDS.  The p column has
// order m, the q column order mq = max(m, 1) (for m = 0 it carries d_l0).
struct ShvTables {
  double *diag;    // [k - 1], k = 1..max(m, 1)
  double *rap, *rbp;   // [l - m], l = m + 2..T
  double *raq, *rbq;   // [l - mq], l = mq + 2..T + 1
  double *lower, *upper;   // [l], l = mq..T: the factors of d_lm (m = 0: lower is sqrt(l (l+1)))
  double* end;
};

__device__ inline ShvTables shv_tables(char* smem, int32_t T) {
  ShvTables t;
  const int32_t n = T + 2;
  t.diag = reinterpret_cast<double*>(smem);
  t.rap = t.diag + n;
  t.rbp = t.rap + n;
  t.raq = t.rbp + n;
  t.rbq = t.raq + n;
  t.lower = t.rbq + n;
  t.upper = t.lower + n;
  t.end = t.upper + n;
  return t;
}
constexpr int kShvTableRows = 7;   // (T + 2 doubles each)

// (the caller synchronises)
__device__ inline void shv_fill_tables(const ShvTables& t, int32_t m, int32_t T, bool with_p) {
  const int32_t mq = m < 1 ? 1 : m;
  for (int32_t k = 1 + threadIdx.x; k <= mq; k += kShThreads) t.diag[k - 1] = sh_diag_factor(k);
  if (with_p)
    for (int32_t l = m + 2 + threadIdx.x; l <= T; l += kShThreads) {
      t.rap[l - m] = sh_rec_a(l, m);
      t.rbp[l - m] = sh_rec_b(l, m);
    }
  for (int32_t l = mq + 2 + threadIdx.x; l <= T + 1; l += kShThreads) {
    t.raq[l - mq] = sh_rec_a(l, mq);
    t.rbq[l - mq] = sh_rec_b(l, mq);
  }
  for (int32_t l = mq + threadIdx.x; l <= T; l += kShThreads) {
    t.lower[l] = m == 0 ? shv_d_zonal_factor(l) : shv_d_lower(l, m);
    t.upper[l] = m == 0 ? 0.0 : shv_d_upper(l, m);
  }
}

// q_{mq,mq} with the diagonal's factors from LDS (shv_qmm's operations).
__device__ inline ShvColumn shv_start_lds(const ShvTables& t, int32_t mq, const ShNode& nd) {
  ShvColumn k;
  double q = shv_q11();
  for (int32_t i = 2; i <= mq; ++i) q = sh_diag_step(t.diag[i - 1], nd.c, q);
  k.qm = 0.0;
  k.q0 = q;
  k.qp = sh_first_step(sh_first_factor(mq), nd, q);
  return k;
}

// b_lm and d_lm at the column's degree l.
__device__ inline void shv_bd(const ShvTables& t, int32_t m, int32_t l, const ShNode& nd, const ShvColumn& k,
                              double* b, double* d) {
  if (m == 0) {
    *b = 0.0;
    *d = shv_d_zonal(t.lower[l], nd.c, k.q0);
  } else {
    *b = shv_b(m, k.q0);
    *d = shv_d(t.lower[l], t.upper[l], k.qm, k.qp);
  }
}

// The forward transform's twiddles, as the definition takes them (shsf._twiddles:
// ang = (2 k) / nlon, cos(pi * ang), sin(pi * ang) -- the product is rounded
// before the cosine).  The analysis multiplies what the transform's rounding
// leaves in an order by m (b_lm = m q_lm), so the divergence of a nearly
// non-divergent wind sees the twiddles' last bits; sincospi(ang), the inverse
// transform's and the filter's, differs from the definition's by up to 5e-16.
__device__ inline void shv_twiddles(int32_t nlon, double* twc, double* tws) {
  for (int32_t i = threadIdx.x; i < nlon; i += kShThreads) {
    const double ang = (2.0 * i) / nlon;
    double s, c;
    sincos(kShPi * ang, &s, &c);
    twc[i] = c;
    tws[i] = s;
  }
}

// u, v [npair][nlat][nlon] float32 -> F [2 npair][M][nlat][2], u's transforms,
// then v's, in one launch: F_m(j) = sum_i f(j, i) exp(-2 pi i m i / nlon).  The
// filter's forward transform (csrc/shsf.hip) with two inputs and the twiddles
// above: a row's sum over longitude is split into S segments of len points,
// each summed in order, and the segments are added in order.
__global__ void __launch_bounds__(kShThreads)
shv_forward_dft_kernel(int32_t nlon, int32_t nlat, int32_t M, int32_t S, int32_t len, int32_t npair,
                       const float* __restrict__ u, const float* __restrict__ v, double* __restrict__ F) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* twc = reinterpret_cast<double*>(smem);
  double* tws = twc + nlon;
  double* row = tws + nlon;
  double* part = row + nlon;
  const int64_t field = blockIdx.y;   // < 2 npair
  const float* in = field < npair ? u + field * nlat * nlon : v + (field - npair) * nlat * nlon;
  shv_twiddles(nlon, twc, tws);
  for (int32_t r = blockIdx.x; r < nlat; r += gridDim.x) {
    __syncthreads();   // the twiddles are there; the last row's segments were read
    const float* src = in + (int64_t)r * nlon;
    for (int32_t i = threadIdx.x; i < nlon; i += kShThreads) row[i] = (double)src[i];
    __syncthreads();
    for (int32_t item = threadIdx.x; item < M * S; item += kShThreads) {
      const int32_t m = item % M, s = item / M;
      const int32_t i0 = s * len, i1 = (i0 + len < nlon) ? i0 + len : nlon;
      int32_t k = (int32_t)(((int64_t)m * i0) % nlon);
      double re = 0.0, im = 0.0;
      for (int32_t i = i0; i < i1; ++i) {
        const double f = row[i];
        re = re + f * twc[k];
        im = im - f * tws[k];
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

// F [2 npair][M][nlat][2] (u's transforms, then v's) -> spec [npair][2][T+1][T+1][2]:
// vrt_lm, div_lm at [l][m], zero for l < m, l = 0 and m >= M.  One block per (m, pair).
__global__ void __launch_bounds__(kShThreads)
shv_analysis_kernel(int32_t nlat, int32_t T, int32_t M, int32_t npair, const double* __restrict__ w,
                    const double* __restrict__ xc, const double* __restrict__ F, double* __restrict__ spec) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int32_t m = blockIdx.x;
  const int64_t pair = blockIdx.y;
  const int32_t n1 = T + 1;
  double* vrt = spec + pair * 2 * n1 * n1 * 2;
  double* div = vrt + (int64_t)n1 * n1 * 2;
  if (m >= M) {   // (an order the longitude grid cannot carry: dropped)
    for (int32_t l = threadIdx.x; l <= T; l += kShThreads) {
      const int64_t e = ((int64_t)l * n1 + m) * 2;
      vrt[e] = vrt[e + 1] = div[e] = div[e + 1] = 0.0;
    }
    return;
  }
  const int32_t mq = m < 1 ? 1 : m;
  const int32_t L = T - mq + 1;   // degrees mq..T
  const ShvTables t = shv_tables(smem, T);
  double* acc = t.end;   // [L][kShWaves][4]
  shv_fill_tables(t, m, T, false);
  for (int32_t e = threadIdx.x; e < L * kShWaves * 4; e += kShThreads) acc[e] = 0.0;
  __syncthreads();
  const int32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double* Um = F + (pair * M + m) * nlat * 2;
  const double* Vm = F + ((npair + pair) * M + m) * nlat * 2;
  for (int32_t j0 = 0; j0 < nlat; j0 += kShThreads) {
    const int32_t j = j0 + threadIdx.x;
    const bool in = j < nlat;
    // (a lane past the last latitude adds +-0.0 to every sum)
    const double x = in ? xc[j] : 0.0, c = in ? xc[nlat + j] : 0.0, wj = in ? w[j] : 0.0;
    const double wur = wj * (in ? Um[2 * j] : 0.0), wui = wj * (in ? Um[2 * j + 1] : 0.0);
    const double wvr = wj * (in ? Vm[2 * j] : 0.0), wvi = wj * (in ? Vm[2 * j + 1] : 0.0);
    const ShNode nd = sh_make_node(x, c);
    ShvColumn k = shv_start_lds(t, mq, nd);
    for (int32_t l = mq; l <= T; ++l) {
      double b, d;
      shv_bd(t, m, l, nd, k, &b, &d);
      // vrt += w (i V b + U d), div += w (i U b - V d)
      const double s0 = sh_wave_sum(wur * d - wvi * b), s1 = sh_wave_sum(wui * d + wvr * b);
      const double s2 = sh_wave_sum(-(wui * b) - wvr * d), s3 = sh_wave_sum(wur * b - wvi * d);
      if (lane == 0) {   // (this lane alone owns the wave's accumulators)
        double* a = acc + ((l - mq) * kShWaves + wave) * 4;
        a[0] = a[0] + s0;
        a[1] = a[1] + s1;
        a[2] = a[2] + s2;
        a[3] = a[3] + s3;
      }
      if (l < T) shv_advance(k, t.raq[l + 2 - mq], t.rbq[l + 2 - mq], nd);
    }
  }
  __syncthreads();
  for (int32_t l = threadIdx.x; l <= T; l += kShThreads) {
    double r[4] = {0.0, 0.0, 0.0, 0.0};
    if (l >= mq) {
      const double* a = acc + (l - mq) * kShWaves * 4;
#pragma unroll
      for (int32_t e = 0; e < 4; ++e) r[e] = (((a[e] + a[4 + e]) + a[8 + e]) + a[12 + e]) / kShvREarth;
    }
    const int64_t e = ((int64_t)l * n1 + m) * 2;
    vrt[e] = r[0];
    vrt[e + 1] = r[1];
    div[e] = r[2];
    div[e + 1] = r[3];
  }
}

struct ShvSum {
  double re, im;
};
__device__ inline void shv_add(ShvSum& s, const double* coef, double fn) {
  s.re = s.re + coef[0] * fn;
  s.im = s.im + coef[1] * fn;
}
// G = fac S for the four factors of the definition: 1, -1/a, i/a, 1/a.
enum { kFacOne, kFacMinusInvA, kFacIInvA, kFacInvA };
__device__ inline void shv_store(double* G, int64_t field, int32_t M, int32_t m, int32_t nlat, int32_t j,
                                 const ShvSum& s, int fac) {
  double* dst = G + ((field * M + m) * nlat + j) * 2;
  double re = s.re, im = s.im;
  if (fac == kFacMinusInvA) {
    re = -(s.re / kShvREarth);
    im = -(s.im / kShvREarth);
  } else if (fac == kFacIInvA) {
    re = -(s.im / kShvREarth);
    im = s.re / kShvREarth;
  } else if (fac == kFacInvA) {
    re = s.re / kShvREarth;
    im = s.im / kShvREarth;
  }
  dst[0] = re;
  dst[1] = im;
}

// spec -> G [npair * nplane][M][nlat][2], the planes of `planes` in bit order;
// G2 (or NULL) [npair * 2][M][nlat][2]: u_rot, v_rot once more.  One block per
// (m, pair, 256 latitudes).
__global__ void __launch_bounds__(kShThreads)
shv_synthesis_kernel(int32_t nlat, int32_t T, int32_t M, uint32_t planes, int32_t nplane,
                     const double* __restrict__ xc, const double* __restrict__ spec, double* __restrict__ G,
                     double* __restrict__ G2) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int32_t m = blockIdx.x;
  const int64_t pair = blockIdx.y;
  const int32_t n1 = T + 1;
  const int32_t mq = m < 1 ? 1 : m;
  const ShvTables t = shv_tables(smem, T);
  double* cv = t.end;          // vrt_lm, [l][2], l <= T (zero below mq)
  double* cd = cv + 2 * n1;    // div_lm
  double* cp = cd + 2 * n1;    // psi_lm
  double* cc = cp + 2 * n1;    // chi_lm
  shv_fill_tables(t, m, T, true);
  const double* sv = spec + pair * 2 * n1 * n1 * 2;
  const double* sd = sv + (int64_t)n1 * n1 * 2;
  for (int32_t e = threadIdx.x; e < 2 * n1; e += kShThreads) {
    const int32_t l = e >> 1, part = e & 1;
    const bool on = l >= mq;
    const double v = on ? sv[((int64_t)l * n1 + m) * 2 + part] : 0.0;
    const double d = on ? sd[((int64_t)l * n1 + m) * 2 + part] : 0.0;
    cv[e] = v;
    cd[e] = d;
    cp[e] = on ? shv_potential(l, v) : 0.0;
    cc[e] = on ? shv_potential(l, d) : 0.0;
  }
  __syncthreads();
  const int32_t j = blockIdx.z * kShThreads + threadIdx.x;
  if (j >= nlat) return;
  const double x = xc[j], c = xc[nlat + j];
  const ShNode nd = sh_make_node(x, c);
  const bool any_p = (planes & (RWRT_SHV_VRT | RWRT_SHV_DIV | RWRT_SHV_PSI | RWRT_SHV_CHI)) != 0;
  const bool any_q = (planes & ~(uint32_t)(RWRT_SHV_VRT | RWRT_SHV_DIV | RWRT_SHV_PSI | RWRT_SHV_CHI)) != 0;
  ShvSum s_vrt = {0.0, 0.0}, s_div = {0.0, 0.0}, s_psi = {0.0, 0.0}, s_chi = {0.0, 0.0};
  ShvSum s_urot = {0.0, 0.0}, s_vrot = {0.0, 0.0}, s_udiv = {0.0, 0.0}, s_vdiv = {0.0, 0.0};
  ShvSum s_vrtx = {0.0, 0.0}, s_vrty = {0.0, 0.0};
  if (any_p) {
    // p_lm, l = m..T; the sums take l >= mq (every l = 0 coefficient is zero)
    double p2 = sqrt(0.5);
    for (int32_t k = 0; k < m; ++k) p2 = sh_diag_step(t.diag[k], c, p2);
    double p1 = 0.0;
    for (int32_t l = m; l <= T; ++l) {
      double p;
      if (l == m) {
        p = p2;
      } else if (l == m + 1) {
        p = p1 = sh_first_step(sh_first_factor(m), nd, p2);
      } else {
        p = sh_rec_step(t.rap[l - m], t.rbp[l - m], nd, p1, p2);
        p2 = p1;
        p1 = p;
      }
      if (l < mq) continue;
      if (planes & RWRT_SHV_VRT) shv_add(s_vrt, cv + 2 * l, p);
      if (planes & RWRT_SHV_DIV) shv_add(s_div, cd + 2 * l, p);
      if (planes & RWRT_SHV_PSI) shv_add(s_psi, cp + 2 * l, p);
      if (planes & RWRT_SHV_CHI) shv_add(s_chi, cc + 2 * l, p);
    }
  }
  if (any_q) {
    ShvColumn k = shv_start_lds(t, mq, nd);
    for (int32_t l = mq; l <= T; ++l) {
      double b, d;
      shv_bd(t, m, l, nd, k, &b, &d);
      if (planes & RWRT_SHV_UROT) shv_add(s_urot, cp + 2 * l, d);
      if (planes & RWRT_SHV_VROT) shv_add(s_vrot, cp + 2 * l, b);
      if (planes & RWRT_SHV_UDIV) shv_add(s_udiv, cc + 2 * l, b);
      if (planes & RWRT_SHV_VDIV) shv_add(s_vdiv, cc + 2 * l, d);
      if (planes & RWRT_SHV_VRTX) shv_add(s_vrtx, cv + 2 * l, b);
      if (planes & RWRT_SHV_VRTY) shv_add(s_vrty, cv + 2 * l, d);
      if (l < T) shv_advance(k, t.raq[l + 2 - mq], t.rbq[l + 2 - mq], nd);
    }
  }
  int64_t f = pair * nplane;
  if (planes & RWRT_SHV_VRT) shv_store(G, f++, M, m, nlat, j, s_vrt, kFacOne);
  if (planes & RWRT_SHV_DIV) shv_store(G, f++, M, m, nlat, j, s_div, kFacOne);
  if (planes & RWRT_SHV_PSI) shv_store(G, f++, M, m, nlat, j, s_psi, kFacOne);
  if (planes & RWRT_SHV_CHI) shv_store(G, f++, M, m, nlat, j, s_chi, kFacOne);
  if (planes & RWRT_SHV_UROT) shv_store(G, f++, M, m, nlat, j, s_urot, kFacMinusInvA);
  if (planes & RWRT_SHV_VROT) shv_store(G, f++, M, m, nlat, j, s_vrot, kFacIInvA);
  if (planes & RWRT_SHV_UDIV) shv_store(G, f++, M, m, nlat, j, s_udiv, kFacIInvA);
  if (planes & RWRT_SHV_VDIV) shv_store(G, f++, M, m, nlat, j, s_vdiv, kFacInvA);
  if (planes & RWRT_SHV_VRTX) shv_store(G, f++, M, m, nlat, j, s_vrtx, kFacIInvA);
  if (planes & RWRT_SHV_VRTY) shv_store(G, f++, M, m, nlat, j, s_vrty, kFacInvA);
  if (G2) {
    shv_store(G2, pair * 2, M, m, nlat, j, s_urot, kFacMinusInvA);
    shv_store(G2, pair * 2 + 1, M, m, nlat, j, s_vrot, kFacIInvA);
  }
}

// Six planes [nfield][nlat][nlon] -> S [nfield][nlat][nlon].
__global__ void __launch_bounds__(kShThreads)
sh_rws_kernel(int64_t n, int32_t nlon, int32_t nlat, int32_t planetary, const double* __restrict__ xc,
              const double* __restrict__ div_a, const double* __restrict__ udiv_a, const double* __restrict__ vdiv_a,
              const double* __restrict__ vrt_b, const double* __restrict__ vrtx_b, const double* __restrict__ vrty_b,
              double* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * kShThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kShThreads) {
    const int32_t j = (int32_t)((e / nlon) % nlat);
    out[e] = shv_rws(planetary, xc[j], xc[nlat + j], div_a[e], udiv_a[e], vdiv_a[e], vrt_b[e], vrtx_b[e], vrty_b[e]);
  }
}

int32_t popcount(uint32_t v) {
  int32_t n = 0;
  for (; v; v &= v - 1) ++n;
  return n;
}

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_sh_helmholtz(int32_t nlon, int32_t nlat, int32_t npair, int32_t trunc, uint32_t planes,
                                         const float* d_u, const float* d_v, const double* d_w, const double* d_x,
                                         double* d_spec, double* d_out64, float* d_rot32, double* d_scratch,
                                         void* stream) {
  // (every check before the first HIP call)
  if (nlat < 3 || nlat % 2 == 0)
    return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: nlat must be odd and at least 3 (both poles are nodes)%s", "");
  if (nlon < 2 || nlon % 2 != 0)
    return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: nlon must be even and at least 2%s", "");
  if (trunc < 1 || trunc > (nlat - 1) / 2)
    return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: trunc must be 1..(nlat-1)/2 (the quadrature's exact range)%s", "");
  if (planes & ~kShvAll) return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: planes has unknown bits%s", "");
  if (planes == 0) return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: planes is empty%s", "");
  const int32_t nplane = popcount(planes);
  if (npair < 0 || (int64_t)npair * (nplane > 2 ? nplane : 2) > 65535)
    return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: npair must be 0..65535 / max(2, planes asked for)%s", "");
  const uint32_t rot = RWRT_SHV_UROT | RWRT_SHV_VROT;
  if (d_rot32 && (planes & rot) != rot)
    return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: d_rot32 needs RWRT_SHV_UROT and RWRT_SHV_VROT in planes%s", "");
  if (!d_out64 && d_rot32 && planes != rot)
    return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: NULL d_out64 with d_rot32 (only planes == UROT | VROT goes "
                              "without it)%s", "");
  const size_t npoint = (size_t)npair * nlat * nlon;
  if (overlap(d_u, npoint * 4, d_v, npoint * 4) || overlap(d_u, npoint * 4, d_rot32, npoint * 8) ||
      overlap(d_v, npoint * 4, d_rot32, npoint * 8) || overlap(d_u, npoint * 4, d_out64, npoint * nplane * 8) ||
      overlap(d_v, npoint * 4, d_out64, npoint * nplane * 8) ||
      overlap(d_rot32, npoint * 8, d_out64, npoint * nplane * 8))
    return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: d_u, d_v, d_out64 and d_rot32 must not alias each other%s", "");
  if (npair == 0) return RWRT_OK;
  if (!d_u || !d_v || !d_w || !d_x || !d_spec || !d_scratch)
    return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: NULL buffer (d_u, d_v, d_w, d_x, d_spec, d_scratch)%s", "");
  const int32_t T = trunc, n1 = T + 1;
  const int32_t M = (T < nlon / 2 - 1 ? T : nlon / 2 - 1) + 1;   // orders 0..min(T, nlon/2 - 1); nlon == 2: order 0
  // the forward sum of a row: S segments per order, at least 16 points each (as the filter's)
  int32_t S = kShThreads / M < 1 ? 1 : kShThreads / M;
  if (S > nlon / 16) S = nlon / 16 < 1 ? 1 : nlon / 16;
  const int32_t len = (nlon + S - 1) / S;
  const size_t lds_fwd = ((size_t)3 * nlon + (size_t)2 * M * S) * sizeof(double);
  const size_t lds_inv = ((size_t)2 * nlon + (size_t)2 * M) * sizeof(double);
  const size_t lds_tab = (size_t)kShvTableRows * (T + 2) * sizeof(double);
  const size_t lds_ana = lds_tab + (size_t)n1 * kShWaves * 4 * sizeof(double);
  const size_t lds_syn = lds_tab + (size_t)8 * n1 * sizeof(double);
  if (lds_fwd > kShLdsMax || lds_inv > kShLdsMax)
    return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: nlon is too large for a row and its twiddles in LDS%s", "");
  if (lds_ana > kShLdsDefault || lds_syn > kShLdsDefault)
    return fail(RWRT_ERR_ARG, "rwrt_sh_helmholtz: trunc is too large for one order's sums in LDS%s", "");
  hipStream_t st = (hipStream_t)stream;
  if (rwrt_status s = allow_lds(shv_forward_dft_kernel, lds_fwd, "hipFuncSetAttribute(shv_forward_dft_kernel)")) return s;
  if (rwrt_status s = allow_lds(sh_inverse_dft_kernel, lds_inv, "hipFuncSetAttribute(sh_inverse_dft_kernel)")) return s;
  const size_t per_field = (size_t)M * nlat * 2;
  double* d_F = d_scratch;                              // [2 npair]
  double* d_G = d_F + (size_t)2 * npair * per_field;    // [npair nplane]
  // u_rot, v_rot once more where the float32 pair is not the whole output
  double* d_G2 = (d_rot32 && planes != rot) ? d_G + (size_t)npair * nplane * per_field : nullptr;
  // a block of the two transforms walks several rows, so that its twiddles are built once for all of them
  int32_t rows = (2048 + 2 * npair - 1) / (2 * npair);
  if (rows > nlat) rows = nlat;
  hipLaunchKernelGGL(shv_forward_dft_kernel, dim3(rows, 2 * npair), dim3(kShThreads), lds_fwd, st, nlon, nlat, M, S,
                     len, npair, d_u, d_v, d_F);
  if (rwrt_status s = check_launch("shv_forward_dft_kernel")) return s;
  hipLaunchKernelGGL(shv_analysis_kernel, dim3(n1, npair), dim3(kShThreads), lds_ana, st, nlat, T, M, npair, d_w, d_x,
                     d_F, d_spec);
  if (rwrt_status s = check_launch("shv_analysis_kernel")) return s;
  if (!d_out64 && !d_rot32) return RWRT_OK;   // coefficients only
  hipLaunchKernelGGL(shv_synthesis_kernel, dim3(M, npair, (nlat + kShThreads - 1) / kShThreads), dim3(kShThreads),
                     lds_syn, st, nlat, T, M, planes, nplane, d_x, d_spec, d_G, d_G2);
  if (rwrt_status s = check_launch("shv_synthesis_kernel")) return s;
  int32_t rows_inv = (2048 + npair * nplane - 1) / (npair * nplane);
  if (rows_inv > nlat) rows_inv = nlat;
  hipLaunchKernelGGL(sh_inverse_dft_kernel, dim3(rows_inv, npair * nplane), dim3(kShThreads), lds_inv, st, nlon, nlat,
                     M, d_G, (d_rot32 && !d_G2) ? d_rot32 : (float*)nullptr, d_out64);
  if (rwrt_status s = check_launch("sh_inverse_dft_kernel")) return s;
  if (d_G2) {
    hipLaunchKernelGGL(sh_inverse_dft_kernel, dim3(rows, 2 * npair), dim3(kShThreads), lds_inv, st, nlon, nlat, M, d_G2,
                       d_rot32, (double*)nullptr);
    return check_launch("sh_inverse_dft_kernel(rot32)");
  }
  return RWRT_OK;
}

extern "C" rwrt_status rwrt_sh_rws(int32_t nlon, int32_t nlat, int32_t nfield, int32_t planetary, const double* d_x,
                                   const double* d_div_a, const double* d_udiv_a, const double* d_vdiv_a,
                                   const double* d_vrt_b, const double* d_vrtx_b, const double* d_vrty_b, double* d_out,
                                   void* stream) {
  if (nlat < 3 || nlat % 2 == 0)
    return fail(RWRT_ERR_ARG, "rwrt_sh_rws: nlat must be odd and at least 3 (both poles are nodes)%s", "");
  if (nlon < 2 || nlon % 2 != 0) return fail(RWRT_ERR_ARG, "rwrt_sh_rws: nlon must be even and at least 2%s", "");
  if (nfield < 0 || nfield > 65535) return fail(RWRT_ERR_ARG, "rwrt_sh_rws: nfield must be 0..65535%s", "");
  if (planetary != 0 && planetary != 1) return fail(RWRT_ERR_ARG, "rwrt_sh_rws: planetary must be 0 or 1%s", "");
  if (nfield == 0) return RWRT_OK;
  if (!d_x || !d_div_a || !d_udiv_a || !d_vdiv_a || !d_vrt_b || !d_vrtx_b || !d_vrty_b || !d_out)
    return fail(RWRT_ERR_ARG, "rwrt_sh_rws: NULL buffer (d_x, the six planes, d_out)%s", "");
  const int64_t n = (int64_t)nfield * nlat * nlon;
  const double* in[6] = {d_div_a, d_udiv_a, d_vdiv_a, d_vrt_b, d_vrtx_b, d_vrty_b};
  for (const double* p : in)
    if (overlap(p, (size_t)n * 8, d_out, (size_t)n * 8))
      return fail(RWRT_ERR_ARG, "rwrt_sh_rws: d_out must not alias a plane%s", "");
  int64_t blocks = (n + kShThreads - 1) / kShThreads;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(sh_rws_kernel, dim3((uint32_t)blocks), dim3(kShThreads), 0, (hipStream_t)stream, n, nlon, nlat,
                     planetary, d_x, d_div_a, d_udiv_a, d_vdiv_a, d_vrt_b, d_vrtx_b, d_vrty_b, d_out);
  return check_launch("sh_rws_kernel");
}
