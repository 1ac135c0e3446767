// shsf_legendre.h -- the quadrature weights and the normalised associated
// Legendre functions of the spherical-harmonic filter (rwrt_sh_filter,
// include/rwrt.h), shared by the device kernels (csrc/shsf.hip) and by host
// programs (tests/host/shsf_legendre_main.cpp runs it under the sanitizers).
//
// The definition is shsf.reference_weights / shsf.reference_legendre (NumPy);
// every function here restates one line of it with the same operations in the
// same order, so a host build equals NumPy bit for bit where both take sin,
// cos and sqrt from the same libm.
//
// Grid: nlat odd, n = nlat - 1, lat_j = -pi/2 + j pi / n, x_j = sin(lat_j),
// c_j = cos(lat_j).  Both come from the node's distance from the nearer pole,
// d = min(j, n - j) pi / n: c = sin(d), x = -+cos(d), so that c keeps its
// relative precision next to the poles (c is exactly 0 at the poles, x
// exactly 0 on the equator).
// Weights (Clenshaw-Curtis in x): w_j = (c_j / n) (1 - S_j),
//   S_j = sum_{k=1..n/2} b_k / (4 k^2 - 1) cos(2 k j pi / n), summed with k
//   ascending from +0.0; b_k = 1 for k = n/2, else 2; c_j = 1 at the poles,
//   else 2.  The cosine's argument is reduced in integers: t = 2 k j mod 2 n,
//   cos(pi t / n).
// Legendre functions, int p_lm^2 dx = 1:
//   p_00 = sqrt(1/2);  p_kk = (sqrt((2k+1)/(2k)) c) p_{k-1,k-1};
//   p_{m+1,m} = sqrt(2m+3) (x p_mm);
//   p_lm = a_lm (x p_{l-1,m} - b_lm p_{l-2,m}),
//   a_lm = sqrt((4 l^2 - 1) / (l^2 - m^2)),
//   b_lm = sqrt(((l-1)^2 - m^2) / (4 (l-1)^2 - 1)).
// A product x q is evaluated as sgn(x) (q - s q) with s = 1 - |x| taken as
// c^2 / (1 + |x|): next to +-1 an fp64 x does not hold the node's distance from
// the pole (half an ulp of x moves p_l0 by l (l + 1) / 2 half-ulps), c does.
#ifndef RWRT_SHSF_LEGENDRE_H
#define RWRT_SHSF_LEGENDRE_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RWRT_SH_HD __host__ __device__
#else
#define RWRT_SH_HD
#endif

namespace rwrt {

constexpr double kShPi = 3.141592653589793;

// sqrt((2k+1)/(2k)), k >= 1: the factor from p_{k-1,k-1} to p_kk.
RWRT_SH_HD inline double sh_diag_factor(int32_t k) { return sqrt((2.0 * k + 1.0) / (2.0 * k)); }

// sqrt(2m+3): the factor from p_mm to p_{m+1,m}.
RWRT_SH_HD inline double sh_first_factor(int32_t m) { return sqrt(2.0 * m + 3.0); }

// a_lm and b_lm of the three-term recurrence, l >= m + 2.
RWRT_SH_HD inline double sh_rec_a(int32_t l, int32_t m) {
  const double l2 = (double)l * l, m2 = (double)m * m;
  return sqrt((4.0 * l2 - 1.0) / (l2 - m2));
}
RWRT_SH_HD inline double sh_rec_b(int32_t l, int32_t m) {
  const double k2 = (double)(l - 1) * (l - 1), m2 = (double)m * m;
  return sqrt((k2 - m2) / (4.0 * k2 - 1.0));
}

// The node as the recurrence sees it: sgn(x) and s = 1 - |x| = c^2 / (1 + |x|).
struct ShNode {
  double sg, s, c;
};
RWRT_SH_HD inline ShNode sh_make_node(double x, double c) {
  ShNode nd;
  nd.sg = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0);
  nd.s = (c * c) / (1.0 + fabs(x));
  nd.c = c;
  return nd;
}
// x q
RWRT_SH_HD inline double sh_xmul(const ShNode& nd, double q) { return nd.sg * (q - nd.s * q); }

// One step along the diagonal, the first step off it, and the recurrence.
RWRT_SH_HD inline double sh_diag_step(double factor, double c, double p) { return (factor * c) * p; }
RWRT_SH_HD inline double sh_first_step(double factor, const ShNode& nd, double pmm) { return factor * sh_xmul(nd, pmm); }
RWRT_SH_HD inline double sh_rec_step(double a, double b, const ShNode& nd, double p1, double p2) {
  return a * (sh_xmul(nd, p1) - b * p2);
}

// p_mm(c) from p_00.
RWRT_SH_HD inline double sh_pmm(int32_t m, double c) {
  double p = sqrt(0.5);
  for (int32_t k = 1; k <= m; ++k) p = sh_diag_step(sh_diag_factor(k), c, p);
  return p;
}

// out[l - m] = p_lm(x), l = m..lmax (lmax >= m), at a node with x = sin(lat),
// c = cos(lat).
RWRT_SH_HD inline void sh_legendre_column(int32_t m, int32_t lmax, double x, double c, double* out) {
  const ShNode nd = sh_make_node(x, c);
  double p2 = sh_pmm(m, c);
  out[0] = p2;
  if (lmax == m) return;
  double p1 = sh_first_step(sh_first_factor(m), nd, p2);
  out[1] = p1;
  for (int32_t l = m + 2; l <= lmax; ++l) {
    const double p = sh_rec_step(sh_rec_a(l, m), sh_rec_b(l, m), nd, p1, p2);
    out[l - m] = p;
    p2 = p1;
    p1 = p;
  }
}

// The nodes: x = sin(lat_j), c = cos(lat_j) from the distance to the nearer
// pole (host libm; the device receives them as tables).
inline void sh_node(int32_t nlat, int32_t j, double* x, double* c) {
  const int32_t n = nlat - 1;
  const int32_t k = j < n - j ? j : n - j;
  const double d = (k * kShPi) / n;
  *c = std::sin(d);
  *x = 2 * j == n ? 0.0 : (j < n - j ? -std::cos(d) : std::cos(d));
}

// The Clenshaw-Curtis weight of node j (host libm).
inline double sh_weight(int32_t nlat, int32_t j) {
  const int32_t n = nlat - 1;
  double s = 0.0;
  for (int32_t k = 1; k <= n / 2; ++k) {
    const double bk = (2 * k == n) ? 1.0 : 2.0;
    const int64_t t = (2 * (int64_t)k * j) % (2 * (int64_t)n);
    s = s + (bk / (4.0 * k * k - 1.0)) * std::cos((kShPi * (double)t) / n);
  }
  const double cj = (j == 0 || j == n) ? 1.0 : 2.0;
  return (cj / n) * (1.0 - s);
}

}  // namespace rwrt

#endif
