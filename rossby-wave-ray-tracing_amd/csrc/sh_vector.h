// sh_vector.h -- the vector basis of the Helmholtz decomposition on the
// filter's grid (rwrt_sh_helmholtz, include/rwrt.h), shared by the device
// kernels (csrc/helmholtz.hip) and by host programs
// (tests/host/sh_vector_main.cpp runs it under the sanitizers).
//
// The definition is helmholtz.reference_vector_basis (NumPy); every function
// here restates one line of it with the same operations in the same order, so
// a host build equals NumPy bit for bit, as csrc/shsf_legendre.h does for p_lm.
//
// For 1 <= l <= T, 0 <= m <= l, with x = sin(lat), c = cos(lat):
//   q_lm = p_lm / c, m >= 1, finite at the poles: the recurrences of p_lm
//          (shsf_legendre.h, the x q rule included) started one power of c
//          lower, q_11 = sqrt(3/2) sqrt(1/2), q_mm = (sqrt((2m+1)/(2m)) c)
//          q_{m-1,m-1}, up to degree T + 1.  Never a division by c.
//   b_lm = m q_lm                                     (m p_lm / cos(lat); b_l0 = 0)
//   d_lm = dp_lm/dlat = ((l+1) eps_lm) q_{l-1,m} - (l eps_{l+1,m}) q_{l+1,m},  m >= 1,
//          eps_lm = sqrt((l^2 - m^2) / (4 l^2 - 1)),  q_{l-1,m} = 0 for l - 1 < m
//   d_l0 = sqrt(l (l+1)) (c q_l1)
// The pointwise Rossby-wave source (rwrt_sh_rws) is here as well.
#ifndef RWRT_SH_VECTOR_H
#define RWRT_SH_VECTOR_H

#include "shsf_legendre.h"

namespace rwrt {

constexpr double kShvREarth = 6.3712e6;   // constants.py rearth
constexpr double kShvOmega = 7.2921e-5;   // constants.py omega

// q_11, and q_mm(c) from it (m >= 1).
RWRT_SH_HD inline double shv_q11() { return sqrt(1.5) * sqrt(0.5); }
RWRT_SH_HD inline double shv_qmm(int32_t m, double c) {
  double q = shv_q11();
  for (int32_t k = 2; k <= m; ++k) q = sh_diag_step(sh_diag_factor(k), c, q);
  return q;
}

// eps_lm, and the two factors of d_lm (m >= 1) and the one of d_l0.
RWRT_SH_HD inline double shv_eps(int32_t l, int32_t m) {
  const double l2 = (double)l * l, m2 = (double)m * m;
  return sqrt((l2 - m2) / (4.0 * l2 - 1.0));
}
RWRT_SH_HD inline double shv_d_lower(int32_t l, int32_t m) { return (l + 1.0) * shv_eps(l, m); }
RWRT_SH_HD inline double shv_d_upper(int32_t l, int32_t m) { return (double)l * shv_eps(l + 1, m); }
RWRT_SH_HD inline double shv_d_zonal_factor(int32_t l) { return sqrt((double)l * (l + 1.0)); }

// b_lm and d_lm from the column's neighbours.
RWRT_SH_HD inline double shv_b(int32_t m, double q) { return (double)m * q; }
RWRT_SH_HD inline double shv_d(double lower, double upper, double qm, double qp) { return lower * qm - upper * qp; }
RWRT_SH_HD inline double shv_d_zonal(double factor, double c, double q1) { return factor * (c * q1); }

// Three neighbours of the q column of order mq = max(m, 1) at degree l:
// q_{l-1}, q_l, q_{l+1}.  start() stands at l = mq; advance(a, b) moves to
// l + 1 with the recurrence's factors of degree l + 2.
struct ShvColumn {
  double qm, q0, qp;
};
RWRT_SH_HD inline ShvColumn shv_start(int32_t mq, const ShNode& nd) {
  ShvColumn k;
  k.qm = 0.0;
  k.q0 = shv_qmm(mq, nd.c);
  k.qp = sh_first_step(sh_first_factor(mq), nd, k.q0);
  return k;
}
RWRT_SH_HD inline void shv_advance(ShvColumn& k, double a, double b, const ShNode& nd) {
  const double next = sh_rec_step(a, b, nd, k.qp, k.q0);
  k.qm = k.q0;
  k.q0 = k.qp;
  k.qp = next;
}

// q[l - mq] = q_{l,mq}, l = mq..T+1; b[l - l0], d[l - l0] = b_lm, d_lm, l = l0..T,
// with mq = l0 = max(m, 1), at a node with x = sin(lat), c = cos(lat).  m <= T, T >= 1.
RWRT_SH_HD inline void shv_basis_column(int32_t m, int32_t T, double x, double c, double* q, double* b, double* d) {
  const ShNode nd = sh_make_node(x, c);
  const int32_t mq = m < 1 ? 1 : m;
  ShvColumn k = shv_start(mq, nd);
  for (int32_t l = mq; l <= T; ++l) {
    q[l - mq] = k.q0;
    if (m == 0) {
      b[l - mq] = 0.0;
      d[l - mq] = shv_d_zonal(shv_d_zonal_factor(l), c, k.q0);
    } else {
      b[l - mq] = shv_b(m, k.q0);
      d[l - mq] = shv_d(shv_d_lower(l, m), shv_d_upper(l, m), k.qm, k.qp);
    }
    if (l < T) shv_advance(k, sh_rec_a(l + 2, mq), sh_rec_b(l + 2, mq), nd);
  }
  q[T + 1 - mq] = k.qp;
}

// psi_lm from vrt_lm (chi_lm from div_lm), one part: -a^2 v / (l (l+1)), l >= 1.
RWRT_SH_HD inline double shv_potential(int32_t l, double v) {
  return (v * -(kShvREarth * kShvREarth)) / ((double)l * (l + 1.0));
}

// S = -(zeta_B + f) delta_A - (u_chi,A dx zeta_B + v_chi,A (dy zeta_B + beta)),
// f = 2 Omega x, beta = (2 Omega c) / a; planetary == 0: f = beta = 0.
RWRT_SH_HD inline double shv_rws(int32_t planetary, double x, double c, double div_a, double udiv_a, double vdiv_a,
                                 double vrt_b, double vrtx_b, double vrty_b) {
  const double f = planetary ? (2.0 * kShvOmega) * x : 0.0;
  const double beta = planetary ? ((2.0 * kShvOmega) * c) / kShvREarth : 0.0;
  const double stretch = (vrt_b + f) * div_a;
  const double advect = udiv_a * vrtx_b + vdiv_a * (vrty_b + beta);
  return -stretch - advect;
}

}  // namespace rwrt

#endif
