// bs_diag.h -- the per-node arithmetic of rwrt_bs_diag (include/rwrt.h): the
// 23 planes of the reference's BS.output (bs.py:481-505) after
// BS.ready(xcyclic=True) (bs.py:318-407), shared by the device kernels
// (csrc/bs_diag.hip) and by host programs (tests/host/bs_diag_main.cpp runs it
// under the sanitizers).
//
// Every function takes its field as an accessor f(i, j) -> double, i the
// longitude index and j the latitude index.  The stencils pass i - 1 and i + 1
// unwrapped (-1 and nlon occur): the accessor applies the periodic rule, so a
// tile held in shared memory with a halo column serves as well as global
// memory.  j always stays inside [0, nlat).
//
// Every expression is + - * / sqrt in fp64 in NumPy's evaluation order; build
// with -ffp-contract=off.  The vorticity, the stencils and smth9 restate what
// rwrt_bs_ready (csrc/rwrt.hip) computes; tests/test_gpu_bsdiag.py pins the two
// copies to each other bit for bit.
#ifndef RWRT_BS_DIAG_H
#define RWRT_BS_DIAG_H

#include <cmath>
#include <cstdint>
#include <limits>

#if defined(__HIPCC__)
#define RWRT_BSD_HD __host__ __device__ __forceinline__
#else
#define RWRT_BSD_HD inline
#endif

namespace rwrt {

constexpr double kBsdREarth = 6.3712e6;   // constants.py rearth
constexpr double kBsdOmega = 7.2921e-5;   // constants.py omega

// plane ids, BS.output's order
enum : int {
  BSD_U = 0, BSD_V, BSD_Q, BSD_UX, BSD_UXX, BSD_UY, BSD_VX, BSD_VXX, BSD_VY, BSD_QX, BSD_QY, BSD_QXX, BSD_QXY,
  BSD_QYX, BSD_QYY, BSD_QXXX, BSD_QXXY, BSD_QXYY, BSD_QYYY, BSD_QYXX, BSD_QYYX, BSD_BETAM, BSD_KS, BSD_NDIAG
};
constexpr uint32_t kBsdAll = (1u << BSD_NDIAG) - 1u;
constexpr uint32_t kBsdBetaKs = (1u << BSD_BETAM) | (1u << BSD_KS);
// the planes that read q or its second derivatives (they need the scratch)
constexpr uint32_t kBsdNeedsQ = (1u << BSD_Q) | (0xfffu << BSD_QX);
// the planes that read v themselves (the q planes read it through the scratch)
constexpr uint32_t kBsdReadsV = (1u << BSD_V) | (1u << BSD_VX) | (1u << BSD_VXX) | (1u << BSD_VY);

// the grid and the divisors of the stencils, as BS builds them (bs.py:77-78)
struct BsdGeom {
  int32_t nlon, nlat;
  double dx2, dy2, dxx, dyy, dxy4, dy;   // 2dx, 2dy, dx**2, dy**2, (4dx)dy, dy
};

RWRT_BSD_HD BsdGeom bsd_geom(int32_t nlon, int32_t nlat, double dx, double dy) {
  return BsdGeom{nlon, nlat, 2.0 * dx, 2.0 * dy, dx * dx, dy * dy, (4.0 * dx) * dy, dy};
}

RWRT_BSD_HD int bsd_wrap(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }
// rows 0 and nlat-1 copy their neighbour (q, gradient_yy, gradient_xy)
RWRT_BSD_HD int bsd_inner(int j, int nlat) { return j < 1 ? 1 : (j > nlat - 2 ? nlat - 2 : j); }
RWRT_BSD_HD double bsd_nan() { return std::numeric_limits<double>::quiet_NaN(); }

// gradient_x (bs.py:121-131), periodic
template <class F>
RWRT_BSD_HD double bsd_grad_x(const F& f, const BsdGeom& g, int i, int j) {
  return (f(i + 1, j) - f(i - 1, j)) / g.dx2;
}

// gradient_y (bs.py:133-142), one-sided at the two edge rows
template <class F>
RWRT_BSD_HD double bsd_grad_y(const F& f, const BsdGeom& g, int i, int j) {
  const int H = g.nlat;
  if (j == 0) return (f(i, 1) - f(i, 0)) / g.dy;
  if (j == H - 1) return (f(i, H - 1) - f(i, H - 2)) / g.dy;
  return (f(i, j + 1) - f(i, j - 1)) / g.dy2;
}

// gradient_xx (bs.py:144-154), periodic
template <class F>
RWRT_BSD_HD double bsd_grad_xx(const F& f, const BsdGeom& g, int i, int j) {
  return ((f(i + 1, j) - 2.0 * f(i, j)) + f(i - 1, j)) / g.dxx;
}

// gradient_yy (bs.py:156-166), the edge rows copy their neighbour
template <class F>
RWRT_BSD_HD double bsd_grad_yy(const F& f, const BsdGeom& g, int i, int j) {
  const int jj = bsd_inner(j, g.nlat);
  return ((f(i, jj + 1) - 2.0 * f(i, jj)) + f(i, jj - 1)) / g.dyy;
}

// gradient_xy (bs.py:168-195), periodic, the edge rows copy their neighbour
template <class F>
RWRT_BSD_HD double bsd_grad_xy(const F& f, const BsdGeom& g, int i, int j) {
  const int jj = bsd_inner(j, g.nlat);
  return (((f(i + 1, jj + 1) - f(i + 1, jj - 1)) - f(i - 1, jj + 1)) + f(i - 1, jj - 1)) / g.dxy4;
}

// calc_absolute_vorticity (bs.py:264-279).  trig[3][nlat]: np.cos(lat), then
// np.cos and np.sin of lat[1:-1] at 1..nlat-2.
template <class FU, class FV>
RWRT_BSD_HD double bsd_vorticity(const FU& u, const FV& v, const double* trig, const BsdGeom& g, int i, int j) {
  const int H = g.nlat;
  const int jj = bsd_inner(j, H);
  const double vx = (v(i + 1, jj) - v(i - 1, jj)) / g.dx2;
  const double ucp = u(i, jj + 1) * trig[jj + 1];
  const double ucm = u(i, jj - 1) * trig[jj - 1];
  const double uy = (ucp - ucm) / g.dy2;
  return (vx - uy) / trig[H + jj] + ((2.0 * kBsdOmega) * trig[2 * H + jj]) * kBsdREarth;
}

// smth9 (bs.py:291-305): f + convolve(f, w, 'constant') on [1:-2, 1:-2], f elsewhere
template <class F>
RWRT_BSD_HD double bsd_smth9_at(const F& f, const BsdGeom& g, int i, int j) {
  const double f0 = f(i, j);
  if (i < 1 || i > g.nlon - 3 || j < 1 || j > g.nlat - 3) return f0;
  // weights q/4 = 0.0625 (corners), p/4 = 0.125 (edges), -(p + q) = -0.75 (centre)
  double acc = 0.0;
  for (int da = -1; da <= 1; ++da)
    for (int db = -1; db <= 1; ++db)
      acc = acc + f(i + da, j + db) * (da == 0 && db == 0 ? -0.75 : (da == 0 || db == 0 ? 0.125 : 0.0625));
  return f0 + acc;
}

// betam (bs.py:379-385): NaN on rows 0 and nlat-1
template <class FU>
RWRT_BSD_HD double bsd_betam(const FU& u, const double* trig, const BsdGeom& g, int i, int j) {
  const int H = g.nlat;
  if (j < 1 || j > H - 2) return bsd_nan();
  const double c = trig[H + j], s = trig[2 * H + j];
  const double uyy = bsd_grad_yy(u, g, i, j), uy = bsd_grad_y(u, g, i, j);
  return ((2.0 * kBsdOmega) * (c * c) + (((-c) * uyy + s * uy) + u(i, j) / c) / kBsdREarth) / kBsdREarth;
}

// KS (bs.py:394-407) of a node's betam, cos(lat) and u: NaN on the edge rows
// and wherever betam > 0 and u > 0 do not both hold
RWRT_BSD_HD double bsd_ks(double betam, double c, double u, int j, int nlat) {
  if (j < 1 || j > nlat - 2 || !(betam > 0.0) || !(u > 0.0)) return bsd_nan();
  return sqrt((betam * c) / u) * kBsdREarth;
}

// The value of plane p at node (i, j).  u, v: the winds; q, qxx, qyy, qxy: the
// vorticity and its unsmoothed second derivatives (looked at only for the
// planes of kBsdNeedsQ).
template <class FU, class FV, class FQ>
RWRT_BSD_HD double bsd_plane(int p, const FU& u, const FV& v, const FQ& q, const FQ& qxx, const FQ& qyy,
                             const FQ& qxy, const double* trig, const BsdGeom& g, int i, int j) {
  switch (p) {
    case BSD_U: return u(i, j);
    case BSD_V: return v(i, j);
    case BSD_Q: return q(i, j);
    case BSD_UX: return bsd_grad_x(u, g, i, j);
    case BSD_UXX: return bsd_grad_xx(u, g, i, j);
    case BSD_UY: return bsd_grad_y(u, g, i, j);
    case BSD_VX: return bsd_grad_x(v, g, i, j);
    case BSD_VXX: return bsd_grad_xx(v, g, i, j);
    case BSD_VY: return bsd_grad_y(v, g, i, j);
    case BSD_QX: return bsd_grad_x(q, g, i, j);
    case BSD_QY: return bsd_grad_y(q, g, i, j);
    case BSD_QXX: return bsd_smth9_at(qxx, g, i, j);
    case BSD_QXY: return bsd_smth9_at(qxy, g, i, j);
    case BSD_QYX: return qxy(i, j);
    case BSD_QYY: return bsd_smth9_at(qyy, g, i, j);
    case BSD_QXXX: return bsd_grad_x(qxx, g, i, j);
    case BSD_QXXY: return bsd_grad_y(qxx, g, i, j);
    case BSD_QXYY: return bsd_grad_y(qxy, g, i, j);
    case BSD_QYYY: return bsd_grad_y(qyy, g, i, j);
    case BSD_QYXX: return bsd_grad_x(qxy, g, i, j);
    case BSD_QYYX: return bsd_grad_x(qyy, g, i, j);
    case BSD_BETAM: return bsd_betam(u, trig, g, i, j);
    default: {
      const double b = bsd_betam(u, trig, g, i, j);
      return bsd_ks(b, trig[g.nlat + bsd_inner(j, g.nlat)], u(i, j), j, g.nlat);
    }
  }
}

}  // namespace rwrt

#endif  // RWRT_BS_DIAG_H
