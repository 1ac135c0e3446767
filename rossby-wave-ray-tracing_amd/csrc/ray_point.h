// ray_point.h -- the device functions of one (point, zonal wavenumber) of the
// initial rays: NumPy's floor modulo and float -> int32 conversions, the packed
// basic state and its bilinear lookup (interp4 / interp11), the Mercator
// factors, the root ordering, and initial_point, what the wavenumber map
// (csrc/wn_map.hip, rwrt_wn_map) evaluates at every grid node.
//
// Included by rwrt.hip (the ray loops and ray_initial_kernel) and by
// wn_map.hip.  Everything up to order_roots was moved here from rwrt.hip as it
// stood, so that rwrt.o stays byte for byte what it was: the placement of the
// run kernels alone moves the C3 step by 2 % (DESIGN_LOG.md, round 5), and a
// kernel added to rwrt.hip itself measured 2.5 % slower.  For the same reason
// ray_initial_kernel keeps its own copy of the body that initial_point
// restates; tests/test_gpu_wn.py holds the two to the same bits at every node.
#ifndef RWRT_RAY_POINT_H
#define RWRT_RAY_POINT_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rwrt.h"
#include "nproots.h"

#ifndef RARE
#define RARE(c) (c)   // (rwrt.hip's analysis build defines its own)
#endif

namespace rwrt {

// constants.py:13-16
constexpr double kPi = 3.14159265358979323846;
constexpr double kHalfPi = 0.5 * kPi;  // "0.5 * pi"  wr.py:508, bs.py:787
constexpr double kTwoPi = 2.0 * kPi;   // "2 * pi"    bs.py:519, interpolation.py:80
constexpr double kNaN = __builtin_nan("");

// Two IEEE f64 divisions qa = a1 / b1, qb = a2 / b2 with the compiler's own
// instruction sequence (v_div_scale, v_rcp, two Newton steps, v_div_fmas,
// v_div_fixup: correctly rounded for every input), interleaved by hand.  The
// compiler emits each division as a dependent chain that waits on the
// v_rcp result and on VCC before v_div_fmas (an s_nop each, 2 of 13 issue
// slots); two chains fill each other's waits.  VCC carries the numerator's
// scale flag from v_div_scale to v_div_fmas, so the two flag windows are
// sequential: A's flag is written early (it only needs the inputs) and read
// 5 instructions later; B's is written after A's v_div_fmas and read after
// 3 instructions + 1 wait state (4 are required).
__device__ __forceinline__ void div2(double a1, double b1, double a2, double b2, double& qa,
                                     double& qb) {
  double dA, dB, rA, rB, eA, eB, nA, nB;
  asm(
      "v_div_scale_f64 %[dA], vcc, %[bA], %[bA], %[aA]\n\t"
      "v_div_scale_f64 %[dB], vcc, %[bB], %[bB], %[aB]\n\t"
      "v_rcp_f64 %[rA], %[dA]\n\t"
      "v_rcp_f64 %[rB], %[dB]\n\t"
      "v_fma_f64 %[eA], -%[dA], %[rA], 1.0\n\t"
      "v_fma_f64 %[eB], -%[dB], %[rB], 1.0\n\t"
      "v_fma_f64 %[rA], %[rA], %[eA], %[rA]\n\t"
      "v_fma_f64 %[rB], %[rB], %[eB], %[rB]\n\t"
      "v_fma_f64 %[eA], -%[dA], %[rA], 1.0\n\t"
      "v_div_scale_f64 %[nA], vcc, %[aA], %[bA], %[aA]\n\t"
      "v_fma_f64 %[eB], -%[dB], %[rB], 1.0\n\t"
      "v_fma_f64 %[rA], %[rA], %[eA], %[rA]\n\t"
      "v_fma_f64 %[rB], %[rB], %[eB], %[rB]\n\t"
      "v_mul_f64 %[qA], %[nA], %[rA]\n\t"
      "v_fma_f64 %[eA], -%[dA], %[qA], %[nA]\n\t"
      "v_div_fmas_f64 %[qA], %[eA], %[rA], %[qA]\n\t"
      "v_div_scale_f64 %[nB], vcc, %[aB], %[bB], %[aB]\n\t"
      "v_mul_f64 %[qB], %[nB], %[rB]\n\t"
      "v_fma_f64 %[eB], -%[dB], %[qB], %[nB]\n\t"
      "v_div_fixup_f64 %[qA], %[qA], %[bA], %[aA]\n\t"
      "s_nop 0\n\t"
      "v_div_fmas_f64 %[qB], %[eB], %[rB], %[qB]\n\t"
      "v_div_fixup_f64 %[qB], %[qB], %[bB], %[aB]"
      : [qA] "=&v"(qa), [qB] "=&v"(qb), [dA] "=&v"(dA), [dB] "=&v"(dB), [rA] "=&v"(rA),
        [rB] "=&v"(rB), [eA] "=&v"(eA), [eB] "=&v"(eB), [nA] "=&v"(nA), [nB] "=&v"(nB)
      : [aA] "v"(a1), [bA] "v"(b1), [aB] "v"(a2), [bB] "v"(b2)
      : "vcc");
}

// fmod(a, b) for b > 0, exact (fmod is always exactly representable): for
// |a| < 2^40 the integer quotient n = trunc(|a|/b) is off by at most one.  The
// remainder r = |a| - n b is a multiple of ulp(b) (or |a| itself), exact from
// one FMA when it lies in (-b, b); a quotient one too large shows as r < 0 and
// r + b is then the exact remainder; one too small as r >= b (possibly
// rounded), recomputed with n + 1.  Branch-free apart from the library call
// for huge, infinite or NaN |a|.  binv (optional) ~ 1/b replaces the
// division: its quotient is off by at most one too (relative error ~2^-52 of
// a quotient below 2^40), which the same correction absorbs.
__device__ __forceinline__ double fmod_pos(double a, double b, double binv = 0.0) {
  const double x = fabs(a);
  const double n = trunc(binv != 0.0 ? x * binv : x / b);
  double r = fma(-n, b, x);
  const double lo = r + b, hi = fma(-(n + 1.0), b, x);
  r = (r < 0.0) ? lo : ((r >= b) ? hi : r);
  if (RARE(!(x < 0x1p40))) {
    asm volatile("");   // NaN, inf, huge: library routine (rare branch)
    r = fabs(fmod(a, b));
  }
  return copysign(r, a);
}

// Python/NumPy floor modulo for float64 (npy_remainder): fmod, then move a
// remainder whose sign differs from b into [0, b); exact zero gets b's sign.
__device__ __forceinline__ double py_mod(double a, double b, double binv = 0.0) {
  double m = fmod_pos(a, b, binv);
  if (m != 0.0) {
    if ((b < 0.0) != (m < 0.0)) m += b;
  } else {
    m = copysign(0.0, b);
  }
  return m;
}
// x % (2 * pi) (bs.py:519, interpolation.py:80)
constexpr double kInvTwoPi = 1.0 / kTwoPi;
__device__ __forceinline__ double py_mod_2pi(double a) { return py_mod(a, kTwoPi, kInvTwoPi); }
// py_mod_2pi(m) for m = py_mod_2pi(x), which lies in [0, 2 pi] or is NaN: the
// identity, except that a remainder that rounded up to 2 pi itself becomes +0.
__device__ __forceinline__ double py_mod_2pi_again(double m) { return (m >= kTwoPi) ? 0.0 : m; }

// np.floor(x).astype('int32') on x86-64 (cvttsd2si): out-of-range and NaN give
// INT32_MIN.  v_cvt_i32_f64 saturates (INT32_MIN below the range, as x86) and
// maps NaN to 0; above the range x86's INT32_MIN is restored.  (NaN -> 0 only
// moves the x1/y1 corner of a lookup whose weights are NaN: same NaN result.)
__device__ __forceinline__ int floor_i32(double x) {
  const double f = floor(x);
  const int i = __double2int_rz(f);
  return (f > 2147483647.0) ? INT32_MIN : i;
}
// x0 + 1 on an int32 array: wraps (NumPy integer arithmetic is modular)
__device__ __forceinline__ int inc_i32(int v) { return (int)((unsigned)v + 1u); }
// np.clip(v, 0, hi) -> v_med3_i32
__device__ __forceinline__ int clip(int v, int hi) { return ::max(0, ::min(v, hi)); }

// ---------------------------------------------------------------------------
// Basic state: packed [W][H][12] fp64, the 11 hot fields of BS.fields
// ---------------------------------------------------------------------------
enum { F_U = 0, F_V, F_UX, F_UY, F_VX, F_VY, F_QX, F_QY, F_QXX, F_QXY, F_QYY, F_PAD };
constexpr int kNF = RWRT_NFIELD_PACK;

struct Field {
  const double* __restrict__ P;
  int W, H;
  double lon0, dlon, lat0, dlat;
};

// Bilinear corner set + weights of batch_linint2_metpy/bilinear_interpolation_
// (interpolation.py:77-85, 103-135) for one in-range point.
struct Corners {
  const double* a;  // F[x0, y1]
  const double* b;  // F[x1, y1]
  const double* c;  // F[x0, y0]
  const double* d;  // F[x1, y0]
  double wa, wb, wc, wd;
  unsigned key_x, key_y;   // x0 | x1 << 16, y0 | y1 << 16 (W, H < 2^16)
  unsigned pa, pb, pc, pd; // grid-point indices x * H + y of a, b, c, d
  unsigned oa, ob, oc, od; // element offsets of a, b, c, d from F.P
  double dx, dy;           // lons - lon0, lat - lat0: the numerators of the cell coordinates
};

__device__ __forceinline__ Corners corners(const Field& F, double lon, double lat) {
  // lon arrives already reduced once (bs.py:519); interpolation.py:80 reduces again.
  const double lons = py_mod_2pi_again(lon);
  double x, y;
  const double dx = lons - F.lon0, dy = lat - F.lat0;
  div2(dx, F.dlon, dy, F.dlat, x, y);
  const int ix = floor_i32(x), iy = floor_i32(y);
  const int x0 = clip(ix, F.W - 1), x1 = clip(inc_i32(ix), F.W - 1);
  const int y0 = clip(iy, F.H - 1), y1 = clip(inc_i32(iy), F.H - 1);
  const double sx = x - (double)x0, sy = y - (double)y0;
  // 32-bit element offsets (a packed state holds < 2^31 doubles; checked on the host)
  // (W, H < 2^24: 24-bit multiplies)
  const unsigned c0 = __umul24(x0, F.H), c1 = __umul24(x1, F.H);
  Corners k;
  k.dx = dx;
  k.dy = dy;
  k.pa = c0 + y1;
  k.pb = c1 + y1;
  k.pc = c0 + y0;
  k.pd = c1 + y0;
  k.oa = __umul24(k.pa, kNF);
  k.ob = __umul24(k.pb, kNF);
  k.oc = __umul24(k.pc, kNF);
  k.od = __umul24(k.pd, kNF);
  k.a = F.P + k.oa;
  k.b = F.P + k.ob;
  k.c = F.P + k.oc;
  k.d = F.P + k.od;
  k.wa = (1.0 - sx) * sy;
  k.wb = sx * sy;
  k.wc = (1.0 - sx) * (1.0 - sy);
  k.wd = sx * (1.0 - sy);
  k.key_x = (unsigned)x0 | ((unsigned)x1 << 16);
  k.key_y = (unsigned)y0 | ((unsigned)y1 << 16);
  return k;
}

// a*wa + b*wb + c*wc + d*wd, left to right (interpolation.py:132-133)
__device__ __forceinline__ double blend(const Corners& k, double a, double b, double c, double d) {
  return ((a * k.wa + b * k.wb) + c * k.wc) + d * k.wd;
}

// Interpolate all 11 hot fields (NaN outside |lat| <= pi/2, bs.py:787,822-836).
__device__ __forceinline__ void interp11(const Field& F, double lon, double lat, double g[11]) {
  if (!(fabs(lat) <= kHalfPi)) {
#pragma unroll
    for (int i = 0; i < 11; ++i) g[i] = kNaN;
    return;
  }
  const Corners k = corners(F, lon, lat);
  const double2* pa = reinterpret_cast<const double2*>(k.a);
  const double2* pb = reinterpret_cast<const double2*>(k.b);
  const double2* pc = reinterpret_cast<const double2*>(k.c);
  const double2* pd = reinterpret_cast<const double2*>(k.d);
  // Three groups of 2 records x 4 corners: bounds the registers held by
  // in-flight loads (the lookup is L2-resident; occupancy hides the latency).
#pragma unroll
  for (int q0 = 0; q0 < 6; q0 += 2) {
#pragma unroll
    for (int q = q0; q < q0 + 2; ++q) {
      const double2 va = pa[q], vb = pb[q], vc = pc[q], vd = pd[q];
      g[2 * q] = blend(k, va.x, vb.x, vc.x, vd.x);
      if (2 * q + 1 < 11) g[2 * q + 1] = blend(k, va.y, vb.y, vc.y, vd.y);
    }
    if (q0 + 2 < 6) __builtin_amdgcn_sched_barrier(0);
  }
}

// Only u, v, qx, qy (what cal_ugvg needs, wr.py:856-865).
__device__ __forceinline__ void interp4(const Field& F, double lon, double lat,
                                        double& fu, double& fv, double& fqx, double& fqy) {
  if (!(fabs(lat) <= kHalfPi)) {
    fu = fv = fqx = fqy = kNaN;
    return;
  }
  const Corners k = corners(F, lon, lat);
  const double2 a0 = *reinterpret_cast<const double2*>(k.a + F_U);
  const double2 b0 = *reinterpret_cast<const double2*>(k.b + F_U);
  const double2 c0 = *reinterpret_cast<const double2*>(k.c + F_U);
  const double2 d0 = *reinterpret_cast<const double2*>(k.d + F_U);
  const double2 a1 = *reinterpret_cast<const double2*>(k.a + F_QX);
  const double2 b1 = *reinterpret_cast<const double2*>(k.b + F_QX);
  const double2 c1 = *reinterpret_cast<const double2*>(k.c + F_QX);
  const double2 d1 = *reinterpret_cast<const double2*>(k.d + F_QX);
  fu = blend(k, a0.x, b0.x, c0.x, d0.x);
  fv = blend(k, a0.y, b0.y, c0.y, d0.y);
  fqx = blend(k, a1.x, b1.x, c1.x, d1.x);
  fqy = blend(k, a1.y, b1.y, c1.y, d1.y);
}

// Mercator factors of cal_bs_mercator_point (bs.py:856-860).
struct Merc {
  double c, s, m, cp;
};
__device__ __forceinline__ Merc merc_factors(double lat, double c, double s) {
  Merc r;
  r.c = c;
  r.s = s;
  r.m = (fabs(c) <= 0.0175) ? 0.0 : 1.0;
  r.cp = c * r.m + (1.0 - r.m) * 1e-6;
  return r;
}

// change_roots_order (bs.py:942-982) on the nreal compacted real roots, then
// the |m| > 100 filter and the reversal of cal_ky (bs.py:1037-1040).
__device__ __forceinline__ void order_roots(double m[3], int nreal) {
  auto swap = [&](int a, int b) { const double t = m[a]; m[a] = m[b]; m[b] = t; };
  if (nreal == 3) {
    if (m[2] >= 0.0 && m[2] < m[1]) swap(1, 2);
    if (m[0] < 0.0) swap(0, 1);
    if ((m[1] < 0.0 && m[2] < 0.0 && m[1] < m[2]) || (m[1] > 0.0 && m[2] < 0.0)) swap(1, 2);
  } else if (nreal == 2) {
    if (!(m[0] > 0.0)) swap(0, 1);
  } else if (nreal == 1) {
    if (m[0] < 0.0) swap(0, 1);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (!isnan(m[q]) && fabs(m[q]) > 100.0) m[q] = kNaN;
  swap(0, 2);
}

// The initial rays of one (point, zonal wavenumber), as ray_initial_kernel
// (rwrt.hip) computes them, operation for operation: the three ordered
// meridional wavenumbers mr and their t = 0 group velocities, NaN where a slot
// has no root.  k, k2, k3, ps = {k, k**2, k**3, freq/k*R} as NumPy evaluates
// them on the host.  Returns true where np.linalg.eigvals would raise
// (non-finite coefficients or a failed solve); every output is NaN then.
__device__ __forceinline__ bool initial_point(const Field& F, double lon, double lat, double cosl, double k,
                                              double k2, double k3, double ps, double mr[3], double ug[3],
                                              double vg[3]) {
  // BS.cal_bs_mercator_point at the point: fmu fmv fmqx fmqy (bs.py:856-883)
  double fu, fv, fqx, fqy;
  interp4(F, py_mod_2pi(lon), lat, fu, fv, fqx, fqy);
  const Merc M = merc_factors(lat, cosl, 0.0);
  const double fmu = (fu / M.cp) * M.m;
  const double fmv = (fv / M.cp) * M.m;
  const double fmqx = fqx * M.m;
  const double fmqy = (fqy * M.cp) * M.m;
  bool raised = false;
  mr[0] = mr[1] = mr[2] = kNaN;
  if (k != 0.0) {
    // cal_ky_numpy coefficients, lowest order first (bs.py:1005-1012)
    const double c[4] = {k3 * ((fmu - ps) - (fmqy / k2)), k2 * fmv + fmqx, k * (fmu - ps), fmv};
    int deg = 3;
    while (deg > 0 && fabs(c[deg]) == 0.0) --deg;    // exact-zero reduction
    if (deg >= 1) {
      double p[4];
      for (int q = 0; q <= deg; ++q) p[q] = c[deg - q];   // highest first
      nproots::cx r[3] = {{kNaN, kNaN}, {kNaN, kNaN}, {kNaN, kNaN}};
      bool finite = true;
      for (int q = 0; q <= deg; ++q) finite = finite && isfinite(p[q]);
      int st = finite ? nproots::np_roots(p, deg, r) : -1;
      raised = st != 0;   // np.linalg.eigvals would raise
      // real roots (|Im| < delt), compacted in np.roots' order (bs.py:1030-1036)
      int nreal = 0;
      for (int q = 0; q < deg; ++q)
        if (st == 0 && fabs(r[q].im) < 1e-8) mr[nreal++] = r[q].re;
      order_roots(mr, nreal);
    }
  }
  for (int slot = 0; slot < 3; ++slot) {
    const double m = mr[slot];
    if (k == 0.0) {
      ug[slot] = 0.0;
      vg[slot] = 0.0;
    } else {
      // cal_ugvg_numpy (wn.py:209-259)
      double nans = ((m * 0.0) * (((fmu * fmqx) * fmqy) * 0.0)) + 1.0;
      if (isnan(nans)) nans = 0.0;
      const double a = (k * k) - (m * m);
      const double b = (2.0 * k) * m;
      const double cc = (k * k) + (m * m);
      const double c2 = cc * cc;
      ug[slot] = (fmu + (((a * fmqy) - (b * fmqx)) / c2)) * nans;
      vg[slot] = (fmv + (((a * fmqx) + (b * fmqy)) / c2)) * nans;
    }
  }
  return raised;
}

}  // namespace rwrt

#endif
