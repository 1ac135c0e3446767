// wn_fill.h -- one entry of the wavenumber map's NaN fill (rwrt_wn_fill,
// include/rwrt.h), shared by the device kernel (csrc/wn_map.hip) and by host
// programs (tests/host/wn_fill_main.cpp runs it under the sanitizers).
//
// The definition is wn.reference_fill (NumPy).  The layout is
// [nlon][nlat][nplane]; a plane is one (zonal wavenumber, root slot), and a
// neighbour is a node next to the entry IN THE SAME PLANE -- the reference's
// uniform_filter(size=3) over the whole array would also average across k and
// across roots.  A non-NaN entry is copied.  A NaN entry becomes acc / cnt over
// its eight neighbours read from the INPUT: i +- 1 wraps when cyclic and is
// skipped outside [0, nlon) otherwise, j +- 1 is skipped outside [0, nlat);
// acc starts at +0.0 and adds the neighbour if it is not NaN, else +0.0, with
// di = -1, 0, 1 outer and dj = -1, 0, 1 inner and the centre left out; cnt
// counts the non-NaN neighbours (infinities count); cnt == 0 leaves NaN.
// The additions are in a fixed order, so the result equals NumPy's bit for bit.
#ifndef RWRT_WN_FILL_H
#define RWRT_WN_FILL_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RWRT_WN_HD __host__ __device__
#else
#define RWRT_WN_HD
#endif

namespace rwrt {

// (x != x: a NaN test no -ffinite-math assumption of a host build can fold)
RWRT_WN_HD inline bool wn_isnan(double x) { return x != x; }

// The filled value of entry (i, j, p) of in[nlon][nlat][nplane].
RWRT_WN_HD inline double wn_fill_entry(const double* in, int32_t nlon, int32_t nlat, int32_t nplane, bool cyclic,
                                       int32_t i, int32_t j, int32_t p) {
  const double v = in[((int64_t)i * nlat + j) * nplane + p];
  if (!wn_isnan(v)) return v;
  double acc = 0.0;
  int cnt = 0;
  for (int di = -1; di <= 1; ++di) {
    int32_t ii = i + di;
    if (ii < 0 || ii >= nlon) {
      if (!cyclic) continue;
      ii = ii < 0 ? ii + nlon : ii - nlon;
    }
    for (int dj = -1; dj <= 1; ++dj) {
      const int32_t jj = j + dj;
      if ((di == 0 && dj == 0) || jj < 0 || jj >= nlat) continue;
      const double w = in[((int64_t)ii * nlat + jj) * nplane + p];
      const bool ok = !wn_isnan(w);
      acc = acc + (ok ? w : 0.0);
      cnt += ok ? 1 : 0;
    }
  }
  return cnt == 0 ? v : acc / (double)cnt;
}

}  // namespace rwrt

#endif
