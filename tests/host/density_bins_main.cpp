// Stand-alone host program over csrc/density_bins.h (the index function the
// density kernel uses), built by tests/support/hostprog.py with
// -fsanitize=undefined,address,float-cast-overflow -fno-sanitize-recover=all
// and run directly: a float -> integer conversion of an unchecked value, or
// any other undefined behaviour in the index arithmetic, aborts the run.
//
// stdin:  nx ny nchan wcol inv_dlon lat0 inv_dlat      (one line; doubles as
//         lon lat w chan                                hex floats, %a)
//         ...
// stdout: one line per point: "<bin index> <wrapped longitude, %a>"
#include <cstdio>
#include <cstdlib>

#include "density_bins.h"

int main() {
  rwrt_density_map m;
  char a[64], b[64], c[64];
  if (scanf("%d %d %d %d %63s %63s %63s", &m.nx, &m.ny, &m.nchan, &m.wcol, a, b, c) != 7) return 2;
  m.inv_dlon = strtod(a, nullptr);
  m.lat0 = strtod(b, nullptr);
  m.inv_dlat = strtod(c, nullptr);
  int chan;
  long n = 0;
  while (scanf("%63s %63s %63s %d", a, b, c, &chan) == 4) {
    const double lon = strtod(a, nullptr), lat = strtod(b, nullptr), w = strtod(c, nullptr);
    const double lam = rwrt::density_wrap_2pi(lon);
    const int32_t idx = rwrt::density_bin(lam, lat, w, chan, m);
    if (idx < -1 || idx >= m.nx * m.ny * m.nchan) return 3;   // (never: the test compares every index)
    printf("%d %a\n", idx, lam);
    ++n;
  }
  fprintf(stderr, "density_bins_main ok: %ld points\n", n);
  return 0;
}
