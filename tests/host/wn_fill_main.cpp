// Stand-alone host program over csrc/wn_fill.h (the per-entry arithmetic the
// fill kernel uses), built by tests/support/hostprog.py with
// -fsanitize=undefined,address -fno-sanitize-recover=all and run directly.
//
// stdin:  nlon nlat nplane cyclic
//         nlon*nlat*nplane values in [nlon][nlat][nplane] order, as bit
//         patterns (hex, 16 digits)
// stdout: the filled array in the same order and format, one value per line
#include <cstdio>
#include <cstring>
#include <vector>

#include "wn_fill.h"

int main() {
  int nlon, nlat, nplane, cyclic;
  if (scanf("%d %d %d %d", &nlon, &nlat, &nplane, &cyclic) != 4 || nlon < 1 || nlat < 1 || nplane < 1) return 2;
  const size_t n = (size_t)nlon * nlat * nplane;
  std::vector<double> in(n), out(n);
  for (size_t e = 0; e < n; ++e) {
    unsigned long long u;
    if (scanf("%llx", &u) != 1) return 2;
    memcpy(&in[e], &u, sizeof u);
  }
  for (int i = 0; i < nlon; ++i)
    for (int j = 0; j < nlat; ++j)
      for (int p = 0; p < nplane; ++p)
        out[((size_t)i * nlat + j) * nplane + p] = rwrt::wn_fill_entry(in.data(), nlon, nlat, nplane, cyclic != 0, i, j, p);
  for (size_t e = 0; e < n; ++e) {
    unsigned long long u;
    memcpy(&u, &out[e], sizeof u);
    printf("%016llx\n", u);
  }
  fprintf(stderr, "wn_fill_main ok: %d x %d x %d, cyclic %d\n", nlon, nlat, nplane, cyclic);
  return 0;
}
