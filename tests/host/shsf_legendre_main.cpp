// Stand-alone host program over csrc/shsf_legendre.h (the quadrature weights
// and the Legendre recurrence of the spherical-harmonic filter), built by
// tests/support/hostprog.py with -fsanitize=undefined,address
// -fno-sanitize-recover=all and run directly.
//
// usage:  shsf_legendre_main NLAT TRUNC
// stdout: as bit patterns (hex, 16 digits), one value per line:
//         nlat weights; nlat values of sin(lat); nlat values of cos(lat);
//         then p_lm(x_j) in [l][m][j] order for l, m <= TRUNC (0 for l < m)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "shsf_legendre.h"

static void put(double v) {
  unsigned long long u;
  memcpy(&u, &v, sizeof u);
  printf("%016llx\n", u);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int nlat = atoi(argv[1]), T = atoi(argv[2]);
  if (nlat < 3 || nlat % 2 == 0 || T < 0 || T > (nlat - 1) / 2) return 2;
  std::vector<double> x(nlat), c(nlat);
  for (int j = 0; j < nlat; ++j) put(rwrt::sh_weight(nlat, j));
  for (int j = 0; j < nlat; ++j) rwrt::sh_node(nlat, j, &x[j], &c[j]);
  for (int j = 0; j < nlat; ++j) put(x[j]);
  for (int j = 0; j < nlat; ++j) put(c[j]);
  const size_t n1 = (size_t)T + 1;
  std::vector<double> p(n1 * n1 * nlat, 0.0), col(n1);
  for (int m = 0; m <= T; ++m)
    for (int j = 0; j < nlat; ++j) {
      rwrt::sh_legendre_column(m, T, x[j], c[j], col.data());
      for (int l = m; l <= T; ++l) p[((size_t)l * n1 + m) * nlat + j] = col[l - m];
    }
  for (double v : p) put(v);
  fprintf(stderr, "shsf_legendre_main ok: nlat %d, trunc %d\n", nlat, T);
  return 0;
}
