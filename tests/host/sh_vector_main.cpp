// Stand-alone host program over csrc/sh_vector.h (the vector basis of the
// Helmholtz decomposition and the pointwise Rossby-wave source), built by
// tests/support/hostprog.py with -fsanitize=undefined,address
// -fno-sanitize-recover=all and run directly.
//
// usage:  sh_vector_main NLAT TRUNC
// stdout: as bit patterns (hex, 16 digits), one value per line:
//         q_lm(x_j) in [l][m][j] order for l, m <= TRUNC + 1 (0 for l < m and m = 0);
//         b_lm, then d_lm, each in [l][m][j] order for l, m <= TRUNC (0 for l < m and l = 0);
//         then S at every node with planetary = 1 and with 0, from the planes
//         div = 1e-6 (j + 1), udiv = 2 + j, vdiv = -3 + j, vrt = 1e-5 (j - 4), vrtx = 1e-11 j, vrty = -2e-11 (j + 2)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sh_vector.h"

static void put(double v) {
  unsigned long long u;
  memcpy(&u, &v, sizeof u);
  printf("%016llx\n", u);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int nlat = atoi(argv[1]), T = atoi(argv[2]);
  if (nlat < 3 || nlat % 2 == 0 || T < 1 || T > (nlat - 1) / 2) return 2;
  std::vector<double> x(nlat), c(nlat);
  for (int j = 0; j < nlat; ++j) rwrt::sh_node(nlat, j, &x[j], &c[j]);
  const size_t n1 = (size_t)T + 1, n2 = (size_t)T + 2;
  std::vector<double> q(n2 * n2 * nlat, 0.0), b(n1 * n1 * nlat, 0.0), d(n1 * n1 * nlat, 0.0);
  std::vector<double> qc(n2), bc(n1), dc(n1);
  for (int m = 0; m <= T; ++m)
    for (int j = 0; j < nlat; ++j) {
      const int mq = m < 1 ? 1 : m;
      rwrt::shv_basis_column(m, T, x[j], c[j], qc.data(), bc.data(), dc.data());
      if (m >= 1)
        for (int l = mq; l <= T + 1; ++l) q[((size_t)l * n2 + m) * nlat + j] = qc[l - mq];
      for (int l = mq; l <= T; ++l) {
        b[((size_t)l * n1 + m) * nlat + j] = bc[l - mq];
        d[((size_t)l * n1 + m) * nlat + j] = dc[l - mq];
      }
    }
  // (the last order of q has one entry: q_{T+1,T+1})
  for (int j = 0; j < nlat; ++j) q[((size_t)(T + 1) * n2 + (T + 1)) * nlat + j] = rwrt::shv_qmm(T + 1, c[j]);
  for (double v : q) put(v);
  for (double v : b) put(v);
  for (double v : d) put(v);
  for (int planetary = 1; planetary >= 0; --planetary)
    for (int j = 0; j < nlat; ++j)
      put(rwrt::shv_rws(planetary, x[j], c[j], 1e-6 * (j + 1), 2.0 + j, -3.0 + j, 1e-5 * (j - 4), 1e-11 * j,
                        -2e-11 * (j + 2)));
  fprintf(stderr, "sh_vector_main ok: nlat %d, trunc %d\n", nlat, T);
  return 0;
}
