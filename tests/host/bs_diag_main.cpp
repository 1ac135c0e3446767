// Stand-alone host program over csrc/bs_diag.h (the per-node arithmetic the
// kernels of rwrt_bs_diag use), built by tests/support/hostprog.py with
// -fsanitize=undefined,address -fno-sanitize-recover=all and run directly.
//
// usage: bs_diag_main IN OUT
// IN  (raw binary): int32 nlon, nlat; uint32 select; int32 0; double dx, dy;
//                   double trig[3][nlat]; float u[nlat][nlon]; float v[nlat][nlon]
// OUT (raw binary): double planes[popcount(select)][nlon][nlat], ascending id
// Every array is a vector of exactly its size, so an index outside one is an
// AddressSanitizer error.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bs_diag.h"

using namespace rwrt;

namespace {

struct HostUV {   // [nlat][nlon] float32, periodic in i
  const std::vector<float>* p;
  int nlon;
  double operator()(int i, int j) const { return (double)(*p)[(size_t)j * nlon + bsd_wrap(i, nlon)]; }
};

struct HostQ {    // [nlon][nlat] double, periodic in i
  const std::vector<double>* p;
  int nlon, nlat;
  double operator()(int i, int j) const { return (*p)[(size_t)bsd_wrap(i, nlon) * nlat + j]; }
};

template <class T>
bool read_all(FILE* f, T* dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t head[4];
  double d[2];
  if (!read_all(in, head, 4) || !read_all(in, d, 2)) return 2;
  const int nlon = head[0], nlat = head[1];
  const uint32_t select = (uint32_t)head[2];
  if (nlon < 3 || nlat < 4 || select == 0 || (select & ~kBsdAll)) return 2;
  const size_t n = (size_t)nlon * nlat;
  std::vector<double> trig(3 * (size_t)nlat);
  std::vector<float> uf(n), vf(n);
  if (!read_all(in, trig.data(), trig.size()) || !read_all(in, uf.data(), n) || !read_all(in, vf.data(), n)) return 2;
  if (fgetc(in) != EOF) return 2;
  fclose(in);

  const BsdGeom g = bsd_geom(nlon, nlat, d[0], d[1]);
  const HostUV u{&uf, nlon}, v{&vf, nlon};
  std::vector<double> q(n), qxx(n), qyy(n), qxy(n);
  const HostQ Q{&q, nlon, nlat}, QXX{&qxx, nlon, nlat}, QYY{&qyy, nlon, nlat}, QXY{&qxy, nlon, nlat};
  if (select & kBsdNeedsQ) {
    for (int i = 0; i < nlon; ++i)
      for (int j = 0; j < nlat; ++j) q[(size_t)i * nlat + j] = bsd_vorticity(u, v, trig.data(), g, i, j);
    for (int i = 0; i < nlon; ++i)
      for (int j = 0; j < nlat; ++j) {
        qxx[(size_t)i * nlat + j] = bsd_grad_xx(Q, g, i, j);
        qyy[(size_t)i * nlat + j] = bsd_grad_yy(Q, g, i, j);
        qxy[(size_t)i * nlat + j] = bsd_grad_xy(Q, g, i, j);
      }
  }
  int nsel = 0;
  for (int p = 0; p < BSD_NDIAG; ++p) nsel += (select >> p) & 1u;
  std::vector<double> out((size_t)nsel * n);
  size_t slot = 0;
  for (int p = 0; p < BSD_NDIAG; ++p) {
    if (!((select >> p) & 1u)) continue;
    for (int i = 0; i < nlon; ++i)
      for (int j = 0; j < nlat; ++j)
        out[slot * n + (size_t)i * nlat + j] = bsd_plane(p, u, v, Q, QXX, QYY, QXY, trig.data(), g, i, j);
    ++slot;
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o || fwrite(out.data(), sizeof(double), out.size(), o) != out.size()) return 3;
  fclose(o);
  fprintf(stderr, "bs_diag_main ok: %d x %d, select 0x%x, %d planes\n", nlon, nlat, select, nsel);
  return 0;
}
