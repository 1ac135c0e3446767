// Stand-alone host program over csrc/tube_rows.h (the validity of a point, the
// stencil fixed at row 0, the wrapped differences, jac and D of a row, the
// caustic test, the deposit's bin and the per-ray walk with its gathers of the
// stencil rays' rows, which the tube kernel uses), built by
// tests/support/hostprog.py with -fsanitize=undefined,address,float-cast-overflow
// -fno-sanitize-recover=all -ffp-contract=off and run directly.
//
// Launches are walked the way the kernel walks them, ray by ray, ray j in
// column j of the state arrays, with an emitter that updates plain arrays
// instead of issuing atomics.  Every buffer has exactly the size its launch
// gives it, so a row, a tail, a neighbour's row or a bin read or written out
// of range is the sanitizer's finding.  Each ray is also walked row by row (its
// own tail and its stencil rays' tails expanded) with a state of its own, and
// the program fails (exit 3) if the counts, the drops or the state (bit for
// bit) that the tails' shortcut gives differ from that.
//
// stdin:  nx ny nchan need nray
//         lat0 inv_dlat inv_dlon max_sep                                    (doubles as hex floats, %a; inf)
//         nbr[4][nray]
//         nlaunch
//         per launch: tests/host/launch_input.h                            (nray the same in every launch)
// stdout: cnt[nmap], ncaus[nmap] as integers, slog[nmap] as hex floats, one
//         line each; "dropped <n> bad <0|1>"; state_i[5 * nray] as integers
//         and state_f[13 * nray] as hex floats (nan for none), one line each
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "launch_input.h"
#include "tube_rows.h"

namespace {

using host_input::read_double;
using host_input::read_int;

struct Arrays {
  std::vector<long long> cnt, ncaus;
  std::vector<double> slog;
  std::vector<int32_t> si;
  std::vector<double> sf;
  unsigned long long dropped = 0;
  int bad = 0;

  Arrays(size_t nmap, size_t nray)
      : cnt(nmap, 0), ncaus(nmap, 0), slog(nmap, 0.0), si(rwrt::kTubeNI * nray, 0), sf(rwrt::kTubeNF * nray, NAN) {
    for (size_t j = 0; j < nray; ++j) si[2 * nray + j] = si[4 * nray + j] = -1;
  }
};

struct PlainEmitter {
  Arrays& a;

  void drop(int32_t n) {
    if (n < 1) exit(4);
    a.dropped += (unsigned long long)n;
  }
  void bad_index() { a.bad = 1; }
  // (.at(): an index out of range ends the program)
  void caustic(int32_t bin) { a.ncaus.at((size_t)bin) += 1; }
  void add(int32_t bin, int32_t n, double slog) {
    if (bin < 0 || n < 1) exit(4);
    a.cnt.at((size_t)bin) += n;
    a.slog.at((size_t)bin) += slog;
  }
};

bool same_bits(const std::vector<double>& x, const std::vector<double>& y) {
  return x.size() == y.size() && (x.empty() || memcmp(x.data(), y.data(), x.size() * sizeof(double)) == 0);
}

}  // namespace

int main() {
  rwrt_tube_map m = {};
  m.nx = read_int();
  m.ny = read_int();
  m.nchan = read_int();
  m.need = read_int();
  const int nray = read_int();
  m.lat0 = read_double();
  m.inv_dlat = read_double();
  m.inv_dlon = read_double();
  m.max_sep = read_double();
  if (m.nx <= 0 || m.ny <= 0 || m.nchan <= 0 || !(m.need == -1 || (m.need >= 2 && m.need <= 6)) || nray < 0 ||
      !(m.inv_dlat > 0.0) || !(m.inv_dlon > 0.0) || !std::isfinite(m.lat0) || !(m.max_sep > 0.0))
    return 2;
  std::vector<int32_t> nbr((size_t)4 * nray);   // (any value: an index out of range must not be followed)
  for (auto& v : nbr) v = read_int();
  const size_t nmap = (size_t)m.nchan * m.ny * m.nx;
  Arrays walked(nmap, nray), each(nmap, nray);
  PlainEmitter ew{walked}, ee{each};
  const rwrt_density_map bins = rwrt::tube_bins(m);

  const int nlaunch = read_int();
  long long rays = 0;
  for (int q = 0; q < nlaunch; ++q) {
    host_input::Launch in;
    in.read();
    if (in.nray != nray || in.it_begin < 0) return 2;
    const rwrt::LaunchRows L = in.rows();
    for (int j = 0; j < nray; ++j) {
      const int32_t ch = in.chan[j];
      if (ch < 0 || ch >= m.nchan) continue;   // (as the kernel: not walked, its columns stay)
      // walked as the kernel walks it
      rwrt::TubeState s = rwrt::tube_state_load(walked.si.data(), walked.sf.data(), nray, j);
      rwrt::tube_ray<2>(L, (int64_t)j, (int64_t)nray, nbr.data(), m, bins, ch, s, ew);
      rwrt::tube_state_store(s, walked.si.data(), walked.sf.data(), nray, j);
      // and row by row
      rwrt::TubeState r = rwrt::tube_state_load(each.si.data(), each.sf.data(), nray, j);
      const rwrt::LaunchRowsSpan own = rwrt::launch_rows_span(L, (int64_t)j);
      if (L.it_begin == 0) rwrt::tube_fix(L, j, nray, nbr.data(), m, rwrt::tube_load(rwrt::tube_row_ptr(L, own, j, 0), m), r, ee);
      if (r.flags & rwrt::kTubeOpen) {
        const rwrt::TubeStencil st = rwrt::tube_stencil(L, j, nray, nbr.data(), r.flags);
        if (!st.ok) {
          ee.bad_index();
          r.flags &= ~rwrt::kTubeOpen;
          r.close_row = L.it_begin;
        }
        for (int i = L.it_begin; i < L.it_end && (r.flags & rwrt::kTubeOpen); ++i) {
          rwrt::TubePoint P[4];
          for (int k = 0; k < 4; ++k) P[k] = rwrt::tube_load(rwrt::tube_row_ptr(L, st.span[k], st.ray[k], i), m);
          rwrt::tube_row(r, i, rwrt::tube_load(rwrt::tube_row_ptr(L, own, j, i), m), P, m, bins, ch, ee);
        }
      }
      rwrt::tube_state_store(r, each.si.data(), each.sf.data(), nray, j);
    }
    rays += nray;
  }
  if (walked.cnt != each.cnt || walked.ncaus != each.ncaus || walked.dropped != each.dropped ||
      walked.si != each.si || !same_bits(walked.sf, each.sf) || walked.bad != each.bad) {
    fprintf(stderr, "the tails' counts, drops or states differ from the row-by-row walk\n");
    return 3;
  }
  for (size_t k = 0; k < nmap; ++k) printf("%lld ", walked.cnt[k]);
  printf("\n");
  for (size_t k = 0; k < nmap; ++k) printf("%lld ", walked.ncaus[k]);
  printf("\n");
  for (size_t k = 0; k < nmap; ++k) printf("%a ", walked.slog[k]);
  printf("\n");
  printf("dropped %llu bad %d\n", walked.dropped, walked.bad);
  for (size_t k = 0; k < walked.si.size(); ++k) printf("%d ", walked.si[k]);
  printf("\n");
  for (size_t k = 0; k < walked.sf.size(); ++k) printf("%a ", walked.sf[k]);
  printf("\n");
  fprintf(stderr, "tube_rows_main ok: %lld rays in %d launches\n", rays, nlaunch);
  return 0;
}
