// Stand-alone host program over csrc/wave_rows.h (the tube's and the phase's
// walks composed in one pass over a ray's rows, and the caustic-aware deposit,
// which the wave kernel uses), built by tests/support/hostprog.py with
// -fsanitize=undefined,address,float-cast-overflow -fno-sanitize-recover=all
// -ffp-contract=off and run directly.
//
// Launches are walked the way the kernel walks them, ray by ray, ray j in
// column j of the state arrays, with an emitter that updates plain arrays
// instead of issuing atomics.  Every buffer has exactly the size its launch
// gives it, so a row, a tail, a neighbour's row or a bin read or written out
// of range is the sanitizer's finding.  Each ray is also walked row by row (its
// own tail and its stencil rays' tails expanded) with a state of its own, and
// the program fails (exit 3) if the counts, the drops, the clipped deposits or
// the state (bit for bit) that the tails' shortcut gives differ from that.
//
// stdin:  nx ny nchan need wcol spread nray
//         lat0 inv_dlat inv_dlon max_sep omega_dt d_floor                  (doubles as hex floats, %a; inf)
//         theta0[nray]
//         nbr[4][nray]
//         nlaunch
//         per launch: tests/host/launch_input.h                            (nray the same in every launch)
// stdout: cnt[nmap] as integers, re[nmap], im[nmap], wabs[nmap] as hex floats,
//         one line each; "dropped <n> clipped <n> bad <0|1>"; state_i[6 * nray]
//         as integers and state_f[9 * nray] as hex floats (nan for none), one
//         line each
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "launch_input.h"
#include "wave_rows.h"

namespace {

using host_input::read_double;
using host_input::read_int;

struct Arrays {
  std::vector<long long> cnt;
  std::vector<double> re, im, wabs;
  std::vector<int32_t> si;
  std::vector<double> sf;
  unsigned long long dropped = 0, clipped = 0;
  int bad = 0;

  Arrays(size_t nmap, size_t nray, const std::vector<double>& theta0)
      : cnt(nmap, 0), re(nmap, 0.0), im(nmap, 0.0), wabs(nmap, 0.0), si(rwrt::kWaveNI * nray, 0),
        sf(rwrt::kWaveNF * nray, NAN) {
    for (size_t j = 0; j < nray; ++j) {
      si[2 * nray + j] = si[4 * nray + j] = -1;
      sf[4 * nray + j] = theta0[j];
    }
  }
};

struct PlainEmitter {
  Arrays& a;

  void drop(int32_t n) {
    if (n < 1) exit(4);
    a.dropped += (unsigned long long)n;
  }
  void clip(int32_t n) {
    if (n < 1) exit(4);
    a.clipped += (unsigned long long)n;
  }
  void bad_index() { a.bad = 1; }
  // (.at(): an index out of range ends the program)
  void add(int32_t bin, int32_t n, double re, double im, double wabs) {
    if (bin < 0 || n < 1) exit(4);
    a.cnt.at((size_t)bin) += n;
    a.re.at((size_t)bin) += re;
    a.im.at((size_t)bin) += im;
    a.wabs.at((size_t)bin) += wabs;
  }
};

bool same_bits(const std::vector<double>& x, const std::vector<double>& y) {
  return x.size() == y.size() && (x.empty() || memcmp(x.data(), y.data(), x.size() * sizeof(double)) == 0);
}

}  // namespace

int main() {
  rwrt_wave_map wm = {};
  wm.nx = read_int();
  wm.ny = read_int();
  wm.nchan = read_int();
  wm.need = read_int();
  wm.wcol = read_int();
  wm.spread = read_int();
  const int nray = read_int();
  wm.lat0 = read_double();
  wm.inv_dlat = read_double();
  wm.inv_dlon = read_double();
  wm.max_sep = read_double();
  wm.omega_dt = read_double();
  wm.d_floor = read_double();
  auto column = [](int c) { return c == -1 || (c >= 2 && c <= 6); };
  if (wm.nx <= 0 || wm.ny <= 0 || wm.nchan <= 0 || !column(wm.need) || !column(wm.wcol) ||
      (wm.spread != 0 && wm.spread != 1) || nray < 0 || !(wm.inv_dlat > 0.0) || !(wm.inv_dlon > 0.0) ||
      !std::isfinite(wm.lat0) || !(wm.max_sep > 0.0) || !std::isfinite(wm.omega_dt) || !(wm.d_floor >= 0.0) ||
      !std::isfinite(wm.d_floor))
    return 2;
  std::vector<double> theta0((size_t)nray);
  for (auto& v : theta0) v = read_double();
  std::vector<int32_t> nbr((size_t)4 * nray);   // (any value: an index out of range must not be followed)
  for (auto& v : nbr) v = read_int();
  const size_t nmap = (size_t)wm.nchan * wm.ny * wm.nx;
  Arrays walked(nmap, nray, theta0), each(nmap, nray, theta0);
  PlainEmitter ew{walked}, ee{each};
  const rwrt::WaveMaps m = rwrt::wave_maps(wm);

  const int nlaunch = read_int();
  long long rays = 0;
  for (int q = 0; q < nlaunch; ++q) {
    host_input::Launch in;
    in.read();
    if (in.nray != nray || in.it_begin < 0) return 2;
    const rwrt::LaunchRows L = in.rows();
    for (int j = 0; j < nray; ++j) {
      const int32_t ch = in.chan[j];
      if (ch < 0 || ch >= wm.nchan) continue;   // (as the kernel: not walked, its columns stay)
      // walked as the kernel walks it
      rwrt::WaveState s = rwrt::wave_state_load(walked.si.data(), walked.sf.data(), nray, j);
      rwrt::wave_ray<2>(L, (int64_t)j, (int64_t)nray, nbr.data(), m, ch, s, ew);
      rwrt::wave_state_store(s, walked.si.data(), walked.sf.data(), nray, j);
      // and row by row
      rwrt::WaveState r = rwrt::wave_state_load(each.si.data(), each.sf.data(), nray, j);
      const rwrt::LaunchRowsSpan own = rwrt::launch_rows_span(L, (int64_t)j);
      const rwrt::TubeStencil st = rwrt::wave_begin(L, (int64_t)j, (int64_t)nray, nbr.data(), m, r, ee);
      for (int i = L.it_begin; i < L.it_end; ++i)
        rwrt::wave_row(r, L, st, (int64_t)j, i, rwrt::phase_load(rwrt::tube_row_ptr(L, own, j, i), m.phase), m, ch, ee);
      rwrt::wave_state_store(r, each.si.data(), each.sf.data(), nray, j);
    }
    rays += nray;
  }
  if (walked.cnt != each.cnt || walked.dropped != each.dropped || walked.clipped != each.clipped ||
      walked.si != each.si || !same_bits(walked.sf, each.sf) || walked.bad != each.bad) {
    fprintf(stderr, "the tails' counts, drops, clipped deposits or states differ from the row-by-row walk\n");
    return 3;
  }
  for (size_t k = 0; k < nmap; ++k) printf("%lld ", walked.cnt[k]);
  printf("\n");
  for (const auto* a : {&walked.re, &walked.im, &walked.wabs}) {
    for (size_t k = 0; k < nmap; ++k) printf("%a ", (*a)[k]);
    printf("\n");
  }
  printf("dropped %llu clipped %llu bad %d\n", walked.dropped, walked.clipped, walked.bad);
  for (size_t k = 0; k < walked.si.size(); ++k) printf("%d ", walked.si[k]);
  printf("\n");
  for (size_t k = 0; k < walked.sf.size(); ++k) printf("%a ", walked.sf[k]);
  printf("\n");
  fprintf(stderr, "wave_rows_main ok: %lld rays in %d launches\n", rays, nlaunch);
  return 0;
}
