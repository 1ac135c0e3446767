// Stand-alone host program over csrc/cross_lines.h (a row's side of every gate,
// the crossing of a segment whose sides differ and the per-ray walk the cross
// kernel uses), built by tests/support/hostprog.py with
// -fsanitize=undefined,address,float-cast-overflow -fno-sanitize-recover=all
// -ffp-contract=off and run directly.
//
// Launches are walked the way the kernel walks them, ray by ray, ray j in
// column j of the carried rows and of the per-ray arrays, with an emitter that
// updates plain arrays instead of issuing atomics.  Every buffer has exactly
// the size its launch gives it, so a row, a tail or a bin read or written out
// of range is the sanitizer's finding, and so is a floor converted to an
// integer it does not fit.  Each ray is also walked row by row (its tail
// expanded) with carried rows of its own, and the program fails (exit 3) if a
// tail's counts or drops differ from that.
//
// stdin:  ngate nbin nchan need wcol window_rows nwin
//         per gate: kind pos org inv_d                                      (doubles as hex floats, %a)
//         nlaunch
//         per launch: nray it_begin it_end has_tails has_slots nblock      (nray the same in every launch)
//                     chan[nray]
//                     with tails: tail_from[nray], then nray lines of 8 doubles
//                     with slots: row_slot[nray]
//                     nblock * (it_end - it_begin) lines of 8 doubles
// stdout: cnt[nmap] as integers, tsum[nmap] and wsum[nmap] as hex floats, one
//         line each; "dropped <n>"; ncross[ngate * 2 * nray] as integers and
//         tfirst[ngate * 2 * nray] as hex floats (nan for none), one line each
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cross_lines.h"
#include "launch_input.h"

namespace {

using host_input::read_double;
using host_input::read_int;

struct Arrays {
  std::vector<long long> cnt;
  std::vector<double> tsum, wsum;
  std::vector<int32_t> ncross;   // [ngate][2][nray], sized by the first launch
  std::vector<double> tfirst;
  std::vector<double> prev;      // [3][nray]
  unsigned long long dropped = 0;

  explicit Arrays(size_t nmap) : cnt(nmap, 0), tsum(nmap, 0.0), wsum(nmap, 0.0) {}

  void size_rays(size_t ngate, size_t nray) {
    ncross.assign(ngate * 2 * nray, 0);
    tfirst.assign(ngate * 2 * nray, NAN);   // the caller writes NaN once
    prev.assign(3 * nray, NAN);
  }
};

struct PlainEmitter {
  Arrays& a;
  const rwrt_cross_map& m;
  size_t nray = 0, col = 0;
  int32_t chan = 0;

  void drop() { ++a.dropped; }

  // (.at(): an index out of range ends the program)
  void hit(int32_t g, int32_t d, int32_t w, int32_t bin, double tc, double wv) {
    if (g < 0 || g >= m.ngate || d < 0 || d > 1 || w < 0 || w >= m.nwin || bin < -1 || bin >= m.nbin) exit(4);
    const size_t k = ((size_t)g * 2 + d) * nray + col;
    a.ncross.at(k) += 1;
    if (a.tfirst.at(k) != a.tfirst.at(k)) a.tfirst.at(k) = tc;
    if (bin < 0) return;
    const int64_t index = rwrt::cross_index(m, w, g, d, chan, bin);
    if (index < 0) exit(4);
    a.cnt.at((size_t)index) += 1;
    a.tsum.at((size_t)index) += tc;
    a.wsum.at((size_t)index) += wv;
  }
};

template <int NG>
rwrt::CrossState<NG> load_state(const Arrays& a, size_t nray, size_t j) {
  rwrt::CrossState<NG> s;
  s.lon = a.prev.at(j);
  s.lat = a.prev.at(nray + j);
  s.v = a.prev.at(2 * nray + j);
  for (int g = 0; g < NG; ++g) s.side[g] = NAN;
  return s;
}

template <int NG>
void store_state(Arrays& a, size_t nray, size_t j, const rwrt::CrossState<NG>& s) {
  a.prev.at(j) = s.lon;
  a.prev.at(nray + j) = s.lat;
  a.prev.at(2 * nray + j) = s.v;
}

// one ray of a launch: walked as the kernel walks it, and row by row
template <int NG>
void walk(const rwrt::LaunchRows& L, size_t nray, size_t j, const rwrt_cross_map& m, Arrays& walked, PlainEmitter& ew,
          Arrays& each, PlainEmitter& ee) {
  rwrt::CrossState<NG> s = load_state<NG>(walked, nray, j);
  rwrt::cross_ray<NG, 4>(L, (int64_t)j, m, s, ew);
  store_state<NG>(walked, nray, j, s);
  const rwrt::LaunchRowsSpan sp = rwrt::launch_rows_span(L, (int64_t)j);
  rwrt::CrossState<NG> r = load_state<NG>(each, nray, j);
  rwrt::cross_begin<NG>(m, r);
  for (int i = L.it_begin; i < L.it_end; ++i) {
    const double* p = i < sp.tf ? sp.block + (size_t)(i - L.it_begin) * RWRT_NOUT : L.tail_row + j * RWRT_NOUT;
    rwrt::cross_row<NG>(r, i, rwrt::cross_load(p, m), m, ee);
  }
  store_state<NG>(each, nray, j, r);
}

}  // namespace

int main() {
  rwrt_cross_map m = {};
  m.ngate = read_int();
  m.nbin = read_int();
  m.nchan = read_int();
  m.need = read_int();
  m.wcol = read_int();
  m.window_rows = read_int();
  m.nwin = read_int();
  auto column_ok = [](int c) { return c == -1 || (c >= 2 && c <= 6); };
  if (m.ngate < 1 || m.ngate > RWRT_CROSS_MAXGATE || m.nbin <= 0 || m.nchan <= 0 || !column_ok(m.need) ||
      !column_ok(m.wcol) || m.window_rows < 0 || m.nwin < 1 || (m.window_rows == 0 && m.nwin != 1))
    return 2;
  for (int g = 0; g < m.ngate; ++g) {
    m.gate[g].kind = read_int();
    m.gate[g].pos = read_double();
    m.gate[g].org = read_double();
    m.gate[g].inv_d = read_double();
    if (m.gate[g].kind != 0 && m.gate[g].kind != 1) return 2;
  }
  const size_t nmap = (size_t)m.nwin * m.ngate * 2 * m.nchan * m.nbin;
  Arrays walked(nmap), each(nmap);
  PlainEmitter ew{walked, m}, ee{each, m};

  const int nlaunch = read_int();
  long long rays = 0;
  int nray0 = -1;
  for (int q = 0; q < nlaunch; ++q) {
    host_input::Launch in;
    in.read();
    const int nray = in.nray, it_begin = in.it_begin, it_end = in.it_end;
    const std::vector<int32_t>& chan = in.chan;
    if (it_begin < 0) return 2;
    if (m.window_rows > 0 && (long long)it_end - 1 > (long long)m.nwin * m.window_rows) return 2;
    if (nray0 < 0) {
      nray0 = nray;
      walked.size_rays(m.ngate, nray);
      each.size_rays(m.ngate, nray);
      ew.nray = ee.nray = (size_t)nray;
    } else if (nray != nray0) {
      return 2;
    }
    const rwrt::LaunchRows L = in.rows();
    for (int j = 0; j < nray; ++j) {
      if (chan[j] < 0 || chan[j] >= m.nchan) continue;   // (as the kernel: not walked, its columns stay)
      ew.col = ee.col = (size_t)j;
      ew.chan = ee.chan = chan[j];
      switch (m.ngate) {   // (the kernel's instantiations)
        case 1: walk<1>(L, nray, j, m, walked, ew, each, ee); break;
        case 2: walk<2>(L, nray, j, m, walked, ew, each, ee); break;
        case 3: walk<3>(L, nray, j, m, walked, ew, each, ee); break;
        case 4: walk<4>(L, nray, j, m, walked, ew, each, ee); break;
        case 5: walk<5>(L, nray, j, m, walked, ew, each, ee); break;
        case 6: walk<6>(L, nray, j, m, walked, ew, each, ee); break;
        case 7: walk<7>(L, nray, j, m, walked, ew, each, ee); break;
        default: walk<8>(L, nray, j, m, walked, ew, each, ee); break;
      }
    }
    rays += nray;
  }
  if (walked.cnt != each.cnt || walked.dropped != each.dropped || walked.ncross != each.ncross) {
    fprintf(stderr, "the tails' crossings or drops differ from the row-by-row walk\n");
    return 3;
  }
  for (size_t k = 0; k < nmap; ++k) printf("%lld ", walked.cnt[k]);
  printf("\n");
  for (size_t k = 0; k < nmap; ++k) printf("%a ", walked.tsum[k]);
  printf("\n");
  for (size_t k = 0; k < nmap; ++k) printf("%a ", walked.wsum[k]);
  printf("\n");
  printf("dropped %llu\n", walked.dropped);
  for (size_t k = 0; k < walked.ncross.size(); ++k) printf("%d ", walked.ncross[k]);
  printf("\n");
  for (size_t k = 0; k < walked.tfirst.size(); ++k) printf("%a ", walked.tfirst[k]);
  printf("\n");
  fprintf(stderr, "cross_lines_main ok: %lld rays in %d launches\n", rays, nlaunch);
  return 0;
}
