// Stand-alone host program over csrc/arrival_rows.h (the per-ray walk the
// arrival kernel uses), built by tests/support/hostprog.py with
// -fsanitize=undefined,address,float-cast-overflow -fno-sanitize-recover=all
// and run directly.
//
// Launches are walked the way the kernel walks them, ray by ray, with an
// emitter that updates plain arrays instead of issuing atomics.  Every buffer
// has exactly the size its launch gives it, so a row, a tail or a bin read or
// written out of range is the sanitizer's finding.  Each ray is also reduced
// row by row (its tail expanded), and the program fails (exit 3) if a tail's
// window split gives another array than that.
//
// stdin:  nx ny nchan wcol inv_dlon lat0 inv_dlat window_rows nwin   (doubles as hex floats, %a)
//         nlaunch
//         per launch: nray it_begin it_end has_tails has_slots nblock
//                     chan[nray]
//                     with tails: tail_from[nray], then nray lines of 8 doubles
//                     with slots: row_slot[nray]
//                     nblock * (it_end - it_begin) lines of 8 doubles
// stdout: first[nbins], last[nbins], then count[nwin * nbins] when window_rows > 0,
//         one line each; then one line "emits <first> <last> <count>"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "arrival_rows.h"
#include "launch_input.h"

namespace {

using host_input::read_double;
using host_input::read_int;

struct Arrays {
  std::vector<int32_t> first, last;
  std::vector<long long> count;
  long long n_first = 0, n_last = 0, n_count = 0;

  Arrays(size_t nbins, size_t ncount) : first(nbins, 0x7fffffff), last(nbins, -1), count(ncount, 0) {}
  // (.at(): an index out of range ends the program)
  void emit_first(int32_t b, int32_t row) {
    int32_t& f = first.at((size_t)b);
    f = row < f ? row : f;
    ++n_first;
  }
  void emit_last(int32_t b, int32_t row) {
    int32_t& l = last.at((size_t)b);
    l = row > l ? row : l;
    ++n_last;
  }
  void emit_count(int64_t index, unsigned long long n) {
    if (index < 0) exit(4);
    count.at((size_t)index) += (long long)n;
    ++n_count;
  }
};

struct PlainEmitter {
  Arrays& a;
  void first(int32_t b, int32_t row) { a.emit_first(b, row); }
  void last(int32_t b, int32_t row) { a.emit_last(b, row); }
  void count(int64_t index, unsigned long long n) { a.emit_count(index, n); }
};

}  // namespace

int main() {
  rwrt_arrival_map m = {};
  m.bins.nx = read_int();
  m.bins.ny = read_int();
  m.bins.nchan = read_int();
  m.bins.wcol = read_int();
  m.bins.inv_dlon = read_double();
  m.bins.lat0 = read_double();
  m.bins.inv_dlat = read_double();
  m.window_rows = read_int();
  m.nwin = read_int();
  if (m.bins.nx <= 0 || m.bins.ny <= 0 || m.bins.nchan <= 0 || m.window_rows < 0 || m.nwin < 0) return 2;
  const size_t nbins = (size_t)m.bins.nx * m.bins.ny * m.bins.nchan;
  const size_t ncount = m.window_rows > 0 ? nbins * (size_t)m.nwin : 0;
  Arrays walked(nbins, ncount), each(nbins, ncount);
  PlainEmitter ew{walked}, ee{each};

  const int nlaunch = read_int();
  long long rays = 0;
  for (int q = 0; q < nlaunch; ++q) {
    host_input::Launch in;
    in.read();
    const int nray = in.nray, it_begin = in.it_begin, it_end = in.it_end;
    const std::vector<int32_t>& chan = in.chan;
    if (it_begin < 0) return 2;
    if (m.window_rows > 0 && (long long)it_end > (long long)m.nwin * m.window_rows) return 2;
    const rwrt::LaunchRows L = in.rows();
    for (int j = 0; j < nray; ++j) {
      rwrt::arrival_ray<4>(L, j, chan[j], m, ew);
      // the same ray row by row, its tail expanded
      if (chan[j] < 0 || chan[j] >= m.bins.nchan) continue;
      const int col = m.bins.wcol >= 0 ? m.bins.wcol : 0;
      const rwrt::LaunchRowsSpan s = rwrt::launch_rows_span(L, j);
      rwrt::ArrivalRun run = rwrt::arrival_begin(m, it_begin);
      for (int i = it_begin; i < it_end; ++i) {
        const double* r = i < s.tf ? s.block + (size_t)(i - it_begin) * RWRT_NOUT : L.tail_row + (size_t)j * RWRT_NOUT;
        const rwrt::ArrivalRow v = rwrt::arrival_load(r, col);
        const int32_t b = rwrt::density_bin(rwrt::density_wrap_2pi(v.lon), v.lat, v.req, chan[j], m.bins);
        rwrt::arrival_points(run, m, i, 1, b, ee);
      }
      rwrt::arrival_flush(run, m, ee);
    }
    rays += nray;
  }
  if (walked.first != each.first || walked.last != each.last || walked.count != each.count) {
    fprintf(stderr, "the tails' window split differs from the row-by-row walk\n");
    return 3;
  }
  for (size_t b = 0; b < nbins; ++b) printf("%d ", walked.first[b]);
  printf("\n");
  for (size_t b = 0; b < nbins; ++b) printf("%d ", walked.last[b]);
  printf("\n");
  if (m.window_rows > 0) {
    for (size_t k = 0; k < ncount; ++k) printf("%lld ", walked.count[k]);
    printf("\n");
  }
  printf("emits %lld %lld %lld\n", walked.n_first, walked.n_last, walked.n_count);
  fprintf(stderr, "arrival_rows_main ok: %lld rays in %d launches\n", rays, nlaunch);
  return 0;
}
