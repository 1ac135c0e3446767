// Stand-alone host program over csrc/flux_rows.h (the accept rule, the bin and
// the per-ray walk the flux kernel uses), built by tests/support/hostprog.py with
// -fsanitize=undefined,address,float-cast-overflow -fno-sanitize-recover=all
// -ffp-contract=off and run directly.
//
// Launches are walked the way the kernel walks them, ray by ray, with an
// emitter that updates plain arrays instead of issuing atomics.  Every buffer
// has exactly the size its launch gives it, so a row, a tail or a bin read or
// written out of range is the sanitizer's finding.  Each ray is also reduced
// row by row (its tail expanded), and the program fails (exit 3) if a tail's
// count or row sum differs from that.
//
// stdin:  nx ny nchan mode lon0 inv_dlon lat0 inv_dlat s2_min s2_max wn_max   (doubles as hex floats, %a)
//         nlaunch
//         per launch: nray it_begin it_end has_tails has_slots nblock
//                     chan[nray]
//                     with tails: tail_from[nray], then nray lines of 8 doubles
//                     with slots: row_slot[nray]
//                     nblock * (it_end - it_begin) lines of 8 doubles
// stdout: cnt[nbins][2] as integers, sum[nbins][3] as hex floats, one line
//         each; then one line "emits <add_cnt calls> <add_sum calls>"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flux_rows.h"
#include "launch_input.h"

namespace {

using host_input::read_double;
using host_input::read_int;

struct Arrays {
  std::vector<long long> cnt;
  std::vector<double> sum;
  long long n_cnt = 0, n_sum = 0;

  explicit Arrays(size_t nbins) : cnt(2 * nbins, 0), sum(3 * nbins, 0.0) {}
};

struct PlainEmitter {
  Arrays& a;
  // (.at(): an index out of range ends the program)
  void add_cnt(int64_t index, unsigned long long n, long long rowsum) {
    if (index < 0) exit(4);
    a.cnt.at(2 * (size_t)index) += (long long)n;
    a.cnt.at(2 * (size_t)index + 1) += rowsum;
    ++a.n_cnt;
  }
  void add_sum(int64_t index, double fx, double fy, double fs) {
    if (index < 0) exit(4);
    a.sum.at(3 * (size_t)index) += fx;
    a.sum.at(3 * (size_t)index + 1) += fy;
    a.sum.at(3 * (size_t)index + 2) += fs;
    ++a.n_sum;
  }
};

}  // namespace

int main() {
  rwrt_flux_map m = {};
  m.nx = read_int();
  m.ny = read_int();
  m.nchan = read_int();
  m.mode = read_int();
  m.lon0 = read_double();
  m.inv_dlon = read_double();
  m.lat0 = read_double();
  m.inv_dlat = read_double();
  m.s2_min = read_double();
  m.s2_max = read_double();
  m.wn_max = read_double();
  if (m.nx <= 0 || m.ny <= 0 || m.nchan <= 0 || m.mode < 0 || m.mode >= 4) return 2;
  const size_t nbins = (size_t)m.nx * m.ny * m.nchan;
  Arrays walked(nbins), each(nbins);
  PlainEmitter ew{walked}, ee{each};

  const int nlaunch = read_int();
  long long rays = 0;
  for (int q = 0; q < nlaunch; ++q) {
    host_input::Launch in;
    in.read();
    const int nray = in.nray, it_begin = in.it_begin, it_end = in.it_end;
    const std::vector<int32_t>& chan = in.chan;
    const rwrt::LaunchRows L = in.rows();
    for (int j = 0; j < nray; ++j) {
      rwrt::flux_ray<4>(L, j, chan[j], m, ew);
      // the same ray row by row, its tail expanded
      if (chan[j] < 0 || chan[j] >= m.nchan) continue;
      const rwrt::LaunchRowsSpan s = rwrt::launch_rows_span(L, j);
      rwrt::FluxRun run;
      for (int i = it_begin; i < it_end; ++i) {
        const double* r = i < s.tf ? s.block + (size_t)(i - it_begin) * RWRT_NOUT : L.tail_row + (size_t)j * RWRT_NOUT;
        rwrt::flux_points(run, i, 1, rwrt::flux_point(rwrt::flux_load(r), chan[j], m), ee);
      }
      rwrt::flux_flush(run, ee);
    }
    rays += nray;
  }
  if (walked.cnt != each.cnt) {
    fprintf(stderr, "the tails' count or row sum differs from the row-by-row walk\n");
    return 3;
  }
  for (size_t k = 0; k < walked.cnt.size(); ++k) printf("%lld ", walked.cnt[k]);
  printf("\n");
  for (size_t k = 0; k < walked.sum.size(); ++k) printf("%a ", walked.sum[k]);
  printf("\n");
  printf("emits %lld %lld\n", walked.n_cnt, walked.n_sum);
  fprintf(stderr, "flux_rows_main ok: %lld rays in %d launches\n", rays, nlaunch);
  return 0;
}
