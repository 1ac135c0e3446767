// Stand-alone host program over csrc/track_cells.h (the drop rule, the walk
// through the cells of a segment and the per-ray run the track kernel uses),
// built by tests/support/hostprog.py with
// -fsanitize=undefined,address,float-cast-overflow -fno-sanitize-recover=all
// -ffp-contract=off and run directly.
//
// Launches are walked the way the kernel walks them, ray by ray, ray j in
// column j of the carried rows, with an emitter that updates plain arrays
// instead of issuing atomics.  Every buffer has exactly the size its launch
// gives it, so a row, a tail or a cell read or written out of range is the
// sanitizer's finding, and so is a floor converted to an integer it does not
// fit.  Each ray is also walked row by row (its tail expanded) with carried
// rows of its own, and the program fails (exit 3) if a tail's visits or drops
// differ from that.
//
// stdin:  nx ny nchan mode need wcol max_cells lon0 inv_dlon lat0 inv_dlat   (doubles as hex floats, %a)
//         nlaunch
//         per launch: nray it_begin it_end has_tails has_slots nblock      (nray the same in every launch)
//                     chan[nray]
//                     with tails: tail_from[nray], then nray lines of 8 doubles
//                     with slots: row_slot[nray]
//                     nblock * (it_end - it_begin) lines of 8 doubles
// stdout: cnt[ncells] as integers, time[ncells] and wsum[ncells] as hex
//         floats, one line each; then "dropped <n>" and "flushes <add calls>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "launch_input.h"
#include "track_cells.h"

namespace {

using host_input::read_double;
using host_input::read_int;

struct Arrays {
  std::vector<long long> cnt;
  std::vector<double> time, wsum;
  std::vector<double> prev;   // [3][nray], sized by the first launch
  unsigned long long dropped = 0;
  long long flushes = 0;

  explicit Arrays(size_t ncells) : cnt(ncells, 0), time(ncells, 0.0), wsum(ncells, 0.0) {}
};

struct PlainEmitter {
  Arrays& a;
  // (.at(): an index out of range ends the program)
  void add(int64_t index, unsigned long long n, double w, double wv) {
    if (index < 0) exit(4);
    a.cnt.at((size_t)index) += (long long)n;
    a.time.at((size_t)index) += w;
    a.wsum.at((size_t)index) += wv;
    ++a.flushes;
  }
};

rwrt::TrackState load_state(const Arrays& a, size_t nray, size_t j) {
  rwrt::TrackState s;
  s.lon = a.prev.at(j);
  s.lat = a.prev.at(nray + j);
  s.v = a.prev.at(2 * nray + j);
  return s;
}

void store_state(Arrays& a, size_t nray, size_t j, const rwrt::TrackState& s) {
  a.prev.at(j) = s.lon;
  a.prev.at(nray + j) = s.lat;
  a.prev.at(2 * nray + j) = s.v;
  a.dropped += s.dropped;
}

}  // namespace

int main() {
  rwrt_track_map m = {};
  m.nx = read_int();
  m.ny = read_int();
  m.nchan = read_int();
  m.mode = read_int();
  m.need = read_int();
  m.wcol = read_int();
  m.max_cells = read_int();
  m.lon0 = read_double();
  m.inv_dlon = read_double();
  m.lat0 = read_double();
  m.inv_dlat = read_double();
  auto column_ok = [](int c) { return c == -1 || (c >= 2 && c <= 6); };
  if (m.nx <= 0 || m.ny <= 0 || m.nchan <= 0 || (m.mode != 0 && m.mode != 2) || m.max_cells < 1 ||
      !column_ok(m.need) || !column_ok(m.wcol))
    return 2;
  const size_t ncells = (size_t)m.nx * m.ny * m.nchan;
  Arrays walked(ncells), each(ncells);
  PlainEmitter ew{walked}, ee{each};

  const int nlaunch = read_int();
  long long rays = 0;
  int nray0 = -1;
  for (int q = 0; q < nlaunch; ++q) {
    host_input::Launch in;
    in.read();
    const int nray = in.nray, it_begin = in.it_begin, it_end = in.it_end;
    const std::vector<int32_t>& chan = in.chan;
    if (it_begin < 0) return 2;
    if (nray0 < 0) {
      nray0 = nray;
      walked.prev.assign((size_t)3 * nray, NAN);   // the caller writes NaN once
      each.prev.assign((size_t)3 * nray, NAN);
    } else if (nray != nray0) {
      return 2;
    }
    const rwrt::LaunchRows L = in.rows();
    for (int j = 0; j < nray; ++j) {
      if (chan[j] < 0 || chan[j] >= m.nchan) continue;   // (as the kernel: not walked, its column stays)
      rwrt::TrackState s = load_state(walked, nray, j);
      rwrt::track_ray<4>(L, j, chan[j], m, s, ew);
      store_state(walked, nray, j, s);
      // the same ray row by row, its tail expanded
      const rwrt::LaunchRowsSpan sp = rwrt::launch_rows_span(L, j);
      rwrt::TrackState r = load_state(each, nray, j);
      for (int i = it_begin; i < it_end; ++i) {
        const double* p = i < sp.tf ? sp.block + (size_t)(i - it_begin) * RWRT_NOUT
                                    : L.tail_row + (size_t)j * RWRT_NOUT;
        rwrt::track_rows(r, rwrt::track_load(p, m), 1, chan[j], m, ee);
      }
      rwrt::track_flush(r, ee);
      store_state(each, nray, j, r);
    }
    rays += nray;
  }
  if (walked.cnt != each.cnt || walked.dropped != each.dropped) {
    fprintf(stderr, "the tails' visits or drops differ from the row-by-row walk\n");
    return 3;
  }
  for (size_t k = 0; k < ncells; ++k) printf("%lld ", walked.cnt[k]);
  printf("\n");
  for (size_t k = 0; k < ncells; ++k) printf("%a ", walked.time[k]);
  printf("\n");
  for (size_t k = 0; k < ncells; ++k) printf("%a ", walked.wsum[k]);
  printf("\n");
  printf("dropped %llu\n", walked.dropped);
  printf("flushes %lld\n", walked.flushes);
  fprintf(stderr, "track_cells_main ok: %lld rays in %d launches\n", rays, nlaunch);
  return 0;
}
