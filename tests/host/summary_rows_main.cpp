// Stand-alone host program over csrc/summary_rows.h (the per-row update the
// summary kernel uses), built by tests/support/hostprog.py with
// -fsanitize=undefined,address,float-cast-overflow -fno-sanitize-recover=all
// and run directly.
//
// Every ray's rows are fed chunk by chunk, the way launches deliver them: the
// accumulator is carried from chunk to chunk, and inside a chunk the rows from
// tail_from on are one constant tail.  Each ray is reduced twice -- the tail
// through summary_tail (the closed form) and row by row -- and the program
// fails (exit 3) if the two accumulators differ in any bit.
//
// stdin:  nreg                                   (doubles as hex floats, %a)
//         lon_w lon_e lat_s lat_n                (nreg lines, radians)
//         nray nt nchunk
//         b_0 .. b_nchunk                        (chunk bounds, b_0 = 0, b_nchunk = nt)
//         per ray: nchunk tail_from values, then nt lines "lon lat l amp"
// stdout: one line per ray: the 9 fp64 fields as bit patterns (hex), then
//         n_valid last_row n_turn prev_valid, first_row[nreg], rows_inside[nreg]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "launch_input.h"
#include "summary_rows.h"

namespace {

struct Row {
  double lon, lat, l, amp;
};

using host_input::read_double;

unsigned long long bits(double x) {
  unsigned long long u;
  memcpy(&u, &x, sizeof u);
  return u;
}

template <int NR>
bool same(const rwrt::SummaryAcc<NR>& a, const rwrt::SummaryAcc<NR>& b, int nreg) {
  const double fa[9] = {a.lon_first, a.lat_first, a.lon_last, a.lat_last, a.l_last, a.lat_min, a.lat_max, a.amp_max, a.path};
  const double fb[9] = {b.lon_first, b.lat_first, b.lon_last, b.lat_last, b.l_last, b.lat_min, b.lat_max, b.amp_max, b.path};
  for (int k = 0; k < 9; ++k)
    if (bits(fa[k]) != bits(fb[k])) return false;
  if (a.n_valid != b.n_valid || a.last_row != b.last_row || a.n_turn != b.n_turn || a.prev_valid != b.prev_valid)
    return false;
  for (int r = 0; r < nreg && r < NR; ++r)
    if (a.first_row[r] != b.first_row[r] || a.rows_inside[r] != b.rows_inside[r]) return false;
  return true;
}

template <int NR>
int run(const rwrt_summary_regions& reg) {
  int nray, nt, nchunk;
  if (scanf("%d %d %d", &nray, &nt, &nchunk) != 3 || nray < 0 || nt < 1 || nchunk < 1) return 2;
  std::vector<int> bound(nchunk + 1), tf(nchunk);
  for (int c = 0; c <= nchunk; ++c)
    if (scanf("%d", &bound[c]) != 1) return 2;
  if (bound[0] != 0 || bound[nchunk] != nt) return 2;
  std::vector<Row> rows(nt);
  for (int j = 0; j < nray; ++j) {
    for (int c = 0; c < nchunk; ++c) {
      if (scanf("%d", &tf[c]) != 1 || tf[c] < bound[c] || tf[c] > bound[c + 1]) return 2;
    }
    for (int i = 0; i < nt; ++i) {
      rows[i].lon = read_double();
      rows[i].lat = read_double();
      rows[i].l = read_double();
      rows[i].amp = read_double();
    }
    rwrt::SummaryAcc<NR> closed, each;
    for (int c = 0; c < nchunk; ++c) {
      // (a launch: the accumulator is stored after a chunk and loaded before the next)
      rwrt::SummaryAcc<NR> a = closed, b = each;
      for (int i = bound[c]; i < tf[c]; ++i) {
        rwrt::summary_row<NR>(a, reg, i, rows[i].lon, rows[i].lat, rows[i].l, rows[i].amp);
        rwrt::summary_row<NR>(b, reg, i, rows[i].lon, rows[i].lat, rows[i].l, rows[i].amp);
      }
      if (tf[c] < bound[c + 1]) {
        const Row& t = rows[tf[c]];
        rwrt::summary_tail<NR>(a, reg, tf[c], bound[c + 1] - tf[c], t.lon, t.lat, t.l, t.amp);
        for (int i = tf[c]; i < bound[c + 1]; ++i) rwrt::summary_row<NR>(b, reg, i, t.lon, t.lat, t.l, t.amp);
      }
      closed = a;
      each = b;
    }
    if (!same<NR>(closed, each, reg.nreg)) {
      fprintf(stderr, "ray %d: the tail's closed form differs from the row-by-row update\n", j);
      return 3;
    }
    const double f[9] = {closed.lon_first, closed.lat_first, closed.lon_last, closed.lat_last, closed.l_last,
                         closed.lat_min,   closed.lat_max,   closed.amp_max,  closed.path};
    for (int k = 0; k < 9; ++k) printf("%016llx ", bits(f[k]));
    printf("%d %d %d %d", closed.n_valid, closed.last_row, closed.n_turn, closed.prev_valid);
    for (int r = 0; r < reg.nreg && r < NR; ++r) printf(" %d", closed.first_row[r]);
    for (int r = 0; r < reg.nreg && r < NR; ++r) printf(" %d", closed.rows_inside[r]);
    printf("\n");
  }
  fprintf(stderr, "summary_rows_main ok: %d rays x %d rows in %d chunks\n", nray, nt, nchunk);
  return 0;
}

}  // namespace

int main() {
  rwrt_summary_regions reg = {};
  if (scanf("%d", &reg.nreg) != 1 || reg.nreg < 0 || reg.nreg > RWRT_SUMMARY_MAXREG) return 2;
  for (int r = 0; r < reg.nreg; ++r)
    for (int k = 0; k < 4; ++k) reg.box[r][k] = read_double();
  // (the accumulator sizes the kernel is instantiated with)
  if (reg.nreg == 0) return run<0>(reg);
  if (reg.nreg <= 2) return run<2>(reg);
  return run<8>(reg);
}
