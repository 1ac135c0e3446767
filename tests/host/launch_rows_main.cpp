// Stand-alone host program over csrc/launch_rows.h (how the density and the
// summary kernels read a launch's rows), built by tests/support/hostprog.py
// with -fsanitize=undefined,address,float-cast-overflow
// -fno-sanitize-recover=all and run directly.  Every array is a heap block of
// exactly the size given, so a read through a missing row block, past the end
// of the buffer or of an absent array aborts the run.
//
// stdin:  layout nray it_begin it_end nvals    layout 0 dense, 1 tails, 2 row blocks;
//                                              nvals: the doubles of the row buffer
//         tail_from[nray]                      (layout >= 1)
//         row_slot[nray]                       (layout 2)
//         the row buffer, nvals doubles
//         tail_row[nray][8]                    (layout >= 1)
// stdout: "R <ray> <row index> <lon> <column 7>" for every row read, in the
//         walk's order, and "T <ray> <tf> <count> <lon> <column 7>" per tail.
#include <cstdio>
#include <cstdlib>

#include "launch_rows.h"

namespace {

struct Cell {
  double lon, last;
};

template <class V>
V* read_array(long n, const char* fmt) {
  V* a = new V[n];
  for (long k = 0; k < n; ++k)
    if (scanf(fmt, &a[k]) != 1) exit(2);
  return a;
}

}  // namespace

int main() {
  int layout, it_begin, it_end;
  long nray, nvals;
  if (scanf("%d %ld %d %d %ld", &layout, &nray, &it_begin, &it_end, &nvals) != 5) return 2;
  int32_t* tail_from = layout >= 1 ? read_array<int32_t>(nray, "%d") : nullptr;
  int32_t* row_slot = layout == 2 ? read_array<int32_t>(nray, "%d") : nullptr;
  double* rows = read_array<double>(nvals, "%lf");
  double* tail_row = layout >= 1 ? read_array<double>(nray * RWRT_NOUT, "%lf") : nullptr;
  const rwrt::LaunchRows L{rows, row_slot, tail_from, tail_row, it_begin, it_end};
  for (long j = 0; j < nray; ++j) {
    const rwrt::LaunchRowsSpan s = rwrt::launch_rows_span(L, j);
    if (s.nread < 0 || s.nread > it_end - it_begin || (s.nread > 0) != (s.block != nullptr)) return 3;
    rwrt::launch_rows_walk<4, Cell>(
        L, j, [](const double* r) { return Cell{r[0], r[RWRT_NOUT - 1]}; },
        [&](int32_t i, const Cell& c) { printf("R %ld %d %.17g %.17g\n", j, i, c.lon, c.last); },
        [&](int32_t tf, int32_t n, const Cell& c) { printf("T %ld %d %d %.17g %.17g\n", j, tf, n, c.lon, c.last); });
  }
  delete[] tail_from;
  delete[] row_slot;
  delete[] rows;
  delete[] tail_row;
  return 0;
}
