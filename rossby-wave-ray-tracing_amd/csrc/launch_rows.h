// launch_rows.h -- the rows a ray-loop launch leaves on the device, as their
// consumers read them (csrc/density.hip, csrc/summary.hip; host programs too:
// tests/host/launch_rows_main.cpp walks them under the sanitizers).
//
// A launch covers rows [it_begin, it_end) of nray rays, 8 doubles a row:
//   dense        rows[nray][it_end - it_begin][8], every row in the buffer;
//   tails        ray j's rows from tail_from[j] on all equal tail_row[j][8] and
//                are not in the buffer;
//   row blocks   with tails: ray j's rows are block row_slot[j] of the buffer,
//                -1 for a ray without a block (every row is its tail).
#ifndef RWRT_LAUNCH_ROWS_H
#define RWRT_LAUNCH_ROWS_H

#include <cstdint>

#include "abi_host.h"
#include "density_bins.h"   // RWRT_HD

namespace rwrt {

struct LaunchRows {
  const double* rows;
  const int32_t* row_slot;    // NULL: ray j's block is j
  const int32_t* tail_from;   // NULL (with tail_row): no tails
  const double* tail_row;
  int32_t it_begin, it_end;
};

// Ray j's rows [it_begin, tf) are the first nread rows of `block`, its rows
// [tf, it_end) repeat tail_row[j].  `block` is formed only for nread > 0: a ray
// without a block never yields a pointer in front of the buffer.
struct LaunchRowsSpan {
  const double* block;
  int32_t nread, tf;
};

RWRT_HD inline LaunchRowsSpan launch_rows_span(const LaunchRows& L, int64_t j) {
  int32_t tf = L.it_end;
  if (L.tail_from) {
    tf = L.tail_from[j];
    tf = (tf < L.it_begin) ? L.it_begin : tf;
    tf = (tf > L.it_end) ? L.it_end : tf;
  }
  int64_t blk = j;
  if (L.row_slot) {
    blk = L.row_slot[j];
    if (blk < 0) tf = L.it_begin;   // no block: every row is the tail
  }
  const int32_t nread = tf - L.it_begin;
  return {nread > 0 ? L.rows + blk * (int64_t)(L.it_end - L.it_begin) * RWRT_NOUT : nullptr, nread, tf};
}

// Ray j's rows in order: row(i, load(row i)) for every row i that is read --
// BATCH loads issued ahead of their uses, then the remainder one at a time --
// and tail(tf, it_end - tf, load(the tail row)) once when there is a tail.
// `load` takes a row's 8 doubles and returns T.
template <int BATCH, class T, class Load, class Row, class Tail>
RWRT_HD inline void launch_rows_walk(const LaunchRows& L, int64_t j, Load load, Row row, Tail tail) {
  const LaunchRowsSpan s = launch_rows_span(L, j);
  if (s.nread > 0) {
    const double* __restrict__ r = s.block;
    int32_t i = 0;
    for (; i + BATCH <= s.nread; i += BATCH) {
      T v[BATCH];
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int k = 0; k < BATCH; ++k) v[k] = load(r + (int64_t)(i + k) * RWRT_NOUT);
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int k = 0; k < BATCH; ++k) row(L.it_begin + i + k, v[k]);
    }
    for (; i < s.nread; ++i) row(L.it_begin + i, load(r + (int64_t)i * RWRT_NOUT));
  }
  if (s.tf < L.it_end) tail(s.tf, L.it_end - s.tf, load(L.tail_row + j * RWRT_NOUT));
}

// The row arguments of the entry point `fn`, checked on the host before the
// first HIP call.  nray == 0 needs no d_rows.
inline rwrt_status check_launch_rows(const char* fn, int64_t nray, int32_t it_begin, int32_t it_end,
                                     const double* d_rows, const int32_t* d_row_slot, const int32_t* d_tail_from,
                                     const double* d_tail_row) {
  const char* bad = nullptr;
  if (it_end <= it_begin) bad = "%s: need it_begin < it_end";
  else if (nray < 0 || nray > 0x7fffffffLL) bad = "%s: nray out of range";
  else if (!d_tail_from != !d_tail_row) bad = "%s: tails need both d_tail_from and d_tail_row";
  else if (d_row_slot && !d_tail_from) bad = "%s: d_row_slot needs tails (d_tail_from, d_tail_row)";
  else if (nray > 0 && !d_rows) bad = "%s: d_rows is NULL";
  else if (nray > 0 && (reinterpret_cast<uintptr_t>(d_rows) | reinterpret_cast<uintptr_t>(d_tail_row)) % 16 != 0)
    bad = "%s: d_rows and d_tail_row must be 16-byte aligned";
  return bad ? fail(RWRT_ERR_ARG, bad, fn) : RWRT_OK;
}

}  // namespace rwrt

#endif  // RWRT_LAUNCH_ROWS_H
