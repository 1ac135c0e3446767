// What the stand-alone host programs of tests/host/ share: the readers of
// stdin and one launch in any of the three row layouts, as
// tests/support/rows.py (layout_text) writes it:
//
//   nray it_begin it_end has_tails has_slots nblock
//   chan[nray]
//   with tails: tail_from[nray], then nray lines of 8 doubles   (doubles as hex floats, %a)
//   with slots: row_slot[nray]
//   nblock * (it_end - it_begin) lines of 8 doubles
//
// Every vector has exactly the size its launch gives it, so a row, a tail or
// a slot read out of range is the sanitizer's finding.  A malformed launch
// ends the program with status 2.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "launch_rows.h"

namespace host_input {

inline double read_double() {
  char s[64];
  if (scanf("%63s", s) != 1) exit(2);
  return strtod(s, nullptr);
}

inline int read_int() {
  int v;
  if (scanf("%d", &v) != 1) exit(2);
  return v;
}

struct Launch {
  int nray = 0, it_begin = 0, it_end = 0, has_tails = 0, has_slots = 0, nblock = 0;
  std::vector<int32_t> chan, tail_from, slot;
  std::vector<double> tail_row, block_rows;

  void read() {
    nray = read_int(), it_begin = read_int(), it_end = read_int();
    has_tails = read_int(), has_slots = read_int(), nblock = read_int();
    if (nray < 0 || it_end <= it_begin || nblock < 0 || (has_slots && !has_tails)) exit(2);
    const int nrow = it_end - it_begin;
    chan.resize(nray);
    for (int j = 0; j < nray; ++j) chan[j] = read_int();
    if (has_tails) {
      tail_from.resize(nray);
      tail_row.resize((size_t)nray * RWRT_NOUT);
      for (int j = 0; j < nray; ++j) tail_from[j] = read_int();
      for (size_t k = 0; k < tail_row.size(); ++k) tail_row[k] = read_double();
    }
    if (has_slots) {
      slot.resize(nray);
      for (int j = 0; j < nray; ++j) {
        slot[j] = read_int();
        if (slot[j] < -1 || slot[j] >= nblock) exit(2);
      }
    } else if (nblock != nray) {
      exit(2);
    }
    block_rows.resize((size_t)nblock * nrow * RWRT_NOUT);
    for (size_t k = 0; k < block_rows.size(); ++k) block_rows[k] = read_double();
  }

  // (a launch without a block has an empty buffer: its data() may be NULL and is never read)
  rwrt::LaunchRows rows() const {
    return rwrt::LaunchRows{block_rows.data(),
                            has_slots ? slot.data() : nullptr,
                            has_tails ? tail_from.data() : nullptr,
                            has_tails ? tail_row.data() : nullptr,
                            it_begin,
                            it_end};
  }
};

}  // namespace host_input
