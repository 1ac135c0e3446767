// Stand-alone host program over csrc/phase_rows.h (the validity of a row, a =
// l / cos(lat), the trapezoid of a segment, the deposit's bin and the per-ray
// walk the phase kernel uses), built by tests/support/hostprog.py with
// -fsanitize=undefined,address,float-cast-overflow -fno-sanitize-recover=all
// -ffp-contract=off and run directly.
//
// Launches are walked the way the kernel walks them, ray by ray, ray j in
// column j of the carried rows and of the per-ray arrays, with an emitter that
// updates plain arrays instead of issuing atomics.  Every buffer has exactly
// the size its launch gives it, so a row, a tail or a bin read or written out
// of range is the sanitizer's finding, and so is a floor converted to an
// integer it does not fit.  Each ray is also walked row by row (its tail
// expanded) with a state of its own, and the program fails (exit 3) if a
// tail's counts, drops, segments, carried row or theta (bit for bit) differ
// from that.
//
// stdin:  nx ny nchan need wcol nray
//         lat0 inv_dlat inv_dlon omega_dt                                   (doubles as hex floats, %a)
//         theta0[nray]
//         nlaunch
//         per launch: tests/host/launch_input.h                            (nray the same in every launch)
// stdout: cnt[nmap] as integers, re[nmap], im[nmap] and wabs[nmap] as hex
//         floats, one line each; "dropped <n>"; theta[nray] as hex floats,
//         nseg[nray] as integers and carry[4 * nray] as hex floats (nan for
//         none), one line each
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "launch_input.h"
#include "phase_rows.h"

namespace {

using host_input::read_double;
using host_input::read_int;

struct Arrays {
  std::vector<long long> cnt;
  std::vector<double> re, im, wabs;
  std::vector<double> carry;   // [4][nray]
  std::vector<double> theta;
  std::vector<int32_t> nseg;
  unsigned long long dropped = 0;

  Arrays(size_t nmap, size_t nray, const std::vector<double>& theta0)
      : cnt(nmap, 0), re(nmap, 0.0), im(nmap, 0.0), wabs(nmap, 0.0), carry(4 * nray, NAN), theta(theta0),
        nseg(nray, 0) {}
};

struct PlainEmitter {
  Arrays& a;

  void drop(int32_t n) {
    if (n < 1) exit(4);
    a.dropped += (unsigned long long)n;
  }

  // (.at(): an index out of range ends the program)
  void add(int32_t bin, int32_t n, double re, double im, double wabs) {
    if (bin < 0 || n < 1) exit(4);
    a.cnt.at((size_t)bin) += n;
    a.re.at((size_t)bin) += re;
    a.im.at((size_t)bin) += im;
    a.wabs.at((size_t)bin) += wabs;
  }
};

rwrt::PhaseState load_state(const Arrays& a, size_t nray, size_t j) {
  return {a.carry.at(j), a.carry.at(nray + j), a.carry.at(2 * nray + j), a.carry.at(3 * nray + j), a.theta.at(j),
          a.nseg.at(j)};
}

void store_state(Arrays& a, size_t nray, size_t j, const rwrt::PhaseState& s) {
  a.carry.at(j) = s.lon;
  a.carry.at(nray + j) = s.lat;
  a.carry.at(2 * nray + j) = s.k;
  a.carry.at(3 * nray + j) = s.a;
  a.theta.at(j) = s.theta;
  a.nseg.at(j) = s.nseg;
}

bool same_bits(const std::vector<double>& x, const std::vector<double>& y) {
  return x.size() == y.size() && (x.empty() || memcmp(x.data(), y.data(), x.size() * sizeof(double)) == 0);
}

}  // namespace

int main() {
  rwrt_phase_map m = {};
  m.nx = read_int();
  m.ny = read_int();
  m.nchan = read_int();
  m.need = read_int();
  m.wcol = read_int();
  const int nray = read_int();
  m.lat0 = read_double();
  m.inv_dlat = read_double();
  m.inv_dlon = read_double();
  m.omega_dt = read_double();
  auto column_ok = [](int c) { return c == -1 || (c >= 2 && c <= 6); };
  if (m.nx <= 0 || m.ny <= 0 || m.nchan <= 0 || !column_ok(m.need) || !column_ok(m.wcol) || nray < 0 ||
      !(m.inv_dlat > 0.0) || !(m.inv_dlon > 0.0) || !std::isfinite(m.lat0) || !std::isfinite(m.omega_dt))
    return 2;
  std::vector<double> theta0((size_t)nray);
  for (int j = 0; j < nray; ++j) theta0[j] = read_double();
  const size_t nmap = (size_t)m.nchan * m.ny * m.nx;
  Arrays walked(nmap, nray, theta0), each(nmap, nray, theta0);
  PlainEmitter ew{walked}, ee{each};
  const rwrt_density_map bins = rwrt::phase_bins(m);

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
      rwrt::PhaseState s = load_state(walked, nray, j);
      rwrt::phase_ray<4>(L, (int64_t)j, m, bins, ch, s, ew);
      store_state(walked, nray, j, s);
      // and row by row
      const rwrt::LaunchRowsSpan sp = rwrt::launch_rows_span(L, (int64_t)j);
      rwrt::PhaseState r = load_state(each, nray, j);
      if (L.it_begin == 0) r.lon = NAN;
      for (int i = L.it_begin; i < L.it_end; ++i) {
        const double* p = i < sp.tf ? sp.block + (size_t)(i - L.it_begin) * RWRT_NOUT : L.tail_row + (size_t)j * RWRT_NOUT;
        rwrt::phase_row(r, i, rwrt::phase_load(p, m), m, bins, ch, ee);
      }
      store_state(each, nray, j, r);
    }
    rays += nray;
  }
  if (walked.cnt != each.cnt || walked.dropped != each.dropped || walked.nseg != each.nseg ||
      !same_bits(walked.theta, each.theta) || !same_bits(walked.carry, each.carry)) {
    fprintf(stderr, "the tails' counts, drops, segments, theta or carried rows differ from the row-by-row walk\n");
    return 3;
  }
  for (size_t k = 0; k < nmap; ++k) printf("%lld ", walked.cnt[k]);
  printf("\n");
  for (size_t k = 0; k < nmap; ++k) printf("%a ", walked.re[k]);
  printf("\n");
  for (size_t k = 0; k < nmap; ++k) printf("%a ", walked.im[k]);
  printf("\n");
  for (size_t k = 0; k < nmap; ++k) printf("%a ", walked.wabs[k]);
  printf("\n");
  printf("dropped %llu\n", walked.dropped);
  for (size_t k = 0; k < walked.theta.size(); ++k) printf("%a ", walked.theta[k]);
  printf("\n");
  for (size_t k = 0; k < walked.nseg.size(); ++k) printf("%d ", walked.nseg[k]);
  printf("\n");
  for (size_t k = 0; k < walked.carry.size(); ++k) printf("%a ", walked.carry[k]);
  printf("\n");
  fprintf(stderr, "phase_rows_main ok: %lld rays in %d launches\n", rays, nlaunch);
  return 0;
}
