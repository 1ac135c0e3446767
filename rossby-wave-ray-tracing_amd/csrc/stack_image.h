// Member stacks (include/rwrt.h rwrt_stack): where the cache image of member
// m lies in the context's scratch, where a grid point's record lies inside an
// image, and how many members a launch may hold.  Host and device code share
// this file: the library's argument check (rwrt_rk45_run_stack), the run
// kernel's refill (CachedStackBG in rwrt.hip) and tests/host/stack_image_main.cpp.
//
// One image per member, each laid out exactly like the static state's cache
// image (rwrt.hip, cache_image_kernel): the records of 64 consecutive grid
// points chunk-major in a 6 KiB tile,
//   chunk q of point p at (p >> 6) * 6 KiB + q * 1 KiB + (p & 63) * 16 B,
// and member m's image at m * stack_image_bytes(npts).  A refill addresses a
// corner by ONE 32-bit offset from the base of the whole stack (the member's
// offset added to the point's), its six chunks by the load's immediate offset
// (up to 3 KiB) from that base and from base + 4 KiB.  So every byte of every
// image, plus those 8 KiB, must lie below 2^32: stack_fits.
#ifndef RWRT_STACK_IMAGE_H
#define RWRT_STACK_IMAGE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RWRT_STACK_FN __host__ __device__ inline
#else
#define RWRT_STACK_FN inline
#endif

namespace rwrt {

constexpr uint32_t kStackTile = 6u * 1024u;        // one tile: 64 points x 6 chunks x 16 B
constexpr uint64_t kStackReach = 8u * 1024u;       // the refill's second base (4 KiB) + largest immediate, rounded up
constexpr uint64_t kStackLimit = 1ull << 32;       // 32-bit offsets

// bytes of one member's image
RWRT_STACK_FN uint64_t stack_image_bytes(int64_t npts) {
  return (uint64_t)((npts + 63) / 64) * kStackTile;
}
// chunk 0 of grid point p inside an image (p < 2^24)
RWRT_STACK_FN uint32_t stack_point_offset(uint32_t p) { return (p >> 6) * (kStackTile - 1024u) + p * 16u; }
// member m's image from the base of the stack
RWRT_STACK_FN uint64_t stack_member_offset(int64_t npts, int32_t m) {
  return (uint64_t)(m < 0 ? 0 : m) * stack_image_bytes(npts);
}
// `bytes` of images within reach of a 32-bit offset: bytes + 8 KiB <= 2^32
RWRT_STACK_FN bool stack_bytes_fit(uint64_t bytes) { return bytes <= kStackLimit - kStackReach; }
// nmember images of npts points each (the product cannot overflow: an image
// that fits is below 2^32 bytes and nmember below 2^31)
RWRT_STACK_FN bool stack_fits(int64_t npts, int64_t nmember) {
  if (npts < 1 || npts > (1LL << 32) || nmember < 1 || nmember > 0x7fffffffLL) return false;
  const uint64_t image = stack_image_bytes(npts);
  return stack_bytes_fit(image) && stack_bytes_fit(image * (uint64_t)nmember);
}
// a member index wherever it addresses memory
RWRT_STACK_FN int32_t stack_clamp_member(int32_t m, int32_t nmember) {
  return m < 0 ? 0 : (m >= nmember ? nmember - 1 : m);
}

}  // namespace rwrt

#endif
