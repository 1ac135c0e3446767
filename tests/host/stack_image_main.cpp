// Stand-alone host program over csrc/stack_image.h (tests/test_stack_host.py
// builds it with -fsanitize=undefined,address).  Commands on stdin, one per
// line, answers on stdout:
//   bytes NPTS            -> stack_image_bytes
//   off NPTS M P          -> stack_member_offset(NPTS, M) + stack_point_offset(P) (64-bit sum)
//   point P               -> stack_point_offset
//   fits NPTS NMEMBER     -> 0 / 1
//   bytesfit BYTES        -> 0 / 1 (stack_bytes_fit: BYTES of images + 8 KiB <= 2^32)
//   clamp M NMEMBER       -> stack_clamp_member
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "stack_image.h"

int main() {
  char cmd[16];
  long long a, b, c;
  while (std::scanf("%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "bytes") && std::scanf("%lld", &a) == 1) {
      std::printf("%llu\n", (unsigned long long)rwrt::stack_image_bytes(a));
    } else if (!std::strcmp(cmd, "off") && std::scanf("%lld %lld %lld", &a, &b, &c) == 3) {
      const uint64_t o = rwrt::stack_member_offset(a, (int32_t)b) + rwrt::stack_point_offset((uint32_t)c);
      std::printf("%llu\n", (unsigned long long)o);
    } else if (!std::strcmp(cmd, "point") && std::scanf("%lld", &a) == 1) {
      std::printf("%u\n", rwrt::stack_point_offset((uint32_t)a));
    } else if (!std::strcmp(cmd, "fits") && std::scanf("%lld %lld", &a, &b) == 2) {
      std::printf("%d\n", rwrt::stack_fits(a, b) ? 1 : 0);
    } else if (!std::strcmp(cmd, "bytesfit") && std::scanf("%lld", &a) == 1) {
      std::printf("%d\n", rwrt::stack_bytes_fit((uint64_t)a) ? 1 : 0);
    } else if (!std::strcmp(cmd, "clamp") && std::scanf("%lld %lld", &a, &b) == 2) {
      std::printf("%d\n", rwrt::stack_clamp_member((int32_t)a, (int32_t)b));
    } else {
      std::fprintf(stderr, "bad command %s\n", cmd);
      return 2;
    }
  }
  return 0;
}
