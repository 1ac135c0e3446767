// abi_host.h -- what rwrt.hip defines for the entry points of the other
// translation units: the calling thread's last error (rwrt_last_error).
#ifndef RWRT_ABI_HOST_H
#define RWRT_ABI_HOST_H

#include "rwrt.h"

namespace rwrt {
rwrt_status fail(rwrt_status s, const char* fmt, const char* detail);   // `fmt` has one %s
rwrt_status check_launch(const char* what);   // RWRT_OK, or RWRT_ERR_HIP and "<what>: <HIP's message>"
}  // namespace rwrt

#endif  // RWRT_ABI_HOST_H
