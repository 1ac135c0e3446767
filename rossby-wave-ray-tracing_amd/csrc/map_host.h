// map_host.h -- the host side the map entry points share (density.hip,
// arrival.hip, flux.hip, track.hip, cross.hip): the checks of a lon-lat grid,
// reporting as the entry point `fn` like check_launch_rows (launch_rows.h) and
// made before the first HIP call, and the launch of one lane per ray.
#ifndef RWRT_MAP_HOST_H
#define RWRT_MAP_HOST_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "abi_host.h"

namespace rwrt {

// nx, ny, nchan: positive, and nchan*ny*nx bins indexed with 32 bits
inline rwrt_status check_map_shape(const char* fn, int32_t nx, int32_t ny, int32_t nchan) {
  const char* bad = nullptr;
  if (nx <= 0 || ny <= 0 || nchan <= 0) bad = "%s: nx, ny and nchan must be positive";
  else if ((int64_t)nx * ny >= (1LL << 31) || (int64_t)nx * ny * nchan >= (1LL << 31))
    bad = "%s: nchan*ny*nx must be below 2^31";
  return bad ? fail(RWRT_ERR_ARG, bad, fn) : RWRT_OK;
}

// the factors and the origins of the index arithmetic; lon0 is 0 unless the map is an unwrapped window
inline rwrt_status check_map_axes(const char* fn, double inv_dlon, double inv_dlat, double lat0, double lon0 = 0.0,
                                  bool unwrapped = false) {
  const char* bad = nullptr;
  if (!(inv_dlon > 0.0) || !std::isfinite(inv_dlon)) bad = "%s: inv_dlon must be finite and positive";
  else if (!(inv_dlat > 0.0) || !std::isfinite(inv_dlat)) bad = "%s: inv_dlat must be finite and positive";
  else if (!std::isfinite(lat0)) bad = "%s: lat0 must be finite";
  else if (!std::isfinite(lon0)) bad = "%s: lon0 must be finite";
  else if (!unwrapped && lon0 != 0.0) bad = "%s: lon0 must be 0 for a wrapped longitude (mode bit 1 clear)";
  return bad ? fail(RWRT_ERR_ARG, bad, fn) : RWRT_OK;
}

// a row column by number: none, or one of k l amp ug vg
inline bool map_column_ok(int32_t col) { return col == -1 || (col >= 2 && col <= 6); }

// `kernel` with one lane per ray in blocks of 256, and check_launch(what)
template <class... P, class... A>
rwrt_status launch_per_ray(const char* what, void (*kernel)(P...), int64_t nray, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((nray + 255) / 256)), dim3(256), 0, (hipStream_t)stream, args...);
  return check_launch(what);
}

}  // namespace rwrt

#endif  // RWRT_MAP_HOST_H
