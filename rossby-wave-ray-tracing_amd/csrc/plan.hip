// plan.hip -- rwrt_launch_plan (ABI 5, additive): what a ray-loop launch needs
// decided beforehand, in one call: each ray's work since the previous launch,
// the frozen verdict, the row slots of the live rays and the queue order
// (live rays longest first, frozen rays last).  A translation unit of its
// own: the ray loops' code object (rwrt.o) does not change with it.
//
// Three kernels over tiles of kPlanTile rays (the scheme of rwrt_row_slots:
// per-tile live counts, one block scans them, each tile numbers its rays),
// one read-back of (live rays, largest key) and a radix sort of the live rays
// alone over the bits the largest key has.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "abi_host.h"

namespace rwrt {
namespace {

constexpr int kPlanTile = 4096;   // 256 threads x 16 rays
constexpr size_t kPlanAlign = 256;
constexpr size_t kPlanMergeLimit = 64 * 1024;
// From 64 Ki live rays on, radix passes over the key's bits (below: rocprim's
// merge sort, which it would choose up to 1 Mi rays -- C3's 716 400 live rays
// in ~20 small kernels, 0.15 ms per launch)
using PlanSort = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                            rocprim::default_config, kPlanMergeLimit>;

// what the host reads back after the three kernels
struct PlanHead {
  unsigned long long max_key;   // the largest work of a live ray
  long long n_live;
};

// The scratch of a plan over nray rays: tile counts, the head, the live rays'
// keys and indices (sort input), the sorted keys, rocprim's own storage.
struct PlanLayout {
  size_t tile, head, keys_in, vals_in, keys_out, temp, temp_bytes, total;
};

size_t plan_up(size_t x) { return (x + kPlanAlign - 1) & ~(kPlanAlign - 1); }

// rocprim's own storage for a sort of n pairs (every key bit)
hipError_t plan_sort_bytes(size_t n, size_t* bytes) {
  return rocprim::radix_sort_pairs_desc<PlanSort>(
      nullptr, *bytes, static_cast<unsigned long long*>(nullptr), static_cast<unsigned long long*>(nullptr),
      static_cast<int64_t*>(nullptr), static_cast<int64_t*>(nullptr), n, 0u, 64u, (hipStream_t) nullptr);
}

hipError_t plan_layout(int64_t nray, PlanLayout* L) {
  const size_t n = (size_t)nray, tiles = (n + kPlanTile - 1) / kPlanTile;
  // the sort's storage for every ray live, and for the largest set that takes
  // the merge path (the live rays decide the path): the most a call needs
  size_t temp = 0, merge = 0;
  hipError_t e = plan_sort_bytes(n, &temp);
  if (e == hipSuccess) e = plan_sort_bytes(n < kPlanMergeLimit ? n : kPlanMergeLimit, &merge);
  if (e != hipSuccess) return e;
  temp = merge > temp ? merge : temp;
  L->tile = 0;
  L->head = plan_up(tiles * sizeof(int32_t));
  L->keys_in = L->head + plan_up(sizeof(PlanHead));
  L->vals_in = L->keys_in + plan_up(n * 8);
  L->keys_out = L->vals_in + plan_up(n * 8);
  L->temp = L->keys_out + plan_up(n * 8);
  L->temp_bytes = plan_up(temp);
  L->total = L->temp + L->temp_bytes;
  return hipSuccess;
}

__device__ __forceinline__ bool plan_live(const double* __restrict__ state, int64_t nray, int64_t i) {
  double sum = state[i];
#pragma unroll
  for (int v = 1; v < 5; ++v) sum = sum + state[v * nray + i];
  return !isnan(sum / 5.0);   // frozen_flag_kernel's and rwrt_row_slots' test
}

// work and prev_work of every ray; the tile's live rays and their largest work
__global__ void __launch_bounds__(256)
plan_count_kernel(const double* __restrict__ state, const int64_t* __restrict__ count,
                  int64_t* __restrict__ prev_work, int64_t* __restrict__ work, int64_t nray, int total,
                  int32_t* __restrict__ tile_count, PlanHead* __restrict__ head) {
  const int64_t base = (int64_t)blockIdx.x * kPlanTile;
  int c = 0;
  unsigned long long mx = 0;
  for (int k = 0; k < kPlanTile / 256; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    if (i < nray) {
      const int64_t all = count[2 * i] + count[2 * i + 1];
      const int64_t w = total ? all : all - prev_work[i];
      work[i] = w;
      prev_work[i] = all;
      if (plan_live(state, nray, i)) {
        ++c;
        const unsigned long long key = (unsigned long long)w;
        mx = key > mx ? key : mx;
      }
    }
  }
  __shared__ int part[4];
  __shared__ unsigned long long pmax[4];
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_xor(c, o);
    const unsigned long long other = __shfl_xor(mx, o);
    mx = other > mx ? other : mx;
  }
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6] = c;
    pmax[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    tile_count[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
    for (int w = 1; w < 4; ++w) mx = pmax[w] > mx ? pmax[w] : mx;
    if (mx) atomicMax(&head->max_key, mx);
  }
}

// tile counts -> exclusive offsets (in place); the number of live rays
__global__ void __launch_bounds__(1024)
plan_offsets_kernel(int64_t tiles, int32_t* __restrict__ tile_count, PlanHead* __restrict__ head,
                    int64_t* __restrict__ nslot) {
  __shared__ int wsum[16];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t t0 = 0; t0 < tiles; t0 += 1024) {
    const int64_t t = t0 + threadIdx.x;
    const int v = t < tiles ? tile_count[t] : 0;
    int x = v;   // inclusive scan within the wave
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (t < tiles) tile_count[t] = before + x - v;   // exclusive
    __syncthreads();
    if (threadIdx.x == 1023) carry = before + x;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    head->n_live = carry;
    *nslot = carry;
  }
}

// Live ray i, the p-th live one: row_slot p, and (work, i) at p of the sort's
// input.  Frozen ray i with p live rays before it: row_slot -1, and place
// n_live + (i - p) of the order -- the frozen rays in ray order behind the
// live ones.
__global__ void __launch_bounds__(256)
plan_assign_kernel(const double* __restrict__ state, const int64_t* __restrict__ work, int64_t nray,
                   const int32_t* __restrict__ tile_off, const PlanHead* __restrict__ head,
                   int32_t* __restrict__ row_slot, unsigned long long* __restrict__ keys,
                   int64_t* __restrict__ vals, int64_t* __restrict__ order) {
  const int64_t base = (int64_t)blockIdx.x * kPlanTile;
  __shared__ int off;
  __shared__ int wcnt[4];
  if (threadIdx.x == 0) off = tile_off[blockIdx.x];
  __syncthreads();
  const int64_t n_live = head->n_live;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = 0; k < kPlanTile / 256; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    const bool live = i < nray && plan_live(state, nray, i);
    const uint64_t m = __ballot(live);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int before = off;
    for (int w = 0; w < wave; ++w) before += wcnt[w];
    const int mine = before + __popcll(m & ((1ull << lane) - 1ull));
    if (i < nray) {
      row_slot[i] = live ? mine : -1;
      if (live) {
        keys[mine] = (unsigned long long)work[i];
        vals[mine] = i;
      } else {
        order[n_live + (i - mine)] = i;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) off += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
}

bool misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

}  // namespace
}  // namespace rwrt

using namespace rwrt;

extern "C" rwrt_status rwrt_launch_plan_bytes(int64_t nray, int64_t* bytes) {
  if (!bytes) return fail(RWRT_ERR_ARG, "rwrt_launch_plan_bytes: bytes is NULL%s", "");
  if (nray < 0 || nray > 0x7fffffffLL) return fail(RWRT_ERR_ARG, "rwrt_launch_plan_bytes: nray out of range%s", "");
  PlanLayout L;
  if (const hipError_t e = plan_layout(nray, &L))
    return fail(RWRT_ERR_HIP, "rwrt_launch_plan_bytes: sort storage query: %s", hipGetErrorString(e));
  *bytes = (int64_t)L.total;
  return RWRT_OK;
}

extern "C" rwrt_status rwrt_launch_plan(int64_t nray, int32_t policy, const double* d_state,
                                        const int64_t* d_count, int64_t* d_prev_work, int64_t* d_work,
                                        int64_t* d_order, int32_t* d_row_slot, int64_t* d_nslot,
                                        int64_t* h_nlive, void* d_scratch, int64_t scratch_bytes, void* stream) {
  // (every check before the first HIP call)
  if (nray < 0 || nray > 0x7fffffffLL) return fail(RWRT_ERR_ARG, "rwrt_launch_plan: nray out of range%s", "");
  if (policy != RWRT_PLAN_SINCE && policy != RWRT_PLAN_TOTAL)
    return fail(RWRT_ERR_ARG, "rwrt_launch_plan: unknown policy (RWRT_PLAN_SINCE or RWRT_PLAN_TOTAL)%s", "");
  if (!d_nslot || !h_nlive) return fail(RWRT_ERR_ARG, "rwrt_launch_plan: NULL d_nslot or h_nlive%s", "");
  if (nray > 0 && (!d_state || !d_count || !d_prev_work || !d_work || !d_order || !d_row_slot || !d_scratch))
    return fail(RWRT_ERR_ARG, "rwrt_launch_plan: NULL buffer%s", "");
  if (misaligned(d_state, 8) || misaligned(d_count, 8) || misaligned(d_prev_work, 8) || misaligned(d_work, 8) ||
      misaligned(d_order, 8) || misaligned(d_nslot, 8) || misaligned(d_row_slot, 4) ||
      misaligned(d_scratch, kPlanAlign))
    return fail(RWRT_ERR_ARG, "rwrt_launch_plan: misaligned buffer (d_scratch: 256 bytes)%s", "");
  hipStream_t st = (hipStream_t)stream;
  if (nray == 0) {
    *h_nlive = 0;
    if (hipMemsetAsync(d_nslot, 0, sizeof(int64_t), st) != hipSuccess) return check_launch("hipMemsetAsync(nslot)");
    return RWRT_OK;
  }
  PlanLayout L;
  if (const hipError_t e = plan_layout(nray, &L))
    return fail(RWRT_ERR_HIP, "rwrt_launch_plan: sort storage query: %s", hipGetErrorString(e));
  if (scratch_bytes < (int64_t)L.total)
    return fail(RWRT_ERR_ARG, "rwrt_launch_plan: d_scratch is smaller than rwrt_launch_plan_bytes asks%s", "");
  char* s = static_cast<char*>(d_scratch);
  int32_t* tile = reinterpret_cast<int32_t*>(s + L.tile);
  PlanHead* head = reinterpret_cast<PlanHead*>(s + L.head);
  unsigned long long* keys_in = reinterpret_cast<unsigned long long*>(s + L.keys_in);
  int64_t* vals_in = reinterpret_cast<int64_t*>(s + L.vals_in);
  unsigned long long* keys_out = reinterpret_cast<unsigned long long*>(s + L.keys_out);
  const int64_t tiles = (nray + kPlanTile - 1) / kPlanTile;
  if (hipMemsetAsync(head, 0, sizeof(PlanHead), st) != hipSuccess) return check_launch("hipMemsetAsync(plan head)");
  hipLaunchKernelGGL(plan_count_kernel, dim3((unsigned)tiles), dim3(256), 0, st, d_state, d_count, d_prev_work,
                     d_work, nray, policy == RWRT_PLAN_TOTAL ? 1 : 0, tile, head);
  hipLaunchKernelGGL(plan_offsets_kernel, dim3(1), dim3(1024), 0, st, tiles, tile, head, d_nslot);
  hipLaunchKernelGGL(plan_assign_kernel, dim3((unsigned)tiles), dim3(256), 0, st, d_state, d_work, nray, tile, head,
                     d_row_slot, keys_in, vals_in, d_order);
  if (rwrt_status e = check_launch("plan kernels")) return e;
  // the one read-back of a launch: how many rays to sort, over how many bits
  PlanHead h;
  if (hipMemcpyAsync(&h, head, sizeof(PlanHead), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return check_launch("rwrt_launch_plan: reading the live count back");
  *h_nlive = h.n_live;
  if (h.n_live > 0) {
    unsigned bits = 1;
    while (bits < 64 && (h.max_key >> bits) != 0) ++bits;
    // stable and descending: equal work keeps ray order, as torch.sort(descending, stable) does
    size_t temp = 0;
    if (plan_sort_bytes((size_t)h.n_live, &temp) != hipSuccess || temp > L.temp_bytes)
      return fail(RWRT_ERR_HIP, "rwrt_launch_plan: the sort's storage exceeds the scratch's share%s", "");
    temp = L.temp_bytes;
    const hipError_t e = rocprim::radix_sort_pairs_desc<PlanSort>(s + L.temp, temp, keys_in, keys_out, vals_in, d_order,
                                                                 (size_t)h.n_live, 0u, bits, st);
    if (e != hipSuccess) return fail(RWRT_ERR_HIP, "rwrt_launch_plan: radix sort: %s", hipGetErrorString(e));
  }
  return check_launch("rwrt_launch_plan");
}
