// link_amd/csrc/block_prims.h -- what a workgroup of the task kernels computes together: a sum of fixed shape, an exclusive scan,
// the rank of the flagged threads; and the small host and device odds those kernels share.
//
// Every collective is called by ALL NT threads of a one-dimensional workgroup of NT / 64 whole waves (NT = 256, four waves, unless
// the caller says otherwise), from uniform control flow.  The scan and the rank open with a barrier, so they may be called again
// on the same LDS words with nothing in between.
//
// Nothing in this file forms a product that feeds a sum: the units that include it differ in `fp contract` (off in some from their
// first line, off in others from box_iou.h on, on in the rest), and a helper here is compiled under whatever holds where it is
// included.  Keep it so -- integer arithmetic, compares and plain adds only.
#pragma once
#include "common.h"

namespace link {

// sum of v over the workgroup by a tree of fixed shape: the same bits whatever the schedule.  lds: NT entries.
template <typename V, int NT = 256>
__device__ __forceinline__ V block_sum_fixed(V v, V *lds) {
  static_assert(NT >= WAVE && (NT & (NT - 1)) == 0, "a power of two of whole waves");
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s) lds[t] = lds[t] + lds[t + s];
    __syncthreads();
  }
  const V r = lds[0];
  __syncthreads();
  return r;
}

// inclusive prefix of x over the wave's 64 lanes
__device__ __forceinline__ int wave_incl_scan(int x, int lane) {
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int y = __shfl_up(x, o, WAVE);
    if (lane >= o) x += y;
  }
  return x;
}

// exclusive prefix of v over the workgroup in thread order; total = the workgroup's sum.  lds: NT / 64 ints.
template <int NT = 256>
__device__ __forceinline__ int block_scan_excl(int v, int *lds, int &total) {
  static_assert(NT % WAVE == 0, "whole waves");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int inc = wave_incl_scan(v, lane);
  __syncthreads();                                                  // lds may still be read from an earlier call
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  int woff = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NT / WAVE; ++i) {
    const int s = lds[i];
    if (i < w) woff += s;
    tot += s;
  }
  total = tot;
  return woff + inc - v;
}

// exclusive rank of the threads with flag among the workgroup in thread order; total = their number.  lds: NT / 64 ints.
template <int NT = 256>
__device__ __forceinline__ int block_rank(bool flag, int *lds, int &total) {
  static_assert(NT % WAVE == 0, "whole waves");
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();                                                  // lds may still be read from an earlier call
  if (lane == 0) lds[w] = __popcll(m);
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NT / WAVE; ++i) {
    const int s = lds[i];
    if (i < w) base += s;
    tot += s;
  }
  total = tot;
  return base + r;
}

__device__ __host__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the sample of point i in a batch laid end to end: the last b with point_offsets[b] <= i (b = 0 when there is none)
__device__ __forceinline__ int sample_of_point(const int32_t *__restrict__ po, int batch, int i) {
  int lo = 0, hi = batch - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (po[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// workspace sections start on 256-byte boundaries
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// is p a multiple of a (a power of two)?
inline bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace link
