// link_amd/csrc/radix_pass.h -- one 8-bit pass of a stable LSD radix sort of (key, uint32 value) pairs, as the three device
// functions its three kernels call.  The kernels stay with their users (segloss.hip: uint32 keys, one segment per class;
// segio.hip: uint64 keys, one segment): they keep their early-outs and work out where their segment starts, the rest is here.
//
// A segment of nv pairs is cut into tiles of RADIX_TILE = 2048 positions; one workgroup of 256 threads takes a tile.
//
//   radix_tile_hist    hist_tile[digit] = the tile's keys with that digit (LDS integer atomics).  A tile's 256 words are
//                      contiguous, so this store, the scan's loads (one thread per digit) and the scatter's load are coalesced;
//                      every tile writes its words (zeros past nv).
//   radix_digit_scan   one workgroup per segment, one thread per digit: where each (digit, tile) starts, in place -- the keys of
//                      smaller digits first, then the digit's own keys in the tiles before this one.
//   radix_tile_scatter stable scatter of one tile.  Its eight rounds run in position order (round r takes positions
//                      r * 256 + thread).  Inside a round the rank of a key among the equal digits of its wave comes from eight
//                      ballots, one per bit of the digit: `same` ends as the mask of the lanes that hold this lane's digit, and the
//                      lanes below this one in it are the keys in front.  The first lane of every digit leaves the wave's count in
//                      LDS and the waves are chained in wave order: a key lands at base[digit] + the counts of the waves before
//                      its own + its rank, and base moves on by the round's counts.  Equal keys therefore keep their order.
#pragma once
#include "block_prims.h"

namespace link {

constexpr int RADIX_T = 256;                          // threads of every workgroup here (4 waves)
constexpr int RADIX_ITEMS = 8;
constexpr int RADIX_TILE = RADIX_T * RADIX_ITEMS;     // pairs per tile

template <typename K>
__device__ __forceinline__ uint32_t radix_digit(K key, int shift) { return (uint32_t)(key >> shift) & 255u; }

template <typename K>
__device__ __forceinline__ void radix_tile_hist(const K *keys, int64_t nv, int64_t tile, int shift,
                                                uint32_t *hist_tile) {
  __shared__ int lh[256];
  const int t = threadIdx.x;
  lh[t] = 0;
  __syncthreads();
  const int64_t p0 = tile * RADIX_TILE;
#pragma unroll
  for (int r = 0; r < RADIX_ITEMS; ++r) {
    const int64_t p = p0 + r * RADIX_T + t;
    if (p < nv) atomicAdd(&lh[radix_digit(keys[p], shift)], 1);
  }
  __syncthreads();
  hist_tile[t] = (uint32_t)lh[t];
}

// hist: the segment's [ntiles][256] words.  Loads are issued eight tiles at a time so their latencies overlap.
__device__ __forceinline__ void radix_digit_scan(uint32_t *hist, int64_t ntiles) {
  __shared__ int il[8];
  uint32_t *h = hist + threadIdx.x;
  int mine = 0;
  const uint32_t *g = h;
  for (int64_t t0 = 0; t0 < ntiles; t0 += 8, g += 8 * 256) {
    int v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = t0 + j < ntiles ? (int)g[j * 256] : 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) mine += v[j];
  }
  int all;
  int run = block_scan_excl<RADIX_T>(mine, il, all);
  uint32_t *o = h;
  for (int64_t t0 = 0; t0 < ntiles; t0 += 8, o += 8 * 256) {
    int v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = t0 + j < ntiles ? (int)o[j * 256] : 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (t0 + j < ntiles) o[j * 256] = (uint32_t)run;
      run += v[j];
    }
  }
}

// keys, vals, keys_out, vals_out: the segment's; hist_tile: the tile's scanned words.  The caller has left when the tile starts at
// or past nv.
template <typename K>
__device__ __forceinline__ void radix_tile_scatter(const K *keys, const uint32_t *vals, int64_t nv,
                                                   int64_t tile, int shift, const uint32_t *hist_tile,
                                                   K *keys_out, uint32_t *vals_out) {
  __shared__ int base[256];
  __shared__ int wcnt[RADIX_T / WAVE][256];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t p0 = tile * RADIX_TILE;
  base[t] = (int)hist_tile[t];
#pragma unroll
  for (int i = 0; i < RADIX_T / WAVE; ++i) wcnt[i][t] = 0;
  __syncthreads();
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int r = 0; r < RADIX_ITEMS; ++r) {
    const int64_t p = p0 + r * RADIX_T + t;
    const bool act = p < nv;
    K key = 0;
    uint32_t val = 0;
    if (act) {
      key = keys[p];
      val = vals[p];
    }
    const uint32_t d = radix_digit(key, shift);
    unsigned long long same = __ballot(act);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(act && bit);
      same &= bit ? m : ~m;
    }
    const int rank = __popcll(same & lt);
    if (act && rank == 0) wcnt[w][d] = __popcll(same);
    __syncthreads();
    if (act) {
      int off = base[d] + rank;
      for (int i = 0; i < w; ++i) off += wcnt[i][d];
      if (off >= 0 && off < nv) {                                   // holds by construction; never write outside the segment
        keys_out[off] = key;
        vals_out[off] = val;
      }
    }
    __syncthreads();
    {
      int s = 0;
#pragma unroll
      for (int i = 0; i < RADIX_T / WAVE; ++i) {
        s += wcnt[i][t];
        wcnt[i][t] = 0;
      }
      base[t] += s;
    }
    __syncthreads();
  }
}

}  // namespace link
