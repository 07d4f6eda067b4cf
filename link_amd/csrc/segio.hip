// link_amd/csrc/segio.hip -- section M of include/link_amd.h: the segmentation front end and the validation back end on the device.
//
// link_seg_quantize: what torchsparse.utils.quantize.sparse_quantize (utils/quantize.py:9-46: a numpy ravel hash and
// np.unique(return_index, return_inverse)) computes per frame, preceded by the rounding and the minimum subtraction of
// segmentation/core/datasets/semantic_kitti.py:219-220, for a batch of clouds in one call.  The implementation is this project's:
//
//   k_sq_init    per-sample records (minimum, maximum per axis, flags) and the header reset
//   k_sq_minmax  the integer coordinate of every point; per-sample minimum and maximum per axis (a wave whose lanes share a sample
//                reduces in registers and issues one atomic per axis), flags for a coordinate that is not finite or leaves int32
//   k_sq_plan    one workgroup: the extents, the extent flag, the widths of the key's fields (the bits the largest extent of every
//                axis needs, then the bits of batch - 1 on top) and with them the number of key bits that can be set
//   k_sq_keys    key = b | x - min | y - min | z - min, value = the point index
//   k_sq_hist / k_sq_hist_scan / k_sq_scatter   a stable LSD radix sort of the (64-bit key, index) pairs, 8 bits per pass, tile
//                histograms in LDS; ranks inside a tile come from wave ballots in position order, so equal keys keep their point
//                order.  A pass whose digit lies above the highest key bit returns at once (all three kernels read the bit count
//                the plan left in the workspace: the host decides nothing), and the kernels that follow pick the buffer the last
//                pass that ran wrote.
//   k_sq_heads / k_sq_heads_top   run heads per 2048 sorted positions, their exclusive prefix, the voxel total
//   k_sq_voff    the voxels before every sample's first point (samples are contiguous in sorted order: the sample index is the
//                key's top field and the sort is stable) = voxel_offsets
//   k_sq_emit    the rank of every sorted position by a block scan on top of the tile prefix; indices and coords by the run heads
//                (the head of a run is its smallest point index), inverse by every position
//   k_sq_tail    zeros in the rows past the total, the status words
//
// link_seg_vote_eval: segmentation/evaluate.py:120-134 (inverse map, stack, sum, argmax) and core/callbacks.py:41-52 (the counters of
// MeanIoU) in one kernel: one thread per point, the votes summed in fp32 in ascending pass order, a workgroup histogram in LDS,
// then at most 3 c 64-bit integer atomics per workgroup.
//
// p / vs is a correctly rounded IEEE divide (no reciprocal), as in voxelize.hip.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "block_prims.h"
#include "dispatch.h"
#include "radix_pass.h"
#include "row_io.h"

using namespace link;

namespace {

constexpr int T = 256;                       // threads per workgroup (4 waves), every kernel here
constexpr int ITEMS = 8;
constexpr int TILE = T * ITEMS;              // pairs per sort tile and positions per scan tile
static_assert(T == RADIX_T && TILE == RADIX_TILE && TILE == LINK_SEGQ_SORT_TILE, "the header names the tile");
constexpr int MAX_BATCH = 1024;
constexpr int64_t MAX_POINTS = 1LL << 28;
constexpr int MAX_NDIM = 16;
constexpr int EXT_BITS = 20;                 // an axis extent below 2^20
constexpr int HDR_WORDS_M = 64;
enum { H_NPTS = 0, H_WX = 1, H_WY = 2, H_WZ = 3, H_WB = 4, H_NBITS = 5, H_FLAGS = 6, H_TOTAL = 7 };
enum { S_MIN = 0, S_MAX = 3, S_FLAGS = 6, S_OK = 7, S_WORDS = 8 };     // a sample's record, int32 words

struct Layout {
  int64_t ntiles;
  size_t hdr, sinfo, voff, keys0, keys1, vals0, vals1, hist, bsum, total;
};

inline bool shape_ok(int64_t n, int32_t batch) { return n >= 0 && n < MAX_POINTS && batch >= 1 && batch <= MAX_BATCH; }

Layout layout_of(int64_t n, int32_t batch) {
  Layout L;
  const size_t m = (size_t)(n > 0 ? n : 1);
  L.ntiles = (int64_t)((m + TILE - 1) / TILE);
  size_t o = 0;
  L.hdr = o; o += up256(HDR_WORDS_M * 4);
  L.sinfo = o; o += up256((size_t)batch * S_WORDS * 4);
  L.voff = o; o += up256((size_t)(batch + 1) * 4);
  L.keys0 = o; o += up256(m * 8);
  L.keys1 = o; o += up256(m * 8);
  L.vals0 = o; o += up256(m * 4);
  L.vals1 = o; o += up256(m * 4);
  L.hist = o; o += up256((size_t)L.ntiles * 256 * 4);
  L.bsum = o; o += up256((size_t)(L.ntiles + 1) * 4);
  L.total = o;
  return L;
}

// the number of points: point_offsets[batch], clamped to the capacity
__device__ __forceinline__ int sq_points(const int32_t *__restrict__ po, int batch, int64_t n) { return clampi(po[batch], 0, (int)n); }

__device__ __forceinline__ int bits_of(uint32_t v) { return v == 0 ? 0 : 32 - __clz((int)v); }

// the integer coordinate of point i before the minimum is subtracted; returns the flags the point raises (then q is not set)
__device__ __forceinline__ int sq_coord(const void *__restrict__ pts, int mode, int ndim, float vs, int64_t i, int q[3]) {
  if (mode == LINK_SEGQ_INT) {
    const int32_t *c = reinterpret_cast<const int32_t *>(pts) + i * 3;
    q[0] = c[0]; q[1] = c[1]; q[2] = c[2];
    return 0;
  }
  const float *p = reinterpret_cast<const float *>(pts) + i * ndim;
  int flags = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float r = rintf(p[d] / vs);                               // IEEE divide, round half to even: np.round(x / vs)
    if (!(fabsf(r) < INFINITY)) flags |= LINK_SEGQ_FLAG_NONFINITE;  // NaN or infinity
    else if (!(fabsf(r) < 2147483648.0f)) flags |= LINK_SEGQ_FLAG_EXTENT;   // leaves int32: never converted
    else q[d] = (int)r;
  }
  return flags;
}

// --------------------------------------------------------------------------------------------------------------- quantisation
__global__ void __launch_bounds__(T) k_sq_init(int *__restrict__ hdr, int *__restrict__ sinfo, int batch) {
  const int t = blockIdx.x * T + threadIdx.x;
  if (t < HDR_WORDS_M) hdr[t] = 0;
  if (t < batch) {
    int *s = sinfo + t * S_WORDS;
    s[S_MIN] = s[S_MIN + 1] = s[S_MIN + 2] = INT_MAX;
    s[S_MAX] = s[S_MAX + 1] = s[S_MAX + 2] = INT_MIN;
    s[S_FLAGS] = 0;
    s[S_OK] = 0;
  }
}

__global__ void __launch_bounds__(T) k_sq_minmax(const void *__restrict__ pts, int mode, int ndim, float vs, const int32_t *__restrict__ po,
                                                 int batch, int64_t n, int *__restrict__ sinfo) {
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  const int npts = sq_points(po, batch, n);
  const bool in = i < npts;
  int b = -1, flags = 0, q[3] = {0, 0, 0};
  if (in) {
    b = sample_of_point(po, batch, (int)i);
    flags = sq_coord(pts, mode, ndim, vs, i, q);
  }
  const bool good = in && flags == 0;
  int mn[3], mx[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    mn[d] = good ? q[d] : INT_MAX;
    mx[d] = good ? q[d] : INT_MIN;
  }
  // one sample in the whole wave (the common case): reduce in registers, lane 0 issues the atomics
  const int b0 = __shfl(b, 0, 64);
  const bool uniform = __all(b == b0 || !in) && b0 >= 0;            // lane 0 is active whenever any lane is (i ascends with the lane)
  if (uniform) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        mn[d] = min(mn[d], __shfl_xor(mn[d], o, 64));
        mx[d] = max(mx[d], __shfl_xor(mx[d], o, 64));
      }
      flags |= __shfl_xor(flags, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      int *s = sinfo + b0 * S_WORDS;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        if (mn[d] != INT_MAX) atomicMin(&s[S_MIN + d], mn[d]);
        if (mx[d] != INT_MIN) atomicMax(&s[S_MAX + d], mx[d]);
      }
      if (flags) atomicOr(&s[S_FLAGS], flags);
    }
  } else if (in) {
    int *s = sinfo + b * S_WORDS;
    if (good) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        atomicMin(&s[S_MIN + d], q[d]);
        atomicMax(&s[S_MAX + d], q[d]);
      }
    } else {
      atomicOr(&s[S_FLAGS], flags);
    }
  }
}

__global__ void __launch_bounds__(T) k_sq_plan(const int32_t *__restrict__ po, int batch, int64_t n, int *__restrict__ hdr,
                                               int *__restrict__ sinfo) {
  __shared__ int ext[3];
  __shared__ int allflags;
  const int t = threadIdx.x;
  if (t < 3) ext[t] = 0;
  if (t == 0) allflags = 0;
  __syncthreads();
  const int npts = sq_points(po, batch, n);
  for (int b = t; b < batch; b += T) {
    int *s = sinfo + b * S_WORDS;
    const int cnt = clampi(po[b + 1], 0, npts) - clampi(po[b], 0, npts);
    int flags = s[S_FLAGS];
    int ok = 0;
    if (cnt > 0 && flags == 0) {
      int64_t e[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) e[d] = (int64_t)s[S_MAX + d] - (int64_t)s[S_MIN + d];
      if (e[0] >= (1LL << EXT_BITS) || e[1] >= (1LL << EXT_BITS) || e[2] >= (1LL << EXT_BITS) || e[0] < 0 || e[1] < 0 || e[2] < 0) {
        flags |= LINK_SEGQ_FLAG_EXTENT;
      } else {
        ok = 1;
#pragma unroll
        for (int d = 0; d < 3; ++d) atomicMax(&ext[d], (int)e[d]);
      }
    }
    s[S_FLAGS] = flags;
    s[S_OK] = ok;
    if (flags) atomicOr(&allflags, flags);
  }
  __syncthreads();
  int wx = bits_of((uint32_t)ext[0]), wy = bits_of((uint32_t)ext[1]), wz = bits_of((uint32_t)ext[2]);
  const int wb = bits_of((uint32_t)(batch - 1));
  const bool wide = wx + wy + wz + wb > 64;                         // only with more than 16 samples and extents near 2^20
  if (wide) {
    wx = wy = wz = 0;
    for (int b = t; b < batch; b += T) sinfo[b * S_WORDS + S_OK] = 0;
  }
  if (t == 0) {
    hdr[H_NPTS] = npts;
    hdr[H_WX] = wx; hdr[H_WY] = wy; hdr[H_WZ] = wz; hdr[H_WB] = wb;
    hdr[H_NBITS] = wx + wy + wz + wb;
    hdr[H_FLAGS] = allflags | (wide ? LINK_SEGQ_FLAG_KEYBITS : 0);
  }
}

__global__ void __launch_bounds__(T) k_sq_keys(const void *__restrict__ pts, int mode, int ndim, float vs, const int32_t *__restrict__ po,
                                               int batch, const int *__restrict__ hdr, const int *__restrict__ sinfo,
                                               uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  if (i >= hdr[H_NPTS]) return;
  const int wy = hdr[H_WY], wz = hdr[H_WZ], sb = hdr[H_WX] + wy + wz;                 // sb <= 60
  const int b = sample_of_point(po, batch, (int)i);
  const int *s = sinfo + b * S_WORDS;
  uint64_t key = (uint64_t)b << sb;
  if (s[S_OK]) {
    int q[3];
    sq_coord(pts, mode, ndim, vs, i, q);                            // no flags: the sample is good
    const uint64_t ux = (uint32_t)(q[0] - s[S_MIN]), uy = (uint32_t)(q[1] - s[S_MIN + 1]), uz = (uint32_t)(q[2] - s[S_MIN + 2]);
    key |= (ux << (wy + wz)) | (uy << wz) | uz;
  }
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

// One pass of radix_pass.h over the one segment of npts pairs: hist[tile * 256 + digit].  A pass whose digit lies above every key
// does nothing (uniform: all three kernels read the same word).
__global__ void __launch_bounds__(T) k_sq_hist(const uint64_t *__restrict__ keys, const int *__restrict__ hdr, int shift,
                                               uint32_t *__restrict__ hist) {
  if (shift >= hdr[H_NBITS]) return;
  radix_tile_hist(keys, (int64_t)hdr[H_NPTS], (int64_t)blockIdx.x, shift, hist + (int64_t)blockIdx.x * 256);
}

__global__ void __launch_bounds__(T) k_sq_hist_scan(uint32_t *__restrict__ hist, int64_t ntiles, const int *__restrict__ hdr, int shift) {
  if (shift >= hdr[H_NBITS]) return;
  radix_digit_scan(hist, ntiles);
}

__global__ void __launch_bounds__(T) k_sq_scatter(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                  const int *__restrict__ hdr, int shift, const uint32_t *__restrict__ hist,
                                                  uint64_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out) {
  if (shift >= hdr[H_NBITS]) return;
  const int64_t nv = hdr[H_NPTS], tile = blockIdx.x;
  if (tile * TILE >= nv) return;                                    // uniform over the workgroup
  radix_tile_scatter(keys, vals, nv, tile, shift, hist + tile * 256, keys_out, vals_out);
}

// the buffer the last pass that ran wrote: passes alternate 0 -> 1 -> 0 ...
__device__ __forceinline__ int sq_sorted_buffer(const int *__restrict__ hdr) { return ((hdr[H_NBITS] + 7) >> 3) & 1; }

// is sorted position p (< the number of points) the head of a run of a good sample?
__device__ __forceinline__ bool sq_head(const uint64_t *__restrict__ k, int64_t p, int sb, const int *__restrict__ sinfo, int batch) {
  const uint64_t key = k[p];
  if (p > 0 && k[p - 1] == key) return false;
  const int b = (int)(key >> sb);                                   // sb <= 60
  return b < batch && sinfo[b * S_WORDS + S_OK] != 0;
}

__global__ void __launch_bounds__(T) k_sq_heads(const uint64_t *__restrict__ keys0, const uint64_t *__restrict__ keys1,
                                                const int *__restrict__ hdr, const int *__restrict__ sinfo, int batch,
                                                int *__restrict__ bsum) {
  __shared__ int il[8];
  const uint64_t *k = sq_sorted_buffer(hdr) ? keys1 : keys0;
  const int64_t nv = hdr[H_NPTS];
  const int sb = hdr[H_WX] + hdr[H_WY] + hdr[H_WZ];
  const int64_t q0 = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * ITEMS;
  int f = 0;
#pragma unroll
  for (int r = 0; r < ITEMS; ++r)
    if (q0 + r < nv) f += sq_head(k, q0 + r, sb, sinfo, batch) ? 1 : 0;
  int tot;
  block_scan_excl(f, il, tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// one workgroup: the exclusive prefix of the tile counts in place, the total behind them and in the header
__global__ void __launch_bounds__(T) k_sq_heads_top(int *__restrict__ bsum, int64_t ntiles, int *__restrict__ hdr) {
  __shared__ int il[8];
  const int t = threadIdx.x;
  int carry = 0;
  for (int64_t b0 = 0; b0 < ntiles; b0 += T) {
    const int64_t b = b0 + t;
    const int v = b < ntiles ? bsum[b] : 0;
    int tot;
    const int ex = block_scan_excl(v, il, tot);
    if (b < ntiles) bsum[b] = carry + ex;
    carry += tot;
  }
  if (t == 0) {
    bsum[ntiles] = carry;
    hdr[H_TOTAL] = carry;
  }
}

// grid batch + 1: the run heads in front of sample b's first point
__global__ void __launch_bounds__(T) k_sq_voff(const uint64_t *__restrict__ keys0, const uint64_t *__restrict__ keys1,
                                               const int32_t *__restrict__ po, const int *__restrict__ hdr, const int *__restrict__ sinfo,
                                               int batch, const int *__restrict__ bsum, int64_t voxel_capacity, int *__restrict__ voff_raw,
                                               int32_t *__restrict__ voxel_offsets) {
  __shared__ int il[8];
  const uint64_t *k = sq_sorted_buffer(hdr) ? keys1 : keys0;
  const int nv = hdr[H_NPTS];
  const int sb = hdr[H_WX] + hdr[H_WY] + hdr[H_WZ];
  const int b = blockIdx.x;
  const int pos = clampi(po[b], 0, nv);
  int raw;
  if (pos >= nv) {
    raw = hdr[H_TOTAL];
  } else {
    const int tile = pos / TILE;
    const int64_t q0 = (int64_t)tile * TILE + (int64_t)threadIdx.x * ITEMS;
    int f = 0;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r)
      if (q0 + r < pos) f += sq_head(k, q0 + r, sb, sinfo, batch) ? 1 : 0;
    int tot;
    block_scan_excl(f, il, tot);
    raw = bsum[tile] + tot;
  }
  if (threadIdx.x == 0) {
    voff_raw[b] = raw;
    voxel_offsets[b] = (int32_t)(raw < voxel_capacity ? raw : voxel_capacity);
  }
}

__global__ void __launch_bounds__(T) k_sq_emit(const uint64_t *__restrict__ keys0, const uint64_t *__restrict__ keys1,
                                               const uint32_t *__restrict__ vals0, const uint32_t *__restrict__ vals1,
                                               const int *__restrict__ hdr, const int *__restrict__ sinfo, int batch,
                                               const int *__restrict__ bsum, const int *__restrict__ voff_raw, int64_t n,
                                               int64_t voxel_capacity, int32_t *__restrict__ coords, int32_t *__restrict__ indices,
                                               int32_t *__restrict__ inverse, int32_t *__restrict__ inverse_local) {
  __shared__ int il[8];
  const int src = sq_sorted_buffer(hdr);
  const uint64_t *k = src ? keys1 : keys0;
  const uint32_t *v = src ? vals1 : vals0;
  const int64_t nv = hdr[H_NPTS];
  const int wy = hdr[H_WY], wz = hdr[H_WZ], wx = hdr[H_WX], sb = wx + wy + wz;
  const int64_t q0 = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * ITEMS;
  bool head[ITEMS];
  int f = 0;
#pragma unroll
  for (int r = 0; r < ITEMS; ++r) {
    head[r] = q0 + r < nv && sq_head(k, q0 + r, sb, sinfo, batch);
    f += head[r] ? 1 : 0;
  }
  int tot;
  int rank = bsum[blockIdx.x] + block_scan_excl(f, il, tot);        // run heads strictly before q0
#pragma unroll
  for (int r = 0; r < ITEMS; ++r) {
    const int64_t p = q0 + r;
    if (p >= nv) break;
    rank += head[r] ? 1 : 0;                                        // inclusive: the voxel of this position is rank - 1
    const uint64_t key = k[p];
    const int64_t i = v[p];
    const int b = (int)(key >> sb);
    const bool ok = b < batch && sinfo[b * S_WORDS + S_OK] != 0;
    const int vox = rank - 1;
    const bool fits = ok && vox >= 0 && vox < voxel_capacity;
    if (i < n) {
      inverse[i] = fits ? vox : -1;
      if (inverse_local) inverse_local[i] = fits ? vox - voff_raw[b] : -1;
    }
    if (head[r] && fits) {
      indices[vox] = (int32_t)i;
      int4 c;
      c.x = (int)((key >> (wy + wz)) & ((1ull << wx) - 1ull));
      c.y = (int)((key >> wz) & ((1ull << wy) - 1ull));
      c.z = (int)(key & ((1ull << wz) - 1ull));
      c.w = b;
      reinterpret_cast<int4 *>(coords)[vox] = c;
    }
  }
}

// rows past the total, the entries of inverse past the points, the status words
__global__ void __launch_bounds__(T) k_sq_tail(const int *__restrict__ hdr, int64_t n, int64_t voxel_capacity, int32_t *__restrict__ coords,
                                               int32_t *__restrict__ indices, int32_t *__restrict__ inverse,
                                               int32_t *__restrict__ inverse_local, int32_t *__restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  const int total = hdr[H_TOTAL];
  if (i >= total && i < voxel_capacity) {
    indices[i] = 0;
    reinterpret_cast<int4 *>(coords)[i] = make_int4(0, 0, 0, 0);
  }
  if (i >= hdr[H_NPTS] && i < n) {
    inverse[i] = -1;
    if (inverse_local) inverse_local[i] = -1;
  }
  if (i == 0) {
    status[0] = total;
    status[1] = hdr[H_FLAGS];
    status[2] = hdr[H_NBITS];
    status[3] = hdr[H_NPTS];
  }
}

// ------------------------------------------------------------------------------------------------------------ vote and count
// IO = LINK_IO_*: rows of logits; IO = -1: int64 predictions
template <int IO>
__global__ void __launch_bounds__(T) k_vote_eval(const void *__restrict__ rows, int64_t n_rows, int c, const int32_t *__restrict__ inverse,
                                                 int votes, int64_t np, const int64_t *__restrict__ labels, int64_t ignore_label,
                                                 const int32_t *__restrict__ lut, int32_t *__restrict__ pred,
                                                 unsigned long long *__restrict__ counters) {
  __shared__ int lh[3][LINK_SEGLOSS_MAX_CLASSES];
  const int t = threadIdx.x;
  if (t < 3 * LINK_SEGLOSS_MAX_CLASSES) (&lh[0][0])[t] = 0;
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * T + t;
  if (p < np) {
    int64_t cls;
    if constexpr (IO < 0) {
      cls = reinterpret_cast<const int64_t *>(rows)[p];
    } else {
      float acc[LINK_SEGLOSS_MAX_CLASSES];
#pragma unroll
      for (int j = 0; j < LINK_SEGLOSS_MAX_CLASSES; ++j) acc[j] = 0.f;
      for (int v = 0; v < votes; ++v) {
        const int64_t row = inverse ? (int64_t)inverse[(int64_t)v * np + p] : p;
        if (row < 0 || row >= n_rows) continue;                      // contributes nothing, indexes nothing
        const int64_t e0 = row * c;
#pragma unroll
        for (int j = 0; j < LINK_SEGLOSS_MAX_CLASSES; ++j)
          if (j < c) acc[j] += row_ld1<IO>(rows, e0 + j);
      }
      float best = -INFINITY;                                        // a NaN sum compares false: it counts as -inf and never wins
      int bi = 0;
#pragma unroll
      for (int j = 0; j < LINK_SEGLOSS_MAX_CLASSES; ++j)
        if (j < c && acc[j] > best) {                                // strict: a tie stays with the lowest class
          best = acc[j];
          bi = j;
        }
      cls = bi;
    }
    const bool cls_in = cls >= 0 && cls < c;
    if (pred) pred[p] = (lut && cls_in) ? lut[cls] : (int32_t)cls;
    if (labels) {
      const int64_t y = labels[p];
      if (y != ignore_label) {
        const bool y_in = y >= 0 && y < c;
        if (y_in) atomicAdd(&lh[0][(int)y], 1);
        if (cls_in) atomicAdd(&lh[1][(int)cls], 1);
        if (y_in && cls == y) atomicAdd(&lh[2][(int)y], 1);
      }
    }
  }
  __syncthreads();
  if (labels && t < 3 * LINK_SEGLOSS_MAX_CLASSES) {
    const int k = t / LINK_SEGLOSS_MAX_CLASSES, j = t % LINK_SEGLOSS_MAX_CLASSES;
    if (j < c && lh[k][j]) atomicAdd(&counters[k * c + j], (unsigned long long)lh[k][j]);
  }
}

}  // namespace

// ----------------------------------------------------------------------------------------------------------------- C entries
extern "C" size_t link_seg_quantize_workspace_bytes(int64_t n, int32_t batch) {
  if (!shape_ok(n, batch)) return 0;
  return layout_of(n, batch).total;
}

extern "C" int link_seg_quantize(const void *points, int32_t mode, int32_t ndim, float voxel_size, const int32_t *point_offsets,
                                 int32_t batch, int64_t n, void *workspace, size_t workspace_bytes, int32_t *coords, int32_t *indices,
                                 int64_t voxel_capacity, int32_t *inverse, int32_t *inverse_local, int32_t *voxel_offsets,
                                 int32_t *status, void *stream) {
  if (!shape_ok(n, batch) || !point_offsets || !workspace || !voxel_offsets || !status || voxel_capacity < 0 ||
      voxel_capacity >= MAX_POINTS || (mode != LINK_SEGQ_INT && mode != LINK_SEGQ_ROUND))
    return LINK_ERR_ARG;
  if (mode == LINK_SEGQ_ROUND && (ndim < 3 || ndim > MAX_NDIM || !(voxel_size > 0.f) || !isfinite(voxel_size))) return LINK_ERR_ARG;
  if ((n > 0 && (!points || !inverse)) || (voxel_capacity > 0 && (!coords || !indices))) return LINK_ERR_ARG;
  const Layout L = layout_of(n, batch);
  if (workspace_bytes < L.total) return LINK_ERR_WORKSPACE;
  char *ws = reinterpret_cast<char *>(workspace);
  int *hdr = reinterpret_cast<int *>(ws + L.hdr);
  int *sinfo = reinterpret_cast<int *>(ws + L.sinfo);
  int *voff = reinterpret_cast<int *>(ws + L.voff);
  uint64_t *keys[2] = {reinterpret_cast<uint64_t *>(ws + L.keys0), reinterpret_cast<uint64_t *>(ws + L.keys1)};
  uint32_t *vals[2] = {reinterpret_cast<uint32_t *>(ws + L.vals0), reinterpret_cast<uint32_t *>(ws + L.vals1)};
  uint32_t *hist = reinterpret_cast<uint32_t *>(ws + L.hist);
  int *bsum = reinterpret_cast<int *>(ws + L.bsum);
  hipStream_t s = S(stream);
  const dim3 pb(blocks_for(n, T)), tb((unsigned)L.ntiles);
  const int64_t longest = n > voxel_capacity ? n : voxel_capacity;

  hipLaunchKernelGGL(k_sq_init, dim3(blocks_for(MAX_BATCH, T)), dim3(T), 0, s, hdr, sinfo, (int)batch);
  hipLaunchKernelGGL(k_sq_minmax, pb, dim3(T), 0, s, points, (int)mode, (int)ndim, voxel_size, point_offsets, (int)batch, n, sinfo);
  hipLaunchKernelGGL(k_sq_plan, dim3(1), dim3(T), 0, s, point_offsets, (int)batch, n, hdr, sinfo);
  hipLaunchKernelGGL(k_sq_keys, pb, dim3(T), 0, s, points, (int)mode, (int)ndim, voxel_size, point_offsets, (int)batch, hdr, sinfo, keys[0],
                     vals[0]);
  for (int pass = 0; pass < 8; ++pass) {
    const int a = pass & 1, b = a ^ 1;
    hipLaunchKernelGGL(k_sq_hist, tb, dim3(T), 0, s, keys[a], hdr, pass * 8, hist);
    hipLaunchKernelGGL(k_sq_hist_scan, dim3(1), dim3(T), 0, s, hist, L.ntiles, hdr, pass * 8);
    hipLaunchKernelGGL(k_sq_scatter, tb, dim3(T), 0, s, keys[a], vals[a], hdr, pass * 8, hist, keys[b], vals[b]);
  }
  hipLaunchKernelGGL(k_sq_heads, tb, dim3(T), 0, s, keys[0], keys[1], hdr, sinfo, (int)batch, bsum);
  hipLaunchKernelGGL(k_sq_heads_top, dim3(1), dim3(T), 0, s, bsum, L.ntiles, hdr);
  hipLaunchKernelGGL(k_sq_voff, dim3((unsigned)batch + 1), dim3(T), 0, s, keys[0], keys[1], point_offsets, hdr, sinfo, (int)batch, bsum,
                     voxel_capacity, voff, voxel_offsets);
  hipLaunchKernelGGL(k_sq_emit, tb, dim3(T), 0, s, keys[0], keys[1], vals[0], vals[1], hdr, sinfo, (int)batch, bsum, voff, n,
                     voxel_capacity, coords, indices, inverse, inverse_local);
  hipLaunchKernelGGL(k_sq_tail, dim3(blocks_for(longest, T)), dim3(T), 0, s, hdr, n, voxel_capacity, coords, indices, inverse, inverse_local,
                     status);
  return check_launch("link_seg_quantize");
}

extern "C" int link_seg_vote_eval(const void *rows, int32_t io_dtype, int32_t input_kind, int64_t n_rows, int32_t c, const int32_t *inverse,
                                  int32_t votes, int64_t n_points, const int64_t *labels, int64_t ignore_label, const int32_t *lut,
                                  int32_t *pred, int64_t *counters, void *stream) {
  if (c < LINK_SEGLOSS_MIN_CLASSES || c > LINK_SEGLOSS_MAX_CLASSES || n_points < 0 || n_points >= (1LL << 31) || n_rows < 0 ||
      (input_kind != LINK_SEGEVAL_ROWS && input_kind != LINK_SEGEVAL_PREDICTIONS))
    return LINK_ERR_ARG;
  if (input_kind == LINK_SEGEVAL_ROWS && (!row_io_ok(io_dtype) || votes < 1 || votes > LINK_SEGEVAL_MAX_VOTES || n_rows >= (1LL << 31)))
    return LINK_ERR_ARG;
  if (labels && !counters) return LINK_ERR_ARG;
  if (n_points == 0) return LINK_OK;
  if (input_kind == LINK_SEGEVAL_ROWS && !inverse && (votes != 1 || n_rows != n_points)) return LINK_ERR_ARG;
  if (!rows && (input_kind == LINK_SEGEVAL_PREDICTIONS || n_rows > 0)) return LINK_ERR_ARG;
  hipStream_t s = S(stream);
  const dim3 g(blocks_for(n_points, T));
  unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counters);
  if (input_kind == LINK_SEGEVAL_PREDICTIONS) {
    hipLaunchKernelGGL(k_vote_eval<-1>, g, dim3(T), 0, s, rows, n_rows, (int)c, inverse, 1, n_points, labels, ignore_label, lut, pred, cnt);
  } else {
    dispatch_row_io(io_dtype, [&](auto io) {
      hipLaunchKernelGGL(k_vote_eval<decltype(io)::value>, g, dim3(T), 0, s, rows, n_rows, (int)c, inverse, (int)votes, n_points, labels,
                         ignore_label, lut, pred, cnt);
    });
  }
  return check_launch("link_seg_vote_eval");
}
