// link_amd/csrc/voxelize.hip -- point clouds to voxels on the device (section J of include/link_amd.h): the hard voxeliser with its
// per-voxel mean reader and the dynamic voxeliser.
//
// Semantics: detection/det3d/ops/point_cloud/point_cloud_ops.py:8-55,112-184 (the sequential loop: voxels numbered by first
// appearance, the first max_points points of a voxel in input order, only the first max_voxels voxels), det3d/models/readers/
// voxel_encoder.py:17-24 (mean of the kept rows), det3d/models/readers/dynamic_voxel_encoder.py:8-17 (inclusive upper bound,
// truncation, unique(dim=0) order, mean of all points).  The implementation is this project's.  Occupancy is one BIT per cell of the
// (sample, z, y, x) grid; a scan over the popcounts of the bitmap's words gives every occupied cell its rank in (sample, z, y, x)
// order, which is the dynamic numbering outright and the index of the per-cell records (minimum point index, count) for the hard
// one: no table of one word per cell, no hashing, no sort of keys.  The hard numbering is a scan over POINTS of "this point is the
// minimum of its cell".  Points are binned by cell in arbitrary order (integer atomics only), each voxel's list is then sorted
// ascending, and every sum runs in that order: bit for bit reproducible.  The bitmap's touched words are cleared on the way, so a
// workspace that starts zeroed serves every later call without a memset.
//
// (p - lo) / vs is an IEEE subtract and a correctly rounded divide: no contraction, no reciprocal.
#pragma clang fp contract(off)
#include <limits.h>
#include <math.h>

#include "block_prims.h"

using namespace link;

namespace {

constexpr int SCAN_ITEMS = 16;                 // consecutive entries of one lane
constexpr int SCAN_TILE = 256 * SCAN_ITEMS;    // entries of one workgroup
constexpr uint32_t NO_CELL = 0xFFFFFFFFu;
constexpr int MAX_BATCH = 1024;                // the per-sample prefix runs in one workgroup's LDS
constexpr int MAX_NDIM = 16;
constexpr int64_t MAX_BITS = 1LL << 31;        // bits of the bitmap over all samples
constexpr int64_t MAX_SAMPLE_CELLS = 1LL << 28;  // index.MAX_CELLS
constexpr int64_t MAX_POINTS = (1LL << 31) - 2 * SCAN_TILE;

struct vx_geom {
  float lo[3], hi[3], vs[3];
  int grid[3], t[3];                           // t = cells per axis of the table: grid (hard) or grid + 1 (dynamic)
  int max_points, max_voxels, ndim, mode, batch, ncap;
  uint32_t cells_pad;                          // cells of one sample, rounded up to whole bitmap words
  int64_t vcap;
};

// the workspace, in int32 words
struct vx_layout {
  int64_t words;                               // bitmap words over all samples (one more, always zero, closes the scan)
  int64_t bitmap, wprefix, pcell, prank, cmin, ccnt, cstart, cfill, plist, cg, vr, frank, voff, bsum, total;
};

bool vx_table(const link_voxelize_geom_t *g, int32_t batch, int t[3], int64_t *cells_pad) {
  int64_t cells = 1;
  for (int d = 0; d < 3; d++) {
    if (g->grid[d] <= 0 || g->grid[d] >= (1 << 24)) return false;
    t[d] = g->grid[d] + (g->mode == LINK_VOXELIZE_DYNAMIC ? 1 : 0);
    cells *= t[d];
    if (cells > MAX_SAMPLE_CELLS) return false;
  }
  *cells_pad = (cells + 31) / 32 * 32;
  return *cells_pad * batch <= MAX_BITS;
}

int vx_check(const link_voxelize_geom_t *g, int64_t ncap, int32_t batch) {
  if (!g || ncap < 0 || ncap > MAX_POINTS || batch < 1 || batch > MAX_BATCH) return LINK_ERR_ARG;
  if (g->mode != LINK_VOXELIZE_HARD && g->mode != LINK_VOXELIZE_DYNAMIC) return LINK_ERR_ARG;
  if (g->ndim < 3 || g->ndim > MAX_NDIM) return LINK_ERR_ARG;
  for (int d = 0; d < 3; d++) {
    if (!(g->vs[d] > 0.f) || !isfinite(g->vs[d]) || !isfinite(g->lo[d]) || g->grid[d] <= 0) return LINK_ERR_ARG;
    if (g->mode == LINK_VOXELIZE_DYNAMIC && !isfinite(g->hi[d])) return LINK_ERR_ARG;
  }
  if (g->mode == LINK_VOXELIZE_HARD && (g->max_points < 1 || g->max_voxels < 1)) return LINK_ERR_ARG;
  int t[3];
  int64_t cells_pad;
  if (!vx_table(g, batch, t, &cells_pad)) return LINK_ERR_ARG;         // the grid is too large for the bitmap
  return LINK_OK;
}

vx_layout vx_lay(int64_t cells_pad, int64_t ncap, int32_t batch) {
  vx_layout L;
  const int64_t n = ncap < 1 ? 1 : ncap;
  int64_t at = 0;
  auto take = [&](int64_t words) { const int64_t r = at; at += (words + 3) / 4 * 4; return r; };
  L.words = cells_pad * batch / 32;
  L.bitmap = take(L.words + 1);
  L.wprefix = take(L.words + 1);
  L.pcell = take(n); L.prank = take(n); L.cmin = take(n); L.ccnt = take(n + 1); L.cstart = take(n + 1); L.cfill = take(n);
  L.plist = take(n); L.cg = take(n); L.vr = take(n); L.frank = take(n + 1); L.voff = take(batch + 1);
  const int64_t longest = L.words + 1 > n + 1 ? L.words + 1 : n + 1;
  L.bsum = take((longest + SCAN_TILE - 1) / SCAN_TILE + 1);
  L.total = at;
  return L;
}

// ---- exclusive scan of int32 entries (MODE 1: of the popcounts of 32-bit words), three launches, any length below 2^31 ----
template <int MODE>
__device__ __forceinline__ int scan_entry(const int *__restrict__ in, int64_t i, int64_t n) {
  if (i >= n) return 0;
  const int v = in[i];
  return MODE == 1 ? __popc((unsigned)v) : v;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_vx_scan_sum(const int *__restrict__ in, int64_t n, int *__restrict__ bsum) {
  __shared__ int s_part[4];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  int v = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) v += scan_entry<MODE>(in, base + k, n);
  int total;
  block_scan_excl(v, s_part, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// the workgroup sums, in place, by one workgroup: lane t takes a run of consecutive sums
__global__ __launch_bounds__(256) void k_vx_scan_top(int *__restrict__ bsum, int nb) {
  __shared__ int s_part[4];
  const int per = (nb + 255) / 256, b0 = threadIdx.x * per;
  int v = 0;
  for (int k = 0; k < per; k++) v += b0 + k < nb ? bsum[b0 + k] : 0;
  int total;
  int run = block_scan_excl(v, s_part, total);
  for (int k = 0; k < per && b0 + k < nb; k++) {
    const int x = bsum[b0 + k];
    bsum[b0 + k] = run;
    run += x;
  }
}

// out may be in: a lane reads its entries before it writes them, and nobody else touches them
template <int MODE>
__global__ __launch_bounds__(256) void k_vx_scan_down(const int *in, int64_t n, const int *__restrict__ bsum, int *out) {
  __shared__ int s_part[4];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  int x[SCAN_ITEMS], v = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) { x[k] = scan_entry<MODE>(in, base + k, n); v += x[k]; }
  int total;
  int run = block_scan_excl(v, s_part, total) + bsum[blockIdx.x];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) {
    if (base + k < n) out[base + k] = run;
    run += x[k];
  }
}

template <int MODE>
int vx_scan(const int *in, int *out, int64_t n, int *bsum, hipStream_t st) {
  const unsigned nb = blocks_for(n, SCAN_TILE);
  hipLaunchKernelGGL(k_vx_scan_sum<MODE>, dim3(nb), dim3(256), 0, st, in, n, bsum);
  hipLaunchKernelGGL(k_vx_scan_top, dim3(1), dim3(256), 0, st, bsum, (int)nb);
  hipLaunchKernelGGL(k_vx_scan_down<MODE>, dim3(nb), dim3(256), 0, st, in, n, bsum, out);
  return check_launch("link_voxelize");
}

// ---- the pipeline ----
__device__ __forceinline__ int vx_points(const int32_t *__restrict__ po, const vx_geom &g) { return clampi(po[g.batch], 0, g.ncap); }

// Point pass: the cell of every point, its bit in the bitmap; the per-call records are reset on the way.  A coordinate that is not
// finite fails the range test (every comparison with a NaN is false, an infinity is outside) and is never converted or indexed with.
__global__ __launch_bounds__(256) void k_vx_mark(const float *__restrict__ pts, const int32_t *__restrict__ po, vx_geom g,
                                                 uint32_t *__restrict__ bitmap, uint32_t *__restrict__ pcell, int *__restrict__ cmin,
                                                 int *__restrict__ ccnt, int *__restrict__ cfill, int *__restrict__ flag) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i64 > g.ncap) return;
  const int i = (int)i64;
  flag[i] = 0;
  ccnt[i] = 0;
  if (i == g.ncap) return;
  cmin[i] = INT_MAX;
  cfill[i] = 0;
  uint32_t cell = NO_CELL;
  if (i < vx_points(po, g)) {
    const float *p = pts + (int64_t)i * g.ndim;
    bool ok = true;
    int c[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const float x = p[d];
      const float q = (x - g.lo[d]) / g.vs[d];
      float f;
      if (g.mode == LINK_VOXELIZE_HARD) {
        f = floorf(q);                                                  // point_cloud_ops.py:36-38
        ok = ok && f >= 0.f && f < (float)g.grid[d];
      } else {
        f = truncf(q);                                                  // dynamic_voxel_encoder.py:9-13
        ok = ok && x >= g.lo[d] && x <= g.hi[d] && f >= 0.f && f <= (float)g.grid[d];
      }
      c[d] = ok ? (int)f : 0;
    }
    if (ok) {
      const int b = sample_of_point(po, g.batch, i);
      cell = (uint32_t)b * g.cells_pad + (uint32_t)((c[2] * g.t[1] + c[1]) * g.t[0] + c[0]);
      atomicOr(&bitmap[cell >> 5], 1u << (cell & 31));
    }
  }
  pcell[i] = cell;
}

// rank of the point's cell among the occupied cells, the cell's minimum point index and its count
__global__ __launch_bounds__(256) void k_vx_cell(const int32_t *__restrict__ po, vx_geom g, const uint32_t *__restrict__ bitmap,
                                                 const int *__restrict__ wprefix, const uint32_t *__restrict__ pcell,
                                                 int *__restrict__ prank, int *__restrict__ cmin, int *__restrict__ ccnt) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= vx_points(po, g)) return;
  const int i = (int)i64;
  const uint32_t cell = pcell[i];
  int r = -1;
  if (cell != NO_CELL) {
    const uint32_t w = bitmap[cell >> 5];
    r = wprefix[cell >> 5] + __popc(w & ((1u << (cell & 31)) - 1u));
    if ((unsigned)r >= (unsigned)g.ncap) r = -1;                         // cannot be: there are no more occupied cells than points
  }
  prank[i] = r;
  if (r >= 0) {
    atomicMin(&cmin[r], i);
    atomicAdd(&ccnt[r], 1);
  }
}

// flag = the point is the first of its cell; the bitmap word of the cell is cleared for the next call
__global__ __launch_bounds__(256) void k_vx_first(const int32_t *__restrict__ po, vx_geom g, uint32_t *__restrict__ bitmap,
                                                  const uint32_t *__restrict__ pcell, const int *__restrict__ prank,
                                                  const int *__restrict__ cmin, int *__restrict__ flag) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= vx_points(po, g)) return;
  const int i = (int)i64;
  const uint32_t cell = pcell[i];
  if (cell != NO_CELL) bitmap[cell >> 5] = 0u;
  const int r = prank[i];
  if (r >= 0 && cmin[r] == i) flag[i] = 1;
}

// voxels per sample -> voxel_offsets (clamped to the capacity of the outputs) and their unclamped twin in the workspace
__global__ __launch_bounds__(256) void k_vx_offsets(const int32_t *__restrict__ po, vx_geom g, const int *__restrict__ frank,
                                                    const int *__restrict__ wprefix, int *__restrict__ voff,
                                                    int32_t *__restrict__ voxel_offsets) {
  __shared__ int s_cnt[MAX_BATCH];
  for (int b = threadIdx.x; b < g.batch; b += 256) {
    int c;
    if (g.mode == LINK_VOXELIZE_HARD) {
      const int s = clampi(po[b], 0, g.ncap);
      int e = clampi(po[b + 1], 0, g.ncap);
      if (e < s) e = s;
      c = frank[e] - frank[s];
      if (c > g.max_voxels) c = g.max_voxels;
    } else {
      const int64_t wps = g.cells_pad / 32;
      c = wprefix[(b + 1) * wps] - wprefix[b * wps];
    }
    s_cnt[b] = c < 0 ? 0 : c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    voff[0] = 0;
    voxel_offsets[0] = 0;
    for (int b = 0; b < g.batch; b++) {
      run += s_cnt[b];
      voff[b + 1] = (int)run;
      voxel_offsets[b + 1] = (int32_t)(run < g.vcap ? run : g.vcap);
    }
  }
}

// every point claims a position in its cell's segment (any order); the first point of a kept cell names the cell's output row
__global__ __launch_bounds__(256) void k_vx_assign(const int32_t *__restrict__ po, vx_geom g, const uint32_t *__restrict__ pcell,
                                                   const int *__restrict__ prank, const int *__restrict__ cmin,
                                                   const int *__restrict__ cstart, int *__restrict__ cfill, int *__restrict__ plist,
                                                   const int *__restrict__ frank, const int *__restrict__ voff, uint32_t *__restrict__ cg,
                                                   int *__restrict__ vr) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= vx_points(po, g)) return;
  const int i = (int)i64;
  const int r = prank[i];
  if (r < 0) return;
  const int pos = cstart[r] + atomicAdd(&cfill[r], 1);
  if ((unsigned)pos < (unsigned)g.ncap) plist[pos] = i;
  if (cmin[r] != i) return;
  cg[r] = pcell[i];
  int64_t v;
  if (g.mode == LINK_VOXELIZE_HARD) {
    const int b = sample_of_point(po, g.batch, i);
    const int local = frank[i] - frank[clampi(po[b], 0, g.ncap)];
    if (local < 0 || local >= g.max_voxels) return;                      // a cell past the first max_voxels: all its points are dropped
    v = (int64_t)voff[b] + local;
  } else {
    v = r;
  }
  if (v < g.vcap && v < g.ncap) vr[v] = r;
}

__device__ void vx_sort(int *a, int n) {
  if (n <= 16) {
    for (int i = 1; i < n; i++) {
      const int x = a[i];
      int j = i - 1;
      while (j >= 0 && a[j] > x) { a[j + 1] = a[j]; j--; }
      a[j + 1] = x;
    }
    return;
  }
  auto sift = [&](int root, int end) {                                   // heap sort in place: n log n whatever the order
    const int x = a[root];
    for (;;) {
      int child = 2 * root + 1;
      if (child >= end) break;
      if (child + 1 < end && a[child + 1] > a[child]) child++;
      if (a[child] <= x) break;
      a[root] = a[child];
      root = child;
    }
    a[root] = x;
  };
  for (int s = n / 2 - 1; s >= 0; s--) sift(s, n);
  for (int e = n - 1; e > 0; e--) {
    const int x = a[0];
    a[0] = a[e];
    a[e] = x;
    sift(0, e);
  }
}

// Finish, one lane per output row: sort the voxel's point list, gather its rows in ascending point order, write voxels (when asked
// for), mean, coors = b, z, y, x and num_points; rows past the total are zeroed.
__global__ __launch_bounds__(256) void k_vx_finish(const float *__restrict__ pts, vx_geom g, const int32_t *__restrict__ voxel_offsets,
                                                   const int *__restrict__ vr, const int *__restrict__ cstart, const int *__restrict__ ccnt,
                                                   int *__restrict__ plist, const uint32_t *__restrict__ cg, float *__restrict__ voxels,
                                                   float *__restrict__ mean, int32_t *__restrict__ coors, int32_t *__restrict__ num_points) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= g.vcap) return;
  const int nd = g.ndim;
  const int64_t vrow = (int64_t)g.max_points * nd;
  int k = 0, c = 0, s = 0;
  int4 co = {0, 0, 0, 0};
  if (v < voxel_offsets[g.batch]) {
    int r = vr[v];
    const bool sane = (unsigned)r < (unsigned)g.ncap;                    // cannot fail: every row below the total was named
    if (!sane) r = 0;
    s = cstart[r];
    c = sane ? ccnt[r] : 0;
    if (s < 0 || c < 0 || (int64_t)s + c > g.ncap) c = 0;                // cannot be: the segments tile the point list
    vx_sort(plist + s, c);
    k = g.mode == LINK_VOXELIZE_HARD && c > g.max_points ? g.max_points : c;
    const uint32_t cell = cg[r];
    const uint32_t lin = cell % g.cells_pad;
    co.x = (int)(cell / g.cells_pad);
    co.y = (int)(lin / ((uint32_t)g.t[0] * (uint32_t)g.t[1]));
    co.z = (int)((lin / (uint32_t)g.t[0]) % (uint32_t)g.t[1]);
    co.w = (int)(lin % (uint32_t)g.t[0]);
  }
  float acc[MAX_NDIM];
#pragma unroll
  for (int d = 0; d < MAX_NDIM; d++) acc[d] = 0.f;
  for (int j = 0; j < k; j++) {
    const float *p = pts + (int64_t)plist[s + j] * nd;
#pragma unroll
    for (int d = 0; d < MAX_NDIM; d++) {
      if (d < nd) {
        const float x = p[d];
        acc[d] = acc[d] + x;
        if (voxels) voxels[v * vrow + (int64_t)j * nd + d] = x;
      }
    }
  }
  if (voxels)
    for (int64_t e = (int64_t)k * nd; e < vrow; e++) voxels[v * vrow + e] = 0.f;
  const float div = (float)(k > 0 ? k : 1);
#pragma unroll
  for (int d = 0; d < MAX_NDIM; d++)
    if (d < nd) mean[v * nd + d] = acc[d] / div;
  reinterpret_cast<int4 *>(coors)[v] = co;
  num_points[v] = k;
}

}  // namespace

extern "C" size_t link_voxelize_workspace_bytes(const link_voxelize_geom_t *geom, int64_t n_points_capacity, int32_t batch) {
  if (vx_check(geom, n_points_capacity, batch) != LINK_OK) return 0;
  int t[3];
  int64_t cells_pad;
  vx_table(geom, batch, t, &cells_pad);
  return (size_t)vx_lay(cells_pad, n_points_capacity, batch).total * 4;
}

extern "C" int link_voxelize(const link_voxelize_geom_t *geom, const float *points, const int32_t *point_offsets, int32_t batch,
                             int64_t n_points_capacity, void *workspace, size_t workspace_bytes, float *voxels, float *mean,
                             int32_t *coors, int32_t *num_points, int64_t voxel_capacity, int32_t *voxel_offsets, void *stream) {
  int rc = vx_check(geom, n_points_capacity, batch);
  if (rc != LINK_OK) return rc;
  if (voxel_capacity < 0 || voxel_capacity > MAX_POINTS) return LINK_ERR_ARG;
  if (!point_offsets || !voxel_offsets || !workspace) return LINK_ERR_ARG;
  if (n_points_capacity > 0 && !points) return LINK_ERR_ARG;
  if (voxel_capacity > 0 && (!mean || !coors || !num_points)) return LINK_ERR_ARG;
  if (geom->mode == LINK_VOXELIZE_DYNAMIC && voxels) return LINK_ERR_ARG;            // the dynamic voxels ARE the mean
  if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(coors)) & 15) return LINK_ERR_ARG;
  vx_geom g;
  int64_t cells_pad;
  vx_table(geom, batch, g.t, &cells_pad);
  const vx_layout L = vx_lay(cells_pad, n_points_capacity, batch);
  if (workspace_bytes < (size_t)L.total * 4) return LINK_ERR_WORKSPACE;
  for (int d = 0; d < 3; d++) { g.lo[d] = geom->lo[d]; g.hi[d] = geom->hi[d]; g.vs[d] = geom->vs[d]; g.grid[d] = geom->grid[d]; }
  g.max_points = geom->mode == LINK_VOXELIZE_HARD ? geom->max_points : 1;
  g.max_voxels = geom->max_voxels; g.ndim = geom->ndim; g.mode = geom->mode; g.batch = batch;
  g.ncap = (int)n_points_capacity; g.cells_pad = (uint32_t)cells_pad; g.vcap = voxel_capacity;

  int *ws = reinterpret_cast<int *>(workspace);
  uint32_t *bitmap = reinterpret_cast<uint32_t *>(ws + L.bitmap), *pcell = reinterpret_cast<uint32_t *>(ws + L.pcell);
  uint32_t *cg = reinterpret_cast<uint32_t *>(ws + L.cg);
  int *wprefix = ws + L.wprefix, *prank = ws + L.prank, *cmin = ws + L.cmin, *ccnt = ws + L.ccnt, *cstart = ws + L.cstart;
  int *cfill = ws + L.cfill, *plist = ws + L.plist, *vr = ws + L.vr, *frank = ws + L.frank, *voff = ws + L.voff, *bsum = ws + L.bsum;
  const hipStream_t st = S(stream);
  const dim3 block(256), per_point(blocks_for(n_points_capacity + 1, 256));
  const char *what = "link_voxelize";

  hipLaunchKernelGGL(k_vx_mark, per_point, block, 0, st, points, point_offsets, g, bitmap, pcell, cmin, ccnt, cfill, frank);
  if ((rc = check_launch(what)) != LINK_OK) return rc;
  if ((rc = vx_scan<1>(reinterpret_cast<const int *>(bitmap), wprefix, L.words + 1, bsum, st)) != LINK_OK) return rc;
  hipLaunchKernelGGL(k_vx_cell, per_point, block, 0, st, point_offsets, g, bitmap, wprefix, pcell, prank, cmin, ccnt);
  hipLaunchKernelGGL(k_vx_first, per_point, block, 0, st, point_offsets, g, bitmap, pcell, prank, cmin, frank);
  if ((rc = check_launch(what)) != LINK_OK) return rc;
  if (g.mode == LINK_VOXELIZE_HARD && (rc = vx_scan<0>(frank, frank, n_points_capacity + 1, bsum, st)) != LINK_OK) return rc;
  if ((rc = vx_scan<0>(ccnt, cstart, n_points_capacity + 1, bsum, st)) != LINK_OK) return rc;
  hipLaunchKernelGGL(k_vx_offsets, dim3(1), block, 0, st, point_offsets, g, frank, wprefix, voff, voxel_offsets);
  hipLaunchKernelGGL(k_vx_assign, per_point, block, 0, st, point_offsets, g, pcell, prank, cmin, cstart, cfill, plist, frank, voff, cg, vr);
  if ((rc = check_launch(what)) != LINK_OK) return rc;
  if (voxel_capacity > 0)
    hipLaunchKernelGGL(k_vx_finish, dim3(blocks_for(voxel_capacity, 256)), block, 0, st, points, g, voxel_offsets, vr, cstart, ccnt, plist, cg,
                       voxels, mean, coors, num_points);
  return check_launch(what);
}
