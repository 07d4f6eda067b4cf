// link_amd/csrc/kmap.hip -- kernel maps of a sparse convolution with any per-axis kernel size and stride
// (include/link_amd.h section D, "general geometries"): candidate output sites of a strided convolution
// (torchsparse/nn/functional/downsample.py:30-44), the per-output gather table over a BOX of offsets
// (nn/functional/conv.py:103-113 with nn/utils/kernel.py:11-32) and the table of the opposite direction.
// Plain index kernels: one lane per element, no LDS, no scratch.
#include "common.h"

using namespace link;

namespace {

constexpr int KMAP_MAX_EXTENT = 7;

__device__ __host__ __forceinline__ int tap_lo(int k) { return -((k + 1) / 2) + 1; }   // -k // 2 + 1 (kernel.py:20)

// ---------------------------------------------------------------------------------------------
// candidate output sites
// ---------------------------------------------------------------------------------------------
// An input at c offers, per axis, the taps j in [tap_lo(k), tap_lo(k) + k) with (c + j * ts) on the lattice of
// s * ts: j = -c / ts (mod s), at most ceil(k / s) of them.  Thread (input, combination of one such tap per axis)
// writes the site in LATTICE units, (b, x / ss, y / ss, z / ss) -- the row form link_index_cells sorts -- or a row
// outside every grid (batch = bad_b) when a tap is past the kernel, the site lies below the inputs' per-axis minimum
// (downsample.py:41) or the input is not a multiple of the tensor stride.  That last case is the reference's own result, not an
// extra filter: (c + j * ts) % (s * ts) == 0 implies c % ts == 0, so such an input has no site there either.  No upper filter
// (downsample.py:39).
struct kmap_geom { int k[3], s[3], ts[3], slots[3], lo[3], bad_b; };

__global__ void __launch_bounds__(256) k_kmap_candidates(const int4 *__restrict__ coords, int64_t n, kmap_geom g, int ncomb,
                                                         int4 *__restrict__ cand) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * ncomb) return;
  const int64_t i = t / ncomb;
  int c = (int)(t - i * ncomb);
  const int4 r = coords[i];                            // (x, y, z, b)
  const int pos[3] = {r.x, r.y, r.z};
  int o[3];
  bool ok = true;
#pragma unroll
  for (int d = 2; d >= 0; d--) {
    const int slot = c % g.slots[d];
    c /= g.slots[d];
    const int q = floordiv(pos[d], g.ts[d]);
    ok &= q * g.ts[d] == pos[d];
    const int jlo = tap_lo(g.k[d]);
    const int a = -(q + jlo);
    const int j = jlo + (a - floordiv(a, g.s[d]) * g.s[d]) + slot * g.s[d];     // first tap on the lattice, then every s-th
    ok &= j < jlo + g.k[d];
    ok &= pos[d] + j * g.ts[d] >= g.lo[d];
    o[d] = floordiv(q + j, g.s[d]);                    // exact: q + j is a multiple of s
  }
  cand[t] = ok ? make_int4(r.w, o[0], o[1], o[2]) : make_int4(g.bad_b, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------
// gather table over a box of offsets
// ---------------------------------------------------------------------------------------------
struct kmap_box { int k[3], step[3]; };

// lane = (row, offset), offset fastest: a wave writes 64 consecutive table entries.  The cell-table load is
// unconditional on a clamped address; the select drops what an outside cell read.
__global__ void __launch_bounds__(256) k_kmap_box_table(const int4 *__restrict__ rows, int64_t m, const int32_t *__restrict__ cell_tab,
                                                        link_grid_t g, kmap_box b, int K, int32_t *__restrict__ table) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m * K) return;
  const int64_t row = t / K;
  const int k = (int)(t - row * K);
  int ix, iy, iz;
  if (K & 1) { ix = k % b.k[0]; iy = (k / b.k[0]) % b.k[1]; iz = k / (b.k[0] * b.k[1]); }        // odd volume: x fastest, z outermost
  else { iz = k % b.k[2]; iy = (k / b.k[2]) % b.k[1]; ix = k / (b.k[2] * b.k[1]); }              // even volume: z fastest, x outermost
  const int4 c = rows[row];
  const int32_t cell = cell_of(g, c.x + (tap_lo(b.k[0]) + ix) * b.step[0], c.y + (tap_lo(b.k[1]) + iy) * b.step[1],
                               c.z + (tap_lo(b.k[2]) + iz) * b.step[2], c.w);
  const int32_t v = cell_tab[cell < 0 ? 0 : cell];
  table[t] = cell < 0 ? -1 : v - 1;
}

// ---------------------------------------------------------------------------------------------
// the opposite direction's table
// ---------------------------------------------------------------------------------------------
// back[i, k] = j  <=>  table[j, k] = i: out + offset_k = in fixes out, so at most one j per (i, k) when the output rows are
// unique; with duplicate output rows the smallest j wins (an unsigned minimum over entries that start at 0xFFFFFFFF = -1), so the
// result does not depend on the order the lanes run in.
__global__ void __launch_bounds__(256) k_kmap_transpose(const int32_t *__restrict__ table, int64_t total, int K, int64_t n_in,
                                                        unsigned int *__restrict__ back) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int32_t i = table[t];
  if (i < 0 || (int64_t)i >= n_in) return;
  const int64_t j = t / K;
  const int k = (int)(t - j * K);
  atomicMin(&back[(int64_t)i * K + k], (unsigned int)j);
}

bool box_ok(const int32_t *kernel, int &K) {
  K = 1;
  for (int d = 0; d < 3; d++) {
    if (kernel[d] < 1 || kernel[d] > KMAP_MAX_EXTENT) return false;
    K *= kernel[d];
  }
  return true;
}

}  // namespace

extern "C" int32_t link_kmap_candidate_count(const int32_t *kernel, const int32_t *stride) {
  int K;
  if (!kernel || !stride || !box_ok(kernel, K)) return -1;
  int32_t ncomb = 1;
  for (int d = 0; d < 3; d++) {
    if (stride[d] < 1) return -1;
    ncomb *= (kernel[d] + stride[d] - 1) / stride[d];
  }
  return ncomb;
}

extern "C" int link_kmap_out_candidates(const int32_t *coords, int64_t n, const int32_t *kernel, const int32_t *stride,
                                        const int32_t *tensor_stride, const int32_t *lo, int32_t *cand, void *stream) {
  if (n < 0 || !kernel || !stride || !tensor_stride || !lo) return LINK_ERR_ARG;
  const int32_t ncomb = link_kmap_candidate_count(kernel, stride);
  if (ncomb < 1) return LINK_ERR_ARG;
  kmap_geom g;
  for (int d = 0; d < 3; d++) {
    if (tensor_stride[d] < 1 || (int64_t)stride[d] * tensor_stride[d] >= (1LL << 30)) return LINK_ERR_ARG;
    g.k[d] = kernel[d]; g.s[d] = stride[d]; g.ts[d] = tensor_stride[d]; g.lo[d] = lo[d];
    g.slots[d] = (kernel[d] + stride[d] - 1) / stride[d];
  }
  if (lo[3] == INT32_MIN) return LINK_ERR_ARG;
  g.bad_b = lo[3] - 1;                                 // below the batch axis of every grid built from these bounds
  if (n == 0) return LINK_OK;
  if (!coords || !cand || n * ncomb >= (1LL << 31)) return LINK_ERR_ARG;
  const int64_t total = n * ncomb;
  hipLaunchKernelGGL(k_kmap_candidates, dim3(blocks_for(total, 256)), dim3(256), 0, S(stream),
                     reinterpret_cast<const int4 *>(coords), n, g, (int)ncomb, reinterpret_cast<int4 *>(cand));
  return check_launch("link_kmap_out_candidates");
}

extern "C" int link_kmap_box_table(const int32_t *rows, int64_t m, const int32_t *cell_tab, const link_grid_t *grid,
                                   const int32_t *kernel, const int32_t *step, int32_t *table, void *stream) {
  int K;
  if (m < 0 || !grid || !kernel || !step || !box_ok(kernel, K)) return LINK_ERR_ARG;
  kmap_box b;
  int64_t cells = 1;
  for (int d = 0; d < 3; d++) {
    if (step[d] < 1) return LINK_ERR_ARG;
    b.k[d] = kernel[d]; b.step[d] = step[d];
  }
  for (int a = 0; a < 4; a++) {
    if (grid->dim[a] <= 0) return LINK_ERR_ARG;
    cells *= grid->dim[a];
    if (cells >= (1LL << 30)) return LINK_ERR_ARG;
  }
  if (m == 0) return LINK_OK;
  if (!rows || !cell_tab || !table || m * K >= (1LL << 31)) return LINK_ERR_ARG;
  hipLaunchKernelGGL(k_kmap_box_table, dim3(blocks_for(m * K, 256)), dim3(256), 0, S(stream),
                     reinterpret_cast<const int4 *>(rows), m, cell_tab, *grid, b, K, table);
  return check_launch("link_kmap_box_table");
}

extern "C" int link_kmap_transpose(const int32_t *table, int64_t m, int32_t kvol, int64_t n_in, int32_t *back, void *stream) {
  if (m < 0 || n_in < 0 || kvol < 1 || kvol > KMAP_MAX_EXTENT * KMAP_MAX_EXTENT * KMAP_MAX_EXTENT) return LINK_ERR_ARG;
  if (m * kvol >= (1LL << 31) || n_in * kvol >= (1LL << 31)) return LINK_ERR_ARG;
  if (n_in == 0) return LINK_OK;
  if (!back || (m > 0 && !table)) return LINK_ERR_ARG;
  hipError_t e = hipMemsetAsync(back, 0xFF, (size_t)n_in * kvol * sizeof(int32_t), S(stream));
  if (e != hipSuccess) {
    set_error("link_kmap_transpose", e);
    return LINK_ERR_LAUNCH;
  }
  if (m == 0) return LINK_OK;
  hipLaunchKernelGGL(k_kmap_transpose, dim3(blocks_for(m * kvol, 256)), dim3(256), 0, S(stream), table, m * kvol, (int)kvol, n_in,
                     reinterpret_cast<unsigned int *>(back));
  return check_launch("link_kmap_transpose");
}
