/*
 * include/link_amd.h -- C ABI of the MI355X-native LinK hot path (liblink_amd.so).
 *
 * This is the drop-in boundary: plain pointers + sizes + a HIP stream, no torch types.  All
 * pointers are DEVICE pointers unless a parameter says "host".  Every entry point
 *   - launches asynchronously on `stream` (a hipStream_t passed as void*; NULL = default stream),
 *   - never allocates, never synchronises, never throws; caller owns every buffer,
 *   - returns LINK_OK (0) or a negative LINK_ERR_* code (argument/launch errors only; data-dependent
 *     conditions are reported through the device-side status word documented per call).
 *
 * Section A replaces, one for one, the functions the reference registers in its pybind11 module
 * `torchsparse.backend` (/root/reference/segmentation/torchsparse-u/torchsparse/backend/
 * pybind_cuda.cpp:18-39) that lie on the LinK path.  Section B is the fused form of the Python layer
 * above them (segmentation/core/models/utils.py:44-84 voxel_to_aux / aux_to_voxel,
 * detection/det3d/models/utils/ts_elk.py:68-107).  Section C is the fused R_core of
 * ELKBlock.forward / TSELKBlock.forward_ (segmentation/core/models/semantic_kitti/linkunet.py:124-185,
 * detection/det3d/models/utils/ts_elk.py:144-230).
 *
 * Feature dtype: fp32 (the shipped reference runs this path in fp32; voxelnet.py:55 has autocast
 * commented out).  Integer results are bit-exact with the reference; fp32 within 1e-4 rel.
 */
#ifndef LINK_AMD_H_
#define LINK_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LINK_OK 0
#define LINK_ERR_ARG (-1)       /* null pointer / negative size / unsupported width */
#define LINK_ERR_LAUNCH (-2)    /* hipGetLastError() != hipSuccess after a launch */
#define LINK_ERR_WORKSPACE (-3) /* caller-provided workspace too small */
#define LINK_BATCH_TIMEOUT (-4) /* link_dc_batch_status: a bounded wait inside a persistent batch kernel gave up (section H) */

/* Version of this ABI (bumped on any signature change). */
int link_abi_version(void);
/* sizeof of the structs crossing this boundary (0 link_grid_t, 1 link_elk_desc_t, 2 link_elk_buffers_t, 3 link_dc_grid_t,
 * 4 link_dc_tuning_t, 5 link_dc_buffers_t, 6 link_lean_buffers_t, 7 link_block_args_t, 8 link_voxelize_geom_t; -1 otherwise): what a binding checks its own layout against. */
int32_t link_abi_struct_size(int32_t which);
/* Human-readable last HIP error string of the calling thread ("" if none). Host pointer. */
const char *link_last_error(void);

/* =============================================================================================
 * A. torchsparse.backend drop-ins
 * ============================================================================================= */

/* hash_cuda(idx[N,4] i32) -> i64[N]           backend/hash/hash_cuda.cu:10-23,67-73
 * 64-bit FNV-1a over the four 32-bit words, folded to 60 bits.  Bit-exact. */
int link_hash(const int32_t *coords, int64_t n, int64_t *out, void *stream);

/* kernel_hash_cuda(idx[N,4] i32, off[K,3] i32) -> i64[K,N] (k-major)
 *                                             backend/hash/hash_cuda.cu:27-55,75-84
 * Hash of (x+ox, y+oy, z+oz, b); batch taken from the row itself (CUDA semantics). Bit-exact. */
int link_kernel_hash(const int32_t *coords, int64_t n, const int32_t *offsets, int64_t k,
                     int64_t *out, void *stream);

/* hash_query_cuda(q i64[n1], tgt i64[n], tgt_idx i64[n]) -> i64[n1]
 *                                             backend/others/query_cuda.cu:9-58,
 *                                             backend/hashmap/hashmap_cuda.cu:9-130
 * out[i] = tgt_idx[j]+1 for the FIRST j with tgt[j]==q[i], else 0 (the Python wrapper subtracts 1,
 * nn/functional/query.py:32).  The reference builds a 3-function cuckoo table with host-side
 * rehash retries and two device syncs per call; here: one open-addressing table in `workspace`
 * (linear probing, wait-free 64-bit CAS insert of the key, atomicMin on the index for first-wins),
 * no sync, no reserved key.  Workspace need not be initialised.  `link_hash_query_workspace_bytes(n)`. */
size_t link_hash_query_workspace_bytes(int64_t n_target);
int link_hash_query(const int64_t *query, int64_t n1, const int64_t *target,
                    const int64_t *target_idx, int64_t n, int64_t *out, void *workspace,
                    size_t workspace_bytes, void *stream);

/* count_cuda(idx i32[N], s) -> i32[s]         backend/others/count_cuda.cu:10-31
 * Histogram; idx<0 (or >= s) ignored.  `out` is zeroed by the call. */
int link_count(const int32_t *idx, int64_t n, int32_t *out, int64_t s, void *stream);

/* calc_ti_weights(coords fp32[P,4] (x,y,z,batch), idx_query i64[8,P], scale) -> fp32[8,P]
 *                                              torchsparse/nn/functional/devoxelize.py:10-48
 * Trilinear weights of a point's 8 corner voxels (corner k = 4 dx + 2 dy + dz), zero where idx_query is -1,
 * renormalised by (their sum + 1e-8).  One kernel, one thread per point. */
int link_ti_weights(const float *coords, const int64_t *idx_query, int64_t p, float scale, float *w, void *stream);

/* voxelize_forward_cuda(in fp[N,c], idx i32[N], counts i32[N1]) -> fp[N1,c]
 *                                             backend/voxelize/voxelize_cuda.cu:12-25,44-61
 * out[idx[i]] += in[i] / (float)counts[idx[i]].  `out` is zeroed by the call.  Generic form for an
 * arbitrary idx (fp32 atomics, like the reference); the indexed, deterministic form is B.2. */
int link_voxelize_forward(const float *in, const int32_t *idx, const int32_t *counts, int64_t n,
                          int64_t c, int64_t n1, float *out, void *stream);

/* voxelize_backward_cuda(top fp[N1,c], idx, counts, N) -> fp[N,c]
 *                                             backend/voxelize/voxelize_cuda.cu:28-42,63-80
 * bottom[i] = top[idx[i]] / counts[idx[i]]  (0 where idx[i] < 0).  Every idx[i] must be below the length of `counts` (an idx
 * built with its counts: the block index); link_voxelize_backward_n1 takes that length n1 and gives a zero row to idx[i] >= n1,
 * the rows link_voxelize_forward skips (voxelize_cuda.cu:38) -- what the drop-in backend function calls. */
int link_voxelize_backward(const float *top, const int32_t *idx, const int32_t *counts, int64_t n,
                           int64_t c, float *bottom, void *stream);
int link_voxelize_backward_n1(const float *top, const int32_t *idx, const int32_t *counts, int64_t n,
                              int64_t c, int64_t n1, float *bottom, void *stream);

/* devoxelize_forward_cuda(feat fp[n,c], ind i32[N,K], w fp[N,K], r) -> fp[N,c],  K = r^3
 *                                             backend/devoxelize/devoxelize_cuda.cu:11-34,63-81
 * out[i] = sum_{k<K, ind>=0} w[i,k]*feat[ind[i,k]], k ascending (deterministic). */
int link_devoxelize_forward(const float *feat, const int32_t *ind, const float *w, int64_t nq,
                            int64_t c, int64_t k, float *out, void *stream);

/* devoxelize_backward_cuda(top fp[N,c], ind, w, n, r) -> fp[n,c]
 *                                             backend/devoxelize/devoxelize_cuda.cu:37-59,85-101
 * bottom[ind[i,k]] += w[i,k]*top[i].  `bottom` is zeroed by the call (fp32 atomics). */
int link_devoxelize_backward(const float *top, const int32_t *ind, const float *w, int64_t nq,
                             int64_t n, int64_t c, int64_t k, float *bottom, void *stream);

/* =============================================================================================
 * B. Block index + indexed aggregation (fused voxel_to_aux / aux_to_voxel)
 * ============================================================================================= */

/* Dense block grid covering the frame.  Block coordinate of a voxel = (floor(x/s), floor(y/s),
 * floor(z/s), b) (utils.py:45); `lo` is the smallest block coordinate per axis, `dim` the extent in
 * blocks.  Cells are linearised x-major: cell = (((bx-lo0)*dim1 + (by-lo1))*dim2 + (bz-lo2))*dim3 +
 * (bb-lo3), which is exactly the signed lexicographic row order torch.unique(dim=0) produces
 * (utils.py:47), so the rank of an occupied cell among occupied cells IS the reference's block id. */
typedef struct {
  int32_t s;       /* block edge in voxel-coordinate units (the `s` of voxel_to_aux) */
  int32_t lo[4];   /* block-coordinate lower bound (x,y,z,b) */
  int32_t dim[4];  /* block-grid extent (x,y,z,b); product = number of cells V (< 2^30) */
} link_grid_t;

/* Host helper: grid from inclusive voxel-coordinate bounds lo/hi[4] (x,y,z,b).  Returns V or -1. */
int64_t link_grid_from_bounds(const int32_t lo[4], const int32_t hi[4], int32_t s, link_grid_t *g);

/* Device bounding box of coords (for callers that do not know the bounds): writes
 * bbox[8] = {min x,y,z,b, max x,y,z,b}.  One pass, per-workgroup reduction + 8 atomics per
 * workgroup.  `bbox` must be initialised by the caller to {INT_MAX x4, INT_MIN x4}. */
int link_coords_bbox(const int32_t *coords, int64_t n, int32_t *bbox, void *stream);

/* Index header written by link_index_build (device int32[LINK_HDR_WORDS]). */
#define LINK_HDR_M 0        /* number of occupied blocks M */
#define LINK_HDR_STATUS 1   /* 0 ok; bit0: a voxel lay outside the grid (index invalid) */
#define LINK_HDR_NVALID 2   /* number of voxels indexed (= N when status == 0) */
#define LINK_HDR_WORDS 8

/* Scratch sizes for link_index_build (bytes). `cell_counts` (V u32) MUST be all-zero on entry and is
 * all-zero again on exit (the scan clears what it consumes), so one allocation zeroed once serves
 * every later call.  `scratch` needs no initialisation. */
size_t link_index_scratch_bytes(int64_t n, int64_t v);

/* Build the block index of a frame: replaces sphash + torch.unique + sphash + sphashquery + spcount
 * of voxel_to_aux (utils.py:45-51) by counting into the dense grid + one decoupled-look-back scan.
 * Outputs (caller-allocated; M <= N so N rows always suffice):
 *   cell_blk   i32[V]    block id + 1 of each cell, 0 = empty       (neighbour lookup table)
 *   vox_blk    i32[N]    block id of each voxel                      (== idx_query, utils.py:50)
 *   idx_query  i64[N]    same as int64 (may be NULL)                 (reference dtype)
 *   perm       i32[N]    voxel ids grouped by block, ascending voxel id inside a block of at most 8192 voxels (a longer
 *                        segment holds the block's ids in the order their atomics ranked them: k_sort_seg, SORT_MAX_SEG)
 *   vox_sorted i32[N,4]  (x, y, z, voxel id) of the voxel at each position of perm: the record the
 *                        fused kernels stream instead of chasing perm -> coords (may be NULL)
 *   pos_blk    i32[N]    block id of the voxel at each position of perm (may be NULL)
 *   blk_start  i32[N+1]  start of each block's segment in perm; blk_start[M] = hdr[LINK_HDR_NVALID] (= N when no voxel
 *                        lies outside the grid; such a voxel gets vox_blk = idx_query = -1 and sets status bit 0, the rest is
 *                        the index of the voxels inside with their ids kept, perm / pos_blk / vox_sorted valid in [0, NVALID))
 *   blk_coords i32[N,4]  block coordinates, rows [0,M) valid         (== small_x.C, utils.py:47)
 *   counts     i32[N]    voxels per block, rows [0,M) valid          (== spcount, utils.py:51)
 *   hdr        i32[8]    see LINK_HDR_*
 * Bit-exact with the reference for small_x.C / idx_query / counts. */
int link_index_build(const int32_t *coords, int64_t n, const link_grid_t *grid /* host */,
                     uint32_t *cell_counts, void *scratch, size_t scratch_bytes, int32_t *cell_blk,
                     int32_t *vox_blk, int64_t *idx_query, int32_t *perm, int32_t *vox_sorted,
                     int32_t *pos_blk, int32_t *blk_start, int32_t *blk_coords, int32_t *counts,
                     int32_t *hdr, void *stream);
/* link_index_build with the blocks numbered in FIRST-VOXEL order instead of cell order: block b is the b-th voxel, in id order,
 * that has the smallest id of its cell.  For callers that need a numbering, not the reference's (ElkCorePlan: block order never
 * leaves the arena): the scan runs over the N voxels instead of the V cells of the grid -- on LiDAR stage frames (1-2 % of the
 * cells occupied) the cell scan is 10-17 us of a 28 us index.  Same outputs and meanings as link_index_build (replaces
 * utils.py:44-58 up to the order of the rows of small_x.C), except: block order; no cell_counts (cell_pair takes its place);
 * the previous frame's entries of cell_blk are cleared through its block list (hdr[LINK_HDR_M] rows of blk_coords as the previous
 * call on these buffers left them), so cell_blk / hdr / blk_coords must be the ones the previous call wrote (or zero-filled).
 * cell_pair: u64[V], zero-filled once by the caller, zero again after every call.  n < 2^30.  Deterministic: voxel ids, not
 * insertion order, decide. */
int link_index_build_first(const int32_t *coords, int64_t n, const link_grid_t *grid /* host */, uint64_t *cell_pair, void *scratch,
                           size_t scratch_bytes, int32_t *cell_blk, int32_t *vox_blk, int64_t *idx_query, int32_t *perm,
                           int32_t *vox_sorted, int32_t *pos_blk, int32_t *blk_start, int32_t *blk_coords, int32_t *counts,
                           int32_t *hdr, void *stream);
/* The cell half of link_index_build alone (no voxel placement): sorted unique block coordinates blk_coords i32[.,4],
 * counts, cell table and hdr[LINK_HDR_M] of the rows `coords` -- rows outside the grid are dropped SILENTLY: nothing places
 * the rows here, so no kernel sets the status bit and hdr[LINK_HDR_STATUS] is written 0; hdr[LINK_HDR_NVALID] counts the rows
 * inside, and NVALID < n is how a caller tells.  (The candidate kernel relies on it: its "no site" row lies outside every grid.)
 * Same scratch / cell_counts contract as link_index_build.  Used for the output-site set of site-creating
 * convolutions, whose candidate rows are mostly duplicates. */
int link_index_cells(const int32_t *coords, int64_t n, const link_grid_t *grid, uint32_t *cell_counts, void *scratch,
                     size_t scratch_bytes, int32_t *cell_blk, int32_t *blk_start, int32_t *blk_coords, int32_t *counts,
                     int32_t *hdr, void *stream);

/* Neighbour map nbr i32[M,K] (K = r^3, offsets in get_kernel_offsets(r) order, nn/utils/kernel.py:
 * 11-32: odd r x fastest, even r z fastest): replaces sphash(C, offsets) + sphash + sphashquery +
 * transpose of aux_to_voxel (utils.py:65-73).  -1 = absent.  `m` may be an upper bound (rows past
 * hdr[M] are not written); offsets are multiplied by `step` (1 for LinK blocks; the tensor stride when
 * the rows are strided voxel coordinates, as sparse-conv kernel maps use them, nn/functional/conv.py:
 * 105-107); transpose != 0 uses negated offsets (the adjoint relation, needed by the backward pass
 * when r is even).  `hdr` may be NULL (then all m rows are valid).  Bit-exact. */
int link_neighbor_map(const int32_t *blk_coords, const int32_t *cell_blk, const link_grid_t *grid,
                      const int32_t *hdr, int64_t m, int32_t r, int32_t step, int32_t transpose,
                      int32_t *nbr, void *stream);

/* Same for arbitrary (foreign) block rows: first scatter row ids into a cell table that the caller
 * zero-initialised (first row wins for duplicates), then look up.  Rows outside the grid -> status. */
int link_cell_table_build(const int32_t *rows, int64_t m, const link_grid_t *grid, int32_t *cell_blk,
                          int32_t *hdr, void *stream);
/* ... and back: zero the cells link_cell_table_build wrote for the same rows (m scattered stores), so that a table kept
 * between calls is all zero again without a memset over every cell of a sparse grid. */
int link_cell_table_clear(const int32_t *rows, int64_t m, const link_grid_t *grid, int32_t *cell_blk, void *stream);

/* Indexed block mean (spvoxelize forward, utils.py:52): out[b] = sum_{i in block b, ascending i}
 * in[i]/counts[b].  Deterministic, no atomics; rows [0,M) of out[.,c] written.  `m_cap` = rows
 * allocated in `out` (>= M). */
int link_block_mean(const float *in, const int32_t *perm, const int32_t *blk_start,
                    const int32_t *hdr, int64_t n, int64_t c, int64_t m_cap, float *out, void *stream);

/* Adjoint of link_block_mean (spvoxelize backward): bottom[i] = top[vox_blk[i]]/counts[vox_blk[i]]
 * is link_voxelize_backward (A). */

/* aux_to_voxel feature half (utils.py:75-82):
 *   new[m] = sum_k small_f[nbr[m,k]]*counts[nbr[m,k]] / sum_k counts[nbr[m,k]] ; out[i] = new[idx[i]].
 * small_f fp[M,c] block means, nbr i32[M,K], idx i64[N].  `new_feat` fp[M,c] and `denom` fp[M]
 * (sum of neighbour counts) are kept for the backward pass.  k ascending, deterministic. */
int link_aux_to_voxel_forward(const float *small_f, const int32_t *counts, const int32_t *nbr,
                              const int64_t *idx, int64_t n, int64_t m, int64_t c, int64_t k,
                              float *new_feat, float *denom, float *out, void *stream);

/* Backward of the above wrt small_f: given g_out fp[N,c]:
 *   g_new[m] = sum_{i: idx[i]==m} g_out[i]            (segmented via perm/blk_start: deterministic)
 *   g_small[j] = counts[j] * sum_{m: j in nbr(m)} g_new[m]/denom[m]   (via the transposed map nbr_t)
 * g_new fp[M,c] is scratch. */
int link_aux_to_voxel_backward(const float *g_out, const int32_t *perm, const int32_t *blk_start,
                               const int32_t *counts, const int32_t *nbr_t, const float *denom,
                               int64_t n, int64_t m, int64_t c, int64_t k, float *g_new,
                               float *g_small, void *stream);
/* aux_to_voxel forward on the dense block grid (same results as link_aux_to_voxel_forward, which takes an
 * explicit neighbour table): means -> sum table, r^3 neighbour sum by the fused path's z-sliding block
 * gather, float4 row gather to voxels.  Needs the index that produced `small_f`'s row order
 * (blk_coords, cell_blk, grid, hdr from link_index_build), w % 8 == 0 or w % 12 == 0, r <= 3
 * (LINK_ERR_ARG otherwise).  S scratch fp[(m+1)*(w+1)]; new_feat fp[m,w]; denom fp[m]; out fp[n,w]. */
int link_aux_to_voxel_forward_grid(const float *small_f, const int32_t *counts, const int32_t *blk_coords,
                                   const int32_t *cell_blk, const link_grid_t *grid /* host */,
                                   const int32_t *hdr, const int64_t *idx, int64_t n, int64_t m, int32_t w,
                                   int32_t r, float *S, float *new_feat, float *denom, float *out,
                                   void *stream);
/* The same result with the rows written by the gather kernel itself: out[perm[p]] = the row of block b for p in
 * [blk_start[b], blk_start[b + 1]) (perm / blk_start of link_index_build).  Two launches; neither the [M, W] table of
 * neighbour means (`new_feat`) nor the row gather exist.  denom f32[M] as above. */
int link_aux_to_voxel_forward_scatter(const float *small_f, const int32_t *counts, const int32_t *blk_coords,
                                      const int32_t *cell_blk, const link_grid_t *grid /* host */, const int32_t *hdr,
                                      const int32_t *blk_start, const int32_t *perm, int64_t n, int64_t m, int32_t w, int32_t r,
                                      float *S /* scratch f32[(M+1)*(W+1)] */, float *denom, float *out, void *stream);

/* =============================================================================================
 * C. Fused ELKBlock core (R_core of SURVEY.md section 8d)
 * ============================================================================================= */

#define LINK_OP_COS 0   /* linkunet.py:150-162 / ts_elk.py:166-177   X = [F cos, F sin]            */
#define LINK_OP_SIN 1   /* linkunet.py:136-148 / ts_elk.py:155-164   X = [F sin, F cos], minus sign */
#define LINK_OP_COSX 2  /* linkunet.py:164-176                       X = [F cos, F sin, F theta]    */

typedef struct {
  int32_t op;            /* LINK_OP_* */
  int32_t c;             /* channels C (inc) */
  int32_t cg;            /* theta channels: channel j uses theta[j % cg]  (C/groups; C for cos_x) */
  int32_t r;             /* neighbourhood edge in blocks */
  float coord_div;       /* theta input = float(coord) / coord_div (float division, as the reference
                            does it): 1.0 everywhere except the encoder cos_x variant, which feeds
                            coords / tensor_stride (linkencoder.py:165) */
  float eps;             /* LayerNorm eps (1e-6, linkunet.py:111,121) */
  int32_t flags;         /* general layout: kernel-path selection of THIS call (0 = defaults; nothing is process-global).  The
                            alternative paths are what the default ones are tested against (tests/test_gpu_split_paths.py) */
} link_elk_desc_t;
#define LINK_ELK_LANE_CHANNEL 1    /* lane = channel kernels instead of the lane-group kernels */
#define LINK_ELK_NO_PAIR 2         /* no voxel-pair sharing of sincos between channels j and j + C/2 */
#define LINK_ELK_FUSED_GATHER 4    /* one fused gather + de-modulate kernel instead of block gather + per-voxel kernel */
#define LINK_ELK_NO_DENSE_GRID 8   /* block gather: column-walking form even on mostly occupied grids */
#define LINK_ELK_LEAN_CS 32        /* link_elk_core_lean_forward: channel-split form of launch 1 whenever C is 64 / 128 */
#define LINK_ELK_LEAN_NO_CS 64     /* ... never (default: by frame size) */
#define LINK_ELK_LEAN_PM 128       /* link_elk_core_lean_forward: the form without the scratch matrix X (pre_mix inside launch 2; C <= 64) */
#define LINK_ELK_LEAN_NO_PM 256    /* ... never (default: by frame size) */
#define LINK_ELK_TILES 16          /* link_elk_core_forward: the tile form (two launches: link_elk_premix_modsum_tiles +
                                      link_elk_gather_demod_tiles); needs link_elk_buffers_t::s_bytes */

/* pre_mix: fin = LayerNorm(F @ Wpre^T) * g + b  (linkunet.py:109-112,132).  F fp[N,C], Wpre fp[C,C]
 * (nn.Linear layout [out,in]).  C <= 256. */
int link_premix_ln(const float *feats, const float *w_pre, const float *ln_w, const float *ln_b,
                   int64_t n, int32_t c, float eps, float *fin, void *stream);

/* Modulate + per-block pre-aggregation (linkunet.py:151-160 + utils.py:52,75-76 fused):
 *   theta = (float(xyz)/coord_div) @ Wpos^T (* alpha), tiled by cg;
 *   S[b] = [ sum_i fin_i*cos(theta_i), sum_i fin_i*sin(theta_i) (, sum_i fin_i*theta_i), count_b ]
 * over the voxels of block b in ascending voxel id.  Block SUMS, not means (mean*count of the
 * reference re-multiplies what it just divided).  S layout: m_cap rows of nparts*C floats (row =
 * 512 B at C=64: four aligned 128-B lines), one extra all-zero row (id m_cap: what absent neighbours
 * point at), then the m_cap+1 counts (fp32) at S + (m_cap+1)*nparts*C, i.e. S has
 * (m_cap+1)*(nparts*C + 1) floats.  The SAME m_cap must be passed to every call that touches S.
 * w_pos fp[cg,3]; alpha fp[cg] or NULL. */
int link_modulate_block_sum(const float *fin, const int32_t *vox_sorted, const float *w_pos,
                            const float *alpha, const int32_t *blk_start,
                            const int32_t *hdr, const link_elk_desc_t *desc /* host */, int64_t n,
                            int64_t m_cap, float *S, void *stream);

/* Neighbour-block sum + normalise + broadcast + de-modulate + LayerNorm(norm)
 * (utils.py:65-82 + linkunet.py:162,178 fused): for every block the r^3 neighbour rows of S are
 * summed in get_kernel_offsets order, divided by the summed count, and every voxel of the block gets
 *   new = A_cos*cos(theta) + A_sin*sin(theta) [+ (A_lin - fin*theta)]   ('sin': A_cos*cos - A_sin*sin
 *   with X=[F sin, F cos]) ; out = LayerNorm(new)*g + b.
 * `fin` is only read for LINK_OP_COSX (may be NULL otherwise).  out fp[N,C]. */
int link_gather_demod_ln(const float *S, const float *fin, const int32_t *vox_sorted,
                         const float *w_pos, const float *alpha, const float *ln_w, const float *ln_b,
                         const int32_t *blk_start, const int32_t *blk_coords,
                         const int32_t *cell_blk, const link_grid_t *grid /* host */,
                         const int32_t *hdr, const link_elk_desc_t *desc /* host */, int64_t n,
                         int64_t m_cap, float *out, void *stream);

/* Split form of link_gather_demod_ln (same result, two simpler kernels; C % 4 == 0, r <= 3):
 *   link_block_gather   A[m] = (sum of the r^3 neighbour rows of S) / (summed count)  -> fp[M, P*C]
 *   link_voxel_demod_ln per voxel (loop-free, one 16-byte-per-lane group per voxel pair): read the
 *                       block's A row, de-modulate, LayerNorm, store out[voxel]. */
int link_block_gather(const float *S, const int32_t *blk_coords, const int32_t *cell_blk,
                      const link_grid_t *grid /* host */, const int32_t *hdr,
                      const link_elk_desc_t *desc /* host */, int64_t m_cap, float *A, void *stream);
int link_voxel_demod_ln(const float *A, const float *fin, const int32_t *vox_sorted,
                        const int32_t *pos_blk, const float *w_pos, const float *alpha, const float *ln_w,
                        const float *ln_b, const int32_t *hdr, const link_elk_desc_t *desc /* host */,
                        int64_t n, float *out, void *stream);

/* One-call form of the whole R_core step (what bench.py times): optional index build (section B)
 * followed by the section-C kernels (pre_mix, modulate+block-sum, block gather, voxel de-modulate),
 * all on `stream`, from caller-owned buffers.  Exists so
 * that a host written in an interpreted language pays ONE FFI crossing per LinK block instead of one
 * per kernel.  All pointers are device pointers with the meanings documented above. */
typedef struct {
  const void *feats;         /* [N,C]  block input (st.F): fp32, or io_dtype rows with LINK_ELK_TILES */
  const int32_t *coords;     /* i32[N,4] (st.C) */
  const float *w_pre, *pre_ln_w, *pre_ln_b;   /* pre_mix.0.weight [C,C], pre_mix.1.{weight,bias} [C] */
  const float *w_pos, *alpha;                 /* pos_weight.0.weight [cg,3]; alpha [cg] or NULL */
  const float *ln_w, *ln_b;                   /* norm.{weight,bias} [C] */
  uint32_t *cell_counts; void *scratch; size_t scratch_bytes;          /* link_index_build scratch */
  int32_t *cell_blk, *vox_blk; int64_t *idx_query; int32_t *perm, *vox_sorted, *pos_blk, *blk_start, *blk_coords, *counts, *hdr;
  float *fin;                /* fp[N,C]            scratch: pre_mix output */
  float *S;                  /* fp[(m_cap+1)*(P*C+1)] scratch: block table rows + zero row + counts */
  float *A;                  /* fp[m_cap, P*C]     scratch: normalised neighbour sums (NULL: fused gather) */
  void *out;                 /* [N,C]              result (new_st_F after self.norm), same element type as feats */
  int64_t s_bytes;           /* bytes available at S (0: the size above); LINK_ELK_TILES needs link_elk_tiles_table_bytes() */
  int32_t io_dtype;          /* LINK_IO_F32 (0) / LINK_IO_F16 / LINK_IO_BF16: element type of feats and out; 16-bit rows need
                                LINK_ELK_TILES (the four-kernel form is fp32) */
  int32_t reserved;
  uint64_t *cell_pair;       /* u64[V] zero-filled once, self-cleaning: link_index_build_first (build_index = 2); NULL otherwise */
} link_elk_buffers_t;

/* Tile form of the section-C kernels on a built index (elk_tiles_impl.h): TWO launches for R_core instead of four, made for
 * the frames the dense-cell layout (section E) does not take: sparse block grids with many voxels per occupied block
 * (LiDAR: linkunet.py:345-363 on SemanticKITTI, scn.py:586-607 on nuScenes), C in {16, 32, 64, 128}, r in {2, 3}.
 *   link_elk_premix_modsum_tiles  = link_premix_ln + link_modulate_block_sum in one pass over the voxels in block order
 *       (pre_mix on the matrix cores; per-block sums by segmented scans in the accumulator layout; blocks of any size are
 *       split over waves and combined in a fixed order: bitwise reproducible, no atomics).  Writes the table S (rows,
 *       zero row, counts -- the layout of link_modulate_block_sum -- followed by scratch rows: S must hold
 *       link_elk_tiles_table_bytes(desc, n, m_cap) bytes) and, for LINK_OP_COSX only, fin.
 *   link_elk_gather_demod_tiles   = link_block_gather + link_voxel_demod_ln in one kernel: a wave per 16-64 sorted positions,
 *       the neighbour sums of the blocks among them formed once in LDS.
 * Same results as the four-kernel form to rounding (sums are formed in a different, fixed order). */
int64_t link_elk_tiles_table_bytes(const link_elk_desc_t *desc /* host */, int64_t n, int64_t m_cap);
int link_elk_premix_modsum_tiles(const float *feats, const int32_t *vox_sorted, const int32_t *pos_blk,
                                 const int32_t *blk_start, const int32_t *hdr, const float *w_pre,
                                 const float *pre_ln_w, const float *pre_ln_b, const float *w_pos, const float *alpha,
                                 const link_elk_desc_t *desc /* host */, int64_t n, int64_t m_cap, float *S,
                                 int64_t s_bytes, float *fin, void *stream);
int link_elk_gather_demod_tiles(const float *S, const float *fin, const int32_t *vox_sorted, const int32_t *pos_blk,
                                const int32_t *blk_coords, const int32_t *cell_blk, const link_grid_t *grid /* host */,
                                const int32_t *hdr, const float *w_pos, const float *alpha, const float *ln_w,
                                const float *ln_b, const link_elk_desc_t *desc /* host */, int64_t n, int64_t m_cap,
                                float *out, void *stream);
/* The two tile-form entries with fp16 / bf16 feature rows at the kernel boundary (io_dtype = LINK_IO_F32 / LINK_IO_F16 /
 * LINK_IO_BF16, section D: feats of the first, out of the second; tables, fin, sums and LayerNorm stay fp32) -- what
 * TSELKBlock runs under autocast on LiDAR-shaped frames, with no cast pass on either side. */
int link_elk_premix_modsum_tiles_io(const void *feats, int32_t io_dtype, const int32_t *vox_sorted, const int32_t *pos_blk,
                                    const int32_t *blk_start, const int32_t *hdr, const float *w_pre, const float *pre_ln_w,
                                    const float *pre_ln_b, const float *w_pos, const float *alpha,
                                    const link_elk_desc_t *desc /* host */, int64_t n, int64_t m_cap, float *S,
                                    int64_t s_bytes, float *fin, void *stream);
int link_elk_gather_demod_tiles_io(const float *S, const float *fin, const int32_t *vox_sorted, const int32_t *pos_blk,
                                   const int32_t *blk_coords, const int32_t *cell_blk, const link_grid_t *grid /* host */,
                                   const int32_t *hdr, const float *w_pos, const float *alpha, const float *ln_w,
                                   const float *ln_b, const link_elk_desc_t *desc /* host */, int64_t n, int64_t m_cap,
                                   void *out, int32_t io_dtype, void *stream);

/* build_index: 0 = the index of the previous call on these buffers (same coordinates); 1 = link_index_build first;
 * 2 = link_index_build_first first (buf->cell_pair must be set). */
int link_elk_core_forward(const link_elk_buffers_t *buf /* host */, const link_grid_t *grid /* host */,
                          const link_elk_desc_t *desc /* host */, int64_t n, int64_t m_cap,
                          int32_t build_index, void *stream);

/* Lean form of R_core with the index REBUILT every call (round 4, csrc/elk_lean_impl.h): THREE launches, none proportional to the
 * grid, for the LiDAR stage frames the reference feeds its blocks (linkunet.py:345-363, scn.py:586-607: a few thousand to a few ten
 * thousand voxels, block grid 1-20 % occupied).  Replaces, per call, what the reference rebuilds per call: sphash + torch.unique +
 * sphashquery (utils.py:44-63, query_cuda.cu:9-58) and the voxelize / devoxelize pair (voxelize_cuda.cu:12-25,
 * devoxelize_cuda.cu:11-34) around linkunet.py:132-178.
 *   launch 1  X rows [F cos | F sin (| F theta)] of the voxels in input order (pre_mix on the matrix cores, LayerNorm, theta,
 *             sincos) into `X`; rank = cnt[cell]++, list[cell][rank] = voxel id; one work item (cell * 16 + chunk) per started
 *             chunk of 32 voxels of a cell, appended to one of 16 item lists (one atomic per workgroup); workgroups behind the
 *             frame's own clear the previous frame's counters through its item lists;
 *   launch 2  a wave per item: the chunk's voxels in ascending id (ranked by counting),
 *             S[cell][chunk] = sum of their X rows, their records (x, y, z, id) in that order -> rec2;
 *   launch 3  a wave per item: chunk rows of the r^3 neighbour cells (present iff cnt > 0; the first chunk of each is requested
 *             together with the counts) summed and divided by the summed count, the chunk's voxels de-modulated and
 *             LayerNorm'ed -> out.  cos_x reads fin * theta back from the voxel's X row.
 * Bitwise reproducible (sums in id order, fixed combination order).  No block numbering exists: tables are addressed by grid
 * cell and touched only where voxels land.  C in {16, 32, 64, 128}, r in {2, 3}, k <= 352, cells < 2^27.
 * The caller alternates (cnt, occ, ctrl) with (cnt_prev, occ_prev, ctrl_prev) between indexed steps (build_index = 1); with
 * build_index = 0 the lists of the previous step on the same buffers are reused (same coordinates) and the *_prev members are
 * not touched.  `n_prev`: voxels of the previous indexed step (0 on the first).
 * hdr: STATUS bit 0 a voxel outside the grid, bit 1 a cell over capacity (such voxels get no output row). */
typedef struct {
  const void *feats;          /* [N,C] io_dtype rows */
  const int32_t *coords;      /* i32[N,4] */
  const float *w_pre, *pre_ln_w, *pre_ln_b, *w_pos, *alpha, *ln_w, *ln_b;   /* as link_elk_buffers_t */
  uint32_t *cnt, *cnt_prev;   /* u32[V << cnt_shift] each, zero-filled once; self-cleaning from then on */
  int32_t *list;              /* i32[V*k]: voxel ids of a cell in arrival order */
  int32_t *rec2;              /* i32[16*seg_cap*32][4]: records (x, y, z, id) of an item's voxels in ascending id */
  int32_t *occ, *occ_prev;    /* i32[16 * seg_cap] each: work items, list l at l * seg_cap */
  uint32_t *ctrl, *ctrl_prev; /* u32[256] each, zero-filled once: item count of list l at word 16 l */
  float *X;                   /* f32[n_cap, P*C] scratch */
  float *S;                   /* f32[V * kch, P*C] chunk rows by cell, kch = ceil(k / 32); needs no initialisation */
  int32_t *hdr;               /* i32[8] zero-filled once */
  void *out;                  /* [N,C] io_dtype rows */
  int64_t seg_cap;            /* items a list holds: >= ceil(ceil(n_cap / 64) / 16) * 64 + 64 */
  int32_t k;                  /* slot capacity of a cell (s^3 clipped to 352) */
  int32_t io_dtype;           /* LINK_IO_* */
  int32_t cnt_shift;          /* the counter of cell c is word c << cnt_shift (0 .. 5): on a small grid every counter gets its own
                                 line, because the atomics of a few hundred cells with hundreds of voxels each would otherwise
                                 serialise on a handful of lines */
  int32_t reserved;
} link_lean_buffers_t;
int link_elk_core_lean_forward(const link_lean_buffers_t *buf /* host */, const link_grid_t *grid /* host */,
                               const link_elk_desc_t *desc /* host */, int64_t n, int64_t n_prev, int32_t build_index,
                               void *stream);

/* ---------------------------------------------------------------------------------------------
 * Training form of R_core (forward with saved state + hand-written backward).
 *
 * The reference differentiates linkunet.py:132-178 through torch autograd: nn.Linear / nn.LayerNorm
 * nodes, the sin/cos/mul/cat graph, and VoxelizeFunction.backward / DevoxelizeFunction.backward
 * (voxelize.py:34-50, devoxelize.py:76-93; voxelize_cuda.cu:28-42, devoxelize_cuda.cu:37-59: fp
 * atomicAdd scatter).  Here the forward is the inference kernels (plus the region counts `den`), and
 * the backward is six kernels, deterministic (no atomics); the only step left to the host's GEMM library
 * is the weight gradient g_pre^T @ F.  Group kernels only: C % 4 == 0 and r <= 3 (pre_mix backward:
 * C % 16 == 0, C <= 128); LINK_ERR_ARG otherwise and the host falls back to its op-by-op composition.
 *
 * All `partials` outputs are fp[link_elk_mid_partial_rows(), Q, C] per-workgroup partial sums which the
 * host adds up over rows (fixed grid -> deterministic).
 *
 * link_elk_mid_forward   fin -> out.  S scratch fp[(m_cap+1)*(P*C+1)]; A fp[m_cap, P*C] and den
 *     fp[m_cap] are SAVED for backward.  ln_w/ln_b NULL: out = new (before self.norm); non-NULL:
 *     out = self.norm(new) (the inference kernels unchanged).
 * link_elk_out_ln_backward   backward of self.norm with its input recomputed from (A, fin, theta):
 *     g_out = d/d(norm output) -> g_new = d/d(new); partials Q=2: [d norm.weight | d norm.bias].
 * link_elk_mid_backward      g_new -> g_fin (d/d(pre_mix output)); S and gS fp[m_cap,P*C] scratch;
 *     partials Q=4: [d alpha (tiled) | d w_pos[:,0] | d w_pos[:,1] | d w_pos[:,2]] per channel; the host
 *     folds channels ch -> ch % cg (theta is tiled, linkunet.py:154).
 * link_premix_ln_backward    backward of pre_mix = LayerNorm(F @ Wpre^T) with the pre-norm activations
 *     recomputed by the forward's MFMA schedule: g_fin -> g_pre fp[N,C] (d/d(F @ Wpre^T), stored for the
 *     weight-gradient GEMM) and g_feats fp[N,C] = g_pre @ Wpre (second MFMA pass); partials Q=2:
 *     [d pre_mix.1.weight | d pre_mix.1.bias]. */
int link_elk_mid_forward(const float *fin, const int32_t *vox_sorted, const int32_t *pos_blk,
                         const int32_t *blk_start, const int32_t *blk_coords, const int32_t *cell_blk,
                         const link_grid_t *grid /* host */, const int32_t *hdr, const float *w_pos,
                         const float *alpha, const link_elk_desc_t *desc /* host */, const float *ln_w,
                         const float *ln_b, int64_t n, int64_t m_cap, float *S, float *A, float *den,
                         float *out, void *stream);
int32_t link_elk_mid_partial_rows(void);
int link_elk_out_ln_backward(const float *g_out, const float *A, const float *fin, const int32_t *vox_sorted,
                             const int32_t *pos_blk, const float *w_pos, const float *alpha,
                             const float *ln_w, const int32_t *hdr, const link_elk_desc_t *desc /* host */,
                             int64_t n, float *g_new, float *partials, void *stream);
int link_elk_mid_backward(const float *g_new, const float *fin, const float *A, const float *den,
                          const int32_t *vox_sorted, const int32_t *pos_blk, const int32_t *blk_start,
                          const int32_t *blk_coords, const int32_t *cell_blk,
                          const link_grid_t *grid /* host */, const int32_t *hdr, const float *w_pos,
                          const float *alpha, const link_elk_desc_t *desc /* host */, int64_t n, int64_t m_cap,
                          float *S, float *gS, float *g_fin, float *partials, void *stream);
int link_premix_ln_backward(const float *feats, const float *w_pre, const float *ln_w, const float *g_fin,
                            int64_t n, int32_t c, float eps, float *g_pre, float *g_feats, float *partials,
                            void *stream);
/* The block's tail for training: y = relu(addend + LayerNorm(x) * ln_w + ln_b)
 * (`st.F = self.activate(new_st_F + self.norm_local(st_local.F))`, linkunet.py:183 / ts_elk.py:228) and its
 * backward: g_addend = g_y * (y > 0); g_x = LayerNorm backward of that (statistics recomputed from x);
 * partials fp[link_elk_mid_partial_rows(), 2, C] = per-workgroup sums of [d ln_w | d ln_b].  C % 4 == 0,
 * C <= 256.  (Inference fuses the tail into the convolution: link_subm_conv_ln_add_relu.) */
int link_ln_add_relu_forward(const float *x, const float *addend, const float *ln_w, const float *ln_b,
                             int64_t n, int32_t c, float eps, float *y, void *stream);
int link_ln_add_relu_backward(const float *g_y, const float *y, const float *x, const float *ln_w, int64_t n,
                              int32_t c, float eps, float *g_addend, float *g_x, float *partials, void *stream);
/* Autocast training (ABI 13): the four training entries above with fp16 / bf16 feature rows at the kernel boundary,
 * io_dtype = LINK_IO_F32 / LINK_IO_F16 / LINK_IO_BF16 (any other value: LINK_ERR_ARG).  The 16-bit rows are widened on load
 * and the 16-bit results rounded to nearest even on store; everything in between is fp32 as in the fp32 entries, so each
 * gives, bit for bit, the fp32 entry's result on the widened rows, rounded once.  Non-finite values stay non-finite.
 *   link_premix_ln_io            feats in io_dtype; w_pre, ln_w / ln_b and fin fp32.  16-bit rows: C % 16 == 0, C <= 128
 *                                (the MFMA path; LINK_ERR_ARG otherwise); LINK_IO_F32 is link_premix_ln.
 *   link_premix_ln_backward_io   feats (read) and g_feats (written) in io_dtype; g_fin, g_pre and partials fp32.
 *   link_ln_add_relu_forward_io  x (the local_mix rows) in io_dtype; addend and y fp32 (autocast's LayerNorm is fp32).
 *   link_ln_add_relu_backward_io x (read) and g_x (written) in io_dtype; g_y, y, g_addend and partials fp32. */
int link_premix_ln_io(const void *feats, int32_t io_dtype, const float *w_pre, const float *ln_w, const float *ln_b,
                      int64_t n, int32_t c, float eps, float *fin, void *stream);
int link_premix_ln_backward_io(const void *feats, int32_t io_dtype, const float *w_pre, const float *ln_w,
                               const float *g_fin, int64_t n, int32_t c, float eps, float *g_pre, void *g_feats,
                               float *partials, void *stream);
int link_ln_add_relu_forward_io(const void *x, int32_t io_dtype, const float *addend, const float *ln_w,
                                const float *ln_b, int64_t n, int32_t c, float eps, float *y, void *stream);
int link_ln_add_relu_backward_io(const float *g_y, const float *y, const void *x, int32_t io_dtype, const float *ln_w,
                                 int64_t n, int32_t c, float eps, float *g_addend, void *g_x, float *partials,
                                 void *stream);
/* Column sums of up to three partial arrays fp[rows, cols_k] (k = 0..2; cols_k == 0 skips one) into
 * out fp[cols0+cols1+cols2], one launch, fixed summation order. */
int link_sum_partials(const float *p0, int32_t cols0, const float *p1, int32_t cols1, const float *p2,
                      int32_t cols2, int64_t rows, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Section D -- row N1 of SURVEY.md section 8f: stride-1 submanifold sparse convolution (what
 * ELKBlock.local_mix = spnn.Conv3d(inc, inc, 3) runs, linkunet.py:109,125).
 * Replaces torchsparse.backend.convolution_forward_cuda (pybind_cuda.cpp:19;
 * convolution/convolution_cuda.cu:53-165: per kernel offset gather -> cuBLAS mm -> scatter-add) for the
 * in-place-coordinates case with ONE output-stationary kernel (accumulators in registers over all
 * offsets, W_k staged in LDS, f32 MFMA), fed by a per-output neighbour table instead of the
 * reference's (in,out) pair lists:
 *   nbr  i32[N, kvol]   nbr[v,k] = input row at coords[v] + offset_k * tensor_stride, -1 absent; offsets
 *                       in get_kernel_offsets order (nn/utils/kernel.py:9-33) -- link_neighbor_map output
 *   w    fp[kvol, Cin, Cout]   the module's `kernel` parameter as stored (nn/modules/conv.py:34-38)
 *   out  fp[N, Cout] = sum_k feats[nbr[:,k]] @ w[k]
 *   order i32[N] or NULL: a permutation of the voxels (e.g. link_index_build's `perm`): tile t of the MFMA
 *                       kernel computes voxels order[16t..16t+15]; spatially sorted voxels let whole tiles
 *                       skip absent offsets.  Results do not depend on it.
 * The table is per OUTPUT row, so the same entry serves down-sampling (kernel 2 / stride 2: N = coarse rows,
 * entries = fine rows) and transposed convolutions (N = fine rows, one non-absent entry = the parent);
 * feats may have any number of rows.  MFMA path for Cin, Cout multiples of 16 up to 128 (the square
 * widths and the channel changes of the reference encoders are instantiated); other widths <= 256 take a
 * lane=channel kernel.
 * The input gradient of this convolution is the same call on grad_out with w'[k] = w[kvol-1-k]^T
 * (the neighbour relation of an odd kernel at stride 1 is symmetric). */
int link_subm_conv_forward(const float *feats, const int32_t *nbr, const float *w, const int32_t *order,
                           int64_t n, int32_t cin, int32_t cout, int32_t kvol, float *out, void *stream);
/* Row N2 (fused epilogue): out = relu(addend + LayerNorm(conv(feats)) * ln_w + ln_b) in the convolution's
 * store phase -- `st.F = self.activate(new_st_F + self.norm_local(st_local.F))` (linkunet.py:183,
 * ts_elk.py:228) with addend = the R_core output.  addend may be NULL; eps of norm_local.
 * `relu` is a flag word: bit 0 = ReLU; bit 1 = ln_w / ln_b are a plain per-channel affine out = conv * ln_w + ln_b
 * (an inference-mode BatchNorm folded to scale / shift, with the convolution's bias folded into the shift) instead
 * of LayerNorm weights -- the BN (+ residual) (+ ReLU) epilogues of the detection stages (scn.py:83-107,482-489)
 * and of the encoders' conv blocks (linkunet.py:18-92,217-224).  Same flag word in link_conv_pairs_sum and
 * link_conv_centre_sum. */
int link_subm_conv_ln_add_relu(const float *feats, const int32_t *nbr, const float *w, const int32_t *order,
                               int64_t n, int32_t cin, int32_t cout, int32_t kvol, const float *ln_w,
                               const float *ln_b, float eps, const float *addend, int32_t relu, float *out,
                               void *stream);
/* Weight gradient of the convolution above: g_w[k][ci][co] = sum_v feats[nbr[v,k]][ci] * g_out[v][co]
 * (replaces the weight half of convolution_backward_cuda, convolution_cuda.cu:167-278: per offset gather +
 * cuBLAS mm(in^T, grad)).  nbr_t i32[kvol, N] is the TRANSPOSED neighbour table (coalesced column
 * reads); C = Cin = Cout <= 64, C % 4 == 0.  partial fp[link_subm_conv_wgrad_chunks(), kvol, C, C]: the
 * host sums the chunk axis (fixed grid -> deterministic). */
int32_t link_subm_conv_wgrad_chunks(void);
int link_subm_conv_wgrad(const float *feats, const float *gout, const int32_t *nbr_t, int64_t n, int32_t c,
                         int32_t kvol, float *partial, void *stream);
/* Round 5: the split is the caller's -- `chunks` pieces of the voxel range per offset, and `centre_extra` MORE pieces for the
 * centre offset kvol / 2, whose column is dense on a submanifold table (every voxel pairs with itself: with one workgroup per
 * (offset, chunk) its workgroups set the kernel's time).  partial f32[kvol * chunks + centre_extra][c][c]; g_w[k] = sum over
 * chunk of slot [chunk * kvol + k], plus for k = kvol / 2 the slots from kvol * chunks on.  (conv.py:67-101, the reference's
 * convolution backward.) */
int link_subm_conv_wgrad_split(const float *feats, const float *gout, const int32_t *nbr_t, int64_t n, int32_t c, int32_t kvol,
                               int32_t chunks, int32_t centre_extra, float *partial, void *stream);
/* ... and its reduction in one launch: g_w f32[kvol][c][c] = sum over chunk of slot [chunk * kvol + k] (+ the centre_extra slots for
 * k = kvol / 2), slot order (deterministic). */
int link_subm_conv_wgrad_reduce(const float *partial, int32_t c, int32_t kvol, int32_t chunks, int32_t centre_extra, float *gw,
                                void *stream);

/* Pair-list form of the same convolution, for sparse frames (few of the K neighbours present per voxel).
 * The kernel map is the reference's own: per kernel offset the list of (input row, output row) pairs
 * (nbmaps / nbsizes, nn/functional/conv.py:109-122; consumed offset by offset in convolution_cuda.cu:90-165
 * as gather -> cuBLAS -> scatter-add).  Here ONE MFMA launch computes every pair's contribution row and ONE
 * output-stationary launch adds them per voxel in a fixed order (no atomics, deterministic) with the optional
 * bias / LayerNorm + add + ReLU epilogue.
 *   rows_pad     contribution rows, a multiple of 128.  Rows are grouped by kernel offset, each group padded to
 *                a 128-row granule; pair_in i32[rows_pad] = input row of the pair (-1: padding);
 *                wg_k i32[rows_pad/128] = kernel offset of each granule (-1: skip).
 *   contrib      fp32[rows_pad, cout] scratch: contrib[p] = feats[pair_in[p]] . w[wg_k[p/128]].
 *   n_direct     output voxels i < n_direct take contrib[i] as their first term (submanifold: the centre
 *                offset's pairs are the identity and occupy rows [0, n)); 0 for strided / transposed maps.
 *   ext_start i32[n+1], ext_list i32[...]: CSR list of the other contribution rows of every output voxel,
 *                ascending kernel offset.
 * Widths: link_conv_pairs_supported(cin, cout) (multiples of 16 the LinK networks use, <= 128). */
int link_conv_pairs_supported(int32_t cin, int32_t cout);
int link_conv_pairs_gemm(const float *feats, const int32_t *pair_in, const int32_t *wg_k, int64_t rows_pad,
                         const float *w, int32_t cin, int32_t cout, float *contrib, void *stream);
int link_conv_pairs_sum(const float *contrib, const int32_t *ext_start, const int32_t *ext_list, int64_t n,
                        int64_t n_direct, int32_t cout, const float *bias, const float *ln_w, const float *ln_b,
                        float eps, const float *addend, int32_t relu, float *out, void *stream);
/* Submanifold tables (odd kernel, identical input and output coordinates: nbr[i, centre] == i): the centre
 * offset's GEMM runs on the output rows themselves and the voxel is finished in the accumulators --
 * out[i] = epilogue(feats[i] . w[centre] + sum of contrib[ext_list[ext_start[i] .. ext_start[i+1])]) with the
 * same epilogue as link_conv_pairs_sum.  contrib (contrib_rows rows, < 4 GiB) then holds only the OTHER offsets' rows (link_conv_pairs_gemm
 * over a pair list without the centre), so the centre term never travels through HBM. */
/* Output sites of a site-creating sparse convolution (spconv's SparseConv3d as the detection backbone uses it,
 * scn.py:496-502: kernel 3 or 1, stride 2 or 1, padding per axis; axes (z, y, x), indices i32[n,4] = (b, z, y, x)):
 * cand i32[n * link_conv_out_candidate_count(kernel, stride), 4] receives every candidate site of every input, rows
 * of -1 where a combination is invalid or outside out_shape.  Sorted unique rows = link_index_build with block
 * edge 1 over `cand` (out-of-range rows are dropped there). */
int32_t link_conv_out_candidate_count(const int32_t *kernel, const int32_t *stride);
int link_conv_out_candidates(const int32_t *indices, int64_t n, const int32_t *kernel, const int32_t *stride,
                             const int32_t *padding, const int32_t *out_shape, int32_t *cand, void *stream);
/* Gather table of such a convolution straight from the (b, z, y, x) rows: link_conv_site_table scatters input row + 1 into a
 * table over (batch, in_shape) that the caller keeps all zero between uses (clear != 0 undoes the scatter of the same rows:
 * no memset over a sparse grid); link_conv_gather_table then writes table i32[m, taps] = the input row at
 * out * stride - padding + tap for the taps (a, b, c) in row-major order over `kernel` (each 1..3), -1 where no site.
 * batch * prod(in_shape) < 2^31. */
int link_conv_site_table(const int32_t *indices, int64_t n, const int32_t *in_shape, int32_t batch, int32_t *table,
                         int32_t clear, void *stream);
int link_conv_gather_table(const int32_t *out_indices, int64_t m, const int32_t *kernel, const int32_t *stride,
                           const int32_t *padding, const int32_t *in_shape, int32_t batch, const int32_t *site_table,
                           int32_t *table, void *stream);
/* General geometries: the kernel map of a convolution with ANY per-axis kernel size (1..7) and stride, as the reference's
 * conv3d builds it (nn/functional/conv.py:103-122).  Coordinates i32[.,4] = (x, y, z, b); per-axis arrays are i32[3] on the host.
 *
 * link_kmap_out_candidates -- the candidate rule of spdownsample (nn/functional/downsample.py:30-44, taken when some axis has
 *   1 < stride != kernel): an output site is every input + offset (offsets per axis arange(-k//2+1, k//2+1) * tensor_stride,
 *   nn/utils/kernel.py:20) whose coordinates are multiples of stride * tensor_stride and not below lo[0..2], the per-axis
 *   minimum of the inputs (lo[3] = the smallest batch index); there is no upper filter, as in the reference.  One thread per
 *   (input, combination of one on-lattice tap per axis): cand i32[n * link_kmap_candidate_count, 4] receives the sites in
 *   LATTICE units, rows (b, x / ss, y / ss, z / ss) with ss = stride * tensor_stride -- the row form link_index_cells sorts
 *   into the (batch, x, y, z) order of downsample.py:46-50 -- and rows (lo[3] - 1, 0, 0, 0), which every grid over the inputs'
 *   batch range drops, where a combination gives no site (an input that is not a multiple of tensor_stride gives none, as in
 *   the reference: (c + j * ts) % (s * ts) == 0 needs c % ts == 0).  lo must be the EXACT per-axis minimum, not a lower bound.  link_kmap_candidate_count = prod ceil(kernel / stride), -1 for
 *   arguments the builder does not take.  (link_conv_out_candidates above is spconv's rule -- padding, an output shape --
 *   and a different relation.)
 * link_kmap_box_table -- table i32[m, K], K = kx * ky * kz: table[j, k] = the input row at rows[j] + offset_k, offsets
 *   (tap_x * step_x, tap_y * step_y, tap_z * step_z) in get_kernel_offsets order (kernel.py:24-30: odd K x fastest and z
 *   outermost, even K z fastest and x outermost), -1 where no input lies; step = the input's tensor stride per axis
 *   (conv.py:105-107: the dilation is not applied).  cell_tab: link_cell_table_build over the input rows on `grid` (block
 *   edge 1).  Replaces sphash(out, offsets) -> sphashquery (conv.py:108-113) for the box; link_neighbor_map is the cubic,
 *   one-step case and stays as it is.  m * K < 2^31.
 * link_kmap_transpose -- the opposite direction: back i32[n_in, K] with back[i, k] = j <=> table[j, k] = i, -1 elsewhere
 *   (out + offset_k = in fixes out, for any geometry): the table of the transposed convolution and of the input gradient,
 *   which the reference reads off the same pair list with the two columns swapped (conv.py:114-118, convolution_cuda.cu:
 *   `transpose`).  A fill with -1 and one launch; entries of `table` outside [0, n_in) are ignored; among duplicate output
 *   rows the smallest j wins (deterministic). */
int32_t link_kmap_candidate_count(const int32_t *kernel, const int32_t *stride);
int link_kmap_out_candidates(const int32_t *coords, int64_t n, const int32_t *kernel, const int32_t *stride,
                             const int32_t *tensor_stride, const int32_t *lo, int32_t *cand, void *stream);
int link_kmap_box_table(const int32_t *rows, int64_t m, const int32_t *cell_tab, const link_grid_t *grid,
                        const int32_t *kernel, const int32_t *step, int32_t *table, void *stream);
int link_kmap_transpose(const int32_t *table, int64_t m, int32_t kvol, int64_t n_in, int32_t *back, void *stream);
/* Building the pair plan from a per-output neighbour table nbr i32[n, kvol] (-1 absent), kvol <= 64 -- the device
 * half of what nn/functional/conv.py:109-122 does with nonzero / sum on the host side.  G = ceil(n / 256) workgroups:
 *   link_pair_plan_count   wg_counts i32[G, kvol + 1]: per workgroup, pairs of every offset, and (last column) rows
 *                          whose centre entry nbr[i, kvol/2] != i (column sum 0 <=> submanifold table);
 *                          row_info i32[n] = (#valid entries of the row) | (centre entry valid) << 16.
 *   link_pair_plan_fill    after the host laid out base_k i32[kvol] (first contribution row of every offset's
 *                          128-row granules), wg_base i32[G, kvol] (exclusive scan of wg_counts over the workgroups)
 *                          and ext_start i32[n+1] (exclusive scan of the rows' list lengths): pair_in[p] = input row
 *                          of pair p, pair_out[p] = its output row (both pre-filled with -1), ext_list = every row's contribution rows in
 *                          ascending offset order.  No atomics: placement is deterministic.  skip_centre != 0 leaves
 *                          the centre offset out (link_conv_centre_sum computes it). */
int link_pair_plan_count(const int32_t *nbr, int64_t n, int32_t kvol, int32_t *wg_counts, int32_t *row_info, void *stream);
int link_pair_plan_fill(const int32_t *nbr, int64_t n, int32_t kvol, int32_t skip_centre, const int32_t *base_k,
                        const int32_t *wg_base, const int32_t *ext_start, int32_t *pair_in, int32_t *pair_out,
                        int32_t *ext_list, void *stream);
/* The step between the two, on the device (no host round trip; one workgroup): from link_pair_plan_count's per-workgroup
 * counts to base_k i32[kvol] (first contribution row of every offset, 128-row granules), wg_base i32[ceil(n/256), kvol]
 * (pairs of earlier workgroups per offset), gran_start i32[kvol + 1], wg_k i32[gran_cap] (offset of every granule, -1 behind
 * the last: the GEMM kernels return there, so they can be launched over the capacity) and hdr i32[8] = {pairs, rows_pad,
 * granules, rows whose centre neighbour is not the row itself, capacity exceeded, 0, 0, 0} for a later, asynchronous read.
 * skip_centre as in link_pair_plan_fill (the caller knows a submanifold table structurally).  A capacity of
 * ceil((n * kvol + 127 * kvol) / 128) granules is never exceeded.  The reference reads its counts back per layer
 * (nn/functional/conv.py:103-122, `nbsizes.cpu()`). */
int link_pair_plan_layout(const int32_t *wg_counts, int64_t n, int32_t kvol, int32_t skip_centre, int64_t gran_cap,
                          int32_t *base_k, int32_t *wg_base, int32_t *gran_start, int32_t *wg_k, int32_t *hdr, void *stream);
/* All three steps in one call, for capacity-sized lists (what link_amd's device-laid-out plans use): the fill pass computes
 * ext_start i32[n + 1] itself (wg_ext i32[ceil(n/256)] scratch: rows of earlier workgroups) and the layout pass writes -1
 * into the unused tail of every offset's last granule, so neither a prefix-sum pass nor a fill of pair_in / pair_out
 * (i32[gran_cap * 128] each, otherwise uninitialised) is needed.  ext_list i32[>= n * kvol].  gran_cap below
 * ceil((n * (kvol - skip_centre) + 127 * kvol) / 128) -- the capacity that can never be exceeded -- is LINK_ERR_ARG: the
 * lists would be written past it before the header's overflow flag exists. */
int link_pair_plan_build(const int32_t *nbr, int64_t n, int32_t kvol, int32_t skip_centre, int64_t gran_cap, int32_t *wg_counts,
                         int32_t *row_info, int32_t *base_k, int32_t *wg_base, int32_t *gran_start, int32_t *wg_ext,
                         int32_t *wg_k, int32_t *hdr, int32_t *ext_start, int32_t *pair_in, int32_t *pair_out,
                         int32_t *ext_list, void *stream);
/* The same three entries with fp16 / bf16 feature rows at the boundary (io_dtype = LINK_IO_F32 / F16 / BF16: feats, addend
 * and out rows in that type; weights, contribution rows, statistics and accumulation fp32) -- the reference's AMP
 * contract for its convolution (custom_fwd(cast_inputs=torch.half), nn/functional/conv.py:18). */
int link_conv_pairs_gemm_io(const void *feats, int32_t io_dtype, const int32_t *pair_in, const int32_t *wg_k, int64_t rows_pad,
                            const float *w, int32_t cin, int32_t cout, float *contrib, void *stream);
int link_conv_pairs_sum_io(const float *contrib, const int32_t *ext_start, const int32_t *ext_list, int64_t n,
                           int64_t n_direct, int32_t cout, const float *bias, const float *ln_w, const float *ln_b, float eps,
                           const void *addend, int32_t relu, void *out, int32_t io_dtype, void *stream);
int link_conv_centre_sum_io(const void *feats, const float *w, int32_t centre, const float *contrib, int64_t contrib_rows,
                            const int32_t *ext_start, const int32_t *ext_list, int64_t n, int32_t cin, int32_t cout,
                            const float *bias, const float *ln_w, const float *ln_b, float eps, const void *addend,
                            int32_t relu, void *out, int32_t io_dtype, void *stream);
/* fp32 rows on the f16 matrix cores: link_conv_pairs_gemm with both operands as fp16 hi + lo pairs (22 mantissa bits,
 * exact products, fp32 accumulation; three 4-pass matrix instructions per 16 input channels instead of four 8-pass).
 * ws = the weights split and transposed per offset, fp16 [kvol][cout][hi(cin) | lo(cin)]; w = the fp32 weights (used when a
 * value lies outside the fp16 range); w_big = device flag, non-zero when some |w| >= 2^15.  Inference form. */
int link_conv_pairs_gemm_split(const float *feats, const int32_t *pair_in, const int32_t *wg_k, int64_t rows_pad, const void *ws,
                               const float *w, const int32_t *w_big, int32_t cin, int32_t cout, float *contrib, void *stream);
/* AMP form of the two MFMA entries: the rows AND the weights are 16-bit (io_dtype = LINK_IO_F16 / LINK_IO_BF16 for both;
 * custom_fwd(cast_inputs=torch.half), nn/functional/conv.py:18, rounds the kernel together with the features), the
 * products run on the f16 / bf16 matrix cores with fp32 accumulation; contribution rows, statistics and epilogue
 * stay fp32.  wt = the weights rounded to the row type and transposed per offset: [kvol][cout][cin].
 * contrib_dtype = LINK_IO_F32, or io_dtype: the contribution rows are stored in the row type too (the reference's half
 * torch.mm output, convolution_cuda.cu:127-140) and summed in fp32 -- half the bytes of the dominant stream. */
int link_conv_pairs_gemm_amp(const void *feats, int32_t io_dtype, const int32_t *pair_in, const int32_t *wg_k, int64_t rows_pad,
                             const void *wt, int32_t cin, int32_t cout, void *contrib, int32_t contrib_dtype, void *stream);
int link_conv_centre_sum_amp(const void *feats, const void *wt, int32_t centre, const void *contrib, int32_t contrib_dtype,
                             int64_t contrib_rows, const int32_t *ext_start, const int32_t *ext_list, int64_t n, int32_t cin,
                             int32_t cout, const float *bias, const float *ln_w, const float *ln_b, float eps,
                             const void *addend, int32_t relu, void *out, int32_t io_dtype, void *stream);
/* Narrow layers in the AMP form without a pair list (conv.hip: every W_k resident in LDS; cin, cout in {16, 32}, kvol <= 27):
 * out = epilogue(sum_k feats[nbr[:, k]] . wt[k]^T) over the per-output neighbour table nbr i32[n, kvol] (as
 * link_subm_conv_forward), rows / addend / out in io_dtype (LINK_IO_F16 or LINK_IO_BF16), wt = [kvol][cout][cin] in the
 * row type (as link_conv_pairs_gemm_amp), fp32 accumulation over all offsets, statistics / affine in fp32.  ln_w NULL: the
 * plain convolution; relu bit 0 ReLU, bit 1 "ln_w / ln_b are a per-channel affine" (folded BatchNorm), as
 * link_subm_conv_ln_add_relu.  Replaces convolution_forward_cuda (pybind_cuda.cpp:19) under autocast for those widths. */
int link_subm_conv_resident_amp(const void *feats, int32_t io_dtype, const int32_t *nbr, const void *wt, const int32_t *order,
                                int64_t n, int32_t cin, int32_t cout, int32_t kvol, const float *ln_w, const float *ln_b,
                                float eps, const void *addend, int32_t relu, void *out, void *stream);
/* Weight gradient over the pair list (the weight half of convolution_backward_cuda, convolution_cuda.cu:167-278):
 * gw[k] = sum over the pairs p of offset k of feats[pair_in[p]]^T . gout[pair_out[p]]   (fp32 [kvol, cin, cout]).
 * One MFMA workgroup per 128-pair granule writes partial fp32[rows_pad/128, cin, cout]; the per-offset sums run in
 * granule order (gran_start i32[kvol+1] = first granule of every offset): deterministic, no atomics.  pair_out
 * i32[rows_pad] as written by link_pair_plan_fill (pre-filled with -1).  n_direct > 0 (a plan built with skip_centre
 * over n_direct voxels): the centre offset's identity pairs i -> i run as ceil(n_direct / 128) further granules, so
 * partial needs rows_pad/128 + ceil(n_direct/128) slots. */
int link_conv_pairs_wgrad(const float *feats, const float *gout, const int32_t *pair_in, const int32_t *pair_out,
                          const int32_t *wg_k, const int32_t *gran_start, int64_t rows_pad, int32_t kvol, int64_t n_direct,
                          int32_t cin, int32_t cout, float *partial, float *gw, void *stream);
int link_conv_centre_sum(const float *feats, const float *w, int32_t centre, const float *contrib,
                         int64_t contrib_rows, const int32_t *ext_start, const int32_t *ext_list, int64_t n, int32_t cin, int32_t cout,
                         const float *bias, const float *ln_w, const float *ln_b, float eps, const float *addend,
                         int32_t relu, float *out, void *stream);

/* =============================================================================================
 * E. Dense-cell form of R_core (the fast path when the block grid is mostly occupied)
 *
 * Same result as section C (linkunet.py:124-185 / ts_elk.py:144-230, R_core of SURVEY.md section 8d), but
 * built for frames whose dense block grid is about as large as the frame itself (V <~ 2 N: cfg1/cfg2
 * S-uniform).  There the reference's hash tables, torch.unique and scatter-add (utils.py:45-52,65-82) and
 * section B's count/scan/place index all disappear: the block table is indexed by GRID CELL, a voxel
 * finds its block by arithmetic, and the only index structure is a per-cell slot list filled by the pre_mix
 * kernel itself (one atomic per voxel).  Three or four launches per step, no scan, no sort, no host sync:
 *   link_dc_premix_insert  fin = LayerNorm(F Wpre^T) (f32 MFMA, software-pipelined) + rank = cnt[cell]++,
 *                          slots[cell][rank] = (x,y,z,id)
 *   link_dc_modsum         per cell: sort the slot list by voxel id (<= 4: network; more: selection), modulate,
 *                          sum -> S[cell] (every interior cell written, empty ones as zero rows); resets cnt
 *   link_dc_gather         r^3 box sum over the padded grid: LDS-DMA plane ring, xy sum from LDS, z ring in
 *                          registers -> A[cell]
 *   link_voxel_demod_ln    (section C kernel, fed with vrec/vcell) per voxel de-modulate + LayerNorm
 * The grid is padded by one empty cell on every spatial side (rows stay zero: the caller zero-fills S, Scnt
 * and A ONCE), so neighbour addressing needs no bounds checks.  Cell id =
 * ((b*pdim0 + x+1)*pdim1 + y+1)*pdim2 + z+1 with (x,y,z,b) the block coordinate minus grid.lo.
 * Slot capacity k = s^3 covers every frame with unique voxel coordinates; a voxel that finds its cell full
 * (duplicate coordinates) or lies outside the grid is dropped and flagged in hdr[LINK_HDR_STATUS]
 * (bit0 outside, bit1 slot overflow) -- callers that cannot rule that out use section C.
 * Supported: C in {16,32,64,128}, r in {2,3}; LINK_ERR_ARG otherwise.
 * ============================================================================================= */
typedef struct {
  int32_t s;        /* block edge in voxel-coordinate units */
  int32_t lo[4];    /* block-coordinate lower bound (x,y,z,b) */
  int32_t dim[4];   /* interior extent in blocks (x,y,z,b) */
  int32_t pdim[3];  /* padded spatial extent = dim + 2 */
  int32_t k;        /* slots per cell */
  int64_t vp;       /* padded cells = pdim0*pdim1*pdim2*dim3 */
} link_dc_grid_t;
/* Host helper: padded grid + slot capacity from a link_grid_t.  k <= 0 selects s^3.  Returns vp or -1
 * (vp*k must stay below 2^31 slots). */
int64_t link_dc_grid_from(const link_grid_t *grid, int32_t k, link_dc_grid_t *out);

#define LINK_HDR_STATUS_ACC 3   /* status bits being collected by the running step (dense-cell path) */

#define LINK_IO_F32 0
#define LINK_IO_F16 1
#define LINK_IO_BF16 2
/* Launch geometry and kernel selection of ONE plan (all zero = defaults).  Part of link_dc_buffers_t, read at every
 * call: nothing about the dense-cell path is process-global, two plans with different settings can run concurrently
 * from different threads / streams (re-entrant, no global state). */
typedef struct {
  int32_t k1_wgs;      /* workgroups (4 waves each) of the fused pre_mix kernel; 0 = 512.  One frame alone wants 2 per CU
                          (512); with several frames in flight 256 co-schedules better */
  int32_t k2_zsplit;   /* z-segments of the fused gather + de-modulate kernel; 0 = auto (enough for ~512 workgroups) */
  int32_t k1_lds_pad;  /* extra dynamic LDS bytes of the fused pre_mix kernel (<= 16384) / the gather kernel (<= 4096): */
  int32_t k2_lds_pad;  /* which workgroups share a CU when several frames are in flight */
  int32_t k1_form;     /* 0 = cell-range form (a wave owns a range of cells: LDS voxel list + X tile; the faster one with frames in
                          flight); 1 = tile form (id slots, in-wave id sort, per-cell sums by segmented DPP scan in the matrix-core
                          accumulator layout; 36 KB of LDS, any cell size up to the slot capacity in one pass structure); 2 = matrix-core
                          sums form (C = 32 / 64).
                          bit 4 (cell-range form): write the id-ordered records back to the slot lists in every cold call.  By default
                          link_elk_core_dense_forward leaves that store out when its own insert filled the lists (build_index 1) and
                          the quad-consumer gather kernel reads them (it takes a cell's records in any order; the pre_mix kernel orders
                          them for itself in every call, warm ones included); rows are the same bit for bit, the bit is what the form
                          without the store is tested and measured against.  link_dc_premix_modsum on its own always writes back */
  int32_t k2_form;     /* 0 = by measurement: producer / consumer form with quad consumers (two-part rows whose channels j and j + C/2
                          share theta), producer / consumer form with pair consumers (other two-part rows), own-cell form (cos_x, r = 3),
                          single-role form (cos_x, r = 2).  bit 3: pair consumers (the round-2 kernel) instead of quad consumers;
                          bit 0: single-role form (workgroup-wide dealing); bit 1: one voxel per lane group instead of a pair (pair
                          forms); bit 2: own-cell form (a lane group de-modulates its own cell from the A row in registers; 2-slot
                          plane ring fed by a dedicated DMA wave; 39 KB of LDS);
                          bit 4 (quad consumers, r = 3): square rim tiles.  By default an axis of the block grid that is 4 m + 1 cells
                          long has its last cell covered by 1 x 10 / 10 x 1 strips of columns instead of 4 x 4 tiles with one real
                          column in four (37 x 37 blocks: 89 tiles instead of 100); the rows are the same bit for bit, the bit is
                          what the strips are tested and measured against.  Measured on cfg2: the batch entry point gains 1.3 us / frame
                          from the strips, three plans on three streams lose 2.8 -- the Python layer sets the bit
                          on ElkCorePlan and clears it on ElkCoreBatch's arenas */
  int32_t mode;        /* 0 = default (7); else bit 0 fused pre_mix+modsum, bit 1 dense-cell demod kernel, bit 2 fused
                          gather + de-modulate (C = 64; the other widths keep box sum and de-modulation as two kernels: a fused form for them
                          measured slower and was removed in round 4) -- the unfused stages are what the fused ones are tested against */
  int32_t reserved0;   /* (was k1_pipe, the software-pipelined tile variant: removed in round 6 -- 35.7 against 34.2 us / frame) */
  int32_t reserved;
  uint64_t *k1_dbg;    /* bench only: device buffer u64[waves*8] for per-wave phase timings of the fused pre_mix kernel; NULL = off */
  uint64_t *k2_dbg;    /* bench only: device buffer u64[workgroups*8*8] for per-wave timings of the producer / consumer gather kernel */
} link_dc_tuning_t;

typedef struct {
  const void *feats;         /* [N,C] in io_dtype */
  const int32_t *coords;     /* i32[N,4] */
  const float *w_pre, *pre_ln_w, *pre_ln_b, *w_pos, *alpha, *ln_w, *ln_b;   /* as link_elk_buffers_t */
  uint32_t *cnt;             /* u32[vp]     voxels per cell; all-zero on entry and on exit (self-cleaning) */
  int32_t *slots;            /* i32[vp*k,4] (x,y,z,id) records; no initialisation needed */
  uint32_t *sid;             /* u32[vp*max(k,8)] voxel ids per cell in arrival order (tile form of the fused pre_mix kernel:
                                8 inline ids per cell = one 32-byte piece, then the overflow region); no initialisation */
  int32_t *vrec;             /* i32[N,4]    (x,y,z,id) per voxel, original order */
  int32_t *vcell;            /* i32[N]      padded cell id per voxel (0 for dropped voxels) */
  int32_t *cell_n;           /* i32[vp]     voxels per cell of the last indexed frame (zero-filled once) */
  int32_t *hdr;              /* i32[8]      LINK_HDR_*; zero-filled once */
  float *fin;                /* fp[N,C] */
  float *S;                  /* fp[(vp+1), P*C] block table, zero-filled once (border rows stay zero) */
  float *A;                  /* fp[(vp+1), P*C] normalised neighbour sums, zero-filled once */
  void *out;                 /* [N,C] in io_dtype */
  int32_t io_dtype;          /* LINK_IO_*: type of feats and out at the kernel boundary.  fp16 / bf16 are honoured
                                by the fused kernels (link_dc_premix_modsum, link_dc_gather_demod, link_dc_demod):
                                rows are converted on load / store, the contraction, theta, the block table and the
                                LayerNorm statistics stay fp32 -- the reference's AMP contract (custom_fwd(cast_inputs
                                = torch.half) on voxelize / devoxelize, nn/functional/voxelize.py:13, devoxelize.py:54,
                                fp32 accumulation) */
  link_dc_tuning_t tune;
} link_dc_buffers_t;

int link_dc_premix_insert(const float *feats, const int32_t *coords, const float *w_pre, const float *ln_w,
                          const float *ln_b, int64_t n, int32_t c, float eps, const link_dc_grid_t *g /* host */,
                          int32_t insert, float *fin, uint32_t *cnt, int32_t *slots, int32_t *vrec,
                          int32_t *vcell, int32_t *hdr, void *stream);
int link_dc_modsum(const float *fin, const int32_t *slots, uint32_t *cnt, int32_t *cell_n, const float *w_pos,
                   const float *alpha, const link_elk_desc_t *desc /* host */, const link_dc_grid_t *g /* host */,
                   int32_t warm, float *S, int32_t *hdr, void *stream);
int link_dc_gather(const float *S, const int32_t *cell_n, const link_elk_desc_t *desc /* host */,
                   const link_dc_grid_t *g /* host */, float *A, void *stream);
/* Fused forms (link_amd/csrc/dense_fused.hip) -- what link_elk_core_dense_forward runs by default:
 *   link_dc_index          the slot insert alone: coords -> cnt / slots / vcell (status bits as above)
 *   link_dc_premix_modsum  pre_mix + LayerNorm + theta + modulate + per-cell sum in ONE kernel: a wave owns a
 *                          range of cells, lays their voxels out id-ordered in LDS, and runs them through MFMA
 *                          tiles of 16 voxels, so `fin` never leaves registers (it is written, for the
 *                          de-modulation, only when op == LINK_OP_COSX); C in {16,32,64}, k <= 352
 *   link_dc_demod          per-voxel de-modulate + LayerNorm in original voxel order from A[vcell] */
int link_dc_index(const int32_t *coords, int64_t n, const link_dc_grid_t *g /* host */, uint32_t *cnt,
                  int32_t *slots, int32_t *vcell, int32_t *hdr, void *stream);
int link_dc_premix_modsum(const link_dc_buffers_t *buf /* host */, const link_dc_grid_t *g /* host */,
                          const link_elk_desc_t *desc /* host */, int64_t n, int32_t warm, void *stream);
int link_dc_demod(const float *A, const float *fin, const int32_t *coords, const int32_t *vcell,
                  const float *w_pos, const float *alpha, const float *ln_w, const float *ln_b,
                  const link_elk_desc_t *desc /* host */, const link_dc_grid_t *g /* host */, int64_t n, void *out,
                  int32_t io_dtype, void *stream);
/*   link_dc_gather_demod   box sum + de-modulate + LayerNorm in ONE kernel (C = 64 only: producer / consumer forms; LINK_ERR_ARG
 *                          at other widths, which run link_dc_gather + link_dc_demod): the normalised neighbour sums
 *                          of a z-plane live in LDS only and the plane's voxels are dealt out to the consumer waves -- a voxel
 *                          per quad of lanes through a map a mapper wave lays out two steps ahead (round 4), or as pairs to 16
 *                          lane groups (round-2 form); neither the A table nor its per-voxel gather exists */
int link_dc_gather_demod(const link_dc_buffers_t *buf /* host */, const link_dc_grid_t *g /* host */,
                         const link_elk_desc_t *desc /* host */, int64_t n, void *stream);
/* One call = one R_core step on the dense-cell path (build_index = 0 reuses slots/cell_n of the previous
 * call on the same coordinates: the "warm" figure; 1 inserts the frame first; 2 = link_dc_index_probe inserted it). */
int link_elk_core_dense_forward(const link_dc_buffers_t *buf /* host */, const link_dc_grid_t *g /* host */,
                                const link_elk_desc_t *desc /* host */, int64_t n, int32_t build_index,
                                void *stream);
/* The slot insert of a step (the form buf->tune picks) that also reports the frame's occupancy on this grid: stats
 * i32[16][16] (device, zeroed by the caller): 16 partial slots on separate cache lines, [k][0] += voxels inside the grid,
 * [k][1] += occupied cells, [k][2] max= fullest cell's count -- the reader sums / sums / maxes over k.  For the
 * first visit of a coordinate set: a caller that accepts the layout continues with build_index = 2, one that does not
 * zero-fills cnt and hdr (nothing else of the frame stays behind). */
int link_dc_index_probe(const link_dc_buffers_t *buf /* host */, const link_dc_grid_t *g /* host */, int64_t n, int32_t *stats,
                        void *stream);
/* The slot insert of the tile form: coords -> cnt / sid / vcell (ids only; the fused pre_mix kernel of the tile form
 * writes the id-ordered (x,y,z,id) records the gather kernel reads into `slots`).  Status bits as link_dc_index. */
int link_dc_index_ids(const int32_t *coords, int64_t n, const link_dc_grid_t *g /* host */, uint32_t *cnt,
                      uint32_t *sid, int32_t *vcell, int32_t *hdr, void *stream);

/* =============================================================================================
 * F. Training-mode BatchNorm statistics over feature rows (row N2; torchsparse/nn/modules/norm.py:10-13 applies
 * nn.BatchNorm1d to the [N, C] feature matrix after every convolution, linkunet.py:18-92).  Two column reductions at
 * memory speed with deterministic (fixed-order) double accumulation; the normalisation itself and the input gradient
 * are one fused multiply-add per element and stay with the caller.  C % 4 == 0, 4 <= C <= 1024.
 *   partial   f64[link_bn_partial_workgroups(n, c) * 2 * c] scratch
 *   forward   mean[c], invstd[c] = 1/sqrt(biased var + eps); running_mean / running_var (may be NULL) updated as
 *             nn.BatchNorm1d does: (1 - momentum) * old + momentum * (mean | unbiased var)
 *             scale = weight * invstd, shift = bias  (y = (x - mean) * scale + shift)
 *   backward  sum_g[c] = sum_i g[i], sum_gx[c] = sum_i g[i] * (x[i] - mean) * invstd  (= grad bias, grad weight);
 *             coef = a | bq | cq with grad_x = a * g + bq * (x - mean) + cq per channel
 * ============================================================================================= */
int32_t link_bn_partial_workgroups(int64_t n, int32_t c);
int link_bn_forward_stats(const float *x, int64_t n, int32_t c, float eps, float momentum, double *partial, float *mean,
                          float *invstd, float *running_mean, float *running_var, const float *weight /* NULL: 1 */,
                          const float *bias /* NULL: 0 */, float *scale /* [c] or NULL */, float *shift, void *stream);
int link_bn_backward_reduce(const float *g, const float *x, const float *mean, const float *invstd, int64_t n, int32_t c,
                            double *partial, float *sum_g, float *sum_gx, const float *weight /* NULL: 1 */,
                            float *coef /* [3c] or NULL */, void *stream);
/* Round 5: the normalisation and the input gradient as ONE pass each, with the ReLU that follows the BatchNorm in the
 * reference's blocks (linkunet.py:23-38: Conv3d -> BatchNorm -> ReLU(True)) folded in -- a training step of the cfg3
 * encoder spent a quarter of its 9 ms in torch's elementwise kernels (x - mean, addcmul, clamp, threshold_backward, ...).
 *   link_bn_apply_forward          y = (x - mean) * scale + shift, relu != 0: y = max(y, 0)
 *   link_bn_backward_reduce_relu   link_bn_backward_reduce on g' = g masked by y > 0 (y recomputed from x, scale, shift)
 *   link_bn_apply_backward         gx = a * g' + bq * (x - mean) + cq; scale / shift NULL: g' = g (no relu in the forward) */
int link_bn_apply_forward(const float *x, const float *mean, const float *scale, const float *shift, int64_t n, int32_t c,
                          int32_t relu, float *y, void *stream);
int link_bn_backward_reduce_relu(const float *g, const float *x, const float *mean, const float *invstd, const float *scale,
                                 const float *shift, int64_t n, int32_t c, double *partial, float *sum_g, float *sum_gx,
                                 const float *weight /* NULL: 1 */, float *coef /* [3c] */, void *stream);
int link_bn_apply_backward(const float *g, const float *x, const float *mean, const float *coef, const float *scale /* NULL: no relu */,
                           const float *shift, int64_t n, int32_t c, float *gx, void *stream);
/* Autocast training (ABI 13): the five entries with the [N, C] rows -- x, g, y, gx -- in io_dtype (LINK_IO_F32 / LINK_IO_F16 /
 * LINK_IO_BF16, anything else LINK_ERR_ARG), widened on load and rounded to nearest even on store.  Statistics, partials,
 * coefficients, scale / shift and the running statistics stay fp32 (f64 partials): the fp32 entries' values on the widened
 * rows.  A BatchNorm after a convolution sees that convolution's half rows under torch.autocast and returns its own in the
 * same type, as torch's batch_norm does for half input with fp32 weight. */
int link_bn_forward_stats_io(const void *x, int32_t io_dtype, int64_t n, int32_t c, float eps, float momentum, double *partial,
                             float *mean, float *invstd, float *running_mean, float *running_var, const float *weight,
                             const float *bias, float *scale, float *shift, void *stream);
int link_bn_apply_forward_io(const void *x, int32_t io_dtype, const float *mean, const float *scale, const float *shift, int64_t n,
                             int32_t c, int32_t relu, void *y, void *stream);
int link_bn_backward_reduce_io(const void *g, const void *x, int32_t io_dtype, const float *mean, const float *invstd, int64_t n,
                               int32_t c, double *partial, float *sum_g, float *sum_gx, const float *weight, float *coef,
                               void *stream);
int link_bn_backward_reduce_relu_io(const void *g, const void *x, int32_t io_dtype, const float *mean, const float *invstd,
                                    const float *scale, const float *shift, int64_t n, int32_t c, double *partial, float *sum_g,
                                    float *sum_gx, const float *weight, float *coef, void *stream);
int link_bn_apply_backward_io(const void *g, const void *x, int32_t io_dtype, const float *mean, const float *coef,
                              const float *scale /* NULL: no relu */, const float *shift, int64_t n, int32_t c, void *gx,
                              void *stream);

/* =============================================================================================
 * G. One host call per LinK block on a NEW coordinate set (round 5)
 *
 * ELKBlock.forward / TSELKBlock.forward_ of the reference is one Python call that rebuilds every map of its coordinate set
 * (linkunet.py:124-185: voxel_to_aux's hash / unique / query chain, utils.py:44-52; the 3x3x3 convolution's kernel map with
 * `nbsizes.cpu()`, nn/functional/conv.py:103-122).  link_elk_block_forward is that call for the inference forward on the
 * dense-cell layout: bounding box + slot insert with occupancy counters -> ONE host round trip -> R_core (section E) on the
 * caller's stream, behind the 27-neighbour table read off the frame's slot lists (link_dc_neighbor_map), while the context's side
 * stream lays the pair plan out on the device and runs the pair GEMM (section D) -> the convolution's finish: centre offset + pair sums + LayerNorm + add(R_core) + ReLU.
 * The frame is TRIED on the plan the caller hands over (the module's last plan: frames of a stream share their grid): when a voxel
 * lies outside that grid or the occupancy is not what the dense-cell kernels are built for (more than mean_max voxels per occupied
 * cell on average / cell_max in the fullest), the call returns
 * LINK_BLOCK_MISS with bbox / stats filled in and nothing of the frame left in the plan (counters and status word zeroed) --
 * the caller continues on its per-stage entry points without measuring the bounds again.
 * fp32 rows, C = cin = cout with link_conv_pairs_supported(C, C), a submanifold table (subm != 0: unique coordinates, so the centre
 * column is the identity -- verified on the device, pair header word 3).  LINK_ERR_WORKSPACE when pair_arena / contrib are smaller
 * than link_pair_plan_arena says.  The context owns a non-blocking side stream, two events and 2 x 1 KB of scratch (device +
 * pinned host); create one per device and host thread.
 * ============================================================================================= */
typedef struct link_block_ctx link_block_ctx_t;
int link_block_ctx_create(link_block_ctx_t **out);     /* on the current device */
int link_block_ctx_destroy(link_block_ctx_t *ctx);
/* Word offsets (16-byte aligned pieces) of the arena link_pair_plan_build works in with capacity-sized lists:
 * offs[0..9] = wg_counts | row_info | base_k + wg_base + gran_start | wg_ext | wg_k | hdr | ext_start | pair_in | pair_out |
 * ext_list, offs[10] = total words.  Returns the granule capacity (contribution rows = 128 x that) or -1. */
int64_t link_pair_plan_arena(int64_t n, int32_t kvol, int32_t skip_centre, int64_t offs[11]);

/* The 3x3x3 neighbour table of a frame from its freshly inserted slot lists (between link_dc_index / link_dc_index_probe and the
 * pre_mix kernel, which re-orders the lists and resets the counters): nbr i32[n, 27], entry [i][k] = row of the voxel at
 * coords[i] + offset_k * step in get_kernel_offsets(3) order, -1 absent -- the table of link_cell_table_build + link_neighbor_map
 * (conv.py:103-113) without the voxel-resolution cell table.  Voxels the insert dropped (outside the grid) are absent. */
int link_dc_neighbor_map(const int32_t *coords, int64_t n, const link_dc_grid_t *g /* host */, const uint32_t *cnt,
                         const int32_t *slots, int32_t step, int32_t *nbr, void *stream);

#define LINK_BLOCK_DONE 0
#define LINK_BLOCK_MISS 1
typedef struct {
  const link_dc_buffers_t *buf;   /* the plan the frame is tried on; feats / coords = the frame, out = R_core's rows [n, C]
                                     (the convolution's addend), parameters bound */
  const link_dc_grid_t *g;
  const link_elk_desc_t *desc;
  int64_t n;
  int32_t mean_max, cell_max;     /* occupancy the dense-cell kernels take: voxels per occupied cell, mean and maximum */
  int32_t ts;                     /* tensor stride: neighbour of voxel i at coords_i + offset * ts (conv.py:105-113) */
  int32_t subm;                   /* the coordinates are unique (must be non-zero) */
  int32_t *nbr;                   /* out: i32[n, 27] neighbour table (kept by the caller for later layers on these coordinates) */
  int32_t *pair_arena;            /* out: the pair plan (link_pair_plan_arena layout) */
  int64_t pair_arena_words;
  float *contrib;                 /* scratch: contribution rows f32[contrib_rows, C] */
  int64_t contrib_rows;
  const float *w;                 /* local_mix kernel f32[27, C, C] */
  const void *ws;                 /* its fp16 hi | lo split (link_conv_pairs_gemm_split), or NULL: link_conv_pairs_gemm_io */
  const int32_t *w_big;
  const float *nl_w, *nl_b;       /* norm_local */
  float nl_eps;
  int32_t flags;                  /* bit 0: ReLU */
  void *out;                      /* [n, C]: relu(R_core + LayerNorm(conv(feats))) */
  int32_t bbox[8];                /* results (host): min x,y,z,b, max x,y,z,b */
  int32_t stats[4];               /* voxels inside the plan's grid, occupied cells, fullest cell, miss reasons (1 outside, 2 occupancy) */
  int32_t verdict;                /* LINK_BLOCK_DONE / LINK_BLOCK_MISS */
  int32_t reserved;
} link_block_args_t;
int link_elk_block_forward(link_block_ctx_t *ctx, link_block_args_t *args /* host, in/out */, void *stream);

/* =============================================================================================
 * H. R_core of a BATCH of independent frames in one call (round 6; csrc/dense_batch.hip)
 *
 * The reference batches frames by the batch column of its coordinates (the batch index is part of every block key,
 * segmentation/core/models/utils.py:45; linkunet.py:132,151-162,178 run one ELKBlock over the whole collated batch) and shards
 * independent frames over GPUs (BASELINE.json configs[3]: "a batch of 8 independent frames").  link_elk_core_dense_forward_batch
 * is the dense-cell R_core (section E) of `nframes` frames -- each with its own link_dc_buffers_t, all on one grid, one block's
 * parameters, one descriptor -- as THREE launches, two of them persistent: the slot insert of every frame (one ordinary grid), a
 * K1-role kernel (one workgroup per CU; parameters staged once; every wave walks the frames: its range of cells of frame f as soon
 * as the insert of f has arrived) and a K2-role kernel (one workgroup per CU pulling (frame, tile) items off per-XCD cursors: a tile
 * of frame f as soon as K1 of f has arrived).  The stages of different frames overlap by construction -- per-frame arrival counters
 * with write-through stores / one agent-scope acquire per item replace the stream-ordered launch boundaries of the per-frame calls.
 * Results: those of link_elk_core_dense_forward(build_index = 1) per frame, bit for bit.
 *
 * Contract: C = 64, cg = 32 (two-part rows whose channels j and j + 32 share theta), op cos / sin, r in {2, 3}, coord_div = 1, no
 * alpha, fp32 / fp16 / bf16 rows (io_dtype: one type for all frames of a call), slot capacity <= 352, every frame its own cnt / slots / vcell / cell_n / S / hdr / out,
 * and per frame 1 <= n[i] < 2^24 voxels (n[i] * 64 * 4 bytes of rows < 2^32; every voxel of a frame is inserted, however many
 * chunks of 256 voxels it has) -- LINK_ERR_ARG otherwise
 * (nothing launched; the caller runs the frames through section E one by one).  frames[i].tune is not read (the geometry is the
 * roles': workgroups = CUs, whole columns per gather tile).  The call returns when everything is ENQUEUED; the results are complete in `stream`
 * order.  Calls whose frames share no buffers overlap on the device (K1 of the next batch starts under K2 of the previous one):
 * a caller that keeps two batches in flight alternates two sets of frame buffers and submits call s + 1 before it joins call s
 * (link_dc_batch_submit / link_dc_batch_join below).  Up to 48 frames form one launch set; a longer call runs as consecutive sets.  The
 * context owns up to five non-blocking streams (drawn at creation so that the roles sit on hardware queues of their own), 21 events
 * and 29 KB of counters; create one per device (and per host thread).
 * link_dc_batch_status synchronises the context's streams and returns LINK_BATCH_TIMEOUT if a bounded wait inside a kernel gave
 * up (the frames' rows are then undefined), LINK_OK otherwise; out[0] = the first error word, out[1] = launch sets so far.
 * ============================================================================================= */
typedef struct link_dc_batch link_dc_batch_t;
int link_dc_batch_create(link_dc_batch_t **out);       /* on the current device */
int link_dc_batch_destroy(link_dc_batch_t *ctx);
int link_elk_core_dense_forward_batch(link_dc_batch_t *ctx, const link_dc_buffers_t *frames /* host [nframes] */,
                                      const int64_t *n /* host [nframes] */, int32_t nframes, const link_dc_grid_t *g /* host */,
                                      const link_elk_desc_t *desc /* host */, void *stream);
/* The same call in two halves, for a caller that keeps several calls in flight from ONE stream: link_dc_batch_submit enqueues the call
 * behind what `stream` holds so far and hands out a ticket; link_dc_batch_join makes `stream` wait for that call's rows.  Submitting
 * call s + 1 BEFORE joining call s lets the pre_mix role of s + 1 start under the gather role of s without a second caller stream --
 * two caller streams that the runtime happens to multiplex onto one hardware queue serialise the calls (the wait of one stream's
 * join sits in front of the other stream's submit: 50 against 37 us / frame).
 * link_elk_core_dense_forward_batch == submit + join. */
int link_dc_batch_submit(link_dc_batch_t *ctx, const link_dc_buffers_t *frames /* host [nframes] */, const int64_t *n /* host [nframes] */,
                         int32_t nframes, const link_dc_grid_t *g /* host */, const link_elk_desc_t *desc /* host */, void *stream,
                         int64_t *ticket /* host, out */);
int link_dc_batch_join(link_dc_batch_t *ctx, int64_t ticket, void *stream);
int link_dc_batch_status(link_dc_batch_t *ctx, int32_t *out /* host [2] */);
/* Measurement hook: with timing on, the three launches of every launch set are bracketed by timed events on their own streams;
 * link_dc_batch_kernel_times waits for the set `ticket` names (one of the last four) and returns the brackets of its insert, pre_mix and
 * gather kernels in ms. */
int link_dc_batch_set_timing(link_dc_batch_t *ctx, int32_t on);
int link_dc_batch_kernel_times(link_dc_batch_t *ctx, int64_t ticket, float *ms /* host [3] */);
/* Profiling hook (tools/batch_timeline.py): device buffers of 8 x u64 rows the K1 / K2 items append 100 MHz timestamps to (word 0 =
 * rows so far, zeroed by the caller; word 1 = capacity in rows).  Honoured by a -DDC_BT_PROF=1 build of csrc/dense_batch.hip (returns
 * LINK_OK), ignored by the default build (returns 1). */
int link_dc_batch_set_debug(link_dc_batch_t *ctx, uint64_t *k1_rows, uint64_t *k2_rows);
/* Do two streams of the caller sit on ONE hardware queue?  *delay_us = how long a kernel on `b` is held up by a 150 us kernel + event
 * record on `a`: ~5 = queues of their own, >= 150 = one queue (frames kept in flight on two such streams run one after the other).
 * Synchronises both streams. */
int link_streams_share_queue(void *stream_a, void *stream_b, double *delay_us /* host, out */);
/* Diagnostic: does a pair of streams sit on ONE hardware queue (GPU_MAX_HW_QUEUES; an event record on one stream then holds up the
 * other's kernels)?  A 150 us spin kernel + an event record on the first stream, a stamp kernel on the second; delays_us[12] = the
 * second's start behind the first's for (pre_mix -> gather), (pre_mix -> insert), (gather -> insert), (stream -> pre_mix),
 * (stream -> gather), (stream -> insert) and the six reverse pairs: ~5 = separate queues, >= 150 = one queue.  Synchronises the
 * streams involved.  (link_dc_batch_create runs the same test to put its role streams on queues of their own.) */
int link_dc_batch_probe_streams(link_dc_batch_t *ctx, hipStream_t stream, double *delays_us /* host [12] */);

/* =============================================================================================
 * I. Detection post-processing (csrc/boxnms.hip): rotated BEV overlap / IoU, NMS, CenterHead decode
 *
 * What the reference's CUDA-only extension iou3d_nms_cuda (detection/det3d/ops/iou3d_nms/src/iou3d_nms_kernel.cu) and the decode of
 * CenterHead.predict (detection/det3d/models/bbox_heads/center_head.py:344-421,461-467) compute.  Boxes are float[n, 7] =
 * x, y, z, dx, dy, dz, heading.  All fp32, no atomics, bitwise reproducible.  Additive entries: the ABI version does not move.
 *
 * NMS is two kernels: the suppression mask uint64[cap, ceil(cap / 64)] (bit c of word [i, cb] = box i suppresses box 64 cb + c;
 * only the words with cb >= i / 64 are computed, and every one of those is written) and the reference's greedy scan
 * (iou3d_nms.cpp:116-132) over it, on the device in one workgroup: keep int64[cap] = the kept indices in ascending order, then -1;
 * count int32[1].  Boxes are taken in the order given (the caller sorts by score).  `n_dev`, when not NULL, is a device int32 with
 * the number of boxes that count, clamped to [0, cap]: the row stride of the mask and the sizes of all buffers follow `cap`, so a
 * caller with a fixed capacity never reads a size back.  post_max > 0 stops the scan after that many kept boxes.
 * Predicates: LINK_NMS_ROTATE rotated IoU > thr; LINK_NMS_NORMAL IoU of the axis-aligned x, y, dx, dy rectangles > thr;
 * LINK_NMS_CIRCLE squared distance of the centres <= thr (circle_nms_jit.py:23-27).
 * n == 0 / cap == 0: LINK_OK, count 0 when a count pointer is given.  Null buffers with n > 0, thr not finite, an unknown predicate,
 * more than 65535 * 16 boxes: LINK_ERR_ARG before anything touches a device.  link_nms_bev: LINK_ERR_WORKSPACE when the mask
 * workspace is smaller than the bytes its size helper names.
 * ============================================================================================= */
#define LINK_NMS_ROTATE 0
#define LINK_NMS_NORMAL 1
#define LINK_NMS_CIRCLE 2
int link_boxes_overlap_bev(const float *boxes_a, int64_t na, const float *boxes_b, int64_t nb, float *out /* [na, nb] */, void *stream);
int link_boxes_iou_bev(const float *boxes_a, int64_t na, const float *boxes_b, int64_t nb, float *out /* [na, nb] */, void *stream);
size_t link_nms_workspace_bytes(int64_t n);            /* 8 * n * ceil(n / 64); host only */
int link_nms_mask(const float *boxes, int64_t cap, const int32_t *n_dev, int32_t pred, float thr, uint64_t *mask, void *stream);
int link_nms_reduce(const uint64_t *mask, int64_t cap, const int32_t *n_dev, int32_t post_max, int64_t *keep /* [cap] */,
                    int32_t *count /* [1] */, void *stream);
int link_nms_bev(const float *boxes, int64_t cap, const int32_t *n_dev, int32_t pred, float thr, int32_t post_max, void *workspace,
                 size_t workspace_bytes, int64_t *keep /* [cap] */, int32_t *count /* [1] */, void *stream);
/* CenterHead decode of one task's NCHW maps, read in place: hm[B, K, H, W], reg[B, 2, H, W], height[B, 1, H, W], dim[B, 3, H, W],
 * rot[B, 2, H, W] (sin, cos), vel[B, 2, H, W] or NULL.  Writes boxes float[B, H W, 7 or 9 with vel] = x, y, z, exp dims, (vel), heading;
 * labels int32[B, H W] = the arg max class; scores float[B, H W] = the max sigmoid, -inf where the score is not above the threshold or
 * the centre lies outside post_center_range (lo x, y, z, hi x, y, z); counts int32[B] = cells per frame that are not masked. */
typedef struct {
  float out_size_factor, voxel_size[2], pc_range[2], score_threshold, post_center_range[6];
} link_center_geom_t;
int link_center_decode(const float *hm, const float *reg, const float *height, const float *dim, const float *rot, const float *vel,
                       int32_t batch, int32_t num_cls, int32_t h, int32_t w, const link_center_geom_t *geom /* host */, float *boxes,
                       int32_t *labels, float *scores, int32_t *counts, void *stream);

/* =============================================================================================
 * J. Point clouds to voxels (csrc/voxelize.hip): the hard voxeliser with its mean reader, the dynamic voxeliser
 *
 * What the reference does on the host per frame, detection/det3d/ops/point_cloud/point_cloud_ops.py:8-55,112-184 (the numba loop
 * points_to_voxel, called through core/input/voxel_generator.py:5-30 by datasets/pipelines/preprocess.py:171-217) followed by
 * models/readers/voxel_encoder.py:17-24 (VoxelFeatureExtractorV3: mean of the kept rows), and what models/readers/
 * dynamic_voxel_encoder.py:8-17,70-102 (virtual=False) does with torch.unique(dim=0) and a scatter mean.  Additive entries: the ABI
 * version does not move.  Integer atomics only; every float sum runs in ascending point index, so two calls are bit for bit equal.
 *
 * points float[n, ndim] (x, y, z first) holds the clouds of `batch` samples one after the other; point_offsets int32[batch + 1]
 * (device) names their rows, point_offsets[batch] (clamped to n_points_capacity, which sizes the launches and the workspace) is the
 * number of points.  Every sample is voxelised on its own and the voxels are concatenated in sample order: voxel_offsets
 * int32[batch + 1] (device, written) names the rows of each sample, clamped to voxel_capacity (voxels beyond it are not written).
 * Outputs, rows past voxel_offsets[batch] zeroed: mean float[voxel_capacity, ndim]; coors int32[voxel_capacity, 4] = b, z, y, x
 * (16-byte aligned); num_points int32[voxel_capacity]; voxels float[voxel_capacity, max_points, ndim] or NULL (hard mode only; a
 * caller that wants the mean alone never materialises it).  No host synchronisation inside.
 *
 * LINK_VOXELIZE_HARD: c = floor((p - lo) / vs) per axis in float32 (an IEEE subtract and a correctly rounded divide), the point is
 *   dropped unless 0 <= c < grid; voxels are numbered by the first point that falls into them, keep their first max_points points in
 *   input order, and only the first max_voxels voxels of a sample exist (points of later cells are dropped); num_points =
 *   min(count, max_points); mean = the sum of the kept rows / num_points.  `hi` is not read.
 * LINK_VOXELIZE_DYNAMIC: the point is kept when lo <= p <= hi per axis (inclusive above, so a coordinate may equal grid),
 *   c = trunc((p - lo) / vs); voxels in ascending (z, y, x) order; mean over ALL points of the voxel; max_points / max_voxels are
 *   not read and `voxels` must be NULL.
 * A coordinate that is not finite is out of range in both modes (the reference's behaviour on it is undefined).
 * grid = round((hi - lo) / vs) in float32, half to even, computed by the caller.
 *
 * The workspace holds one bit per cell and sample plus forty bytes per point of capacity.  It must be ZERO before the first call
 * and whenever geometry or batch change; every call leaves it as the next call needs it (n_points_capacity may differ from call to
 * call while the workspace is large enough).
 * One workspace serves one stream at a time.
 * Errors, before anything is launched: LINK_ERR_ARG for ndim outside 3..16, a voxel size or grid that is not positive, an unknown
 * mode, max_points / max_voxels < 1 in hard mode, batch outside 1..1024, a null pointer, and a grid that is too large (more than
 * 2^28 cells per sample, 2^31 over all samples, or an axis of 2^24); LINK_ERR_WORKSPACE for a workspace smaller than the bytes the
 * size helper names (which returns 0 where the call itself would return LINK_ERR_ARG).
 * ============================================================================================= */
#define LINK_VOXELIZE_HARD 0
#define LINK_VOXELIZE_DYNAMIC 1
typedef struct {
  float lo[3], hi[3], vs[3];          /* x, y, z */
  int32_t grid[3];                    /* x, y, z */
  int32_t max_points, max_voxels, ndim, mode;
} link_voxelize_geom_t;               /* link_abi_struct_size(8) */
size_t link_voxelize_workspace_bytes(const link_voxelize_geom_t *geom /* host */, int64_t n_points_capacity, int32_t batch); /* host only */
int link_voxelize(const link_voxelize_geom_t *geom /* host */, const float *points, const int32_t *point_offsets /* [batch + 1], device */,
                  int32_t batch, int64_t n_points_capacity, void *workspace, size_t workspace_bytes, float *voxels /* nullable */,
                  float *mean, int32_t *coors /* [voxel_capacity, 4] = b, z, y, x */, int32_t *num_points, int64_t voxel_capacity,
                  int32_t *voxel_offsets /* [batch + 1], device */, void *stream);

/* =============================================================================================
 * K. Segmentation criterion (csrc/segloss.hip): cross-entropy + Lovasz-softmax, forward and gradient, in one call
 *
 * What the reference's trainer computes per step, segmentation/core/trainers.py:64-73 with the pair core/builder.py:61-72 builds:
 * nn.CrossEntropyLoss(ignore_index=255)(outputs, targets) + lovasz_softmax(softmax(outputs), targets, ignore=0), the latter being
 * core/lovasz_losses.py:156-225 (flatten_probas: a nonzero(); lovasz_softmax_flat: a Python loop over the classes with a host
 * test `fg.sum() == 0`, a full sort, a gather, lovasz_grad:21-33 = two cumsums and a shifted difference, a dot).  Additive entries:
 * the ABI version does not move.  No host synchronisation, no allocation, integer atomics only; every float sum has a fixed
 * order, so two calls on the same inputs are bit for bit equal.  The launches are sized by (n, c) alone and read the counts they
 * need from the workspace, so a call can be captured in a graph.
 *
 * rows [n, c] in io_dtype (LINK_IO_F32 / F16 / BF16), widened to fp32 on load; labels int64 [n]; LINK_SEGLOSS_MIN_CLASSES <= c <=
 * LINK_SEGLOSS_MAX_CLASSES and n * c < 2^31 - 2048.
 * input_kind LINK_SEGLOSS_LOGITS: p = softmax(rows) in fp32; CE = the mean over rows with label != ce_ignore (and inside [0, c):
 *   a label outside the range never indexes anything) of -log p[label]  (F.cross_entropy(rows.float(), labels, ignore_index),
 *   0 / 0 = NaN when no row counts, as torch returns it).
 * input_kind LINK_SEGLOSS_PROBAS: p = rows (lovasz_losses.py:156-202 itself: probabilities in [0, 1]); CE = 0 and unit_grad is d/dp.
 * Lovasz: rows with label != lov_ignore are valid (all rows when use_lov_ignore == 0); a valid row whose label lies outside
 *   [0, c) is background for every class (lovasz_losses.py:188 does the same).  For every class taken -- n_c > 0 valid rows of that
 *   label with LINK_SEGLOSS_PRESENT, every class with LINK_SEGLOSS_ALL -- the errors e = |[y = c] - p_c| are sorted descending,
 *   stable in row order, and loss_c = sum_k e_(k) g_k with lovasz_grad:21-33 in closed form, F_k / B_k the inclusive foreground /
 *   background counts and U_k = n_c + B_k:  g_k = 1 / U_k (foreground), (n_c - F_k) / (U_{k-1} U_k) (background; 1 where U_{k-1} = 0).
 *   lovasz = the mean of loss_c over the classes taken, 0 when none is or no row is valid.  g_k is a constant of the gradient, as
 *   in the reference (lovasz_losses.py:201 wraps it in Variable()); d/dp = -+g / n_taken, 0 where e == 0.
 * out float[3] (device) = total, CE, lovasz.  A non-finite p makes lovasz (and the total) NaN.
 * unit_grad float[c, n] (device, CLASS-MAJOR, the caller's; written in full): d total / d rows for an upstream gradient of 1
 *   (d lovasz / d p with LINK_SEGLOSS_PROBAS).  link_segloss_backward writes grad_rows[n, c] = unit_grad * upstream[0] in io_dtype,
 *   rounded once; upstream is a DEVICE scalar (a GradScaler's scale lives there).
 * The workspace holds 20 bytes per (row, class) plus the sort's tile histograms; it needs no initialisation and serves one
 * stream at a time.  Errors, before anything is launched: LINK_ERR_ARG for a null pointer, n < 0, c or n * c outside the range, an
 * unknown io_dtype / input_kind / classes; LINK_ERR_WORKSPACE for fewer bytes than link_segloss_workspace_bytes names (host only,
 * needs no device; 0 where the call would return LINK_ERR_ARG).
 * ============================================================================================= */
#define LINK_SEGLOSS_LOGITS 0
#define LINK_SEGLOSS_PROBAS 1
#define LINK_SEGLOSS_PRESENT 0
#define LINK_SEGLOSS_ALL 1
#define LINK_SEGLOSS_MIN_CLASSES 2
#define LINK_SEGLOSS_MAX_CLASSES 32
size_t link_segloss_workspace_bytes(int64_t n, int32_t c); /* host only */
int link_segloss_forward(const void *rows, int32_t io_dtype, int32_t input_kind, const int64_t *labels, int64_t n, int32_t c,
                         int64_t ce_ignore, int64_t lov_ignore, int32_t use_lov_ignore, int32_t classes, void *workspace,
                         size_t workspace_bytes, float *out /* [3] */, float *unit_grad /* [c, n] */, void *stream);
int link_segloss_backward(const float *unit_grad /* [c, n] */, const float *upstream /* device scalar */, int64_t n, int32_t c,
                          int32_t io_dtype, void *grad_rows /* [n, c] */, void *stream);

/* =============================================================================================
 * L. CenterHead training (csrc/centerloss.hip): target assignment, focal loss and L1 regression loss, forward and gradient
 *
 * What the reference does on the host per sample, detection/det3d/datasets/pipelines/preprocess.py:283-467 (AssignLabel: a numpy loop
 * over objects with gaussian_radius and draw_umich_gaussian of det3d/core/utils/center_utils.py:17-63), and what
 * det3d/models/losses/centernet_loss.py (FastFocalLoss, RegLoss: a permuted copy of every map, a gather, `if num_pos == 0` on the
 * host) and det3d/models/bbox_heads/center_head.py:248-293 (CenterHead.loss: in-place sigmoid and clamp, a torch.cat of five maps,
 * .cpu() on two results per task) compute per step.  Additive entries: the ABI version does not move.  fp32 arithmetic unless
 * stated, integer atomics only, every float sum in a fixed order (two calls are bit for bit equal), no host synchronisation, no
 * allocation, launch geometry a function of the shapes alone: every call can be captured in a graph.
 *
 * link_center_assign: the targets of all tasks of a batch in one call (two launches).
 *   gt_boxes float[batch, n_cap, 9] = x, y, z, w, l, h, vx, vy, rot (the nuScenes order AssignLabel reads); gt_classes
 *   int32[batch, n_cap] = the global 1-based class, 0 (or anything outside 1..sum of num_classes) for an empty slot.  Task t owns the
 *   global classes after those of the tasks before it, num_classes[t] of them.  Per task t, written in full, zeros included:
 *   hm float[batch, num_classes[t], h, w]; anno_box float[batch, max_objs, 10]; ind int64[batch, max_objs]; mask uint8[batch, max_objs];
 *   cat int64[batch, max_objs].
 *   Slot order: a task's objects class by class, in input order inside a class (the task_masks / np.concatenate of lines 320-348);
 *   only the first max_objs count; object k of that order owns slot k whether or not it is drawn (new_idx = k).
 *   Sizes and centre: w' = w / vs[0] / osf, l' = l / vs[1] / osf, ct = ((x - lo) / vs) / osf, every operation an IEEE fp32 one rounded on
 *   its own.  Cell ct_int = truncation toward zero: a centre in (-1, 0) lands in cell 0 with a negative offset.  An object with
 *   w' <= 0, l' <= 0 or a cell outside the map is skipped: its slot stays zero.  (NaN sizes or centres are skipped as well.)
 *   Radius = max(min_radius, int(gaussian_radius((l', w'), gaussian_overlap))), the three quadratic roots in float64.
 *   Heat map: exp(-(dx^2 + dy^2) / (2 sigma^2)), sigma = (2 r + 1) / 6, in float64, rounded once to fp32, over the window
 *   [x - min(x, r), x + min(w - x, r + 1)) x [y - min(y, r), y + min(h - y, r + 1)) (the left / right / top / bottom clipping of
 *   draw_umich_gaussian), combined by max: the values are >= 0, so an integer atomic max on the bit pattern is order-independent.
 *   The reference's cut `h[h < eps * h.max()] = 0` never fires: the smallest value of a window is exp(-36 r^2 / (2 r + 1)^2) > e^-9.
 *   anno_box row = ct - ct_int (2), z, log w, log l, log h, vx, vy, sin rot', cos rot' with rot' = rot - floor(rot / P + 0.5) * P,
 *   P = fp32(2 pi), in fp32 with separate roundings (limit_period); log / sin / cos in float64, rounded once.
 *   ind = y * w + x; cat = the class inside the task, 0-based.
 *   Errors, before anything touches a device: LINK_ERR_ARG for a null pointer, batch < 1, n_cap outside 0..LINK_CENTER_MAX_OBJECTS,
 *   num_tasks outside 1..LINK_CENTER_MAX_TASKS, a class count outside 1..LINK_CENTER_MAX_CLASSES, w / h / max_objs / out_size_factor
 *   < 1, min_radius < 0, batch * classes * h * w or batch * max_objs * 10 >= 2^31, a voxel size that is not positive, an overlap
 *   outside (0, 1).  n_cap == 0: every target is written as zeros.
 *
 * link_center_loss_forward / link_center_loss_backward: one task's loss, three launches / two launches.
 *   hm [batch, k, h, w] and the regression maps reg [batch, 2, h, w], height [.., 1, ..], dim [.., 3, ..], vel [.., 2, ..] or NULL,
 *   rot [.., 2, ..] are read in place as NCHW in io_dtype (LINK_IO_F32 / F16 / BF16), widened on load; the targets are those of
 *   link_center_assign (mask holds 0 or 1).  reg_batch_strides, when not NULL, names for reg, height, dim, vel, rot the elements from
 *   one frame of the map to the next (at least channels * h * w), so that the five maps may be channel slices of ONE [batch, 10 or 8,
 *   h, w] tensor (RegLoss's `output`); NULL: every map contiguous.  Either term may be left out: hm == NULL (with hm_target, cat,
 *   unit_hm / grad_hm) gives hm_loss = 0 and a slot then counts whatever its cat; reg == height == dim == rot == NULL (with vel,
 *   anno_box, code_weights, unit_box and the five gradients) gives loc_loss = 0.  code_weights float[10] (host): with vel all ten, without vel the first eight weigh the
 *   target columns 0, 1, 2, 3, 4, 5, 8, 9.
 *   input_kind LINK_CENTER_LOGITS: y = clamp(sigmoid(x), 1e-4, 1 - 1e-4) (CenterHead._sigmoid), its derivative included and zero
 *   where the clamp is active (inclusive at the bounds, torch's rule).  LINK_CENTER_PROBAS: y = the map (FastFocalLoss itself).
 *   neg = sum over the map of log(1 - y) y^2 (1 - t)^4; pos = sum over slots of mask log(y[b, cat, ind]) (1 - y)^2; num_pos = sum mask;
 *   hm_loss = -(pos + neg) / num_pos, -neg when num_pos == 0 (selected on the device); box_loss[c] = sum over slots of
 *   mask |pred[b, c, ind] - target[b, m, c]| / (num_pos + 1e-4); loc_loss = sum_c box_loss[c] code_weights[c];
 *   loss = hm_loss + weight * loc_loss.
 *   out float[16] (device) = loss, hm_loss, loc_loss, num_pos, box_loss[0..9] (zero past the last column), two spare entries (zero).
 *   A logit that is not finite makes the loss and its gradient NaN (the reference clamps sigmoid(inf) to a finite loss with a zero
 *   gradient; a GradScaler has to see the overflow).
 *   Two deliberate differences from the reference: a slot with mask == 0 is not read at all (the reference multiplies by 0, so a NaN
 *   there poisons its sums), and an ind or cat outside the map never indexes anything (such a slot counts in num_pos and in nothing
 *   else).
 *   Forward also writes the gradients for an upstream of 1: unit_hm float[batch, k, h, w] (dense) and unit_box
 *   float[batch, max_objs, 10] (per slot and column, zero for a slot that does not count); both the caller's, written in full.
 *   link_center_loss_backward multiplies by upstream[0], a DEVICE scalar (a GradScaler's scale lives there), and writes every
 *   gradient tensor in full in io_dtype, rounded once: d hm dense, the regression gradients zero except at the ind cells.  Slots of
 *   one frame that share a cell ADD in ascending slot order, by the thread that owns the lowest slot.
 *   Sums: a workgroup's part by a tree of fixed shape, the workgroups' parts in workgroup order by one workgroup.
 *   The workspace (link_center_loss_workspace_bytes; host only) holds the partial sums; it needs no initialisation and serves one
 *   stream at a time.  Errors, before anything touches a device: LINK_ERR_ARG for a null pointer (vel / grad_vel excepted, which go
 *   together), batch / k / h / w < 1, k > LINK_CENTER_MAX_CLASSES, batch * k * h * w or batch * 3 * h * w >= 2^31, max_objs outside
 *   1..LINK_CENTER_MAX_SLOTS, batch > LINK_CENTER_MAX_BATCH, an unknown io_dtype / input_kind; LINK_ERR_WORKSPACE for fewer bytes than
 *   the size helper names (0 where the call would return LINK_ERR_ARG).
 * ============================================================================================= */
#define LINK_CENTER_LOGITS 0
#define LINK_CENTER_PROBAS 1
#define LINK_CENTER_MAX_TASKS 8
#define LINK_CENTER_MAX_CLASSES 16
#define LINK_CENTER_MAX_OBJECTS 2048
#define LINK_CENTER_MAX_SLOTS 4096
#define LINK_CENTER_MAX_BATCH 1024
typedef struct {
  float pc_range[2], voxel_size[2];   /* x, y */
  float gaussian_overlap;
  int32_t out_size_factor, w, h, max_objs, min_radius, num_tasks;
  int32_t num_classes[LINK_CENTER_MAX_TASKS];
} link_center_assign_geom_t;          /* link_abi_struct_size(9) */
int link_center_assign(const link_center_assign_geom_t *geom /* host */, const float *gt_boxes /* [batch, n_cap, 9] */,
                       const int32_t *gt_classes /* [batch, n_cap] */, int32_t batch, int32_t n_cap,
                       float *const *hm /* host [num_tasks] of device pointers, as the four below */, float *const *anno_box,
                       int64_t *const *ind, uint8_t *const *mask, int64_t *const *cat, void *stream);
size_t link_center_loss_workspace_bytes(int32_t batch, int32_t k, int32_t h, int32_t w, int32_t max_objs); /* host only */
int link_center_loss_forward(const void *hm, const void *reg, const void *height, const void *dim, const void *vel /* nullable */,
                             const void *rot, const int64_t *reg_batch_strides /* host [5], nullable */, int32_t io_dtype, int32_t input_kind, const float *hm_target, const float *anno_box,
                             const int64_t *ind, const uint8_t *mask, const int64_t *cat, int32_t batch, int32_t k, int32_t h, int32_t w,
                             int32_t max_objs, const float *code_weights /* host [10] */, float weight, void *workspace,
                             size_t workspace_bytes, float *out /* [16] */, float *unit_hm /* [batch, k, h, w] */,
                             float *unit_box /* [batch, max_objs, 10] */, void *stream);
int link_center_loss_backward(const float *unit_hm, const float *unit_box, const int64_t *ind, const uint8_t *mask,
                              const float *upstream /* device scalar */, int32_t batch, int32_t k, int32_t h, int32_t w, int32_t max_objs,
                              int32_t io_dtype, void *grad_hm, void *grad_reg, void *grad_height, void *grad_dim,
                              void *grad_vel /* nullable */, void *grad_rot, const int64_t *reg_batch_strides /* host [5], nullable */,
                              void *stream);

/* =============================================================================================
 * M. Segmentation front end and validation (csrc/segio.hip): quantise point clouds to voxels by a sort, vote, count for mIoU
 *
 * What the reference does on the host per frame: torchsparse.utils.quantize.sparse_quantize (segmentation/torchsparse-u/torchsparse/
 * utils/quantize.py:9-46: a numpy ravel hash and np.unique with return_index and return_inverse) behind the rounding and the minimum
 * subtraction of segmentation/core/datasets/semantic_kitti.py:219-220; and per validation step segmentation/evaluate.py:120-134 (voxel
 * logits back to points through inverse_map, the test-time-augmentation passes stacked, summed, argmax) followed by core/callbacks.py:
 * 41-52 (MeanIoU: 3 (num_classes - 1) read-backs).  Additive entries: the ABI version does not move.  Integer atomics only, no host
 * synchronisation, no allocation, launch geometry a function of the shapes alone (every call can be captured in a graph); every
 * result is an integer, so two calls are bit for bit equal.
 *
 * link_seg_quantize: `batch` clouds one after the other, point_offsets int32[batch + 1] (device; point_offsets[0] = 0, ascending)
 *   names their rows, point_offsets[batch] (clamped to n, which sizes the launches and the workspace) is the number of points.
 *   mode LINK_SEGQ_INT: points = int32[n, 3], the coordinates themselves (ndim and voxel_size are not read).
 *   mode LINK_SEGQ_ROUND: points = float[n, ndim] (x, y, z first); the coordinate is rint(p / voxel_size), a correctly rounded fp32
 *     divide, rounded half to even, then converted to int32: np.round(block[:, :3] / voxel_size).astype(np.int32).
 *   In both modes the minimum of every axis over the sample is subtracted (pc_ -= pc_.min(0); the x -= min of ravel_hash).
 *   Per sample the voxels are the distinct coordinates in ascending lexicographic (x, y, z) order, x most significant (the order
 *   the ravel hash induces); the samples' voxels are concatenated in sample order.  Outputs:
 *     coords int32[voxel_capacity, 4] = x, y, z, b after the minimum is subtracted (16-byte aligned); rows past the total zeroed;
 *     indices int32[voxel_capacity]: the smallest point index of the voxel (what np.unique's return_index gives), indexing the
 *       concatenated points; entries past the total zeroed;
 *     inverse int32[n]: the voxel of every point as a row of coords (global); inverse_local int32[n] (nullable): the same counted from
 *       the first voxel of the point's sample (what evaluate.py indexes one scene with).  -1 for a point of a flagged sample, for a
 *       point whose voxel lies at or past voxel_capacity, and for the entries past the number of points: nothing ever names a row
 *       that does not exist;
 *     voxel_offsets int32[batch + 1]: the rows of each sample, clamped to voxel_capacity (voxels beyond it are not written);
 *     status int32[4] = the voxel total before clamping, the flag word, the number of key bits sorted, the number of points.
 *   Flags: LINK_SEGQ_FLAG_EXTENT -- an axis of a sample spans 2^20 or more after the minimum is subtracted, or a rounded coordinate
 *   leaves int32; LINK_SEGQ_FLAG_NONFINITE -- a coordinate is NaN or infinite.  A sample that raises either produces zero voxels; the
 *   other samples are not affected.  The sort key holds x, y, z in the bits the largest extent of each axis over the batch needs and
 *   the sample index on top; LINK_SEGQ_FLAG_KEYBITS -- together they exceed 64 bits (possible only with more than 16 samples of
 *   extents near 2^20): then no sample produces a voxel.
 *   The sort is a stable LSD radix sort of (64-bit key, point index) pairs in tiles of LINK_SEGQ_SORT_TILE pairs, 8 bits per pass;
 *   the passes above the highest key bit return at once, decided on the device.  33 launches whatever the data.
 *   The workspace (link_seg_quantize_workspace_bytes; host only, needs no device) holds 24.5 bytes per point -- two key buffers, two
 *   index buffers, the tile histograms -- plus 32 bytes per sample; it needs no initialisation and serves one stream at a time.
 *   Errors, before anything is launched: LINK_ERR_ARG for n outside [0, 2^28), batch outside 1..1024, voxel_capacity outside
 *   [0, 2^28), an unknown mode, with LINK_SEGQ_ROUND ndim outside 3..16 or a voxel size that is not positive and finite, a null
 *   pointer (points and inverse may be null when n == 0, coords and indices when voxel_capacity == 0, inverse_local always);
 *   LINK_ERR_WORKSPACE for fewer bytes than the size helper names (which returns 0 where the call would return LINK_ERR_ARG).
 *
 * link_seg_vote_eval: one kernel, one thread per point.
 *   input_kind LINK_SEGEVAL_ROWS: rows [n_rows, c] in io_dtype (LINK_IO_F32 / F16 / BF16), LINK_SEGLOSS_MIN_CLASSES <= c <=
 *     LINK_SEGLOSS_MAX_CLASSES; inverse int32[votes, n_points] names rows: pass v of point p reads rows[inverse[v, p]], an entry
 *     outside [0, n_rows) contributes nothing (inverse == NULL: votes == 1, n_rows == n_points, point p reads row p).  The votes
 *     (1..LINK_SEGEVAL_MAX_VOTES) are summed in fp32 in ascending pass order, starting from zero; the class is the arg max, the
 *     lowest class index among equals; a NaN sum counts as -inf and never wins (class 0 when every sum is NaN or -inf).
 *   input_kind LINK_SEGEVAL_PREDICTIONS: rows = int64[n_points], the classes themselves (the training-time callback receives
 *     arg-maxed outputs); io_dtype, n_rows, inverse and votes are not read.
 *   pred int32[n_points] (nullable) = the class, or lut[class] when lut int32[c] is given (the remap of evaluate.py:215-243; the
 *   counters always take the class itself).  labels int64[n_points] (nullable: then nothing is counted); a point counts when
 *   label != ignore_label.  counters int64[3, c] = seen, positive, correct; the call ADDS to them (the caller zeroes them once per
 *   epoch):  seen[t] += 1 when 0 <= t < c;  positive[class] += 1 when 0 <= class < c;  correct[t] += 1 when class == t.
 *   Per workgroup a histogram in LDS, then at most 3 c 64-bit integer atomics.
 *   Errors, before anything is launched: LINK_ERR_ARG for c outside the range, n_points outside [0, 2^31), an unknown input_kind or
 *   io_dtype, votes outside the range, n_rows outside [0, 2^31), labels without counters, null rows with points to read.
 *   n_points == 0: LINK_OK, nothing is launched.
 * ============================================================================================= */
#define LINK_SEGQ_INT 0
#define LINK_SEGQ_ROUND 1
#define LINK_SEGQ_SORT_TILE 2048
#define LINK_SEGQ_FLAG_EXTENT 1
#define LINK_SEGQ_FLAG_NONFINITE 2
#define LINK_SEGQ_FLAG_KEYBITS 4
#define LINK_SEGEVAL_ROWS 0
#define LINK_SEGEVAL_PREDICTIONS 1
#define LINK_SEGEVAL_MAX_VOTES 16
size_t link_seg_quantize_workspace_bytes(int64_t n, int32_t batch); /* host only */
int link_seg_quantize(const void *points, int32_t mode, int32_t ndim, float voxel_size, const int32_t *point_offsets /* [batch + 1], device */,
                      int32_t batch, int64_t n, void *workspace, size_t workspace_bytes, int32_t *coords /* [voxel_capacity, 4] = x, y, z, b */,
                      int32_t *indices /* [voxel_capacity] */, int64_t voxel_capacity, int32_t *inverse /* [n] */,
                      int32_t *inverse_local /* [n], nullable */, int32_t *voxel_offsets /* [batch + 1], device */, int32_t *status /* [4] */,
                      void *stream);
int link_seg_vote_eval(const void *rows, int32_t io_dtype, int32_t input_kind, int64_t n_rows, int32_t c,
                       const int32_t *inverse /* [votes, n_points], nullable */, int32_t votes, int64_t n_points,
                       const int64_t *labels /* nullable */, int64_t ignore_label, const int32_t *lut /* [c], nullable */,
                       int32_t *pred /* [n_points], nullable */, int64_t *counters /* [3, c] */, void *stream);

/* =============================================================================================
 * N. CenterHead test-time augmentation (csrc/dettta.hip): the four flipped views, the fused decode of their maps, class-wise NMS
 *
 * What the reference does for its reported nuScenes results (configs/nusc/voxelnet/..._elkv3_flip.py and ..._flip_rot.py:
 * double_flip=True, tt_rotation): on the host per frame, datasets/pipelines/test_aug.py:12-32 (three flipped copies of the cloud)
 * after preprocess.py:153-156 (the rotation, core/bbox/box_np_ops.py:182-204); on the device in about forty torch ops per task,
 * models/bbox_heads/center_head.py:320-421 (the maps of views 1-3 flipped back in place, sigmoid / exp, the mean of the four
 * views) and :461-467 (the masks); on the host again :489-503 (the kept boxes rotated back); and detection/nms_better2.py:266-297
 * (the passes of several angles merged: one rotate_nms_pcdet per class with that class's threshold, then the 500 best).
 * Additive entries: the ABI version does not move.  All fp32, no atomics, no allocation, no host round trip; every entry takes a
 * stream, keeps no state and is bitwise reproducible.
 *
 * link_tta_views: points float[n, ndim] = `batch` clouds one after the other, point_offsets int32[batch + 1] (device; [0] = 0,
 *   ascending, [batch] = n).  out float[4 n, ndim] = the 4 batch clouds frame-major, view-minor: view v of cloud b occupies the
 *   n_b rows from 4 point_offsets[b] + v n_b; out_offsets int32[4 batch + 1] (device) names them.  View 0 is the cloud with
 *   columns 0, 1 rotated: x' = x cos_a + y sin_a, y' = x (-sin_a) + y cos_a, each product and sum rounded on its own (cos_a,
 *   sin_a: the caller's float64 cos / sin of tt_rotation rounded to fp32, as the reference's matrix holds them); view 1 has
 *   y = -y, view 2 x = -x, view 3 both; columns 2.. are copied.  cos_a == 1 and sin_a == 0: no arithmetic, bit for bit copies.
 *   One launch.  Offsets that do not describe n rows write nothing for the clouds concerned (never out of bounds).
 *   LINK_ERR_ARG: batch outside 1..16383, n outside [0, 2^29), ndim outside 3..16, cos_a / sin_a not finite, null pointers.
 *
 * link_center_decode_flip4: link_center_decode for maps of batch 4 frames in that order, read in place: cell (h, w) of a frame
 *   reads view 1 at (h_size-1-h, w), view 2 at (h, w_size-1-w), view 3 at both.  Per view first: sigmoid of hm, exp of dim,
 *   1 - reg_y in view 1, 1 - reg_x in view 2, both in view 3, rot's cos negated in view 1, its sin in view 2, both in view 3, vel's
 *   y negated in view 1, its x in view 2, both in view 3; then the mean of the four views as ((v0 + v1) + v2) + v3) / 4; then as
 *   link_center_decode (arg max of the mean scores, lowest class among equals; atan2f of the mean sin and cos; box assembly; the
 *   masks).  Outputs as link_center_decode with batch = frames.  LINK_ERR_ARG as link_center_decode, with 4 frames > 65535.
 *
 * link_nms_mask_classwise: link_nms_mask's words (same layout, same n_dev convention; link_nms_reduce consumes them) for the
 *   predicate labels[i] == labels[j] and rotated IoU > thr[labels[i]].  labels int32[cap], thr float[num_cls] (device).  A label
 *   outside [0, num_cls) neither suppresses nor is suppressed.  A 64 x 64 tile without a common class costs no IoU work.
 *
 * link_tta_rotate_back: out float[m, ncol] (ncol 7, or 9 with the velocity pair in columns 6, 7) = boxes[idx[j]] (idx int64[m],
 *   device; NULL: row j; then m <= n_src is the caller's business only in that rows past n_src are zeros) with columns 0, 1 and
 *   6, 7 rotated as above by (cos_a, sin_a) and `angle` added to the last column -- center_head.py:489-503 with cos_a, sin_a,
 *   angle of -tt_rotation.  angle == 0: a plain gather.  idx[j] < 0 or >= n_src: a row of zeros.  out must not overlap boxes.
 * ============================================================================================= */
int link_tta_views(const float *points, const int32_t *point_offsets /* [batch + 1], device */, int32_t batch, int64_t n, int32_t ndim,
                   float cos_a, float sin_a, float *out /* [4 n, ndim] */, int32_t *out_offsets /* [4 batch + 1], device */, void *stream);
int link_center_decode_flip4(const float *hm, const float *reg, const float *height, const float *dim, const float *rot, const float *vel,
                             int32_t frames, int32_t num_cls, int32_t h, int32_t w, const link_center_geom_t *geom /* host */, float *boxes,
                             int32_t *labels, float *scores, int32_t *counts, void *stream);
int link_nms_mask_classwise(const float *boxes, const int32_t *labels, int64_t cap, const int32_t *n_dev, const float *thr /* [num_cls] */,
                            int32_t num_cls, uint64_t *mask, void *stream);
int link_tta_rotate_back(const float *boxes, int64_t n_src, int32_t ncol, const int64_t *idx /* [m], nullable */, int64_t m, float cos_a,
                         float sin_a, float angle, float *out /* [m, ncol] */, void *stream);

/* =============================================================================================
 * O. Two-stage ROI head (csrc/roihead.hip): BEV features of the proposals, target assignment, loss, box refinement
 *
 * What the reference's TwoStageDetector does behind its first stage (detection/det3d/models/detectors/two_stage.py,
 * models/second_stage/bird_eye_view.py, models/roi_heads/roi_head.py and roi_head_template.py,
 * models/roi_heads/target_assigner/proposal_target_layer.py): a permuted copy of the whole BEV map, features for every proposal, a
 * host loop over frames and classes with one boxes_iou3d_gpu call each, np.random draws on the host, two .item() calls in the
 * loss.  Additive entries: the ABI version does not move.  fp32 arithmetic inside, every product and sum rounded on its own,
 * cos / sin correctly rounded; no atomics, every float sum in a fixed order (two calls are bit for bit equal), no allocation, no host
 * synchronisation, launch geometry a function of the shapes alone: every call can be captured in a graph.  Argument errors
 * (LINK_ERR_ARG) are returned before anything touches a device.
 *
 * link_roi_bev_features: one launch.  bev = the map [batch, c, h, w] in io_dtype, read in place through strides int64[4] (host;
 *   elements from one frame / channel / row / column to the next, each in [0, 2^40)): contiguous NCHW, channels_last and slices
 *   alike.  boxes float[batch, r, box_len], box_len 7..64, heading in column rot_col, extents in columns 3, 4.  labels int64[batch, r]
 *   (nullable): a row with label 0 is an unused slot.  sel int32[batch, s] (nullable; then s == r): output row j of frame b reads
 *   box sel[b, j]; repeats allowed; an index outside [0, r) is an unused slot.  out [batch, s, num_point c] in io_dtype, the channels
 *   of point p at [p c, (p + 1) c); an unused slot gives a row of zeros.
 *   Points (two_stage.py:51-78): the centre; with num_point 5 also the midpoints of the front, back, left and right edges:
 *   corners (-,-), (-,+), (+,+), (+,-) of (dx, dy) / 2 rotated by x' = x cos + y sin, y' = -x sin + y cos, plus the centre; front =
 *   (c0 + c1) / 2, back = (c2 + c3) / 2, left = (c0 + c3) / 2, right = (c1 + c2) / 2.
 *   Map coordinates: ((x - pc_start[0]) / voxel_size[0]) / out_stride and likewise y, IEEE divisions.
 *   Interpolation (center_utils.py:92-121): x0 = floor(x), x1 = x0 + 1, both clamped to [0, w - 1] (y alike), the four weights from
 *   the CLAMPED corners, ((Ia wa + Ib wb) + Ic wc) + Id wd with Ia = map[y0, x0], Ib = [y1, x0], Ic = [y0, x1], Id = [y1, x1];
 *   rounded once into io_dtype.  A point off the map therefore does not get plain border replication.
 *   One wave per (output row, point); lanes along the channels, four channels per lane in one load where the channel stride is 1,
 *   c % 4 == 0, the other strides are multiples of 4 and both pointers are aligned to four elements.
 *   LINK_ERR_ARG: a null pointer, an unknown io_dtype, num_point outside {1, 5}, batch outside 0..65535, c / h / w < 1, box_len or
 *   rot_col out of range, s != r without sel, batch r or batch s num_point >= 2^31, a voxel size or out_stride that is not positive
 *   and finite.  batch == 0 or s == 0: LINK_OK, nothing is launched.
 *
 * link_roi_assign: ProposalTargetLayer.forward + RoIHeadTemplate.assign_targets for a batch, two launches.
 *   rois float[batch, r, code], code 7 or 9, heading in column 6; roi_labels int64[batch, r]; roi_scores float[batch, r];
 *   gt float[batch, g, code + 1], the class last (g == 0: one row of zeros serves); trailing rows whose sum is 0 are cut, one row
 *   always stays.  1 <= r <= LINK_ROI_MAX_ROIS, g <= LINK_ROI_MAX_GT, 1 <= m <= LINK_ROI_MAX_SAMPLES.
 *   Overlaps: boxes_iou3d_gpu's formula (to_pcdet on both sides, the rotated BEV overlap of section I times the height overlap,
 *   over max(vol_a + vol_b - overlap, 1e-6)) of columns 0..6 of every ROI against every ground-truth row that counts; by_class: only
 *   rows whose class (truncated to an integer) equals the ROI's label, and an ROI without such a row keeps overlap 0 and
 *   assignment 0.  The maximum, the lowest index among equals: max_overlaps float[batch, r], gt_assignment int32[batch, r].
 *   code 9 needs by_class (the reference's other branch asserts 7 columns).
 *   Sampling (subsample_rois, :133-208), one workgroup per frame: fg = overlap >= min(reg_fg, cls_fg); easy bg = overlap <
 *   cls_bg_lo; hard bg = overlap < reg_fg and >= cls_bg_lo; each list in ascending ROI order.  fg_per_image = fg_ratio m rounded
 *   half to even.  With fg and bg: min(fg_per_image, |fg|) foreground rows without replacement -- the candidates with the smallest
 *   noise[b, i], in ascending order of (noise, i) -- then m minus that background rows; fg only: m draws with replacement; bg
 *   only: m background rows.  Background: with both lists min(int(n hard_bg_ratio), |hard|) hard rows then easy rows, else all from
 *   the list that exists.  Every draw with replacement for output slot j takes entry min(floor(noise[b, r + j] n), n - 1) of its
 *   list of n.  noise float[batch, r + m] in [0, 1).  No candidate at all (overlaps that are not finite): status[b] =
 *   LINK_ROI_STATUS_NO_CANDIDATE and every slot names row 0.  sel_in int32[batch, m] (nullable) replaces the sampling (noise may
 *   then be NULL); an index outside [0, r) reads row 0 and sets LINK_ROI_STATUS_BAD_INDEX.
 *   Targets of the m rows, written in full: sel int32, rois, roi_labels int64, roi_scores, gt_iou_of_rois (= max_overlaps),
 *   gt_of_rois_src float[.., code + 1], reg_valid_mask int64 (overlap > reg_fg), rcnn_cls_labels float (soft_labels 0: overlap >
 *   cls_fg, -1 where cls_bg < overlap < cls_fg; 1: 1 above cls_fg, 0 below cls_bg, (overlap - cls_bg) / (cls_fg - cls_bg) between),
 *   gt_of_rois float[.., code + 1] in the ROI's canonical frame (roi_head_template.py:52-82): ry = limit_period(heading, 0.5, 2 pi);
 *   columns 0..5 minus the ROI's, column 6 minus ry, columns 0, 1 rotated by -ry (x' = x cos + y sin, y' = -x sin + y cos), columns
 *   7, 8 minus the ROI's for code 9; the heading floor-mod 2 pi, plus pi floor-mod 2 pi where it lies strictly between pi / 2 and
 *   3 pi / 2, minus 2 pi where above pi, clamped to +-pi / 2.
 *   LINK_ERR_ARG: a null pointer (gt with g == 0, sel_in, and noise with sel_in excepted), code outside {7, 9}, sizes out of range, a
 *   ratio outside [0, 1], thresholds that are not finite or not ordered cls_bg_lo <= reg_fg, cls_bg_lo <= cls_fg, cls_bg < cls_fg.
 *
 * link_roi_loss_forward / link_roi_loss_backward: RoIHeadTemplate.get_loss with CLS_LOSS BinaryCrossEntropy and REG_LOSS L1; one
 *   workgroup each.  rcnn_cls [n], rcnn_reg [n, code] in io_dtype, 1 <= n <= LINK_ROI_MAX_LOSS_ROWS; the targets of link_roi_assign.
 *   cls = sum over rows with label >= 0 of -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)), p = sigmoid(x), over
 *   max(number of such rows, 1), times cls_weight; a row with label < 0 is not read.  reg = sum over rows with reg_valid_mask > 0 and
 *   columns of |reg - gt_of_rois| code_weights[c] over max(fg_sum, 1), times reg_weight, selected on the device.  out float[4]
 *   (device) = total, cls, reg, fg_sum.  Forward also writes the gradients for an upstream of 1: unit_cls float[n] (autograd's
 *   ((p - t) / max(p (1 - p), 1e-12)) p (1 - p) over the count, weighted) and unit_reg float[n, code]; backward multiplies them by
 *   upstream[0], a DEVICE scalar, and writes both gradients in io_dtype, rounded once.  Sums: rows t, t + 256, .. per thread in
 *   ascending order, then a tree of fixed shape.
 *
 * link_roi_refine: generate_predicted_boxes + TwoStageDetector.post_process, one workgroup per frame.  Per slot with label != 0:
 *   v = rcnn_reg + the ROI with its centre zeroed; columns 0, 1 rotated by the ROI's heading (x' = x cos + y sin, y' = -x sin + y
 *   cos), then the centre added to columns 0..2; score = sqrt(sigmoid(rcnn_cls) roi_score); label - 1; for code 9 the columns reordered
 *   to 0..5, 7, 8, 6.  The slots in use are packed to the front of boxes float[batch, r, code], scores float[batch, r], labels
 *   int64[batch, r] in slot order; the rest is zeros with label -1; counts int32[batch].
 * ============================================================================================= */
#define LINK_ROI_MAX_ROIS 4096
#define LINK_ROI_MAX_GT 512
#define LINK_ROI_MAX_SAMPLES 1024
#define LINK_ROI_MAX_LOSS_ROWS (1 << 20)
#define LINK_ROI_STATUS_NO_CANDIDATE 1
#define LINK_ROI_STATUS_BAD_INDEX 2
int link_roi_bev_features(const void *bev, int32_t io_dtype, const int64_t *strides /* host [4] */, int32_t batch, int32_t c, int32_t h,
                          int32_t w, const float *boxes /* [batch, r, box_len] */, int64_t r, int32_t box_len, int32_t rot_col,
                          const int64_t *labels /* [batch, r], nullable */, const int32_t *sel /* [batch, s], nullable */, int64_t s,
                          int32_t num_point, const float *pc_start /* host [2] */, const float *voxel_size /* host [2] */,
                          float out_stride, void *out /* [batch, s, num_point c] */, void *stream);
int link_roi_assign(const float *rois, const int64_t *roi_labels, const float *roi_scores, const float *gt /* [batch, g, code + 1] */,
                    const float *noise /* [batch, r + m] */, const int32_t *sel_in /* [batch, m], nullable */, int32_t batch, int64_t r,
                    int64_t g, int64_t m, int32_t code, double fg_ratio, int32_t by_class, int32_t soft_labels, double cls_fg_thresh,
                    double cls_bg_thresh, double cls_bg_thresh_lo, double hard_bg_ratio, double reg_fg_thresh,
                    float *max_overlaps /* [batch, r] */, int32_t *gt_assignment /* [batch, r] */, int32_t *sel /* [batch, m] */,
                    float *out_rois, int64_t *out_roi_labels, float *out_roi_scores, float *gt_iou_of_rois, float *gt_of_rois_src,
                    float *gt_of_rois, int64_t *reg_valid_mask, float *rcnn_cls_labels, int32_t *status /* [batch] */, void *stream);
int link_roi_loss_forward(const void *rcnn_cls, const void *rcnn_reg, int32_t io_dtype, int64_t n, int32_t code,
                          const float *rcnn_cls_labels, const float *gt_of_rois, const int64_t *reg_valid_mask,
                          const float *code_weights /* host [code] */, float rcnn_cls_weight, float rcnn_reg_weight, float *out /* [4] */,
                          float *unit_cls /* [n] */, float *unit_reg /* [n, code] */, void *stream);
int link_roi_loss_backward(const float *unit_cls, const float *unit_reg, const float *upstream /* device scalar */, int64_t n,
                           int32_t code, int32_t io_dtype, void *grad_cls, void *grad_reg, void *stream);
int link_roi_refine(const float *rois, const int64_t *roi_labels, const float *roi_scores, const void *rcnn_cls, const void *rcnn_reg,
                    int32_t io_dtype, int32_t batch, int64_t r, int32_t code, float *boxes, float *scores, int64_t *labels,
                    int32_t *counts, void *stream);

/* =============================================================================================
 * P. Detection training front end (csrc/detaug.hip): points against rotated boxes, BEV collisions, ground-truth paste, global augmentation
 *
 * What the reference's training pipeline (detection/det3d/datasets/pipelines/preprocess.py::Preprocess) does on the host between
 * "points and annotations are loaded" and the voxeliser: box_np_ops.points_in_rbbox / points_count_rbbox (the minimum-points
 * filter), box_np_ops.center_to_corner_box2d and core/sampler/preprocess.py::box_collision_test (the ground-truth sampler's
 * acceptance test), the sampler's scan and paste, the four global transforms, the shuffle and the range filter on the boxes.
 * Additive entries: the ABI version does not move.  fp32 arithmetic inside, every product and sum
 * rounded on its own, cos / sin correctly rounded; integer atomics only, so two calls are bit for bit equal; no allocation, no host
 * synchronisation, launch geometry a function of the shapes alone: every call can be captured in a graph.  Argument errors
 * (LINK_ERR_ARG) are returned before anything touches a device.
 *
 * link_points_in_rbbox: one launch (plus the clearing of counts).  points float[n_points, ndim], ndim 3..64, x y z first.
 *   point_offsets int32[batch + 1] (device; NULL needs batch == 1: all points belong to frame 0): frame b owns rows
 *   [point_offsets[b], point_offsets[b + 1]), cut to [0, n_points].  boxes float[batch, n_boxes, box_len], box_len 7..64: centre,
 *   extents, heading in the LAST column; the centre is the box's middle on all three axes (origin (0.5, 0.5, 0.5)).
 *   A point is inside when, with q = p - centre turned back by the heading (x = qx cos - qy sin, y = qx sin + qy cos: the inverse of
 *   rotation_3d_in_axis(axis = 2), which turns clockwise for a positive angle), |x| < dx / 2, |y| < dy / 2 and |qz| < dz / 2, all
 *   strictly: what geometry.py:273 decides with `sign >= 0` means outside.  A box with a zero extent holds nothing; a NaN
 *   coordinate is in no box.  mask uint8[n_points, n_boxes] (nullable), 1 = inside, row p against the boxes of p's frame; rows no
 *   frame owns are not written.  counts int32[batch, n_boxes] (nullable): points of the frame inside each box; one wave reduction
 *   and one integer atomic per (wave, box).  At least one of mask and counts.
 *   LINK_ERR_ARG: sizes out of range (batch 1..65535, n_points < 2^31 - 256, n_boxes <= 2^24, n_points n_boxes <= 2^40 with a
 *   mask), a null pointer.  n_boxes == 0: LINK_OK, nothing is launched.
 *
 * link_box2d_corners: box_np_ops.center_to_corner_box2d.  centers float[n, 2], dims float[n, 2], angles float[n] (nullable: no
 *   rotation) -> out float[n, 4, 2]: the corners (-,-), (-,+), (+,+), (+,-) of dims (u - origin), turned by x' = x cos + y sin,
 *   y' = -x sin + y cos, plus the centre: clockwise from the minimum corner, the order link_box_collision's `clockwise` names.
 *
 * link_box_collision: box_collision_test.  corners_a float[n, 4, 2], corners_b float[k, 4, 2] -> out uint8[n, k].  A pair collides
 *   when the axis-aligned bounds of the two quadrilaterals overlap by more than 0 on both axes, and then either one of the 16
 *   pairs of edges (A B of a, C D of b) crosses -- acd != bcd and abc != abd with acd = (Dy - Ay)(Cx - Ax) > (Cy - Ay)(Dx - Ax)
 *   and likewise -- or one quadrilateral holds all four corners of the other strictly (cross >= 0 on any edge: not held).
 *   n k < 2^31 - 256.
 *
 * link_detaug_sample: DataBaseSamplerV2.sample_all without group sampling (sample_ops.py:97-172, 250-296) and the bookkeeping of
 *   Preprocess.__call__ around it (datasets/pipelines/preprocess.py:73-122), one launch, one workgroup per frame.
 *   gt_boxes float[batch, max_gt, box_len], box_len 7 or 9, heading last; gt_classes int32[batch, max_gt]: 0 an empty slot (or a
 *   DontCare row), k >= 1 the k-th name of the detector's class list, negative a name outside that list (it stays in the avoid set
 *   and is dropped from the output, as gt_boxes_mask does); gt_counts int32[batch, max_gt] (link_points_in_rbbox's counts on the
 *   untransformed scene; NULL with min_points <= 0): a row with fewer than min_points points does not survive.
 *   The database: db_boxes float[db_size, box_len], db_classes int32[db_size] (>= 1), db_offsets int64[db_size + 1] (rows of the
 *   packed object-centred points).  candidates int32[batch, n_groups, max_candidates] with cand_len int32[batch, n_groups]:
 *   database indices in the order the reference's BatchSampler would hand them out.
 *   For group q in order: n = clamp(round_half_even(rate (group_max[q] - survivors of class group_class[q])), 0, cand_len) heads of
 *   the list are tested with link_box_collision's rule against the avoid set (the surviving ground truth, then everything
 *   accepted for earlier groups) and against each other; candidate i is rejected when it collides with the avoid set, with an
 *   accepted earlier candidate or with ANY later candidate of the n (sample_class_v2 clears a rejected row and column only when
 *   it reaches it); the accepted join the avoid set.  An index outside [0, db_size) is rejected and sets
 *   LINK_DETAUG_STATUS_BAD_INDEX.
 *   Out, with max_accept = n_groups max_candidates: accepted int32[batch, max_accept] (database indices in acceptance order, then
 *   -1), paste_start int32[batch, max_accept + 1] (first point slot of every accepted object, the pasted total from n_accept on),
 *   n_accept int32[batch]; merged_boxes float[batch, max_gt + max_accept, box_len] / merged_classes int32[..] / n_merged
 *   int32[batch]: the survivors of a class >= 1 in order, then the accepted database boxes; status int32[batch], written in full.
 *   LINK_ERR_ARG: n_groups > LINK_DETAUG_MAX_GROUPS, max_candidates > LINK_DETAUG_MAX_CANDIDATES, max_gt + n_groups max_candidates
 *   > LINK_DETAUG_MAX_BOXES (the avoid set and the collision rows live in LDS), a class < 1, a negative rate, a null pointer.
 *
 * link_detaug_transform: the paste, random_flip_both, global_rotation, global_scaling_v2, global_translate_ (core/sampler/
 *   preprocess.py:803-839, 771-788, 940-962), the point shuffle and filter_gt_box_outside_range (:108-122); two launches.
 *   draws float[batch, 7], device: u_flip_x, u_flip_y, u_rot, u_scale uniform in [0, 1) and three standard normals.  A flip happens
 *   when its u >= 1 - flip_probability (np.random.choice's rule); angle = rot_lo + (rot_hi - rot_lo) u_rot and scale likewise, in
 *   double; the translation is std[0] n0, std[1] n1, std[0] n2 (the reference draws z with std[0]), added in double.
 *   Points: slot r of frame b is, in this order, a point of the accepted objects (object-centred point + its box centre, in
 *   acceptance order), a point of the frame's scene (points float[n_points, ndim] by point_offsets int32[batch + 1]), or nothing;
 *   it is transformed (x flip: y = -y; y flip: x = -x; x' = x cos + y sin, y' = -x sin + y cos; times scale; plus translation)
 *   and written to row perm[b, r] of out_points float[batch, point_capacity, ndim]; a slot past the frame's total writes a row of
 *   NaN (link_voxelize's range test rejects it), a frame with more points than point_capacity loses the last and sets
 *   LINK_DETAUG_STATUS_POINTS_CUT.  perm int32[batch, point_capacity]: a permutation of 0 .. point_capacity - 1 per frame (the
 *   reference's np.random.shuffle); an entry out of range writes nothing.
 *   Boxes: the merged boxes get the same steps with the reference's quirks -- heading = -heading + pi (x flip), -heading + 2 pi
 *   (y flip), + angle; the velocity columns 6, 7 of box_len 9 are flipped, rotated (in double) and scaled like every column but the
 *   heading -- and stay when one BEV corner lies strictly inside range = xmin, ymin, xmax, ymax; the kept are packed in order into
 *   out_boxes float[batch, max_objs, box_len] and out_classes int32[batch, max_objs] (0 = empty; rows past the count are zeros;
 *   more than max_objs: the last are cut and LINK_DETAUG_STATUS_BOXES_CUT is set); n_boxes, n_out_points int32[batch].
 *   status is OR-ed into what link_detaug_sample wrote.
 * ============================================================================================= */
#define LINK_DETAUG_MAX_GROUPS 16
#define LINK_DETAUG_MAX_CANDIDATES 64
#define LINK_DETAUG_MAX_BOXES 1024
#define LINK_DETAUG_STATUS_BAD_INDEX 1
#define LINK_DETAUG_STATUS_POINTS_CUT 2
#define LINK_DETAUG_STATUS_BOXES_CUT 4
typedef struct {
  double rate;
  int32_t n_groups, max_candidates, max_gt, min_points, box_len, reserved;
  int32_t group_class[LINK_DETAUG_MAX_GROUPS]; /* 1-based class of every sampled group, in sample_groups' order */
  int32_t group_max[LINK_DETAUG_MAX_GROUPS];   /* its target number of objects per frame */
} link_detaug_sample_cfg_t;
typedef struct {
  double rot_lo, rot_hi, scale_lo, scale_hi, translate_std[3], flip_probability;
  double range[4]; /* xmin, ymin, xmax, ymax */
  int32_t max_objs, point_capacity;
} link_detaug_transform_cfg_t;
int link_points_in_rbbox(const float *points, int32_t ndim, const int32_t *point_offsets /* [batch + 1], device, nullable */,
                         int32_t batch, int64_t n_points, const float *boxes /* [batch, n_boxes, box_len] */, int64_t n_boxes,
                         int32_t box_len, uint8_t *mask /* [n_points, n_boxes], nullable */, int32_t *counts /* [batch, n_boxes], nullable */,
                         void *stream);
int link_box2d_corners(const float *centers, const float *dims, const float *angles /* nullable */, int64_t n, float origin,
                       float *out /* [n, 4, 2] */, void *stream);
int link_box_collision(const float *corners_a, int64_t n, const float *corners_b, int64_t k, int32_t clockwise,
                       uint8_t *out /* [n, k] */, void *stream);
int link_detaug_sample(const link_detaug_sample_cfg_t *cfg /* host */, int32_t batch, const float *gt_boxes, const int32_t *gt_classes,
                       const int32_t *gt_counts /* nullable */, const int32_t *candidates, const int32_t *cand_len, const float *db_boxes,
                       const int32_t *db_classes, const int64_t *db_offsets, int64_t db_size, int32_t *accepted, int32_t *paste_start,
                       int32_t *n_accept, float *merged_boxes, int32_t *merged_classes, int32_t *n_merged, int32_t *status, void *stream);
int link_detaug_transform(const link_detaug_transform_cfg_t *cfg /* host */, int32_t batch, const float *draws, const float *points,
                          const int32_t *point_offsets, int64_t n_points, int32_t ndim, const float *db_points, const int64_t *db_offsets,
                          const float *db_boxes, int32_t box_len, const int32_t *accepted, const int32_t *paste_start,
                          const int32_t *n_accept, int32_t max_accept, const int32_t *perm, float *out_points, const float *merged_boxes,
                          const int32_t *merged_classes, const int32_t *n_merged, int32_t max_merged, float *out_boxes,
                          int32_t *out_classes, int32_t *n_boxes, int32_t *n_out_points, int32_t *status, void *stream);

/* =============================================================================================
 * Q. Multi-object tracker (csrc/track.hip): greedy centre matching of one frame against the track list, for a batch of sequences
 *
 * The CenterPoint tracker of detection/tools/nusc_tracking/pub_tracker.py:45-154 (with track_utils.py:3-12) and
 * detection/tools/waymo_tracking/tracker.py:42-136.  Additive entries: the ABI version does not move.  One launch, one workgroup
 * per sequence, no allocation, no host synchronisation, ordinary vector stores only: a call can be captured in a graph.
 * Argument errors (LINK_ERR_ARG) are returned before anything touches a device.
 *
 * link_track_state_bytes(capacity): bytes of ONE sequence's state, 0 for a capacity outside 1..LINK_TRACK_MAX_CAPACITY.  The
 *   caller owns state[n_seq][that many bytes], zeroed before the first call (all zero = no tracks, id_count 0).  Layout of one
 *   sequence: int32 header[8] = n_tracks, id_count, status, capacity, 4 x reserved; then the track list, then a second list of
 *   the same shape which a call builds the new list in before it replaces the first (what a caller reads is always the first).
 *   One list of K = capacity tracks: ct double[K][2], tracking double[K][2], label int32[K] (tracking label), tracking_id
 *   int32[K], age int32[K], active int32[K], src int32[K] (the detection slot, -1 for a track carried over without one).
 *
 * link_track_step: advances n_seq independent sequences by one frame.  boxes float[n_seq, n, box_len], box_len 6..64: centre in
 *   columns 0..2, velocity in columns box_len - 3 and box_len - 2 (6 and 7 of a 9-wide box); scores float[n_seq, n]; labels
 *   int32 or int64 [n_seq, n] (labels_int64), -1 (or anything outside the label table) an unused slot; counts int32[n_seq]
 *   (nullable: only the labels mark unused slots); time_lag double[n_seq]; reset uint8[n_seq] (nullable); pose double[n_seq, 12]
 *   (nullable): the row-major 3 x 4 lidar-to-global transform.  All on the device.
 *   The steps, in this arithmetic:
 *    1. reset[s] clears the list and id_count before the frame (PubTracker.reset).
 *    2. A frame with no detection of a tracked class -- none at all, or only untracked ones -- clears the list, returns nothing
 *       and keeps id_count (pub_tracker.py:50-52; for untracked-only frames the reference raises an IndexError at :71 -- a
 *       deliberate difference).
 *    3. Detections whose label maps to -1 are removed; the order of the rest is kept (:55-63).
 *    4. With a pose, in double: ct = ((r0 x + r1 y) + r2 z) + t per row, velocity = (r0 vx + r1 vy) per row; without, the doubles
 *       of the floats.
 *    5. tracking = velocity * -1 * time_lag in double (:61).
 *    6. The matched position is float(ct + double(float(tracking))) (:71-74); 7. a track's centre is float(ct) (:84-85).
 *    8. dist = sqrt(dx dx + dy dy) in float, every operation rounded on its own, the root correctly rounded (:88-90).
 *    9. A pair is invalid when dist > max_dist[label of the detection] (strictly) or the labels differ (:92-93).
 *   10. Greedy scan in detection order; a detection takes the first minimum among the valid free tracks (track_utils.py:7-11).
 *   11. The new list: matched detections in detection order (the track's id, age 1, active + 1; :123-128), unmatched detections
 *       in detection order (id = ++id_count, age 1, active 1; with a score threshold only those with score > threshold,
 *       tracker.py:113), unmatched old tracks with age < max_age in their old order (age + 1, active 0, ct -= tracking: the move
 *       forward ignores the present time lag; tracking unchanged; :140-151).  12. A carried-over track that matches later gets
 *       active 1.
 *   Out: det_tracking_id int32[n_seq, n] (-1: filtered, dropped or unused), det_active int32[n_seq, n] (0 there), and the state.
 *   status bit 0 (LINK_TRACK_STATUS_OVERFLOW, rewritten by every call): the new list had more than capacity entries; its tail
 *   was dropped, which is carried-over tracks only since n <= capacity.  Non-finite centres or velocities: unspecified matches.
 *   LINK_ERR_ARG: a null pointer, n > capacity, capacity or a table size out of range, a label_map entry outside
 *   -1 .. n_track_labels - 1, a max_dist that is negative, NaN or >= 1e16 (the reference's "no match" sentinel), max_age < 0.
 * ============================================================================================= */
#define LINK_TRACK_MAX_LABELS 32
#define LINK_TRACK_MAX_CAPACITY 1024
#define LINK_TRACK_STATUS_OVERFLOW 1
typedef struct {
  int32_t n_det_labels, n_track_labels, max_age, capacity;
  float score_thresh; /* NaN: no threshold (the nuScenes form) */
  int32_t reserved;
  int32_t label_map[LINK_TRACK_MAX_LABELS]; /* detection label -> tracking label, -1 = not tracked */
  float max_dist[LINK_TRACK_MAX_LABELS];    /* per tracking label */
} link_track_cfg_t;
size_t link_track_state_bytes(int32_t capacity);
int link_track_step(const link_track_cfg_t *cfg /* host */, int32_t n_seq, int32_t n, int32_t box_len, const float *boxes,
                    const float *scores, const void *labels, int32_t labels_int64, const int32_t *counts /* nullable */,
                    const double *time_lag, const uint8_t *reset /* nullable */, const double *pose /* nullable */, void *state,
                    int32_t *det_tracking_id, int32_t *det_active, void *stream);

/* =============================================================================================
 * R. Deformable convolution, DCN v1 (csrc/dcn.hip): forward, grad_input + grad_offset, grad_weight
 *
 * The DeformConv of detection/det3d/ops/dcn (deform_conv.py:14-112 over src/deform_conv_cuda.cpp and
 * src/deform_conv_cuda_kernel.cu), which CenterHead(dcn_head=True) builds its FeatureAdaption modules on
 * (models/bbox_heads/center_head.py:27-65).  Additive entries: the ABI version does not move.  Modulated (v2) convolution and
 * deformable ROI pooling are not built.
 *
 * input [B, C, H, W], offset [B, dg 2 kh kw, Ho, Wo] (channel 2 (i kw + j) of deformable group g is the row offset of tap (i, j),
 * the next one its column offset), weight [O, C, kh, kw], output [B, O, Ho, Wo], all contiguous, no bias;
 * Ho = (H + 2 pad_h - (dil_h (kh - 1) + 1)) / stride_h + 1, Wo likewise.  For output pixel (ho, wo), tap (i, j) and input channel c
 * of deformable group g = c / (C / dg): h = ho stride_h - pad_h + i dil_h + dh, w = wo stride_w - pad_w + j dil_w + dw; the sample
 * is the bilinear value at (h, w) with floor for the low corner, a corner off the map counting 0, and a sample that fails
 * h > -1 && w > -1 && h < H && w < W counting 0 (deformable_im2col_gpu_kernel, deform_conv_cuda_kernel.cu:191).  The output is
 * the sum over c, i, j of weight[o, c, i, j] sample.  A deliberate difference: the range test is made on the float value before any
 * conversion to an index, so a NaN, an infinity or an offset no int holds contributes exactly 0, receives a zero offset gradient
 * and scatters nothing (the reference's backward converts such a value to int, which is undefined).
 *
 * No column matrix is written to memory: the columns are sampled into LDS and multiplied on the matrix cores with the exact
 * f32-input instruction, accumulating in fp32.  LINK_DCN_RELU applies max(x, 0) to the output and, in the two backward entries,
 * masks grad_out where output <= 0 (they then read `output`, which may be null otherwise).  io_dtype: the forward entry takes
 * LINK_IO_F32 / LINK_IO_F16 / LINK_IO_BF16 tensors (all four in that type, widened on load, rounded to nearest even on store;
 * coordinates, samples and sums are fp32); the backward entries are fp32 only (LINK_ERR_ARG otherwise; the Python layer widens).
 *
 * Every entry launches on the caller's stream, allocates nothing, reads nothing back and keeps no state: a call can be captured
 * in a graph.  grad_offset and grad_weight are reproducible run to run (fixed summation order; grad_weight goes through
 * per-wave partials in the workspace and one fixed-order reduce).  grad_input is zeroed by the call (hipMemsetAsync on the stream)
 * and summed with no-return fp32 atomics, so its last bits depend on the order in which the adds arrive.
 *
 * Envelope: groups == 1, kh kw <= LINK_DCN_MAX_TAPS, C and O <= LINK_DCN_MAX_CHANNELS, deformable_groups dividing C (any channel
 * count per group: chunks are padded inside LDS), stride and dilation >= 1, padding >= 0, Ho and Wo >= 1, every tensor at most
 * 2^31 elements, offset_channels == dg 2 kh kw.  Outside it, or with a null pointer: LINK_ERR_ARG before anything touches a device
 * (link_deform_conv_workspace_bytes: 0).  grad_input or grad_offset may be null (not both): that gradient is not computed.
 * LINK_ERR_WORKSPACE for fewer workspace bytes than the size helper names.
 *
 * link_deform_conv_forward          replaces deform_conv_forward_cuda (deform_conv_cuda.cpp:152)
 * link_deform_conv_backward_data    replaces deform_conv_backward_input_cuda (:262; deformable_col2im_gpu_kernel and
 *                                   deformable_col2im_coord_gpu_kernel with get_coordinate_weight, deform_conv_cuda_kernel.cu:280, 374, 146)
 * link_deform_conv_backward_weight  replaces deform_conv_backward_parameters_cuda (:376)
 * ============================================================================================= */
#define LINK_DCN_MAX_TAPS 49
#define LINK_DCN_MAX_CHANNELS 256
#define LINK_DCN_RELU 1
typedef struct {
  int32_t batch, c, h, w, o, kh, kw;
  int32_t stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  int32_t groups, deformable_groups, offset_channels;
  int32_t io_dtype; /* LINK_IO_* */
  int32_t flags;    /* LINK_DCN_RELU */
} link_deform_conv_geom_t;            /* link_abi_struct_size(14) */
size_t link_deform_conv_workspace_bytes(const link_deform_conv_geom_t *geom);
int link_deform_conv_forward(const link_deform_conv_geom_t *geom, const void *input, const void *offset, const void *weight,
                             void *output, void *stream);
int link_deform_conv_backward_data(const link_deform_conv_geom_t *geom, const float *input, const float *offset,
                                   const float *weight, const float *output /* nullable without LINK_DCN_RELU */,
                                   const float *grad_out, float *grad_input /* nullable */, float *grad_offset /* nullable */,
                                   void *stream);
int link_deform_conv_backward_weight(const link_deform_conv_geom_t *geom, const float *input, const float *offset,
                                     const float *output /* nullable without LINK_DCN_RELU */, const float *grad_out,
                                     float *grad_weight, void *workspace, size_t workspace_bytes, void *stream);

/* =============================================================================================
 * Section S: the PointPillars reader and its BEV scatter (csrc/pillar.hip)
 * Reference: detection/det3d/models/readers/pillar_encoder.py.
 *
 * voxels [P, T, D] fp32 are the padded pillars (x, y, z first), num_points int32 [P], coors int32 [P, 4] = b, z, y, x.  A pillar's
 * row t < num = clamp(num_points[p], 0, T) is decorated to K1 = D + 5 (+ 1) values: the D raw ones, xyz minus the pillar's mean,
 * x - (coors[p][3] vx + x_offset), y - (coors[p][2] vy + y_offset) and, with_distance, |xyz|; x_offset = vx / 2 + x_min as the
 * reference's constructor forms it.  Each PFN layer is a bias-free linear map, BatchNorm in eval mode as a per-channel affine
 * (scale = gamma / sqrt(var + eps), shift = beta - mean scale, formed inside the kernel from the module's own five tensors -- no
 * folded copy of the parameters exists anywhere) applied AFTER the dot product, ReLU and a max over ALL T rows.  A
 * layer that is not the last has width / 2 units and hands [x, x_max repeated] to the next one.
 *
 * Mean contract: the mean is the sum over rows t < num divided by num.  The reference sums all T rows; the two agree because
 * padded input rows are zero, as every voxel generator of this library and of the reference writes them.  Rows t >= num are
 * never read.  (The sum is formed as row 0 plus the summed offsets from row 0 over num: the same number, fewer lost bits.)
 * Padded rows: the reference masks them to zero and still runs them through the layers, so they leave layer 1 as relu(shift1) and
 * take part in the max.  All padded rows of a pillar are equal in both layers; one representative is evaluated where num < T.
 * num == 0 (the reference divides 0 by 0 there and returns NaN) gives the value of an all-padded pillar: no NaN.
 * count (nullable): a device int32; pillars p >= min(max(*count, 0), P) are inert: nothing of them is read but nothing is computed
 * or written (link_pillar_gather and link_pillar_decorate write zeros for them).  voxel_offsets + B of link_voxelize is one.
 * A pillar whose (b, y, x) lies outside (batch, ny, nx) writes nothing to a canvas and gathers zero.  Duplicate (b, y, x) among
 * the live pillars make the canvas depend on the order of the writes (as in the reference); the voxelisers produce none.
 *
 * io_dtype is the type of rows and canvas: LINK_IO_F32 / F16 / BF16.  The reader computes in fp32 and rounds once at the store.
 * The canvas entries zero-fill the canvas themselves (hipMemsetAsync on the stream) and use no atomics: every result is
 * reproducible bit for bit, and the reader's canvas form equals link_pillar_scatter of its row form bit for bit.
 * Every entry launches on the caller's stream, allocates nothing, reads nothing back and keeps no state (graph capture is fine).
 *
 * Native range of the reader (link_pillar_native; LINK_ERR_ARG outside it): 1 or 2 layers, every width a multiple of 16 up to
 * LINK_PILLAR_MAX_WIDTH, 3 <= D <= LINK_PILLAR_MAX_D, 1 <= T <= LINK_PILLAR_MAX_T.  struct_bytes = sizeof(link_pillar_geom_t)
 * (checked by every entry: the layout has no id in link_abi_struct_size).  Every entry: n_pillars <= 2^31, the canvas at most 2^40
 * elements with ny nx <= 2^31; scatter, gather and decorate also n_pillars channels (n_pillars t) <= 2^38.  LINK_ERR_ARG otherwise,
 * before anything is launched.
 *
 * link_pillar_reader    replaces PillarFeatureNet.forward (pillar_encoder.py:116-162) with PFNLayer.forward (:40-55) and, with
 *                       `canvas`, PointPillarsScatter.forward (:182-218) as well.  Exactly one of rows [P, C] / canvas
 *                       [batch, C, ny, nx] is non-null, C = width[layers - 1].  layer1.weight [U1, K1], layer2.weight
 *                       [width[1], 2 U1] row-major, U1 = width[0] / 2 with two layers, width[0] with one; gamma, beta,
 *                       running_mean, running_var one fp32 per unit.  layer2 may be null with one layer.
 * link_pillar_scatter   replaces PointPillarsScatter.forward (:182-218): zero-fill, then rows [P, channels] -> canvas
 * link_pillar_gather    its adjoint (what autograd derives from `canvas[:, indices] = voxels`, :208): rows <- grad_canvas
 * link_pillar_decorate  replaces the decoration and the mask of PillarFeatureNet.forward (:129-156) for the training path:
 *                       decorated [P, T, K1] fp32, rows t >= num and inert pillars zero.  Uses t, d, with_distance, vx .. y_offset.
 * ============================================================================================= */
#define LINK_PILLAR_MAX_T 64
#define LINK_PILLAR_MAX_D 8
#define LINK_PILLAR_MAX_WIDTH 128
typedef struct {
  int32_t struct_bytes;      /* sizeof(link_pillar_geom_t) */
  int32_t t, d;              /* rows per pillar, raw values per row */
  int32_t with_distance;
  int32_t layers;            /* 1 or 2 */
  int32_t width[2];          /* num_filters as configured */
  int32_t batch, ny, nx;     /* the canvas */
  int32_t io_dtype;          /* LINK_IO_*: rows and canvas */
  float vx, vy, x_offset, y_offset;
} link_pillar_geom_t;
typedef struct {
  const float *weight, *gamma, *beta, *running_mean, *running_var;   /* Linear.weight and the BatchNorm1d's tensors, on the device */
  float eps;
  int32_t reserved;
} link_pillar_layer_t;
int link_pillar_native(const link_pillar_geom_t *geom);   /* 1 inside the reader's native range, 0 outside */
int link_pillar_reader(const link_pillar_geom_t *geom, const float *voxels, const int32_t *num_points, const int32_t *coors,
                       int64_t n_pillars, const int32_t *count /* nullable */, const link_pillar_layer_t *layer1,
                       const link_pillar_layer_t *layer2 /* nullable with one layer */, void *rows, void *canvas, void *stream);
int link_pillar_scatter(const link_pillar_geom_t *geom, const void *rows, const int32_t *coors, int64_t n_pillars, int32_t channels,
                        const int32_t *count /* nullable */, void *canvas, void *stream);
int link_pillar_gather(const link_pillar_geom_t *geom, const void *grad_canvas, const int32_t *coors, int64_t n_pillars,
                       int32_t channels, const int32_t *count /* nullable */, void *grad_rows, void *stream);
int link_pillar_decorate(const link_pillar_geom_t *geom, const float *voxels, const int32_t *num_points, const int32_t *coors,
                         int64_t n_pillars, const int32_t *count /* nullable */, float *decorated, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LINK_AMD_H_ */
