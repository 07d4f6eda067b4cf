// link_amd/csrc/elk_host.h -- what elk_train.hip calls in elk.hip: the training form runs the forward's modulate + block-sum,
// block-gather and voxel kernels (instantiated in elk.hip only).  Internal to the library: hidden, not part of link_amd.h.
#pragma once
#include "common.h"

// Optional epilogue of the block gather: the finished row of block `b` goes straight to the rows of the block's voxels
// (perm[blk_start[b] .. blk_start[b + 1]) = their ids) instead of -- or besides -- the [M, P*C] table: what aux_to_voxel
// needs (utils.py:84, `new_feat[idx]`), without the table's round trip through memory and the row-gather launch.
struct bg_scatter_t {
  const int32_t *blk_start;
  const int32_t *perm;
  float *out;                                          // nullptr: no scatter
};

namespace link {
#pragma GCC visibility push(hidden)

int check_desc(const link_elk_desc_t *d);

// modulate + block sums on the group kernels; false: not a group-kernel shape (the caller falls back or refuses).
// op >= 0 overrides d->op (the backward forms LINK_OPI_*, elk_common.h); row_den: rows divided by these denominators.
bool modsum_group_path(const link_elk_desc_t *d, hipStream_t st, const float *fin, const int4 *vox, const float *w_pos,
                       const float *alpha, const int32_t *blk_start, const int32_t *hdr, float *S_, int64_t m_cap,
                       int op = -1, const float *row_den = nullptr);

// flags bit0: transposed neighbourhood, bit1: plain sum (k_block_gather_g); den_out: the denominators, may be NULL
int block_gather_impl(const float *S_, const int32_t *blk_coords, const int32_t *cell_blk, const link_grid_t *grid,
                      const int32_t *hdr, const link_elk_desc_t *desc, int64_t m_cap, float *A, int flags, float *den_out,
                      void *stream, const bg_scatter_t &sc = bg_scatter_t{nullptr, nullptr, nullptr});

// ln_w == NULL: no LayerNorm (the training forward, whose LayerNorm is differentiated by the host)
int voxel_demod_impl(const float *A, const float *fin, const int32_t *vox_sorted, const int32_t *pos_blk,
                     const float *w_pos, const float *alpha, const float *ln_w, const float *ln_b, const int32_t *hdr,
                     const link_elk_desc_t *desc, int64_t n, float *out, void *stream);

#pragma GCC visibility pop
}  // namespace link
