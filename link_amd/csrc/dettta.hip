// link_amd/csrc/dettta.hip -- CenterHead test-time augmentation on the device (section N of include/link_amd.h): the four flipped
// (and rotated) views of a batch of point clouds, the decode of the head's maps of those four views fused with the flips back and
// the average, the class-wise NMS suppression mask that merges rotated passes, and the rotation of the kept boxes back.
//
// Semantics: detection/det3d/datasets/pipelines/test_aug.py:12-32 (DoubleFlip) and preprocess.py:153-156 over
// core/bbox/box_np_ops.py:182-204 (rotation_points_single_angle) for the views; detection/det3d/models/bbox_heads/center_head.py:
// 320-421 and the masks of :461-467 for the decode, :489-503 for the rotation back; detection/nms_better2.py:266-297 for the merge
// (one rotate_nms_pcdet per class with that class's threshold).  The implementation is this project's.
//
// Contraction is off (box_iou.h): the reference forms x c + y s from rounded products, and so do the rotations here.
#pragma clang fp contract(off)
#include <math.h>

#include "box_iou.h"

using namespace link;

namespace {

// ---- views ----------------------------------------------------------------------------------------------------------------------
// One lane per float of the packed [n, C] source: the source is read once (a lane of column 0 or 1 of a rotated cloud also reads
// its neighbour column, which lies in the same cache line), and the lane writes its float to the same place of the four views,
// so every view is written in the order the source is read: four coalesced streams.  View v of cloud b starts at row
// 4 off[b] + v n_b (frame-major, view-minor: the order collate_kitti gives the four bundles and center_head.py:332 reshapes by).
// The first 4 B + 1 lanes also write the offsets of the 4 B clouds.
template <bool ROT>
__global__ __launch_bounds__(256) void k_tta_views(const float *__restrict__ pts, const int32_t *__restrict__ off, int B, int64_t n, int C,
                                                   float cs, float sn, float *__restrict__ out, int32_t *__restrict__ out_off) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid <= 4 * (int64_t)B) {
    const int b = (int)(gid >> 2), v = (int)(gid & 3);
    if (b == B) {
      int64_t t = off[B];
      t = t < 0 ? 0 : (t > n ? n : t);
      out_off[gid] = (int32_t)(4 * t);
    } else {
      const int64_t o = off[b], nb = (int64_t)off[b + 1] - o;
      out_off[gid] = (int32_t)(4 * o + v * nb);
    }
  }
  if (gid >= n * C) return;
  const int64_t p = gid / C;
  const int c = (int)(gid - p * C);
  int lo = 0, hi = B;                          // the cloud of point p: the last b with off[b] <= p
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)off[mid] <= p) lo = mid; else hi = mid;
  }
  const int64_t o = off[lo], nb = (int64_t)off[lo + 1] - o;
  if (o < 0 || nb <= 0 || p < o || p >= o + nb || o + nb > n) return;          // offsets that do not describe n rows write nothing
  float v = pts[gid];
  if (ROT && c < 2) {                          // box_np_ops.py:192-195, 204: [x, y, z] @ [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    const float x = pts[p * C], y = pts[p * C + 1];
    v = c == 0 ? x * cs + y * sn : x * (-sn) + y * cs;
  }
  const int64_t r0 = 4 * o + (p - o);
  out[r0 * C + c] = v;
  out[(r0 + nb) * C + c] = c == 1 ? -v : v;                                    // test_aug.py:14-15
  out[(r0 + 2 * nb) * C + c] = c == 0 ? -v : v;                                // :20-21
  out[(r0 + 3 * nb) * C + c] = c < 2 ? -v : v;                                 // :26-28
}

// ---- decode ---------------------------------------------------------------------------------------------------------------------
// The mean of the four views: ((v0 + v1) + v2) + v3, then * 0.25 (exact: a power of two) -- the views in ascending order, which
// is also the order a sequential sum over dim 1 of the reference's [B, 4, H, W, C] tensor takes.
__device__ __forceinline__ float mean4(float a, float b, float c, float d) { return (((a + b) + c) + d) * 0.25f; }

// center_head.py:320-421 + the masks of :461-467, one lane per cell of one frame's H x W map.  The maps are NCHW with batch 4 B,
// read in place: cell (h, w) reads view 1 at (H-1-h, w), view 2 at (h, W-1-w), view 3 at (H-1-h, W-1-w) (:333-335).  A wave's 64
// consecutive cells are 64 consecutive floats of a channel row in every view, ascending in views 0 and 1 and descending in 2 and
// 3: the same cache lines either way, so the mirrored loads coalesce like the straight ones and nothing is staged or reversed.
template <bool VEL>
__global__ __launch_bounds__(256) void k_center_decode_flip4(const float *__restrict__ hm, const float *__restrict__ reg,
                                                             const float *__restrict__ height, const float *__restrict__ dim,
                                                             const float *__restrict__ rot, const float *__restrict__ vel, int K, int H, int W,
                                                             decode_geom g, float *__restrict__ boxes, int32_t *__restrict__ labels,
                                                             float *__restrict__ scores) {
  const int hw = H * W, cell = blockIdx.x * 256 + threadIdx.x, bi = blockIdx.y;
  if (cell >= hw) return;
  const int wq = cell % W, hq = cell / W;
  const int c1 = (H - 1 - hq) * W + wq, c2 = hq * W + (W - 1 - wq), c3 = (H - 1 - hq) * W + (W - 1 - wq);
  const int64_t m0 = (int64_t)bi * 4;          // the frame's first map
  // channel c of an [4 B, C, H, W] map in the four views
#define LINK_TTA_LOAD4(ptr, C, c, a0, a1, a2, a3)                                       \
  const float a0 = ptr[((m0 + 0) * (C) + (c)) * hw + cell], a1 = ptr[((m0 + 1) * (C) + (c)) * hw + c1], \
              a2 = ptr[((m0 + 2) * (C) + (c)) * hw + c2], a3 = ptr[((m0 + 3) * (C) + (c)) * hw + c3];
  float best = 0.f;
  int label = 0;
  for (int k = 0; k < K; k++) {                // the sigmoid per view, then the mean (:344, 354)
    LINK_TTA_LOAD4(hm, K, k, h0, h1, h2, h3)
    const float s = mean4(1.f / (1.f + expf(-h0)), 1.f / (1.f + expf(-h1)), 1.f / (1.f + expf(-h2)), 1.f / (1.f + expf(-h3)));
    if (k == 0 || s > best) { best = s; label = k; }
  }
  LINK_TTA_LOAD4(reg, 2, 0, rx0, rx1, rx2, rx3)
  LINK_TTA_LOAD4(reg, 2, 1, ry0, ry1, ry2, ry3)
  const float rx = mean4(rx0, rx1, 1.f - rx2, 1.f - rx3), ry = mean4(ry0, 1.f - ry1, ry2, 1.f - ry3);       // :359-364
  float xs = (float)wq + rx, ys = (float)hq + ry;
  xs = xs * g.osf * g.vx + g.px;
  ys = ys * g.osf * g.vy + g.py;
  LINK_TTA_LOAD4(height, 1, 0, z0, z1, z2, z3)
  const float z = mean4(z0, z1, z2, z3);
  constexpr int C = VEL ? 9 : 7;
  const int64_t f = (int64_t)bi * hw;
  float *o = boxes + (f + cell) * C;
  o[0] = xs; o[1] = ys; o[2] = z;
#pragma unroll
  for (int d = 0; d < 3; d++) {                // the exp per view, then the mean (:346, 356)
    LINK_TTA_LOAD4(dim, 3, d, d0, d1, d2, d3)
    o[3 + d] = mean4(expf(d0), expf(d1), expf(d2), expf(d3));
  }
  if (VEL) {                                   // :410-416
    LINK_TTA_LOAD4(vel, 2, 0, vx0, vx1, vx2, vx3)
    LINK_TTA_LOAD4(vel, 2, 1, vy0, vy1, vy2, vy3)
    o[6] = mean4(vx0, vx1, -vx2, -vx3);
    o[7] = mean4(vy0, -vy1, vy2, -vy3);
  }
  LINK_TTA_LOAD4(rot, 2, 0, s0, s1, s2, s3)
  LINK_TTA_LOAD4(rot, 2, 1, q0, q1, q2, q3)
  o[C - 1] = atan2f(mean4(s0, s1, -s2, -s3), mean4(q0, -q1, q2, -q3));                                      // :370-384
#undef LINK_TTA_LOAD4
  const bool ok = best > g.thr && xs >= g.lo[0] && ys >= g.lo[1] && z >= g.lo[2] && xs <= g.hi[0] && ys <= g.hi[1] && z <= g.hi[2];
  labels[f + cell] = label;
  scores[f + cell] = ok ? best : -INFINITY;
}

// unmasked cells per frame (box_iou.h)
__global__ __launch_bounds__(256) void k_tta_count(const float *__restrict__ scores, int hw, int32_t *__restrict__ counts) {
  center_count_frame(scores, hw, counts);
}

// ---- class-wise mask ------------------------------------------------------------------------------------------------------------
// The words of k_nms_mask (boxnms.hip) with the predicate label[i] == label[j] && IoU > thr[label[i]].  The labels of the tile's
// rows and columns are staged first: a tile whose rows and columns share no class writes its zero words and leaves before any
// box is staged (the staging is where the double-precision trigonometry is).  A label outside [0, num_cls) never matches.
__global__ __launch_bounds__(256) void k_nms_mask_classwise(const float *__restrict__ boxes, const int32_t *__restrict__ labels, int cap,
                                                            const int32_t *__restrict__ n_dev, const float *__restrict__ thr, int num_cls,
                                                            unsigned long long *__restrict__ mask) {
  __shared__ float sr[NF][64];
  __shared__ float sc[NF][64];
  __shared__ int lr[64], lc[64];
  __shared__ int shared_class;
  const int rb = blockIdx.y, cb = blockIdx.x;
  if (rb > cb) return;
  const int n = device_count(n_dev, cap);
  if (cb * 64 >= n) return;
  const int stride = (cap + 63) / 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < 64) {
    const int i = rb * 64 + tid;
    const int l = i < n ? labels[i] : -1;
    lr[tid] = l >= 0 && l < num_cls ? l : -1;
  } else if (tid < 128) {
    const int t = tid - 64, j = cb * 64 + t;
    const int l = j < n ? labels[j] : -1;
    lc[t] = l >= 0 && l < num_cls ? l : -2;
  } else if (tid == 128) {
    shared_class = 0;
  }
  __syncthreads();
  if (tid < 64) {
    const int mine = lc[tid];
    bool hit = false;
    for (int r = 0; r < 64; r++) hit |= lr[r] == mine;
    if (hit) shared_class = 1;                 // every writer writes the same value
  }
  __syncthreads();
  if (!shared_class) {
    if (tid < 64 && rb * 64 + tid < n) mask[(int64_t)(rb * 64 + tid) * stride + cb] = 0ull;
    return;
  }
  if (tid < 64) {
    if (rb * 64 + tid < n) stage_box<64, true>(boxes + (int64_t)(rb * 64 + tid) * 7, sr, tid);
  } else if (tid < 128) {
    const int t = tid - 64;
    if (cb * 64 + t < n) stage_box<64, true>(boxes + (int64_t)(cb * 64 + t) * 7, sc, t);
    else {
#pragma unroll
      for (int f = 0; f < NF; f++) sc[f][t] = 0.f;
    }
  }
  __syncthreads();
  const int j = cb * 64 + lane;
  const Rec B = load_box<64, true>(sc, lane);
  const int lb = lc[lane];
  for (int r = 0; r < 16; r++) {
    const int il = w * 16 + r, i = rb * 64 + il;
    if (i >= n) break;
    const int la = lr[il];                     // uniform over the wave
    bool p = false;
    if (la == lb && j < n && (rb != cb || lane > il)) {
      const Rec A = load_box<64, true>(sr, il);
      p = iou_from_overlap(A, B, box_overlap(A, B)) > thr[la];
    }
    const unsigned long long word = __ballot(p);
    if (lane == 0) mask[(int64_t)i * stride + cb] = word;
  }
}

// ---- rotation back --------------------------------------------------------------------------------------------------------------
// center_head.py:489-503 on the selected rows, fused with the gather that selects them: out[j] = boxes[idx[j]] (idx == NULL: row
// j) with centre and velocity pair rotated by the fp32 matrix of (cs, sn) = cos / sin of the angle and the angle added to the
// heading; a negative index, or one past n_src, leaves a row of zeros (an unused slot of a padded result).  One lane per row.
template <int C, bool ROT>
__global__ __launch_bounds__(256) void k_tta_rotate_back(const float *__restrict__ boxes, int64_t n_src, const long long *__restrict__ idx,
                                                         int64_t m, float cs, float sn, float angle, float *__restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const int64_t src = idx ? (int64_t)idx[j] : j;
  float v[C];
  if (src < 0 || src >= n_src) {
#pragma unroll
    for (int c = 0; c < C; c++) v[c] = 0.f;
  } else {
#pragma unroll
    for (int c = 0; c < C; c++) v[c] = boxes[src * C + c];
    if (ROT) {
      const float x = v[0], y = v[1];
      v[0] = x * cs + y * sn; v[1] = x * (-sn) + y * cs;
      if (C == 9) {
        const float vx = v[6], vy = v[7];
        v[6] = vx * cs + vy * sn; v[7] = vx * (-sn) + vy * cs;
      }
      v[C - 1] = v[C - 1] + angle;
    }
  }
#pragma unroll
  for (int c = 0; c < C; c++) out[j * C + c] = v[c];
}

constexpr int64_t MAX_BOXES = 65535LL * 16;              // the limit of section I's masks
constexpr int64_t MAX_VIEW_POINTS = (1LL << 29) - 1;     // 4 n stays an int32 offset

}  // namespace

extern "C" int link_tta_views(const float *points, const int32_t *point_offsets, int32_t batch, int64_t n, int32_t ndim, float cos_a,
                              float sin_a, float *out, int32_t *out_offsets, void *stream) {
  if (batch < 1 || batch > 16383 || n < 0 || n > MAX_VIEW_POINTS || ndim < 3 || ndim > 16) return LINK_ERR_ARG;
  if (!isfinite(cos_a) || !isfinite(sin_a)) return LINK_ERR_ARG;
  if (!point_offsets || !out_offsets || (n > 0 && (!points || !out))) return LINK_ERR_ARG;
  const int64_t lanes = n * ndim > 4 * (int64_t)batch + 1 ? n * ndim : 4 * (int64_t)batch + 1;
  const dim3 grid(blocks_for(lanes, 256)), block(256);
  if (cos_a == 1.f && sin_a == 0.f)            // angle 0: the views are copies, bit for bit
    hipLaunchKernelGGL(k_tta_views<false>, grid, block, 0, S(stream), points, point_offsets, (int)batch, n, (int)ndim, cos_a, sin_a, out,
                       out_offsets);
  else
    hipLaunchKernelGGL(k_tta_views<true>, grid, block, 0, S(stream), points, point_offsets, (int)batch, n, (int)ndim, cos_a, sin_a, out,
                       out_offsets);
  return check_launch("link_tta_views");
}

extern "C" int link_center_decode_flip4(const float *hm, const float *reg, const float *height, const float *dim, const float *rot,
                                        const float *vel, int32_t frames, int32_t num_cls, int32_t h, int32_t w, const link_center_geom_t *geom,
                                        float *boxes, int32_t *labels, float *scores, int32_t *counts, void *stream) {
  if (frames < 0 || num_cls < 1 || h < 0 || w < 0 || !geom || (int64_t)frames * 4 > 65535) return LINK_ERR_ARG;
  if ((int64_t)h * w >= (1LL << 24)) return LINK_ERR_ARG;
  if (!isfinite(geom->score_threshold) || !isfinite(geom->out_size_factor)) return LINK_ERR_ARG;
  for (int d = 0; d < 2; d++)
    if (!isfinite(geom->voxel_size[d]) || !isfinite(geom->pc_range[d])) return LINK_ERR_ARG;
  for (int d = 0; d < 6; d++)
    if (isnan(geom->post_center_range[d])) return LINK_ERR_ARG;
  if (frames == 0 || h * w == 0) return LINK_OK;
  if (!hm || !reg || !height || !dim || !rot || !boxes || !labels || !scores || !counts) return LINK_ERR_ARG;
  decode_geom g;
  g.osf = geom->out_size_factor; g.vx = geom->voxel_size[0]; g.vy = geom->voxel_size[1];
  g.px = geom->pc_range[0]; g.py = geom->pc_range[1]; g.thr = geom->score_threshold;
  for (int d = 0; d < 3; d++) { g.lo[d] = geom->post_center_range[d]; g.hi[d] = geom->post_center_range[3 + d]; }
  const dim3 grid(blocks_for((int64_t)h * w, 256), frames), block(256);
  if (vel) hipLaunchKernelGGL(k_center_decode_flip4<true>, grid, block, 0, S(stream), hm, reg, height, dim, rot, vel, (int)num_cls, (int)h,
                              (int)w, g, boxes, labels, scores);
  else hipLaunchKernelGGL(k_center_decode_flip4<false>, grid, block, 0, S(stream), hm, reg, height, dim, rot, vel, (int)num_cls, (int)h,
                          (int)w, g, boxes, labels, scores);
  int rc = check_launch("link_center_decode_flip4");
  if (rc != LINK_OK) return rc;
  hipLaunchKernelGGL(k_tta_count, dim3(frames), dim3(256), 0, S(stream), scores, h * w, counts);
  return check_launch("link_center_decode_flip4");
}

extern "C" int link_nms_mask_classwise(const float *boxes, const int32_t *labels, int64_t cap, const int32_t *n_dev, const float *thr,
                                       int32_t num_cls, uint64_t *mask, void *stream) {
  if (cap < 0 || cap > MAX_BOXES || num_cls < 1) return LINK_ERR_ARG;
  if (cap == 0) return LINK_OK;
  if (!boxes || !labels || !thr || !mask) return LINK_ERR_ARG;
  const dim3 grid(blocks_for(cap, 64), blocks_for(cap, 64)), block(256);
  hipLaunchKernelGGL(k_nms_mask_classwise, grid, block, 0, S(stream), boxes, labels, (int)cap, n_dev, thr, (int)num_cls,
                     reinterpret_cast<unsigned long long *>(mask));
  return check_launch("link_nms_mask_classwise");
}

extern "C" int link_tta_rotate_back(const float *boxes, int64_t n_src, int32_t ncol, const int64_t *idx, int64_t m, float cos_a, float sin_a,
                                    float angle, float *out, void *stream) {
  if ((ncol != 7 && ncol != 9) || n_src < 0 || m < 0 || m > (1LL << 31) - 256) return LINK_ERR_ARG;
  if (!isfinite(cos_a) || !isfinite(sin_a) || !isfinite(angle)) return LINK_ERR_ARG;
  if (m == 0) return LINK_OK;
  if (!out || (n_src > 0 && !boxes)) return LINK_ERR_ARG;
  const dim3 grid(blocks_for(m, 256)), block(256);
  const long long *ix = reinterpret_cast<const long long *>(idx);
  const bool rotate = angle != 0.f;
#define LINK_TTA_BACK(C, R) \
  hipLaunchKernelGGL((k_tta_rotate_back<C, R>), grid, block, 0, S(stream), boxes, n_src, ix, m, cos_a, sin_a, angle, out)
  if (ncol == 7) { if (rotate) LINK_TTA_BACK(7, true); else LINK_TTA_BACK(7, false); }
  else { if (rotate) LINK_TTA_BACK(9, true); else LINK_TTA_BACK(9, false); }
#undef LINK_TTA_BACK
  return check_launch("link_tta_rotate_back");
}
