// link_amd/csrc/boxnms.hip -- detection post-processing on the device (section I of include/link_amd.h): rotated BEV overlap / IoU
// of box pairs, the NMS suppression mask for three predicates, the greedy scan over that mask, and the CenterHead decode.
//
// Semantics: detection/det3d/ops/iou3d_nms/src/iou3d_nms_kernel.cu:35-234 (overlap of two rotated rectangles: edge crossings,
// corners inside with a 1e-2 margin, centroid, angular order, fan area), :267-372 (mask), iou3d_nms.cpp:116-132 (greedy scan),
// detection/det3d/core/utils/circle_nms_jit.py:23-27 (centre-distance predicate), detection/det3d/models/bbox_heads/
// center_head.py:344-421,461-467 (decode).  The implementation is this project's: one lane per pair with the wave's 64 lanes on 64
// boxes of the b / column tile and the a / row box uniform per wave, so a mask word is one ballot; boxes are staged in LDS with
// their corners and trigonometry worked out once per box, not once per pair; the point list lives in registers (every index is a
// compile-time constant after unrolling) and holds 24 points -- the reference's 16 overflow when the margin admits corners next
// to 8 crossings; the greedy scan runs in one workgroup on the device, so nothing is copied to the host.
//
// The reference rounds every product and sum on its own (nvcc contracts a * b + c, the host compiler of the CPU twin does not; the
// twin is what the fixtures pin), and the strict inequalities s1 * s2 > 0 and |rot| < half + margin decide which points exist:
// contraction is off for this whole translation unit.
#pragma clang fp contract(off)
#include <math.h>

#include "box_iou.h"

using namespace link;

namespace {

constexpr int REDUCE_WORDS = 64;      // remv words the scan holds at a time: one per lane of a wave

__device__ __forceinline__ float iou_normal(const Rec &a, const Rec &b) {                          // :314-325
  const float left = fmaxf(a.x - a.dx / 2, b.x - b.dx / 2), right = fminf(a.x + a.dx / 2, b.x + b.dx / 2);
  const float top = fmaxf(a.y - a.dy / 2, b.y - b.dy / 2), bottom = fminf(a.y + a.dy / 2, b.y + b.dy / 2);
  const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
  const float inter = width * height;
  return inter / fmaxf(a.area + b.area - inter, BOX_EPS);
}

template <int PRED>
__device__ __forceinline__ bool suppresses(const Rec &A, const Rec &B, float thr) {
  if (PRED == LINK_NMS_ROTATE) return iou_from_overlap(A, B, box_overlap(A, B)) > thr;
  if (PRED == LINK_NMS_NORMAL) return iou_normal(A, B) > thr;
  const float ddx = A.x - B.x, ddy = A.y - B.y;                                                    // circle_nms_jit.py:23-26
  return ddx * ddx + ddy * ddy <= thr;
}

// out[i, j] for a tile of 16 a x 64 b: lane = b box, each of the four waves takes four a boxes in turn
constexpr int PAIR_ROWS = 16;
template <bool IOU>
__global__ __launch_bounds__(256) void k_boxes_pair(const float *__restrict__ a, int na, const float *__restrict__ b, int nb,
                                                    float *__restrict__ out) {
  __shared__ float sb[NF][64];
  __shared__ float sa[NF][PAIR_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b0 = blockIdx.x * 64, a0 = blockIdx.y * PAIR_ROWS;
  if (tid < 64) {
    if (b0 + tid < nb) stage_box<64, true>(b + (int64_t)(b0 + tid) * 7, sb, tid);
  } else if (tid < 64 + PAIR_ROWS) {
    if (a0 + tid - 64 < na) stage_box<PAIR_ROWS, true>(a + (int64_t)(a0 + tid - 64) * 7, sa, tid - 64);
  }
  __syncthreads();
  const int j = b0 + lane;
  if (j >= nb) return;
  const Rec B = load_box<64>(sb, lane);
  for (int r = 0; r < PAIR_ROWS / 4; r++) {
    const int il = w * (PAIR_ROWS / 4) + r, i = a0 + il;
    if (i >= na) break;
    const Rec A = load_box<PAIR_ROWS>(sa, il);
    const float ov = box_overlap(A, B);
    out[(int64_t)i * nb + j] = IOU ? iou_from_overlap(A, B, ov) : ov;
  }
}

// mask[i, cb] bit c = box i suppresses box cb * 64 + c (c > i inside the diagonal tile), for the tiles with cb >= rb that hold a
// box.  Lane = column box, each wave takes 16 row boxes in turn: a word is one ballot.
template <int PRED>
__global__ __launch_bounds__(256) void k_nms_mask(const float *__restrict__ boxes, int cap, const int32_t *__restrict__ n_dev, float thr,
                                                  unsigned long long *__restrict__ mask) {
  __shared__ float sr[NF][64];
  __shared__ float sc[NF][64];
  const int rb = blockIdx.y, cb = blockIdx.x;
  if (rb > cb) return;
  const int n = device_count(n_dev, cap);
  if (cb * 64 >= n) return;
  const int stride = (cap + 63) / 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  constexpr bool FULL = PRED == LINK_NMS_ROTATE;
  if (tid < 64) {
    if (rb * 64 + tid < n) stage_box<64, FULL>(boxes + (int64_t)(rb * 64 + tid) * 7, sr, tid);
  } else if (tid < 128) {
    const int t = tid - 64;
    if (cb * 64 + t < n) stage_box<64, FULL>(boxes + (int64_t)(cb * 64 + t) * 7, sc, t);
    else {
#pragma unroll
      for (int f = 0; f < NF; f++) sc[f][t] = 0.f;
    }
  }
  __syncthreads();
  const int j = cb * 64 + lane;
  const Rec B = load_box<64, FULL>(sc, lane);
  for (int r = 0; r < 16; r++) {
    const int il = w * 16 + r, i = rb * 64 + il;
    if (i >= n) break;
    const Rec A = load_box<64, FULL>(sr, il);
    const bool p = suppresses<PRED>(A, B, thr) && j < n && (rb != cb || lane > il);
    const unsigned long long word = __ballot(p);
    if (lane == 0) mask[(int64_t)i * stride + cb] = word;
  }
}

// iou3d_nms.cpp:116-132 in one workgroup of four waves.  The remv words of REDUCE_WORDS column blocks are held at a time, one per
// lane; for the next chunk they are rebuilt from the rows kept so far (read back from `keep`).  Per 64-box block: wave 0 walks
// the diagonal tile, lane i holding row i's word and the running remv word passing through readlane; then the kept rows' words
// of the later blocks of the chunk are ORed in, lanes on words and the four waves on a quarter of the rows each.
__global__ __launch_bounds__(256) void k_nms_reduce(const unsigned long long *__restrict__ mask, int cap, const int32_t *__restrict__ n_dev,
                                                    int post_max, long long *keep, int32_t *__restrict__ count) {
  __shared__ unsigned long long part[4][REDUCE_WORDS];
  __shared__ unsigned long long remv[REDUCE_WORDS];
  __shared__ unsigned long long s_kept;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = device_count(n_dev, cap);
  const int stride = (cap + 63) / 64, nblk = (n + 63) / 64;
  const int limit = post_max > 0 && post_max < cap ? post_max : cap;
  int cnt = 0;
  for (int c0 = 0; c0 < nblk && cnt < limit; c0 += REDUCE_WORDS) {
    const int j = c0 + lane;
    unsigned long long acc = 0;
    if (j < nblk)
      for (int k = w; k < cnt; k += 4) acc |= mask[(int64_t)keep[k] * stride + j];
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0) remv[lane] = part[0][lane] | part[1][lane] | part[2][lane] | part[3][lane];
    __syncthreads();
    const int bend = c0 + REDUCE_WORDS < nblk ? c0 + REDUCE_WORDS : nblk;
    for (int b = c0; b < bend && cnt < limit; b++) {
      if (w == 0) {
        const int row = b * 64 + lane;
        const unsigned long long d = row < n ? mask[(int64_t)row * stride + b] : 0ull;
        unsigned long long R = remv[b - c0];
        const int rows = n - b * 64;
        if (rows < 64) R |= ~0ull << rows;                       // rows past n are nobody's candidates
        unsigned long long kept = 0;
        int c = cnt;
#pragma unroll
        for (int i = 0; i < 64; i++) {
          const unsigned long long di = __shfl(d, i, 64);
          if (!((R >> i) & 1ull) && c < limit) { kept |= 1ull << i; R |= di; c++; }
        }
        if ((kept >> lane) & 1ull) keep[cnt + __popcll(kept & ((1ull << lane) - 1ull))] = row;
        if (lane == 0) s_kept = kept;
      }
      __threadfence_block();
      __syncthreads();
      const unsigned long long kept = s_kept;
      unsigned sub = (unsigned)(kept >> (w * 16)) & 0xFFFFu;
      acc = 0;
      if (j > b && j < nblk)
        while (sub) {
          const int i = __ffs(sub) - 1;
          sub &= sub - 1;
          acc |= mask[(int64_t)(b * 64 + w * 16 + i) * stride + j];
        }
      part[w][lane] = acc;
      __syncthreads();
      if (w == 0) remv[lane] |= part[0][lane] | part[1][lane] | part[2][lane] | part[3][lane];
      cnt += __popcll(kept);
      __syncthreads();
    }
  }
  for (int k = cnt + tid; k < cap; k += 256) keep[k] = -1;
  if (tid == 0) *count = cnt;
}

// center_head.py:344-421 + the masks of :461-467, one lane per cell of one frame's H x W map (NCHW maps read in place: a wave reads
// 64 consecutive cells of every channel)
template <bool VEL>
__global__ __launch_bounds__(256) void k_center_decode(const float *__restrict__ hm, const float *__restrict__ reg, const float *__restrict__ height,
                                                       const float *__restrict__ dim, const float *__restrict__ rot, const float *__restrict__ vel,
                                                       int K, int H, int W, decode_geom g, float *__restrict__ boxes,
                                                       int32_t *__restrict__ labels, float *__restrict__ scores) {
  const int hw = H * W, cell = blockIdx.x * 256 + threadIdx.x, bi = blockIdx.y;
  if (cell >= hw) return;
  const int64_t f = (int64_t)bi * hw;
  float best = 0.f;
  int label = 0;
  for (int k = 0; k < K; k++) {
    const float s = 1.f / (1.f + expf(-hm[(f * K + (int64_t)k * hw) + cell]));
    if (k == 0 || s > best) { best = s; label = k; }
  }
  const int wq = cell % W, hq = cell / W;
  float xs = (float)wq + reg[f * 2 + cell], ys = (float)hq + reg[f * 2 + hw + cell];
  xs = xs * g.osf * g.vx + g.px;
  ys = ys * g.osf * g.vy + g.py;
  const float z = height[f + cell];
  constexpr int C = VEL ? 9 : 7;
  float *o = boxes + (f + cell) * C;
  o[0] = xs; o[1] = ys; o[2] = z;
#pragma unroll
  for (int d = 0; d < 3; d++) o[3 + d] = expf(dim[f * 3 + (int64_t)d * hw + cell]);
  if (VEL) { o[6] = vel[f * 2 + cell]; o[7] = vel[f * 2 + hw + cell]; }
  o[C - 1] = atan2f(rot[f * 2 + cell], rot[f * 2 + hw + cell]);
  const bool ok = best > g.thr && xs >= g.lo[0] && ys >= g.lo[1] && z >= g.lo[2] && xs <= g.hi[0] && ys <= g.hi[1] && z <= g.hi[2];
  labels[f + cell] = label;
  scores[f + cell] = ok ? best : -INFINITY;
}

// unmasked cells per frame (box_iou.h)
__global__ __launch_bounds__(256) void k_center_count(const float *__restrict__ scores, int hw, int32_t *__restrict__ counts) {
  center_count_frame(scores, hw, counts);
}

constexpr int64_t MAX_BOXES = 65535LL * PAIR_ROWS;       // grid.y of the pair kernel; 65535 * 64 boxes for the mask is above it

template <bool IOU>
int pair_entry(const char *what, const float *a, int64_t na, const float *b, int64_t nb, float *out, void *stream) {
  if (na < 0 || nb < 0 || na > MAX_BOXES || nb > MAX_BOXES) return LINK_ERR_ARG;
  if (na == 0 || nb == 0) return LINK_OK;
  if (!a || !b || !out) return LINK_ERR_ARG;
  hipLaunchKernelGGL(k_boxes_pair<IOU>, dim3(blocks_for(nb, 64), blocks_for(na, PAIR_ROWS)), dim3(256), 0, S(stream), a, (int)na, b, (int)nb,
                     out);
  return check_launch(what);
}

bool nms_args_ok(int64_t cap, int32_t pred, float thr) {
  return cap >= 0 && cap <= MAX_BOXES && pred >= LINK_NMS_ROTATE && pred <= LINK_NMS_CIRCLE && isfinite(thr);
}

int zero_count(int32_t *count, void *stream, const char *what) {
  if (!count) return LINK_OK;
  hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t), S(stream));
  if (e != hipSuccess) {
    set_error(what, e);
    return LINK_ERR_LAUNCH;
  }
  return LINK_OK;
}

}  // namespace

extern "C" int link_boxes_overlap_bev(const float *boxes_a, int64_t na, const float *boxes_b, int64_t nb, float *out, void *stream) {
  return pair_entry<false>("link_boxes_overlap_bev", boxes_a, na, boxes_b, nb, out, stream);
}

extern "C" int link_boxes_iou_bev(const float *boxes_a, int64_t na, const float *boxes_b, int64_t nb, float *out, void *stream) {
  return pair_entry<true>("link_boxes_iou_bev", boxes_a, na, boxes_b, nb, out, stream);
}

extern "C" size_t link_nms_workspace_bytes(int64_t n) {
  if (n <= 0 || n > MAX_BOXES) return 0;
  return (size_t)8 * (size_t)n * (size_t)((n + 63) / 64);
}

extern "C" int link_nms_mask(const float *boxes, int64_t cap, const int32_t *n_dev, int32_t pred, float thr, uint64_t *mask, void *stream) {
  if (!nms_args_ok(cap, pred, thr)) return LINK_ERR_ARG;
  if (cap == 0) return LINK_OK;
  if (!boxes || !mask) return LINK_ERR_ARG;
  const dim3 grid(blocks_for(cap, 64), blocks_for(cap, 64)), block(256);
  unsigned long long *m = reinterpret_cast<unsigned long long *>(mask);
  if (pred == LINK_NMS_ROTATE) hipLaunchKernelGGL(k_nms_mask<LINK_NMS_ROTATE>, grid, block, 0, S(stream), boxes, (int)cap, n_dev, thr, m);
  else if (pred == LINK_NMS_NORMAL) hipLaunchKernelGGL(k_nms_mask<LINK_NMS_NORMAL>, grid, block, 0, S(stream), boxes, (int)cap, n_dev, thr, m);
  else hipLaunchKernelGGL(k_nms_mask<LINK_NMS_CIRCLE>, grid, block, 0, S(stream), boxes, (int)cap, n_dev, thr, m);
  return check_launch("link_nms_mask");
}

extern "C" int link_nms_reduce(const uint64_t *mask, int64_t cap, const int32_t *n_dev, int32_t post_max, int64_t *keep, int32_t *count,
                               void *stream) {
  if (cap < 0 || cap > MAX_BOXES || post_max < 0) return LINK_ERR_ARG;
  if (cap == 0) return zero_count(count, stream, "link_nms_reduce");
  if (!mask || !keep || !count) return LINK_ERR_ARG;
  hipLaunchKernelGGL(k_nms_reduce, dim3(1), dim3(256), 0, S(stream), reinterpret_cast<const unsigned long long *>(mask), (int)cap, n_dev,
                     (int)post_max, reinterpret_cast<long long *>(keep), count);
  return check_launch("link_nms_reduce");
}

extern "C" int link_nms_bev(const float *boxes, int64_t cap, const int32_t *n_dev, int32_t pred, float thr, int32_t post_max, void *workspace,
                            size_t workspace_bytes, int64_t *keep, int32_t *count, void *stream) {
  if (!nms_args_ok(cap, pred, thr) || post_max < 0) return LINK_ERR_ARG;
  if (cap == 0) return zero_count(count, stream, "link_nms_bev");
  if (!boxes || !workspace || !keep || !count) return LINK_ERR_ARG;
  if (workspace_bytes < link_nms_workspace_bytes(cap)) return LINK_ERR_WORKSPACE;
  const int rc = link_nms_mask(boxes, cap, n_dev, pred, thr, reinterpret_cast<uint64_t *>(workspace), stream);
  if (rc != LINK_OK) return rc;
  return link_nms_reduce(reinterpret_cast<const uint64_t *>(workspace), cap, n_dev, post_max, keep, count, stream);
}

extern "C" int link_center_decode(const float *hm, const float *reg, const float *height, const float *dim, const float *rot, const float *vel,
                                  int32_t batch, int32_t num_cls, int32_t h, int32_t w, const link_center_geom_t *geom, float *boxes,
                                  int32_t *labels, float *scores, int32_t *counts, void *stream) {
  if (batch < 0 || num_cls < 1 || h < 0 || w < 0 || !geom || batch > 65535) return LINK_ERR_ARG;
  if ((int64_t)h * w >= (1LL << 24)) return LINK_ERR_ARG;
  if (!isfinite(geom->score_threshold) || !isfinite(geom->out_size_factor)) return LINK_ERR_ARG;
  for (int d = 0; d < 2; d++)
    if (!isfinite(geom->voxel_size[d]) || !isfinite(geom->pc_range[d])) return LINK_ERR_ARG;
  for (int d = 0; d < 6; d++)
    if (isnan(geom->post_center_range[d])) return LINK_ERR_ARG;
  if (batch == 0 || h * w == 0) return LINK_OK;
  if (!hm || !reg || !height || !dim || !rot || !boxes || !labels || !scores || !counts) return LINK_ERR_ARG;
  decode_geom g;
  g.osf = geom->out_size_factor; g.vx = geom->voxel_size[0]; g.vy = geom->voxel_size[1];
  g.px = geom->pc_range[0]; g.py = geom->pc_range[1]; g.thr = geom->score_threshold;
  for (int d = 0; d < 3; d++) { g.lo[d] = geom->post_center_range[d]; g.hi[d] = geom->post_center_range[3 + d]; }
  const dim3 grid(blocks_for((int64_t)h * w, 256), batch), block(256);
  if (vel) hipLaunchKernelGGL(k_center_decode<true>, grid, block, 0, S(stream), hm, reg, height, dim, rot, vel, (int)num_cls, (int)h, (int)w, g,
                              boxes, labels, scores);
  else hipLaunchKernelGGL(k_center_decode<false>, grid, block, 0, S(stream), hm, reg, height, dim, rot, vel, (int)num_cls, (int)h, (int)w, g,
                          boxes, labels, scores);
  int rc = check_launch("link_center_decode");
  if (rc != LINK_OK) return rc;
  hipLaunchKernelGGL(k_center_count, dim3(batch), dim3(256), 0, S(stream), scores, h * w, counts);
  return check_launch("link_center_decode");
}
