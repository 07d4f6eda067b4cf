// link_amd/csrc/roihead.hip -- section O of include/link_amd.h: the second stage of a two-stage CenterPoint on the device.
//
// Semantics: detection/det3d/models/detectors/two_stage.py:51-78 (get_box_center) and :123-153 (post_process),
// models/second_stage/bird_eye_view.py with core/utils/center_utils.py:92-121 (bilinear_interpolate_torch),
// models/roi_heads/target_assigner/proposal_target_layer.py (ProposalTargetLayer), models/roi_heads/roi_head_template.py:43-86
// (assign_targets), :88-151 (get_loss) and :153-183 (generate_predicted_boxes).  The implementation is this project's.
//
//   k_roi_bev       one wave per (output row, sample point): the point from the box, the four clamped corners and their weights once
//                   per wave, then lanes along the channels -- four channels per lane in one 16- or 8-byte load where the channel
//                   stride is 1 and everything is aligned, one channel per lane through the four strides otherwise
//   k_roi_overlap   a workgroup per 16 ROIs of a frame, 16 lanes per ROI over interleaved slices of the frame's ground truth (staged
//                   in LDS once per workgroup): 3-D IoU against every row that counts, the maximum with the lowest index
//   k_roi_sample    one workgroup per frame: the three ordered lists by ballot scans, the counts, the draws from `noise`, then the
//                   targets of the M sampled rows
//   k_roi_loss      one workgroup: counts, then both sums by a tree of fixed shape, and the unit gradients
//   k_roi_loss_bwd  unit gradients times the device scalar, rounded once
//   k_roi_refine    one workgroup per frame: the refined boxes of the slots in use, packed to the front by ballot scans
//
// Contraction is off (box_iou.h): the reference forms x c + y s from rounded products, and so do the rotations here.
#pragma clang fp contract(off)
#include <math.h>

#include "block_prims.h"
#include "box_iou.h"
#include "dispatch.h"
#include "row_io.h"

using namespace link;

namespace {

constexpr int T = 256;
constexpr float PI_F = 3.14159265358979323846f;          // fp32(pi), fp32(2 pi), fp32(pi / 2), fp32(3 pi / 2): what a float32 tensor
constexpr float TWO_PI_F = 6.28318530717958647692f;      // op sees of the reference's python scalars
constexpr float HALF_PI_F = 1.57079632679489661923f;
constexpr float PI15_F = 4.71238898038468985769f;

__device__ __forceinline__ float cosd(float a) { return (float)cos((double)a); }       // correctly rounded, as box_iou.h's staging
__device__ __forceinline__ float sind(float a) { return (float)sin((double)a); }

// ---- O1: features ---------------------------------------------------------------------------------------------------------------
struct BevGeom {
  int64_t sb, sc, sh, sw;
  float px, py, vx, vy, os;
  int C, H, W, R, S, P, box_len, rot_col;
};

// floor of a map coordinate as an integer in [-2, n]: everything below -1 clamps like -2, everything from n on like n (NaN: -2)
__device__ __forceinline__ int floor_cell(float v, int n) {
  const float f = floorf(v);
  if (!(f > -2.f)) return -2;
  if (f >= (float)n) return n;
  return (int)f;
}

template <int IO, bool VEC>
__global__ __launch_bounds__(T) void k_roi_bev(const void *__restrict__ bev, BevGeom g, const float *__restrict__ boxes,
                                               const long long *__restrict__ labels, const int32_t *__restrict__ sel, int64_t waves,
                                               void *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (T / 64) + (threadIdx.x >> 6);      // (frame, output row, point)
  if (wv >= waves) return;
  const int p = (int)(wv % g.P);
  const int64_t row = wv / g.P;
  const int b = (int)(row / g.S), s = (int)(row % g.S);
  const int64_t o0 = wv * g.C;
  int src = sel ? sel[(int64_t)b * g.S + s] : s;
  bool used = src >= 0 && src < g.R;
  if (used && labels) used = labels[(int64_t)b * g.R + src] != 0;
  if (!used) {                                                                 // an unused slot: the reference's new_zeros row
    if (VEC) {
      for (int c = lane * 4; c < g.C; c += 256) row_st4<IO>(out, o0 + c, make_float4(0.f, 0.f, 0.f, 0.f));
    } else {
      for (int c = lane; c < g.C; c += 64) row_st1<IO>(out, o0 + c, 0.f);
    }
    return;
  }
  const float *bx = boxes + ((int64_t)b * g.R + src) * g.box_len;
  float x = bx[0], y = bx[1];
  if (p > 0) {
    // center_to_corner_box2d (box_torch_ops.py:184-203): corners (-,-), (-,+), (+,+), (+,-) of dims / 2, rotated by
    // x' = x c + y s, y' = -x s + y c (rotation_2d), plus the centre; then the midpoints of two_stage.py:66-69
    const float dx = bx[3], dy = bx[4], h = bx[g.rot_col];
    const float c = cosd(h), sn = sind(h);
    const float ux[4] = {dx * -0.5f, dx * -0.5f, dx * 0.5f, dx * 0.5f}, uy[4] = {dy * -0.5f, dy * 0.5f, dy * 0.5f, dy * -0.5f};
    const int ia = (p == 1 || p == 3) ? 0 : (p == 2 ? 2 : 1);                  // front 0+1, back 2+3, left 0+3, right 1+2
    const int ib = p == 1 ? 1 : (p == 4 ? 2 : 3);
    const float ax = (ux[ia] * c + uy[ia] * sn) + x, ay = (ux[ia] * -sn + uy[ia] * c) + y;
    const float qx = (ux[ib] * c + uy[ib] * sn) + x, qy = (ux[ib] * -sn + uy[ib] * c) + y;
    x = (ax + qx) / 2.f;
    y = (ay + qy) / 2.f;
  }
  const float fx = (x - g.px) / g.vx / g.os, fy = (y - g.py) / g.vy / g.os;    // absl_to_relative, every operation rounded
  const int xf = floor_cell(fx, g.W), yf = floor_cell(fy, g.H);
  const int x0 = clampi(xf, 0, g.W - 1), x1 = clampi(xf + 1, 0, g.W - 1), y0 = clampi(yf, 0, g.H - 1), y1 = clampi(yf + 1, 0, g.H - 1);
  // center_utils.py:116-119: the weights from the CLAMPED corners
  const float wa = ((float)x1 - fx) * ((float)y1 - fy), wb = ((float)x1 - fx) * (fy - (float)y0);
  const float wc = (fx - (float)x0) * ((float)y1 - fy), wd = (fx - (float)x0) * (fy - (float)y0);
  const int64_t base = (int64_t)b * g.sb;
  const int64_t ea = base + y0 * g.sh + x0 * g.sw, eb = base + y1 * g.sh + x0 * g.sw;
  const int64_t ec = base + y0 * g.sh + x1 * g.sw, ed = base + y1 * g.sh + x1 * g.sw;
  if (VEC) {                                                                   // channel stride 1: four channels per lane
    for (int c = lane * 4; c < g.C; c += 256) {
      const float4 a = row_ld4<IO>(bev, ea + c), bq = row_ld4<IO>(bev, eb + c), cq = row_ld4<IO>(bev, ec + c), d = row_ld4<IO>(bev, ed + c);
      float4 r;
      r.x = ((a.x * wa + bq.x * wb) + cq.x * wc) + d.x * wd;
      r.y = ((a.y * wa + bq.y * wb) + cq.y * wc) + d.y * wd;
      r.z = ((a.z * wa + bq.z * wb) + cq.z * wc) + d.z * wd;
      r.w = ((a.w * wa + bq.w * wb) + cq.w * wc) + d.w * wd;
      row_st4<IO>(out, o0 + c, r);
    }
  } else {
    for (int c = lane; c < g.C; c += 64) {
      const int64_t k = (int64_t)c * g.sc;
      const float a = row_ld1<IO>(bev, ea + k), bq = row_ld1<IO>(bev, eb + k), cq = row_ld1<IO>(bev, ec + k), d = row_ld1<IO>(bev, ed + k);
      row_st1<IO>(out, o0 + c, ((a * wa + bq * wb) + cq * wc) + d * wd);
    }
  }
}

// ---- O2: overlaps -----------------------------------------------------------------------------------------------------------------
// to_pcdet (iou3d_nms_utils.py:29-33): extents swapped, heading -> -heading - pi / 2
__device__ __forceinline__ void pcdet_box(const float *src, float *dst) {
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[4]; dst[4] = src[3]; dst[5] = src[5];
  dst[6] = -src[6] - HALF_PI_F;
}

// rows of the frame's ground truth that count: trailing rows whose sum is 0 are cut, one row always stays (:107-111)
__device__ __forceinline__ int gt_rows(const float *gt, int G, int ncol) {
  int k = G - 1;
  while (k > 0) {
    float s = 0.f;
    for (int c = 0; c < ncol; c++) s = s + gt[(int64_t)k * ncol + c];
    if (s != 0.f) break;
    k--;
  }
  return k + 1;
}

constexpr int OV_ROIS = 16, OV_SLICES = T / OV_ROIS;       // a workgroup: 16 ROIs x 16 interleaved slices of the ground truth

__global__ __launch_bounds__(T) void k_roi_overlap(const float *__restrict__ rois, const long long *__restrict__ roi_labels,
                                                   const float *__restrict__ gt, int R, int G, int code, int by_class,
                                                   float *__restrict__ max_overlaps, int32_t *__restrict__ gt_assignment) {
  __shared__ float sg[NF][LINK_ROI_MAX_GT];
  __shared__ float gz[2][LINK_ROI_MAX_GT];                 // z extent: min, max
  __shared__ float gvol[LINK_ROI_MAX_GT];
  __shared__ long long glab[LINK_ROI_MAX_GT];
  __shared__ float sa[NF][OV_ROIS];
  __shared__ float az[3][OV_ROIS];                         // z min, z max, volume
  __shared__ float sbest[OV_SLICES][OV_ROIS];
  __shared__ int sarg[OV_SLICES][OV_ROIS];                 // -1: the slice saw no row of the ROI's class
  __shared__ int s_n;
  const int t = threadIdx.x, b = blockIdx.y, ncol = code + 1;
  const int r = t % OV_ROIS, sl = t / OV_ROIS;
  const float *g = G > 0 ? gt + (int64_t)b * G * ncol : nullptr;
  if (t == 0) s_n = G > 0 ? gt_rows(g, G, ncol) : 1;
  __syncthreads();
  const int n = s_n;
  for (int j = t; j < n; j += T) {
    float raw[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, pb[7];
    float lab = 0.f;
    if (g) {
#pragma unroll
      for (int c = 0; c < 7; c++) raw[c] = g[(int64_t)j * ncol + c];
      lab = g[(int64_t)j * ncol + code];
    }
    pcdet_box(raw, pb);
    stage_box<LINK_ROI_MAX_GT, true>(pb, sg, j);
    gz[0][j] = pb[2] - pb[5] / 2; gz[1][j] = pb[2] + pb[5] / 2;
    gvol[j] = pb[3] * pb[4] * pb[5];
    glab[j] = (long long)lab;                                // .long(): toward zero
  }
  const int i = blockIdx.x * OV_ROIS + r;
  const bool live = i < R;
  if (sl == 0 && live) {
    float raw[7], pa[7];
#pragma unroll
    for (int c = 0; c < 7; c++) raw[c] = rois[((int64_t)b * R + i) * code + c];
    pcdet_box(raw, pa);
    stage_box<OV_ROIS, true>(pa, sa, r);
    az[0][r] = pa[2] - pa[5] / 2; az[1][r] = pa[2] + pa[5] / 2; az[2][r] = pa[3] * pa[4] * pa[5];
  }
  __syncthreads();
  float best = 0.f;
  int arg = -1;
  if (live) {
    const Rec A = load_box<OV_ROIS, true>(sa, r);
    const float amin = az[0][r], amax = az[1][r], avol = az[2][r];
    const long long la = roi_labels[(int64_t)b * R + i];
    for (int j = sl; j < n; j += OV_SLICES) {
      if (by_class && glab[j] != la) continue;
      const Rec Bq = load_box<LINK_ROI_MAX_GT, true>(sg, j);
      const float bev = box_overlap(A, Bq);
      const float dh = fminf(amax, gz[1][j]) - fmaxf(amin, gz[0][j]);
      const float o3 = bev * (dh < 0.f ? 0.f : dh);
      const float den = avol + gvol[j] - o3;                 // torch.clamp keeps a NaN: a box that is not finite stays visible
      const float iou = o3 / (den < 1e-6f ? 1e-6f : den);
      if (arg < 0 || iou > best) { best = iou; arg = j; }
    }
  }
  sbest[sl][r] = best;
  sarg[sl][r] = arg;
  __syncthreads();
  if (sl != 0 || !live) return;
  // the slices in ascending order: the maximum, the lowest index among equals (a slice's own candidate is its lowest)
  best = 0.f;
  arg = -1;
  for (int q = 0; q < OV_SLICES; q++) {
    const int aq = sarg[q][r];
    if (aq < 0) continue;
    const float v = sbest[q][r];
    if (arg < 0 || v > best || (v == best && aq < arg)) { best = v; arg = aq; }
  }
  max_overlaps[(int64_t)b * R + i] = arg < 0 ? 0.f : best;
  gt_assignment[(int64_t)b * R + i] = arg < 0 ? 0 : arg;
}

// ---- O2: sampling and targets -------------------------------------------------------------------------------------------------------
struct SampleCfg {
  int R, G, M, code, fg_per_image, soft_labels, has_sel_in;
  double hard_ratio;
  float reg_fg, cls_fg, cls_bg, bg_lo, fg_thresh, soft_den;
};

// floor-mod of a by 2 pi in fp32 (torch's remainder)
__device__ __forceinline__ float mod_2pi(float a) {
  float r = fmodf(a, TWO_PI_F);
  if (r != 0.f && r < 0.f) r = r + TWO_PI_F;
  return r;
}

// draw with replacement for output slot j out of n candidates
__device__ __forceinline__ int draw(const float *noise, int R, int j, int n) {
  const float f = floorf(noise[R + j] * (float)n);
  int k = f >= (float)n ? n - 1 : (f > 0.f ? (int)f : 0);
  return k > n - 1 ? n - 1 : k;
}

__global__ __launch_bounds__(T) void k_roi_sample(SampleCfg cf, const float *__restrict__ rois, const long long *__restrict__ roi_labels,
                                                  const float *__restrict__ roi_scores, const float *__restrict__ gt,
                                                  const float *__restrict__ noise_all, const int32_t *__restrict__ sel_in,
                                                  const float *__restrict__ max_overlaps, const int32_t *__restrict__ gt_assignment,
                                                  int32_t *__restrict__ sel, float *__restrict__ o_rois, long long *__restrict__ o_labels,
                                                  float *__restrict__ o_scores, float *__restrict__ o_iou, float *__restrict__ o_gt_src,
                                                  float *__restrict__ o_gt, long long *__restrict__ o_reg_valid,
                                                  float *__restrict__ o_cls_labels, int32_t *__restrict__ status) {
  __shared__ unsigned short lists[3][LINK_ROI_MAX_ROIS];    // fg, hard bg, easy bg: ascending ROI index
  __shared__ int wtot[3][T / 64];
  __shared__ int cnt[3];
  __shared__ int s_sel[LINK_ROI_MAX_SAMPLES];
  __shared__ int s_status;
  const int t = threadIdx.x, b = blockIdx.x, lane = t & 63, wave = t >> 6;
  const int R = cf.R, M = cf.M, code = cf.code, ncol = code + 1;
  const float *mo = max_overlaps + (int64_t)b * R;
  const float *noise = noise_all ? noise_all + (int64_t)b * (R + M) : nullptr;
  if (t < 3) cnt[t] = 0;
  if (t == 0) s_status = 0;
  __syncthreads();
  if (!cf.has_sel_in) {
    // the three lists of subsample_rois (:138-141), comparisons as written
    for (int base = 0; base < R; base += T) {
      const int i = base + t;
      bool f[3] = {false, false, false};
      if (i < R) {
        const float v = mo[i];
        f[0] = v >= cf.fg_thresh;
        f[1] = v < cf.reg_fg && v >= cf.bg_lo;
        f[2] = v < cf.bg_lo;
      }
      int pos[3];
#pragma unroll
      for (int l = 0; l < 3; l++) {
        const unsigned long long bal = __ballot(f[l]);
        pos[l] = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[l][wave] = __popcll(bal);
      }
      __syncthreads();
#pragma unroll
      for (int l = 0; l < 3; l++) {
        int off = cnt[l];
        for (int w = 0; w < wave; w++) off += wtot[l][w];
        if (f[l]) lists[l][off + pos[l]] = (unsigned short)i;
      }
      __syncthreads();
      if (t < 3) cnt[t] += wtot[t][0] + wtot[t][1] + wtot[t][2] + wtot[t][3];
      __syncthreads();
    }
    const int nfg = cnt[0], nhard = cnt[1], neasy = cnt[2], nbg = nhard + neasy;
    int take_fg = 0, fg_repl = 0, n_bg_slots = 0;
    if (nfg > 0 && nbg > 0) {
      take_fg = cf.fg_per_image < nfg ? cf.fg_per_image : nfg;
      n_bg_slots = M - take_fg;
    } else if (nfg > 0) {
      fg_repl = M;
    } else if (nbg > 0) {
      n_bg_slots = M;
    } else if (t == 0) {
      s_status = LINK_ROI_STATUS_NO_CANDIDATE;
    }
    if (take_fg > M) { take_fg = M; n_bg_slots = 0; }
    int nh = 0;
    if (nhard > 0 && neasy > 0) {
      const int want = (int)((double)n_bg_slots * cf.hard_ratio);               // int(): toward zero
      nh = want < nhard ? want : nhard;
      nh = nh < 0 ? 0 : (nh > n_bg_slots ? n_bg_slots : nh);
    } else if (nhard > 0) {
      nh = n_bg_slots;
    }
    for (int j = t; j < M; j += T) s_sel[j] = 0;
    __syncthreads();
    // foreground without replacement: the take_fg smallest keys, ascending, ties by index
    for (int a = t; a < nfg && take_fg > 0; a += T) {
      const int i = lists[0][a];
      const float key = noise[i];
      int rank = 0;
      for (int q = 0; q < nfg; q++) {
        const int iq = lists[0][q];
        const float kq = noise[iq];
        rank += (kq < key || (kq == key && iq < i)) ? 1 : 0;
      }
      if (rank < take_fg) s_sel[rank] = i;
    }
    for (int j = t; j < M; j += T) {
      if (j < fg_repl) s_sel[j] = lists[0][draw(noise, R, j, nfg)];
      else if (j >= take_fg + fg_repl && j < take_fg + fg_repl + nh) s_sel[j] = lists[1][draw(noise, R, j, nhard)];
      else if (j >= take_fg + fg_repl + nh && n_bg_slots > 0 && neasy > 0) s_sel[j] = lists[2][draw(noise, R, j, neasy)];
    }
  } else {
    for (int j = t; j < M; j += T) {
      int i = sel_in[(int64_t)b * M + j];
      if (i < 0 || i >= R) { i = 0; s_status = LINK_ROI_STATUS_BAD_INDEX; }     // every writer writes the same value
      s_sel[j] = i;
    }
  }
  __syncthreads();
  if (t == 0) status[b] = s_status;
  // the targets of the M rows (ProposalTargetLayer.forward :42-70 and assign_targets, roi_head_template.py:52-82)
  for (int j = t; j < M; j += T) {
    const int i = s_sel[j];
    const int64_t o = (int64_t)b * M + j, ri = (int64_t)b * R + i;
    const float iou = mo[i];
    float roi[9], gg[10];
    for (int c = 0; c < code; c++) roi[c] = rois[ri * code + c];
    const int ga = gt_assignment[ri];
    for (int c = 0; c < ncol; c++) gg[c] = cf.G > 0 ? gt[((int64_t)b * cf.G + ga) * ncol + c] : 0.f;
    sel[o] = i;
    for (int c = 0; c < code; c++) o_rois[o * code + c] = roi[c];
    o_labels[o] = roi_labels[ri];
    o_scores[o] = roi_scores[ri];
    o_iou[o] = iou;
    for (int c = 0; c < ncol; c++) o_gt_src[o * ncol + c] = gg[c];
    o_reg_valid[o] = iou > cf.reg_fg ? 1 : 0;
    float lab;
    if (!cf.soft_labels) {
      lab = iou > cf.cls_fg ? 1.f : 0.f;
      if (iou > cf.cls_bg && iou < cf.cls_fg) lab = -1.f;
    } else {
      const bool fg = iou > cf.cls_fg, bg = iou < cf.cls_bg;
      lab = fg ? 1.f : 0.f;
      if (!fg && !bg) lab = (iou - cf.cls_bg) / cf.soft_den;
    }
    o_cls_labels[o] = lab;
    const float ry = roi[6] - floorf(roi[6] / TWO_PI_F + 0.5f) * TWO_PI_F;      // limit_period(.., 0.5, 2 pi)
    for (int c = 0; c < 6; c++) gg[c] = gg[c] - roi[c];
    gg[6] = gg[6] - ry;
    const float ca = cosd(-ry), sa = sind(-ry);                                 // rotate_points_along_z by -ry: [x y z] @ matrix
    const float x = gg[0], y = gg[1];
    gg[0] = x * ca + y * sa;
    gg[1] = x * -sa + y * ca;
    if (code == 9) { gg[7] = gg[7] - roi[7]; gg[8] = gg[8] - roi[8]; }
    float h = mod_2pi(gg[6]);
    if (h > HALF_PI_F && h < PI15_F) h = mod_2pi(h + PI_F);
    if (h > PI_F) h = h - TWO_PI_F;
    h = fminf(fmaxf(h, -HALF_PI_F), HALF_PI_F);
    gg[6] = h;
    for (int c = 0; c < ncol; c++) o_gt[o * ncol + c] = gg[c];
  }
}

// ---- O3: loss ---------------------------------------------------------------------------------------------------------------------
struct CodeW {
  float w[9];
};

// F.binary_cross_entropy(sigmoid(x), t) and its autograd gradient with respect to x, as torch forms them in fp32
__device__ __forceinline__ void bce_term(float x, float tg, float &val, float &grad) {
  const float p = 1.0f / (1.0f + expf(-x));
  const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(log1pf(-p), -100.f);
  val = (tg - 1.f) * lq - tg * lp;
  const float pq = (1.f - p) * p;
  grad = ((p - tg) / fmaxf(pq, 1e-12f)) * pq;
}

template <int IO>
__global__ __launch_bounds__(T) void k_roi_loss(const void *__restrict__ cls, const void *__restrict__ reg, int n, int code,
                                                const float *__restrict__ labels, const float *__restrict__ gt_of_rois,
                                                const long long *__restrict__ reg_valid, CodeW cw, float cls_weight, float reg_weight,
                                                float *__restrict__ out, float *__restrict__ unit_cls, float *__restrict__ unit_reg) {
  __shared__ float fl[T];
  __shared__ int il[T];
  const int t = threadIdx.x, ncol = code + 1;
  int nv = 0, nf = 0;
  for (int i = t; i < n; i += T) {
    nv += labels[i] >= 0.f ? 1 : 0;
    nf += reg_valid[i] > 0 ? 1 : 0;
  }
  const int valid = block_sum_fixed<int>(nv, il), fg = block_sum_fixed<int>(nf, il);
  const float vden = valid > 1 ? (float)valid : 1.f, fden = fg > 1 ? (float)fg : 1.f;
  float sc = 0.f, sr = 0.f;
  for (int i = t; i < n; i += T) {
    const float tg = labels[i];
    float g = 0.f;
    if (tg >= 0.f) {                                                            // a masked row is not read
      float v;
      bce_term(row_ld1<IO>(cls, i), tg, v, g);
      sc = sc + v;
      g = g / vden * cls_weight;
    }
    unit_cls[i] = g;
    const bool on = reg_valid[i] > 0;
    float row = 0.f;
    for (int c = 0; c < code; c++) {
      float u = 0.f;
      if (on) {
        const float d = row_ld1<IO>(reg, (int64_t)i * code + c) - gt_of_rois[(int64_t)i * ncol + c];
        row = row + fabsf(d) * cw.w[c];
        u = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * cw.w[c] / fden * reg_weight;
      }
      unit_reg[(int64_t)i * code + c] = u;
    }
    sr = sr + row;
  }
  const float tc = block_sum_fixed<float>(sc, fl), tr = block_sum_fixed<float>(sr, fl);
  if (t == 0) {
    const float lc = tc / vden * cls_weight, lr = tr / fden * reg_weight;
    out[0] = lc + lr;
    out[1] = lc;
    out[2] = lr;
    out[3] = (float)fg;
  }
}

template <int IO>
__global__ __launch_bounds__(T) void k_roi_loss_bwd(const float *__restrict__ unit_cls, const float *__restrict__ unit_reg,
                                                    const float *__restrict__ upstream, int n, int code, void *__restrict__ grad_cls,
                                                    void *__restrict__ grad_reg) {
  const int e = blockIdx.x * T + threadIdx.x;
  const float s = upstream[0];
  if (e < n) row_st1<IO>(grad_cls, e, unit_cls[e] * s);
  if (e < n * code) row_st1<IO>(grad_reg, e, unit_reg[e] * s);
}

// ---- O4: refine -------------------------------------------------------------------------------------------------------------------
template <int IO>
__global__ __launch_bounds__(T) void k_roi_refine(const float *__restrict__ rois, const long long *__restrict__ roi_labels,
                                                  const float *__restrict__ roi_scores, const void *__restrict__ cls,
                                                  const void *__restrict__ reg, int R, int code, float *__restrict__ o_boxes,
                                                  float *__restrict__ o_scores, long long *__restrict__ o_labels,
                                                  int32_t *__restrict__ counts) {
  __shared__ int wtot[T / 64];
  __shared__ int run;
  const int t = threadIdx.x, b = blockIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) run = 0;
  __syncthreads();
  for (int base = 0; base < R; base += T) {
    const int i = base + t;
    const int64_t ri = (int64_t)b * R + i;
    const long long lab = i < R ? roi_labels[ri] : 0;
    const bool keep = lab != 0;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int slot = run + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) slot += wtot[w];
    if (keep) {
      float roi[9], v[9];
      for (int c = 0; c < code; c++) roi[c] = rois[ri * code + c];
      for (int c = 0; c < code; c++) v[c] = row_ld1<IO>(reg, ri * code + c) + (c < 3 ? 0.f : roi[c]);      // the ROI with its centre zeroed
      const float ca = cosd(roi[6]), sa = sind(roi[6]);
      const float x = v[0], y = v[1];
      v[0] = (x * ca + y * sa) + roi[0];                                        // rotate_points_along_z, then the centre back
      v[1] = (x * -sa + y * ca) + roi[1];
      v[2] = v[2] + roi[2];
      const int64_t o = (int64_t)b * R + slot;
      if (code == 9) {                                                          // two_stage.py:132-134: heading last
        const float h = v[6];
        v[6] = v[7]; v[7] = v[8]; v[8] = h;
      }
      for (int c = 0; c < code; c++) o_boxes[o * code + c] = v[c];
      const float p = 1.0f / (1.0f + expf(-row_ld1<IO>(cls, ri)));
      o_scores[o] = sqrtf(p * roi_scores[ri]);
      o_labels[o] = lab - 1;
    }
    __syncthreads();
    if (t == 0) run += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  const int kept = run;
  for (int i = kept + t; i < R; i += T) {
    const int64_t o = (int64_t)b * R + i;
    for (int c = 0; c < code; c++) o_boxes[o * code + c] = 0.f;
    o_scores[o] = 0.f;
    o_labels[o] = -1;
  }
  if (t == 0) counts[b] = kept;
}

inline bool finite_pos(float v) { return isfinite(v) && v > 0.f; }

}  // namespace

// ----------------------------------------------------------------------------------------------------------------- C entries
extern "C" int link_roi_bev_features(const void *bev, int32_t io_dtype, const int64_t *strides, int32_t batch, int32_t c, int32_t h,
                                     int32_t w, const float *boxes, int64_t r, int32_t box_len, int32_t rot_col, const int64_t *labels,
                                     const int32_t *sel, int64_t s, int32_t num_point, const float *pc_start, const float *voxel_size,
                                     float out_stride, void *out, void *stream) {
  if (!row_io_ok(io_dtype) || !strides || !pc_start || !voxel_size || (num_point != 1 && num_point != 5)) return LINK_ERR_ARG;
  if (batch < 0 || batch > 65535 || c < 1 || h < 1 || w < 1 || r < 0 || s < 0 || box_len < 7 || box_len > 64 || rot_col < 5 ||
      rot_col >= box_len)
    return LINK_ERR_ARG;
  if (r >= (1LL << 31) || s >= (1LL << 31) || (int64_t)batch * r >= (1LL << 31) || (int64_t)batch * s * num_point >= (1LL << 31))
    return LINK_ERR_ARG;
  if (!finite_pos(voxel_size[0]) || !finite_pos(voxel_size[1]) || !finite_pos(out_stride) || !isfinite(pc_start[0]) || !isfinite(pc_start[1]))
    return LINK_ERR_ARG;
  for (int d = 0; d < 4; d++)
    if (strides[d] < 0 || strides[d] >= (1LL << 40)) return LINK_ERR_ARG;
  if (!sel && s != r) return LINK_ERR_ARG;
  if (batch == 0 || s == 0) return LINK_OK;
  if (!bev || !out || (r > 0 && !boxes) || (sel && r == 0)) return LINK_ERR_ARG;
  BevGeom g;
  g.sb = strides[0]; g.sc = strides[1]; g.sh = strides[2]; g.sw = strides[3];
  g.px = pc_start[0]; g.py = pc_start[1]; g.vx = voxel_size[0]; g.vy = voxel_size[1]; g.os = out_stride;
  g.C = c; g.H = h; g.W = w; g.R = (int)r; g.S = (int)s; g.P = num_point; g.box_len = box_len; g.rot_col = rot_col;
  const int64_t waves = (int64_t)batch * s * num_point;
  const size_t vb = io_dtype == LINK_IO_F32 ? 16 : 8;                           // bytes of four channels
  const bool vec = g.sc == 1 && c % 4 == 0 && g.sb % 4 == 0 && g.sh % 4 == 0 && g.sw % 4 == 0 && aligned_to(bev, vb) &&
                   aligned_to(out, vb);
  const dim3 grid(blocks_for(waves, T / 64)), block(T);
  const long long *lb = reinterpret_cast<const long long *>(labels);
  dispatch_row_io(io_dtype, [&](auto io) {
    constexpr int IO = decltype(io)::value;
    if (vec) hipLaunchKernelGGL((k_roi_bev<IO, true>), grid, block, 0, S(stream), bev, g, boxes, lb, sel, waves, out);
    else hipLaunchKernelGGL((k_roi_bev<IO, false>), grid, block, 0, S(stream), bev, g, boxes, lb, sel, waves, out);
  });
  return check_launch("link_roi_bev_features");
}

extern "C" int link_roi_assign(const float *rois, const int64_t *roi_labels, const float *roi_scores, const float *gt, const float *noise,
                               const int32_t *sel_in, int32_t batch, int64_t r, int64_t g, int64_t m, int32_t code, double fg_ratio,
                               int32_t by_class, int32_t soft_labels, double cls_fg_thresh, double cls_bg_thresh, double cls_bg_thresh_lo,
                               double hard_bg_ratio, double reg_fg_thresh, float *max_overlaps, int32_t *gt_assignment, int32_t *sel,
                               float *o_rois, int64_t *o_labels, float *o_scores, float *o_iou, float *o_gt_src, float *o_gt,
                               int64_t *o_reg_valid, float *o_cls_labels, int32_t *status, void *stream) {
  if ((code != 7 && code != 9) || batch < 1 || batch > 65535 || r < 1 || r > LINK_ROI_MAX_ROIS || g < 0 || g > LINK_ROI_MAX_GT || m < 1 ||
      m > LINK_ROI_MAX_SAMPLES)
    return LINK_ERR_ARG;
  if ((by_class != 0 && by_class != 1) || (soft_labels != 0 && soft_labels != 1)) return LINK_ERR_ARG;
  if (code == 9 && !by_class) return LINK_ERR_ARG;                  // boxes_iou3d_gpu asserts 7 columns; only the by-class branch slices
  if (!(fg_ratio >= 0.0 && fg_ratio <= 1.0) || !(hard_bg_ratio >= 0.0 && hard_bg_ratio <= 1.0)) return LINK_ERR_ARG;
  if (!isfinite(cls_fg_thresh) || !isfinite(cls_bg_thresh) || !isfinite(cls_bg_thresh_lo) || !isfinite(reg_fg_thresh)) return LINK_ERR_ARG;
  // the order the three lists and the soft label rest on: lo <= both foreground thresholds, bg < fg (its difference divides)
  if (cls_bg_thresh_lo > reg_fg_thresh || cls_bg_thresh_lo > cls_fg_thresh || !(cls_bg_thresh < cls_fg_thresh)) return LINK_ERR_ARG;
  if (!rois || !roi_labels || !roi_scores || (g > 0 && !gt) || (!noise && !sel_in)) return LINK_ERR_ARG;
  if (!max_overlaps || !gt_assignment || !sel || !o_rois || !o_labels || !o_scores || !o_iou || !o_gt_src || !o_gt || !o_reg_valid ||
      !o_cls_labels || !status)
    return LINK_ERR_ARG;
  SampleCfg cf;
  cf.R = (int)r; cf.G = (int)g; cf.M = (int)m; cf.code = code;
  cf.fg_per_image = (int)nearbyint(fg_ratio * (double)m);            // np.round: half to even (the default rounding mode)
  cf.soft_labels = soft_labels; cf.has_sel_in = sel_in != nullptr;
  cf.hard_ratio = hard_bg_ratio;
  cf.reg_fg = (float)reg_fg_thresh; cf.cls_fg = (float)cls_fg_thresh; cf.cls_bg = (float)cls_bg_thresh; cf.bg_lo = (float)cls_bg_thresh_lo;
  cf.fg_thresh = (float)(reg_fg_thresh < cls_fg_thresh ? reg_fg_thresh : cls_fg_thresh);
  cf.soft_den = (float)(cls_fg_thresh - cls_bg_thresh);
  const long long *lb = reinterpret_cast<const long long *>(roi_labels);
  hipLaunchKernelGGL(k_roi_overlap, dim3(blocks_for(r, OV_ROIS), batch), dim3(T), 0, S(stream), rois, lb, gt, (int)r, (int)g, (int)code,
                     (int)by_class, max_overlaps, gt_assignment);
  int rc = check_launch("link_roi_assign");
  if (rc != LINK_OK) return rc;
  hipLaunchKernelGGL(k_roi_sample, dim3(batch), dim3(T), 0, S(stream), cf, rois, lb, roi_scores, gt, noise, sel_in, max_overlaps,
                     gt_assignment, sel, o_rois, reinterpret_cast<long long *>(o_labels), o_scores, o_iou, o_gt_src, o_gt,
                     reinterpret_cast<long long *>(o_reg_valid), o_cls_labels, status);
  return check_launch("link_roi_assign");
}

extern "C" int link_roi_loss_forward(const void *rcnn_cls, const void *rcnn_reg, int32_t io_dtype, int64_t n, int32_t code,
                                     const float *cls_labels, const float *gt_of_rois, const int64_t *reg_valid_mask,
                                     const float *code_weights, float cls_weight, float reg_weight, float *out, float *unit_cls,
                                     float *unit_reg, void *stream) {
  if (!row_io_ok(io_dtype) || (code != 7 && code != 9) || n < 1 || n > LINK_ROI_MAX_LOSS_ROWS) return LINK_ERR_ARG;
  if (!rcnn_cls || !rcnn_reg || !cls_labels || !gt_of_rois || !reg_valid_mask || !code_weights || !out || !unit_cls || !unit_reg)
    return LINK_ERR_ARG;
  if (!isfinite(cls_weight) || !isfinite(reg_weight)) return LINK_ERR_ARG;
  CodeW cw;
  for (int c = 0; c < 9; c++) cw.w[c] = c < code ? code_weights[c] : 0.f;
  const long long *rv = reinterpret_cast<const long long *>(reg_valid_mask);
  dispatch_row_io(io_dtype, [&](auto io) {
    hipLaunchKernelGGL(k_roi_loss<decltype(io)::value>, dim3(1), dim3(T), 0, S(stream), rcnn_cls, rcnn_reg, (int)n, (int)code, cls_labels,
                       gt_of_rois, rv, cw, cls_weight, reg_weight, out, unit_cls, unit_reg);
  });
  return check_launch("link_roi_loss_forward");
}

extern "C" int link_roi_loss_backward(const float *unit_cls, const float *unit_reg, const float *upstream, int64_t n, int32_t code,
                                      int32_t io_dtype, void *grad_cls, void *grad_reg, void *stream) {
  if (!row_io_ok(io_dtype) || (code != 7 && code != 9) || n < 1 || n > LINK_ROI_MAX_LOSS_ROWS) return LINK_ERR_ARG;
  if (!unit_cls || !unit_reg || !upstream || !grad_cls || !grad_reg) return LINK_ERR_ARG;
  const dim3 grid(blocks_for(n * code, T)), block(T);
  dispatch_row_io(io_dtype, [&](auto io) {
    hipLaunchKernelGGL(k_roi_loss_bwd<decltype(io)::value>, grid, block, 0, S(stream), unit_cls, unit_reg, upstream, (int)n, (int)code,
                       grad_cls, grad_reg);
  });
  return check_launch("link_roi_loss_backward");
}

extern "C" int link_roi_refine(const float *rois, const int64_t *roi_labels, const float *roi_scores, const void *rcnn_cls,
                               const void *rcnn_reg, int32_t io_dtype, int32_t batch, int64_t r, int32_t code, float *boxes, float *scores,
                               int64_t *labels, int32_t *counts, void *stream) {
  if (!row_io_ok(io_dtype) || (code != 7 && code != 9) || batch < 0 || batch > 65535 || r < 0 || r >= (1LL << 31) ||
      (int64_t)batch * r * code >= (1LL << 31))
    return LINK_ERR_ARG;
  if (batch == 0) return LINK_OK;
  if (!counts) return LINK_ERR_ARG;
  if (r > 0 && (!rois || !roi_labels || !roi_scores || !rcnn_cls || !rcnn_reg || !boxes || !scores || !labels)) return LINK_ERR_ARG;
  const long long *lb = reinterpret_cast<const long long *>(roi_labels);
  long long *ol = reinterpret_cast<long long *>(labels);
  dispatch_row_io(io_dtype, [&](auto io) {
    hipLaunchKernelGGL(k_roi_refine<decltype(io)::value>, dim3(batch), dim3(T), 0, S(stream), rois, lb, roi_scores, rcnn_cls, rcnn_reg, (int)r,
                       (int)code, boxes, scores, ol, counts);
  });
  return check_launch("link_roi_refine");
}
