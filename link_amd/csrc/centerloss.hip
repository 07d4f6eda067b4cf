// link_amd/csrc/centerloss.hip -- section L of include/link_amd.h: CenterHead training on the device.  Target assignment
// (detection/det3d/datasets/pipelines/preprocess.py:283-467 with det3d/core/utils/center_utils.py:17-63), the focal loss and the L1
// regression loss (det3d/models/losses/centernet_loss.py) as CenterHead.loss combines them (det3d/models/bbox_heads/center_head.py:
// 248-293), forward and gradient, with no host read-back, no allocation and no float atomics.
//
//   k_assign_clear   zeroes the heat maps of every task (one grid over all of them)
//   k_assign         one workgroup per (frame, task): task-local class of every object into LDS, class counts (LDS integer atomics),
//                    the slot of every object (objects of smaller classes + earlier objects of its own class), then slot by slot the
//                    anno_box / ind / mask / cat rows in full, then one wave per drawn slot splats its clipped Gaussian by an integer
//                    atomic max on the bit pattern (values >= 0: order-independent)
//   k_loss_map       the map pass: 1024 elements per workgroup, one 4-wide load per thread; neg part by a fixed-shape tree into the
//                    workspace, the dense unit gradient -d neg / num_pos (num_pos: every workgroup sums the mask bytes itself -- an
//                    integer sum, a few KB out of L2, instead of one more launch in front)
//   k_loss_slots     one workgroup per frame: the pos part, the L1 parts per column, unit_box, and the pos gradient added into unit_hm
//                    at the slots' cells -- slots sharing a cell add in ascending slot order by the thread of the lowest slot
//   k_loss_final     one workgroup: the workgroups' parts in workgroup order, out[16]
//   k_bwd_map        d hm = unit_hm * upstream, rounded once; zero fill of the five regression gradients
//   k_bwd_slots      one workgroup per frame: the regression gradients at the ind cells, duplicates added as above
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>

#include "block_prims.h"
#include "dispatch.h"
#include "row_io.h"

#pragma clang fp contract(off)

using namespace link;

namespace {

constexpr int T = 256;
constexpr int VEC = 4;
constexpr int TILE = T * VEC;              // map elements per workgroup
constexpr int NCOL = 10;

struct AssignPtrs {
  float *hm[LINK_CENTER_MAX_TASKS];
  float *anno[LINK_CENTER_MAX_TASKS];
  int64_t *ind[LINK_CENTER_MAX_TASKS];
  uint8_t *mask[LINK_CENTER_MAX_TASKS];
  int64_t *cat[LINK_CENTER_MAX_TASKS];
  int64_t hm_end[LINK_CENTER_MAX_TASKS];   // running end of every task's heat map in the concatenation k_assign_clear walks
  int32_t first_class[LINK_CENTER_MAX_TASKS];
};

struct RegMaps {
  const void *p[5];                        // reg, height, dim, vel, rot
  int64_t bs[5];                           // elements from one frame of the map to the next
};
struct RegGrads {
  void *p[5];
  int64_t bs[5];
};
struct Weights {
  float cw[NCOL];
};

// column c of the box code -> (map, channel of the map, column of the target row)
__device__ __forceinline__ void column_of(int c, bool has_vel, int &map, int &ch, int &tcol) {
  if (c < 2) { map = 0; ch = c; tcol = c; }
  else if (c == 2) { map = 1; ch = 0; tcol = 2; }
  else if (c < 6) { map = 2; ch = c - 3; tcol = c; }
  else if (has_vel && c < 8) { map = 3; ch = c - 6; tcol = c; }
  else { map = 4; ch = has_vel ? c - 8 : c - 6; tcol = has_vel ? c : c + 2; }
}
__device__ __forceinline__ int channels_of(int map) { return map == 1 ? 1 : (map == 2 ? 3 : 2); }

// ------------------------------------------------------------------------------------------------------------------- assign
__global__ void __launch_bounds__(T) k_assign_clear(AssignPtrs P, int ntasks, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * T;
  for (int64_t e = (int64_t)blockIdx.x * T + threadIdx.x; e < total; e += stride) {
    int t = 0;
    while (t < ntasks - 1 && e >= P.hm_end[t]) ++t;
    const int64_t off = e - (t ? P.hm_end[t - 1] : 0);
    P.hm[t][off] = 0.f;
  }
}

// min(r1, r2, r3) of center_utils.py:17-37 in float64 (the third root as the reference writes it)
__device__ __forceinline__ double gaussian_radius64(double height, double width, double ov) {
  const double b1 = height + width;
  const double c1 = width * height * (1.0 - ov) / (1.0 + ov);
  const double r1 = (b1 + sqrt(b1 * b1 - 4.0 * c1)) / 2.0;
  const double b2 = 2.0 * (height + width);
  const double c2 = (1.0 - ov) * width * height;
  const double r2 = (b2 + sqrt(b2 * b2 - 16.0 * c2)) / 2.0;
  const double a3 = 4.0 * ov;
  const double b3 = -2.0 * ov * (height + width);
  const double c3 = (ov - 1.0) * width * height;
  const double r3 = (b3 + sqrt(b3 * b3 - 4.0 * a3 * c3)) / 2.0;
  return fmin(r1, fmin(r2, r3));
}

__global__ void __launch_bounds__(T) k_assign(link_center_assign_geom_t G, AssignPtrs P, const float *__restrict__ boxes,
                                              const int32_t *__restrict__ classes, int n_cap) {
  __shared__ signed char tcls[LINK_CENTER_MAX_OBJECTS];     // class inside the task, -1: not this task's
  __shared__ int owner[LINK_CENTER_MAX_OBJECTS];            // object of slot k, -1: none
  __shared__ int dxy[LINK_CENTER_MAX_OBJECTS];              // drawn slots: x | y << 16, -1: not drawn
  __shared__ int drad[LINK_CENTER_MAX_OBJECTS];
  __shared__ int cnt[LINK_CENTER_MAX_CLASSES], cbase[LINK_CENTER_MAX_CLASSES];
  const int t = threadIdx.x, task = blockIdx.x, b = blockIdx.y;
  const int K = G.num_classes[task], first = P.first_class[task];
  const int M = G.max_objs, W = G.w, H = G.h;
  const int nslots = n_cap < M ? n_cap : M;                 // slots past the objects stay empty
  const int32_t *cls = classes + (int64_t)b * n_cap;
  if (t < LINK_CENTER_MAX_CLASSES) cnt[t] = 0;
  for (int i = t; i < n_cap; i += T) owner[i] = -1;
  __syncthreads();
  for (int i = t; i < n_cap; i += T) {
    const int64_t c = (int64_t)cls[i] - 1 - first;
    const bool mine = c >= 0 && c < K;
    tcls[i] = mine ? (signed char)c : (signed char)-1;
    if (mine) atomicAdd(&cnt[c], 1);
  }
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int c = 0; c < K; ++c) {
      cbase[c] = run;
      run += cnt[c];
    }
  }
  __syncthreads();
  for (int i = t; i < n_cap; i += T) {
    const int c = tcls[i];
    if (c < 0) continue;
    int rank = cbase[c];
    for (int j = 0; j < i; ++j) rank += tcls[j] == c;
    if (rank < nslots) owner[rank] = i;
  }
  __syncthreads();
  float *anno = P.anno[task] + (int64_t)b * M * NCOL;
  int64_t *ind = P.ind[task] + (int64_t)b * M;
  uint8_t *mask = P.mask[task] + (int64_t)b * M;
  int64_t *cat = P.cat[task] + (int64_t)b * M;
  const float osf = (float)G.out_size_factor;
  for (int k = t; k < M; k += T) {
    float row[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) row[c] = 0.f;
    int64_t o_ind = 0, o_cat = 0;
    uint8_t o_mask = 0;
    int draw_xy = -1, draw_r = 0;
    const int i = k < nslots ? owner[k] : -1;
    if (i >= 0) {
      const float *g = boxes + ((int64_t)b * n_cap + i) * 9;
      const float w = __fdiv_rn(__fdiv_rn(g[3], G.voxel_size[0]), osf);
      const float l = __fdiv_rn(__fdiv_rn(g[4], G.voxel_size[1]), osf);
      const float cx = __fdiv_rn(__fdiv_rn(__fsub_rn(g[0], G.pc_range[0]), G.voxel_size[0]), osf);
      const float cy = __fdiv_rn(__fdiv_rn(__fsub_rn(g[1], G.pc_range[1]), G.voxel_size[1]), osf);
      // ct_int = trunc(ct) inside the map  <=>  -1 < ct < size (NaN fails every comparison)
      if (w > 0.f && l > 0.f && cx > -1.f && cx < (float)W && cy > -1.f && cy < (float)H) {
        const int x = (int)cx, y = (int)cy;
        const double rr = gaussian_radius64((double)l, (double)w, (double)G.gaussian_overlap);
        int r = rr >= 2147483000.0 ? 2147483000 : (rr > 0.0 ? (int)rr : 0);      // int(): toward zero; NaN -> 0
        if (rr < 0.0) r = (int)fmax(rr, -2147483000.0);
        r = r > G.min_radius ? r : G.min_radius;
        draw_xy = x | (y << 16);
        draw_r = r;
        o_ind = (int64_t)y * W + x;
        o_cat = tcls[i];
        o_mask = 1;
        const float P2 = 6.28318530717958647692f;                                  // fp32(2 pi)
        const float rot = __fsub_rn(g[8], __fmul_rn(floorf(__fadd_rn(__fdiv_rn(g[8], P2), 0.5f)), P2));
        row[0] = __fsub_rn(cx, (float)x);
        row[1] = __fsub_rn(cy, (float)y);
        row[2] = g[2];
        row[3] = (float)log((double)g[3]);
        row[4] = (float)log((double)g[4]);
        row[5] = (float)log((double)g[5]);
        row[6] = g[6];
        row[7] = g[7];
        row[8] = (float)sin((double)rot);
        row[9] = (float)cos((double)rot);
      }
    }
#pragma unroll
    for (int c = 0; c < NCOL; ++c) anno[(int64_t)k * NCOL + c] = row[c];
    ind[k] = o_ind;
    mask[k] = o_mask;
    cat[k] = o_cat;
    if (k < nslots) {
      dxy[k] = draw_xy;
      drad[k] = draw_r;
    }
  }
  __syncthreads();
  // one wave per drawn slot
  const int lane = t & 63, wave = t >> 6;
  unsigned *hm = reinterpret_cast<unsigned *>(P.hm[task]) + (int64_t)b * K * H * W;
  for (int k = wave; k < nslots; k += T / 64) {
    const int xy = dxy[k];
    if (xy < 0) continue;                                                          // uniform over the wave
    const int x = xy & 0xFFFF, y = xy >> 16, r = drad[k];
    if (r < 0) continue;                                                           // a negative radius draws an empty window
    const int c = tcls[owner[k]];
    const int left = x < r ? x : r, right = W - x < r + 1 ? W - x : r + 1;
    const int top = y < r ? y : r, bottom = H - y < r + 1 ? H - y : r + 1;
    const int ww = left + right, hh = top + bottom;
    if (ww <= 0 || hh <= 0) continue;
    const double sigma = (2.0 * (double)r + 1.0) / 6.0;
    const double den = 2.0 * sigma * sigma;
    unsigned *plane = hm + (int64_t)c * H * W;
    for (int e = lane; e < ww * hh; e += 64) {
      const int px = x - left + e % ww, py = y - top + e / ww;
      if (px < 0 || px >= W || py < 0 || py >= H) continue;                        // holds by construction
      const double dx = (double)(px - x), dy = (double)(py - y);
      const float v = (float)exp(-(dx * dx + dy * dy) / den);
      atomicMax(&plane[(int64_t)py * W + px], __float_as_uint(v));
    }
  }
}

// --------------------------------------------------------------------------------------------------------------------- loss
constexpr float CLAMP_LO = 1e-4f, CLAMP_HI = 1.0f - 1e-4f;

// y and dy / dx of one heat-map input
__device__ __forceinline__ void activate(float x, int probas, float &y, float &dydx) {
  if (probas) {
    y = x;
    dydx = 1.f;
    return;
  }
  const float s = 1.0f / (1.0f + expf(-x));
  y = fminf(fmaxf(s, CLAMP_LO), CLAMP_HI);
  dydx = (s >= CLAMP_LO && s <= CLAMP_HI) ? s * (1.0f - s) : 0.f;
  if (!(fabsf(x) < INFINITY)) {                                                     // a logit that is not finite stays visible: NaN
    y = NAN;
    dydx = NAN;
  }
}

__device__ __forceinline__ void neg_term(float x, float tg, int probas, float &val, float &grad) {
  float y, dydx;
  activate(x, probas, y, dydx);
  const float om = 1.0f - tg, g4 = (om * om) * (om * om);
  const float l1 = log1pf(-y);                                                      // log(1 - y)
  val = l1 * (y * y) * g4;
  grad = (2.0f * y * l1 - (y * y) / (1.0f - y)) * g4 * dydx;
}

__device__ __forceinline__ int count_mask(const uint8_t *__restrict__ mask, int64_t n, int *lds) {
  int c = 0;
  for (int64_t i = threadIdx.x; i < n; i += T) c += mask[i] != 0;
  return block_sum_fixed(c, lds);
}

template <int IO, bool VEC4>
__global__ void __launch_bounds__(T) k_loss_map(const void *__restrict__ hm, const float *__restrict__ target, int64_t n, int probas,
                                                const uint8_t *__restrict__ mask, int64_t nmask, float *__restrict__ part,
                                                float *__restrict__ unit_hm) {
  __shared__ float fl[T];
  __shared__ int il[T];
  const int t = threadIdx.x;
  const int npos = count_mask(mask, nmask, il);
  const float scale = npos > 0 ? -1.0f / (float)npos : -1.0f;
  const int64_t e0 = (int64_t)blockIdx.x * TILE + (int64_t)t * VEC;
  float acc = 0.f;
  if (VEC4 && e0 + VEC <= n) {
    const float4 x = row_ld4<IO>(hm, e0);
    const float4 tg = *reinterpret_cast<const float4 *>(target + e0);
    float4 g;
    float v0, v1, v2, v3;
    neg_term(x.x, tg.x, probas, v0, g.x);
    neg_term(x.y, tg.y, probas, v1, g.y);
    neg_term(x.z, tg.z, probas, v2, g.z);
    neg_term(x.w, tg.w, probas, v3, g.w);
    acc = ((v0 + v1) + v2) + v3;
    g.x *= scale; g.y *= scale; g.z *= scale; g.w *= scale;
    *reinterpret_cast<float4 *>(unit_hm + e0) = g;
  } else {
    for (int j = 0; j < VEC; ++j) {
      const int64_t e = e0 + j;
      if (e < n) {
        float v, g;
        neg_term(row_ld1<IO>(hm, e), target[e], probas, v, g);
        acc = j ? acc + v : v;
        unit_hm[e] = g * scale;
      }
    }
  }
  const float s = block_sum_fixed(acc, fl);
  if (t == 0) part[blockIdx.x] = s;
}

template <int IO>
__global__ void __launch_bounds__(T) k_loss_slots(const void *__restrict__ hm, RegMaps R, int has_vel, int probas,
                                                  const float *__restrict__ anno, const int64_t *__restrict__ ind,
                                                  const uint8_t *__restrict__ mask, const int64_t *__restrict__ cat, int B, int K,
                                                  int HW, int M, Weights Wt, float weight, float *__restrict__ fpart,
                                                  float *__restrict__ unit_hm, float *__restrict__ unit_box) {
  __shared__ int key[LINK_CENTER_MAX_SLOTS];                 // cat * HW + ind of a slot that counts, -1 otherwise
  __shared__ float gpos[LINK_CENTER_MAX_SLOTS];
  __shared__ float fl[T];
  __shared__ int il[T];
  const int t = threadIdx.x, b = blockIdx.x;
  const int ncol = has_vel ? NCOL : NCOL - 2;
  const bool has_hm = hm != nullptr, has_reg = R.p[0] != nullptr;
  const int npos = count_mask(mask, (int64_t)B * M, il);
  const float hscale = npos > 0 ? -1.0f / (float)npos : -1.0f;
  const float bscale = weight / ((float)npos + 1e-4f);
  float pos = 0.f, box[NCOL];
#pragma unroll
  for (int c = 0; c < NCOL; ++c) box[c] = 0.f;
  for (int m = t; m < M; m += T) {
    const int64_t s = (int64_t)b * M + m;
    int kk = -1;
    float gp = 0.f;
    float u[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) u[c] = 0.f;
    if (mask[s] != 0) {
      const int64_t id = ind[s], ct = has_hm ? cat[s] : 0;
      if (id >= 0 && id < HW && ct >= 0 && ct < K) {
        kk = (int)(ct * HW + id);
        if (has_hm) {
          float y, dydx;
          activate(row_ld1<IO>(hm, (int64_t)b * K * HW + kk), probas, y, dydx);
          const float ly = logf(y), om = 1.0f - y;
          pos += ly * (om * om);
          gp = ((om * om) / y - 2.0f * om * ly) * dydx * hscale;
        }
#pragma unroll
        for (int c = 0; c < NCOL; ++c) {
          if (has_reg && c < ncol) {
            int map, ch, tcol;
            column_of(c, has_vel != 0, map, ch, tcol);
            const float pred = row_ld1<IO>(R.p[map], (int64_t)b * R.bs[map] + (int64_t)ch * HW + id);
            const float d = pred - anno[s * NCOL + tcol];
            box[c] += fabsf(d);
            u[c] = (d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.f)) * (Wt.cw[c] * bscale);
          }
        }
      }
    }
    key[m] = kk;
    gpos[m] = gp;
    if (has_reg) {
#pragma unroll
      for (int c = 0; c < NCOL; ++c) unit_box[s * NCOL + c] = u[c];
    }
  }
  __syncthreads();
  float *fp = fpart + (int64_t)b * (NCOL + 1);
  {
    const float s = block_sum_fixed(pos, fl);
    if (t == 0) fp[0] = s;
  }
#pragma unroll
  for (int c = 0; c < NCOL; ++c) {
    const float s = block_sum_fixed(box[c], fl);
    if (t == 0) fp[1 + c] = s;
  }
  // the pos gradient into the dense map: one writer per cell, the slots of a cell in ascending order
  if (!has_hm) return;
  for (int m = t; m < M; m += T) {
    const int kk = key[m];
    if (kk < 0) continue;
    bool lowest = true;
    for (int j = 0; j < m; ++j) lowest &= key[j] != kk;
    if (!lowest) continue;
    float g = gpos[m];
    for (int j = m + 1; j < M; ++j)
      if (key[j] == kk) g += gpos[j];
    unit_hm[(int64_t)b * K * HW + kk] += g;
  }
}

__global__ void __launch_bounds__(T) k_loss_final(const float *__restrict__ part, int64_t nblk, const float *__restrict__ fpart, int B,
                                                  const uint8_t *__restrict__ mask, int64_t nmask, int has_vel, Weights Wt, float weight,
                                                  float *__restrict__ out) {
  __shared__ float fl[T];
  __shared__ int il[T];
  __shared__ float res[NCOL + 1];
  const int t = threadIdx.x;
  const int npos = count_mask(mask, nmask, il);
  float a = 0.f;
  for (int64_t i = t; i < nblk; i += T) a += part[i];
  const float neg = block_sum_fixed(a, fl);
  for (int c = 0; c < NCOL + 1; ++c) {
    float v = 0.f;
    for (int i = t; i < B; i += T) v += fpart[(int64_t)i * (NCOL + 1) + c];
    const float s = block_sum_fixed(v, fl);
    if (t == 0) res[c] = s;
  }
  __syncthreads();
  if (t == 0) {
    const int ncol = has_vel ? NCOL : NCOL - 2;
    const float pos = res[0];
    const float hm_loss = npos > 0 ? -(pos + neg) / (float)npos : -neg;
    float loc = 0.f;
    for (int c = 0; c < NCOL; ++c) {
      const float bl = c < ncol ? res[1 + c] / ((float)npos + 1e-4f) : 0.f;
      out[4 + c] = bl;
      if (c < ncol) loc += bl * Wt.cw[c];
    }
    out[0] = hm_loss + weight * loc;
    out[1] = hm_loss;
    out[2] = loc;
    out[3] = (float)npos;
    out[14] = 0.f;
    out[15] = 0.f;
  }
}

// ----------------------------------------------------------------------------------------------------------------- backward
// blocks [0, nblk_hm): d hm; blocks after them: zero fill of the regression gradients, laid end to end as [B, 10 or 8, HW]
template <int IO, bool VEC4>
__global__ void __launch_bounds__(T) k_bwd_map(const float *__restrict__ unit_hm, const float *__restrict__ upstream, int64_t n,
                                               int64_t nblk_hm, void *__restrict__ grad_hm, RegGrads G, int has_vel, int B, int HW) {
  const int t = threadIdx.x;
  if ((int64_t)blockIdx.x < nblk_hm) {
    const float s = upstream[0];
    const int64_t e0 = (int64_t)blockIdx.x * TILE + (int64_t)t * VEC;
    if (VEC4 && e0 + VEC <= n) {
      float4 u = *reinterpret_cast<const float4 *>(unit_hm + e0);
      u.x *= s; u.y *= s; u.z *= s; u.w *= s;
      row_st4<IO>(grad_hm, e0, u);
    } else {
      for (int j = 0; j < VEC; ++j)
        if (e0 + j < n) row_st1<IO>(grad_hm, e0 + j, unit_hm[e0 + j] * s);
    }
    return;
  }
  const int64_t q0 = ((int64_t)blockIdx.x - nblk_hm) * TILE + (int64_t)t * VEC;
  for (int j = 0; j < VEC; ++j) {
    int64_t q = q0 + j;                                                            // element of the concatenation of the five maps
    for (int map = 0; map < 5; ++map) {
      if (map == 3 && !has_vel) continue;
      const int64_t per = (int64_t)channels_of(map) * HW, sz = (int64_t)B * per;
      if (q < sz) {
        row_st1<IO>(G.p[map], (q / per) * G.bs[map] + q % per, 0.f);
        break;
      }
      q -= sz;
    }
  }
}

template <int IO>
__global__ void __launch_bounds__(T) k_bwd_slots(const float *__restrict__ unit_box, const int64_t *__restrict__ ind,
                                                 const uint8_t *__restrict__ mask, const float *__restrict__ upstream, int HW, int M,
                                                 RegGrads G, int has_vel) {
  __shared__ int key[LINK_CENTER_MAX_SLOTS];
  const int t = threadIdx.x, b = blockIdx.x;
  const int ncol = has_vel ? NCOL : NCOL - 2;
  for (int m = t; m < M; m += T) {
    const int64_t s = (int64_t)b * M + m;
    int kk = -1;
    if (mask[s] != 0) {
      const int64_t id = ind[s];
      if (id >= 0 && id < HW) kk = (int)id;
    }
    key[m] = kk;
  }
  __syncthreads();
  const float up = upstream[0];
  for (int m = t; m < M; m += T) {
    const int kk = key[m];
    if (kk < 0) continue;
    bool lowest = true;
    for (int j = 0; j < m; ++j) lowest &= key[j] != kk;
    if (!lowest) continue;
    float g[NCOL];
    const float *u = unit_box + ((int64_t)b * M + m) * NCOL;
#pragma unroll
    for (int c = 0; c < NCOL; ++c) g[c] = u[c];
    for (int j = m + 1; j < M; ++j) {
      if (key[j] != kk) continue;
      const float *uj = unit_box + ((int64_t)b * M + j) * NCOL;
#pragma unroll
      for (int c = 0; c < NCOL; ++c) g[c] += uj[c];
    }
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      if (c < ncol) {
        int map, ch, tcol;
        column_of(c, has_vel != 0, map, ch, tcol);
        row_st1<IO>(G.p[map], (int64_t)b * G.bs[map] + (int64_t)ch * HW + kk, g[c] * up);
      }
    }
  }
}

inline bool loss_shape_ok(int32_t batch, int32_t k, int32_t h, int32_t w, int32_t max_objs) {
  if (batch < 1 || batch > LINK_CENTER_MAX_BATCH || k < 1 || k > LINK_CENTER_MAX_CLASSES || h < 1 || w < 1 || max_objs < 1 ||
      max_objs > LINK_CENTER_MAX_SLOTS)
    return false;
  const int64_t hw = (int64_t)h * w;                       // < 2^62
  if (hw >= (1LL << 31)) return false;
  const int64_t kk = k > 3 ? k : 3;
  return (int64_t)batch * kk * hw < (1LL << 31) - TILE;
}

inline int64_t map_blocks(int64_t n) { return (n + TILE - 1) / TILE; }

}  // namespace

// ----------------------------------------------------------------------------------------------------------------- C entries
extern "C" int link_center_assign(const link_center_assign_geom_t *geom, const float *gt_boxes, const int32_t *gt_classes, int32_t batch,
                                  int32_t n_cap, float *const *hm, float *const *anno_box, int64_t *const *ind, uint8_t *const *mask,
                                  int64_t *const *cat, void *stream) {
  if (!geom || !hm || !anno_box || !ind || !mask || !cat || batch < 1 || n_cap < 0 || n_cap > LINK_CENTER_MAX_OBJECTS) return LINK_ERR_ARG;
  if (n_cap > 0 && (!gt_boxes || !gt_classes)) return LINK_ERR_ARG;
  const link_center_assign_geom_t &g = *geom;
  if (g.num_tasks < 1 || g.num_tasks > LINK_CENTER_MAX_TASKS || g.w < 1 || g.h < 1 || g.w > 32767 || g.h > 32767 || g.max_objs < 1 ||
      g.out_size_factor < 1 || g.min_radius < 0 || !(g.voxel_size[0] > 0.f) || !(g.voxel_size[1] > 0.f) ||
      !(g.gaussian_overlap > 0.f && g.gaussian_overlap < 1.f) || !(g.pc_range[0] == g.pc_range[0]) || !(g.pc_range[1] == g.pc_range[1]))
    return LINK_ERR_ARG;
  if ((int64_t)batch * g.max_objs * NCOL >= (1LL << 31)) return LINK_ERR_ARG;
  AssignPtrs P;
  int64_t total = 0;
  int32_t first = 0;
  for (int t = 0; t < LINK_CENTER_MAX_TASKS; ++t) {
    const bool on = t < g.num_tasks;
    if (on) {
      if (g.num_classes[t] < 1 || g.num_classes[t] > LINK_CENTER_MAX_CLASSES) return LINK_ERR_ARG;
      if (!hm[t] || !anno_box[t] || !ind[t] || !mask[t] || !cat[t]) return LINK_ERR_ARG;
      const int64_t sz = (int64_t)batch * g.num_classes[t] * g.h * g.w;
      if (sz >= (1LL << 31)) return LINK_ERR_ARG;
      total += sz;
    }
    P.hm[t] = on ? hm[t] : nullptr;
    P.anno[t] = on ? anno_box[t] : nullptr;
    P.ind[t] = on ? ind[t] : nullptr;
    P.mask[t] = on ? mask[t] : nullptr;
    P.cat[t] = on ? cat[t] : nullptr;
    P.hm_end[t] = total;
    P.first_class[t] = first;
    if (on) first += g.num_classes[t];
  }
  hipStream_t s = S(stream);
  int64_t nb = (total + T - 1) / T;
  nb = nb > 2048 ? 2048 : nb;
  hipLaunchKernelGGL(k_assign_clear, dim3((unsigned)nb), dim3(T), 0, s, P, (int)g.num_tasks, total);
  hipLaunchKernelGGL(k_assign, dim3((unsigned)g.num_tasks, (unsigned)batch), dim3(T), 0, s, g, P, gt_boxes, gt_classes, (int)n_cap);
  return check_launch("link_center_assign");
}

extern "C" size_t link_center_loss_workspace_bytes(int32_t batch, int32_t k, int32_t h, int32_t w, int32_t max_objs) {
  if (!loss_shape_ok(batch, k, h, w, max_objs)) return 0;
  const int64_t n = (int64_t)batch * k * h * w;
  return up256((size_t)map_blocks(n) * 4) + up256((size_t)batch * (NCOL + 1) * 4);
}

namespace {
// the five regression maps: all or none (vel aside); frames of a map `strides[i]` elements apart (NULL: contiguous)
inline bool reg_table(const void *reg, const void *height, const void *dim, const void *vel, const void *rot, const int64_t *strides,
                      int64_t hw, const void **p, int64_t *bs, bool &has_reg) {
  const int some = (reg != nullptr) + (height != nullptr) + (dim != nullptr) + (rot != nullptr);
  if (some != 0 && some != 4) return false;
  has_reg = some == 4;
  if (!has_reg && vel) return false;
  const void *q[5] = {reg, height, dim, vel, rot};
  const int ch[5] = {2, 1, 3, 2, 2};
  for (int i = 0; i < 5; ++i) {
    p[i] = q[i];
    bs[i] = strides ? strides[i] : ch[i] * hw;
    if (q[i] && (bs[i] < ch[i] * hw || bs[i] >= (1LL << 40))) return false;
  }
  return true;
}
}  // namespace

extern "C" int link_center_loss_forward(const void *hm, const void *reg, const void *height, const void *dim, const void *vel, const void *rot,
                                        const int64_t *reg_batch_strides, int32_t io_dtype, int32_t input_kind, const float *hm_target,
                                        const float *anno_box, const int64_t *ind, const uint8_t *mask, const int64_t *cat, int32_t batch,
                                        int32_t k, int32_t h, int32_t w, int32_t max_objs, const float *code_weights, float weight,
                                        void *workspace, size_t workspace_bytes, float *out, float *unit_hm, float *unit_box, void *stream) {
  if (!ind || !mask || !workspace || !out || !loss_shape_ok(batch, k, h, w, max_objs) || !row_io_ok(io_dtype) ||
      (input_kind != LINK_CENTER_LOGITS && input_kind != LINK_CENTER_PROBAS))
    return LINK_ERR_ARG;
  RegMaps R;
  bool has_reg = false;
  if (!reg_table(reg, height, dim, vel, rot, reg_batch_strides, (int64_t)h * w, R.p, R.bs, has_reg)) return LINK_ERR_ARG;
  if (!hm && !has_reg) return LINK_ERR_ARG;
  if (hm && (!hm_target || !cat || !unit_hm)) return LINK_ERR_ARG;
  if (has_reg && (!anno_box || !code_weights || !unit_box)) return LINK_ERR_ARG;
  const int64_t n = (int64_t)batch * k * h * w, nblk = map_blocks(n), nmask = (int64_t)batch * max_objs;
  const size_t need = up256((size_t)nblk * 4) + up256((size_t)batch * (NCOL + 1) * 4);
  if (workspace_bytes < need) return LINK_ERR_WORKSPACE;
  float *part = reinterpret_cast<float *>(workspace);
  float *fpart = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + up256((size_t)nblk * 4));
  const int probas = input_kind == LINK_CENTER_PROBAS, has_vel = vel != nullptr, HW = h * w;
  const bool v4 = aligned_to(hm, 16) && aligned_to(hm_target, 16) && aligned_to(unit_hm, 16);
  Weights Wt;
  for (int c = 0; c < NCOL; ++c) Wt.cw[c] = has_reg && c < (has_vel ? NCOL : NCOL - 2) ? code_weights[c] : 0.f;
  hipStream_t s = S(stream);
  const dim3 gm((unsigned)nblk), gb((unsigned)batch), tb(T);
  dispatch_row_io(io_dtype, [&](auto io) {
    constexpr int IO = decltype(io)::value;
    if (hm && v4)
      hipLaunchKernelGGL((k_loss_map<IO, true>), gm, tb, 0, s, hm, hm_target, n, probas, mask, nmask, part, unit_hm);
    else if (hm)
      hipLaunchKernelGGL((k_loss_map<IO, false>), gm, tb, 0, s, hm, hm_target, n, probas, mask, nmask, part, unit_hm);
    hipLaunchKernelGGL(k_loss_slots<IO>, gb, tb, 0, s, hm, R, has_vel, probas, anno_box, ind, mask, cat, (int)batch, (int)k, HW,
                       (int)max_objs, Wt, weight, fpart, unit_hm, unit_box);
  });
  hipLaunchKernelGGL(k_loss_final, dim3(1), tb, 0, s, part, hm ? nblk : (int64_t)0, fpart, (int)batch, mask, nmask, has_vel, Wt, weight, out);
  return check_launch("link_center_loss_forward");
}

extern "C" int link_center_loss_backward(const float *unit_hm, const float *unit_box, const int64_t *ind, const uint8_t *mask,
                                         const float *upstream, int32_t batch, int32_t k, int32_t h, int32_t w, int32_t max_objs,
                                         int32_t io_dtype, void *grad_hm, void *grad_reg, void *grad_height, void *grad_dim, void *grad_vel,
                                         void *grad_rot, const int64_t *reg_batch_strides, void *stream) {
  if (!ind || !mask || !upstream || !loss_shape_ok(batch, k, h, w, max_objs) || !row_io_ok(io_dtype)) return LINK_ERR_ARG;
  RegGrads G;
  bool has_reg = false;
  {
    const void *p[5];
    if (!reg_table(grad_reg, grad_height, grad_dim, grad_vel, grad_rot, reg_batch_strides, (int64_t)h * w, p, G.bs, has_reg)) return LINK_ERR_ARG;
    void *q[5] = {grad_reg, grad_height, grad_dim, grad_vel, grad_rot};
    for (int i = 0; i < 5; ++i) G.p[i] = q[i];
  }
  if ((!grad_hm && !has_reg) || (grad_hm && !unit_hm) || (has_reg && !unit_box)) return LINK_ERR_ARG;
  const int has_vel = grad_vel != nullptr, HW = h * w;
  const int64_t n = (int64_t)batch * k * HW, nblk = grad_hm ? map_blocks(n) : 0;
  const int64_t nreg = has_reg ? (int64_t)batch * (has_vel ? NCOL : NCOL - 2) * HW : 0;      // batch * 3 * hw < 2^31: < 2^33
  const int64_t nblk_reg = map_blocks(nreg);
  if (nblk + nblk_reg >= (1LL << 31)) return LINK_ERR_ARG;
  const bool v4 = aligned_to(unit_hm, 16) && aligned_to(grad_hm, 16);
  hipStream_t s = S(stream);
  const dim3 gm((unsigned)(nblk + nblk_reg)), gb((unsigned)batch), tb(T);
  dispatch_row_io(io_dtype, [&](auto io) {
    constexpr int IO = decltype(io)::value;
    if (v4)
      hipLaunchKernelGGL((k_bwd_map<IO, true>), gm, tb, 0, s, unit_hm, upstream, n, nblk, grad_hm, G, has_vel, (int)batch, HW);
    else
      hipLaunchKernelGGL((k_bwd_map<IO, false>), gm, tb, 0, s, unit_hm, upstream, n, nblk, grad_hm, G, has_vel, (int)batch, HW);
    if (has_reg) hipLaunchKernelGGL(k_bwd_slots<IO>, gb, tb, 0, s, unit_box, ind, mask, upstream, HW, (int)max_objs, G, has_vel);
  });
  return check_launch("link_center_loss_backward");
}
