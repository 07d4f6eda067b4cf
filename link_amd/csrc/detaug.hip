// link_amd/csrc/detaug.hip -- the detection training front end on the device (section P of include/link_amd.h): points against
// rotated boxes (the mask and the per-box counts), the corners of BEV boxes, the BEV collision matrix, the ground-truth sampler's
// acceptance scan for a batch, and the paste fused with the global flips, rotation, scaling, translation and the point shuffle.
//
// Semantics: detection/det3d/core/bbox/box_np_ops.py:15-20, 641-647 (points_count_rbbox, points_in_rbbox) over geometry.py:215-276
// (a point is outside when any surface has a p + d >= 0), box_np_ops.py:55-85, 207-220, 265-285 (center_to_corner_box2d) and
// detection/det3d/core/sampler/preprocess.py:854-937 (box_collision_test), :108-122, 771-839, 940-962 (the range filter and the global
// transforms), core/sampler/sample_ops.py:97-296 (sample_all, sample_class_v2) and datasets/pipelines/preprocess.py:51-167
// (Preprocess).  The implementation is this project's.
//
// Contraction is off: the collision test compares products the reference rounds one by one, and so do the products here.
#pragma clang fp contract(off)
#include <math.h>

#include "block_prims.h"

using namespace link;

namespace {

constexpr int BOX_TILE = 256;                  // boxes staged per pass: 8 floats each, 8 KiB of LDS

// ---- P1: points against rotated boxes -------------------------------------------------------------------------------------------
// The reference builds eight corners and six inward surfaces per box and calls a point outside when any surface gives
// a p + d >= 0.  The same decision in the box frame: q = p - centre turned back by the heading (the corners are turned by
// x' = x c + y s, y' = -x s + y c, so the way back is x = x' c - y' s, y = x' s + y' c), inside when |q| < half extent on all
// three axes, strictly.  A box with a zero (or negative, or NaN) extent holds nothing; a NaN point is in no box.
//
// blockIdx.y is the frame, blockIdx.x a run of 256 of the frame's points: a lane keeps one point in registers and walks the
// frame's boxes, which the workgroup stages 256 at a time in LDS as centre, half extents, sin, cos.  MASK writes one byte per
// (point, box); COUNT takes one ballot per (wave, box) and lane 0 adds its population count with one integer atomic (skipped
// when the wave has no hit), so the counts do not depend on any order.
template <bool MASK, bool COUNT>
__global__ __launch_bounds__(256) void k_points_in_rbbox(const float *__restrict__ pts, int F, const int32_t *__restrict__ off, int64_t P,
                                                         const float *__restrict__ boxes, int N, int L, uint8_t *__restrict__ mask,
                                                         int32_t *__restrict__ counts) {
  __shared__ float sb[8][BOX_TILE];
  const int b = blockIdx.y, tid = threadIdx.x;
  int64_t lo = 0, hi = P;
  if (off) {                                   // offsets that do not describe P rows are cut to them
    lo = off[b]; hi = off[b + 1];
    lo = lo < 0 ? 0 : (lo > P ? P : lo);
    hi = hi < lo ? lo : (hi > P ? P : hi);
  }
  if ((int64_t)blockIdx.x * 256 >= hi - lo) return;          // uniform over the workgroup
  const int64_t p = lo + (int64_t)blockIdx.x * 256 + tid;
  const bool valid = p < hi;
  float x = NAN, y = NAN, z = NAN;
  if (valid) { x = pts[p * F]; y = pts[p * F + 1]; z = pts[p * F + 2]; }
  const float *fb = boxes + (int64_t)b * N * L;
  for (int n0 = 0; n0 < N; n0 += BOX_TILE) {
    const int nt = N - n0 < BOX_TILE ? N - n0 : BOX_TILE;
    __syncthreads();
    if (tid < nt) {
      const float *r = fb + (int64_t)(n0 + tid) * L;
      const double a = (double)r[L - 1];
      sb[0][tid] = r[0]; sb[1][tid] = r[1]; sb[2][tid] = r[2];
      sb[3][tid] = r[3] * 0.5f; sb[4][tid] = r[4] * 0.5f; sb[5][tid] = r[5] * 0.5f;
      sb[6][tid] = (float)sin(a); sb[7][tid] = (float)cos(a);
    }
    __syncthreads();
    for (int n = 0; n < nt; n++) {
      const float qx = x - sb[0][n], qy = y - sb[1][n], qz = z - sb[2][n];
      const float sn = sb[6][n], cs = sb[7][n];
      const float lx = qx * cs - qy * sn, ly = qx * sn + qy * cs;
      const bool in = fabsf(lx) < sb[3][n] && fabsf(ly) < sb[4][n] && fabsf(qz) < sb[5][n];
      if (MASK && valid) mask[p * N + n0 + n] = in ? 1 : 0;
      if (COUNT) {
        const unsigned long long hits = __ballot(in);
        if ((tid & 63) == 0 && hits) atomicAdd(counts + (int64_t)b * N + n0 + n, (int32_t)__popcll(hits));
      }
    }
  }
}

// ---- P2: corners and the collision matrix ---------------------------------------------------------------------------------------
// box_np_ops.py:265-285: the corners (-,-), (-,+), (+,+), (+,-) of dims (shifted by `origin`), turned by rotation_2d (x' = x c +
// y s, y' = -x s + y c: clockwise for a positive angle), plus the centre.  One lane per box.
template <typename Out>
__device__ __forceinline__ void box2d_corners(float cx, float cy, float dx, float dy, bool rotate, float angle, float origin, Out out) {
  float sn = 0.f, cs = 1.f;
  if (rotate) { const double a = (double)angle; sn = (float)sin(a); cs = (float)cos(a); }
  const float ux[4] = {0.f, 0.f, 1.f, 1.f}, uy[4] = {0.f, 1.f, 1.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float x = dx * (ux[k] - origin), y = dy * (uy[k] - origin);
    float rx = x, ry = y;
    if (rotate) { rx = x * cs + y * sn; ry = x * (-sn) + y * cs; }
    out[2 * k] = rx + cx;
    out[2 * k + 1] = ry + cy;
  }
}

__global__ __launch_bounds__(256) void k_box2d_corners(const float *__restrict__ centers, const float *__restrict__ dims,
                                                       const float *__restrict__ angles, int64_t n, float origin, float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  box2d_corners(centers[2 * i], centers[2 * i + 1], dims[2 * i], dims[2 * i + 1], angles != nullptr, angles ? angles[i] : 0.f, origin,
                out + 8 * i);
}

struct Quad {
  float x[4], y[4];
};

__device__ __forceinline__ Quad load_quad(const float *__restrict__ c) {
  Quad q;
#pragma unroll
  for (int k = 0; k < 4; k++) { q.x[k] = c[2 * k]; q.y[k] = c[2 * k + 1]; }
  return q;
}

// every corner of `in` strictly on the inner side of every edge of `out` (preprocess.py:905-917 and 920-932)
__device__ __forceinline__ bool quad_holds(const Quad &out, const Quad &in, bool clockwise) {
#pragma unroll
  for (int l = 0; l < 4; l++)
#pragma unroll
    for (int k = 0; k < 4; k++) {
      float vx = out.x[k] - out.x[(k + 1) & 3], vy = out.y[k] - out.y[(k + 1) & 3];
      if (clockwise) { vx = -vx; vy = -vy; }
      float cross = vy * (out.x[k] - in.x[l]);
      cross -= vx * (out.y[k] - in.y[l]);
      if (cross >= 0.f) return false;
    }
  return true;
}

// preprocess.py:854-937 for one pair: a of `boxes`, q of `qboxes`
__device__ __forceinline__ bool quads_collide(const Quad &A, const Quad &Q, bool clockwise) {
  const float iw = fminf(fmaxf(fmaxf(A.x[0], A.x[1]), fmaxf(A.x[2], A.x[3])), fmaxf(fmaxf(Q.x[0], Q.x[1]), fmaxf(Q.x[2], Q.x[3]))) -
                   fmaxf(fminf(fminf(A.x[0], A.x[1]), fminf(A.x[2], A.x[3])), fminf(fminf(Q.x[0], Q.x[1]), fminf(Q.x[2], Q.x[3])));
  const float ih = fminf(fmaxf(fmaxf(A.y[0], A.y[1]), fmaxf(A.y[2], A.y[3])), fmaxf(fmaxf(Q.y[0], Q.y[1]), fmaxf(Q.y[2], Q.y[3]))) -
                   fmaxf(fminf(fminf(A.y[0], A.y[1]), fminf(A.y[2], A.y[3])), fminf(fminf(Q.y[0], Q.y[1]), fminf(Q.y[2], Q.y[3])));
  if (!(iw > 0.f && ih > 0.f)) return false;
  bool hit = false;
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const float ax = A.x[s], ay = A.y[s], bx = A.x[(s + 1) & 3], by = A.y[(s + 1) & 3];
      const float cx = Q.x[t], cy = Q.y[t], dx = Q.x[(t + 1) & 3], dy = Q.y[(t + 1) & 3];
      const bool acd = (dy - ay) * (cx - ax) > (cy - ay) * (dx - ax);
      const bool bcd = (dy - by) * (cx - bx) > (cy - by) * (dx - bx);
      if (acd != bcd) {
        const bool abc = (cy - ay) * (bx - ax) > (by - ay) * (cx - ax);
        const bool abd = (dy - ay) * (bx - ax) > (by - ay) * (dx - ax);
        hit |= abc != abd;
      }
    }
  return hit || quad_holds(A, Q, clockwise) || quad_holds(Q, A, clockwise);
}

// one lane per pair, the pairs of a row of the matrix on consecutive lanes
__global__ __launch_bounds__(256) void k_box_collision(const float *__restrict__ ca, int64_t n, const float *__restrict__ cb, int64_t k,
                                                       int clockwise, uint8_t *__restrict__ out) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n * k) return;
  const int64_t i = gid / k, j = gid - i * k;
  out[gid] = quads_collide(load_quad(ca + 8 * i), load_quad(cb + 8 * j), clockwise != 0) ? 1 : 0;
}

// ---- P3: the sampler's acceptance scan ------------------------------------------------------------------------------------------
// sample_ops.py:97-172 + 250-296 for one frame per workgroup.  The frame's avoid set -- the BEV corners of the surviving ground
// truth, then of everything accepted -- lives in LDS (1024 x 8 floats), as do the corners of the class in hand (at most 64) and
// its collision rows: one 64-bit word per candidate against its own class (a wave takes a row, a lane a column, the word is the
// ballot) and one flag against the avoid set.  Thread 0 then runs the scan of sample_class_v2 on the words: candidate i is
// rejected by the avoid set, by an accepted earlier candidate, or by ANY later candidate of its class (whose row and column are
// still set when row i is looked at); a rejected candidate's row and column are out of every later decision.
__global__ __launch_bounds__(256) void k_detaug_sample(link_detaug_sample_cfg_t cfg, const float *__restrict__ gt_boxes,
                                                       const int32_t *__restrict__ gt_cls, const int32_t *__restrict__ gt_cnt,
                                                       const int32_t *__restrict__ cand, const int32_t *__restrict__ cand_len,
                                                       const float *__restrict__ db_boxes, const int32_t *__restrict__ db_cls,
                                                       const long long *__restrict__ db_off, int D, int32_t *__restrict__ accepted,
                                                       int32_t *__restrict__ paste_start, int32_t *__restrict__ n_accept,
                                                       float *__restrict__ mboxes, int32_t *__restrict__ mcls,
                                                       int32_t *__restrict__ n_merged, int32_t *__restrict__ status) {
  __shared__ float av[LINK_DETAUG_MAX_BOXES][8];
  __shared__ float cc[LINK_DETAUG_MAX_CANDIDATES][8];
  __shared__ unsigned long long roww[LINK_DETAUG_MAX_CANDIDATES];
  __shared__ int rowav[LINK_DETAUG_MAX_CANDIDATES], cidx[LINK_DETAUG_MAX_CANDIDATES];
  __shared__ int cnt[LINK_DETAUG_MAX_GROUPS], wsum[4];
  __shared__ int sh_av, sh_acc, sh_paste, sh_status;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int G = cfg.max_gt, M = cfg.max_candidates, C = cfg.n_groups, L = cfg.box_len, A = C * M, T = G + A;
  if (tid < LINK_DETAUG_MAX_GROUPS) cnt[tid] = 0;
  if (tid == 0) sh_status = 0;
  __syncthreads();
  // the ground truth that survives the minimum-points filter, in order: the avoid set; those of a known class: the merged list
  int n_av = 0, n_m = 0;
  for (int g0 = 0; g0 < G; g0 += 256) {
    const int g = g0 + tid;
    const int c = g < G ? gt_cls[(int64_t)b * G + g] : 0;
    const bool s = c != 0 && (cfg.min_points <= 0 || gt_cnt[(int64_t)b * G + g] >= cfg.min_points);
    const float *row = gt_boxes + ((int64_t)b * G + (g < G ? g : 0)) * L;
    int tot;
    int r = block_rank(s, wsum, tot);
    if (s) {
      box2d_corners(row[0], row[1], row[3], row[4], true, row[L - 1], 0.5f, av[n_av + r]);
      for (int q = 0; q < C; q++)
        if (c == cfg.group_class[q]) atomicAdd(&cnt[q], 1);
    }
    n_av += tot;
    const bool m = s && c >= 1;
    r = block_rank(m, wsum, tot);
    if (m) {
      float *o = mboxes + ((int64_t)b * T + n_m + r) * L;
      for (int f = 0; f < L; f++) o[f] = row[f];
      mcls[(int64_t)b * T + n_m + r] = c;
    }
    n_m += tot;
  }
  __syncthreads();
  int n_acc = 0, paste = 0;
  for (int q = 0; q < C; q++) {
    int len = cand_len[(int64_t)b * C + q];
    len = len < 0 ? 0 : (len > M ? M : len);
    const double want = rint(cfg.rate * (double)(cfg.group_max[q] - cnt[q]));      // np.round: half to even
    const int n = want > 0.0 ? (want < (double)len ? (int)want : len) : 0;
    if (n == 0) continue;                      // uniform: cnt is read after a barrier and never written again
    if (tid < n) {
      const int idx = cand[((int64_t)b * C + q) * M + tid];
      const bool ok = idx >= 0 && idx < D;
      cidx[tid] = ok ? idx : -1;
      if (ok) {
        const float *row = db_boxes + (int64_t)idx * L;
        box2d_corners(row[0], row[1], row[3], row[4], true, row[L - 1], 0.5f, cc[tid]);
      } else {
        for (int f = 0; f < 8; f++) cc[tid][f] = 0.f;
        atomicOr(&sh_status, LINK_DETAUG_STATUS_BAD_INDEX);
      }
    }
    __syncthreads();
    for (int i = w; i < n; i += 4) {           // uniform over the wave
      const Quad Ai = load_quad(cc[i]);
      const bool same = lane < n && lane != i && cidx[lane] >= 0 && quads_collide(Ai, load_quad(cc[lane]), true);
      const unsigned long long word = __ballot(same);
      bool hit = false;
      for (int a0 = 0; a0 < n_av; a0 += 64)
        if (a0 + lane < n_av) hit |= quads_collide(Ai, load_quad(av[a0 + lane]), true);
      const unsigned long long any = __ballot(hit);
      if (lane == 0) { roww[i] = word; rowav[i] = (any != 0ull || cidx[i] < 0) ? 1 : 0; }
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long acc = 0ull;
      for (int i = 0; i < n; i++) {
        const unsigned long long later = i >= 63 ? 0ull : (~0ull << (i + 1));
        if (!rowav[i] && !(roww[i] & (later | acc))) acc |= 1ull << i;
      }
      for (int i = 0; i < n; i++)
        if ((acc >> i) & 1ull) {
          for (int f = 0; f < 8; f++) av[n_av][f] = cc[i][f];
          n_av++;
          accepted[(int64_t)b * A + n_acc] = cidx[i];
          paste_start[(int64_t)b * (A + 1) + n_acc] = paste;
          paste += (int)(db_off[cidx[i] + 1] - db_off[cidx[i]]);
          n_acc++;
        }
      sh_av = n_av; sh_acc = n_acc; sh_paste = paste;
    }
    __syncthreads();
    n_av = sh_av; n_acc = sh_acc; paste = sh_paste;
  }
  __syncthreads();
  for (int k = tid; k < n_acc; k += 256) {     // the accepted boxes and classes behind the frame's own
    const int d = accepted[(int64_t)b * A + k];
    float *o = mboxes + ((int64_t)b * T + n_m + k) * L;
    for (int f = 0; f < L; f++) o[f] = db_boxes[(int64_t)d * L + f];
    mcls[(int64_t)b * T + n_m + k] = db_cls[d];
  }
  for (int k = n_acc + tid; k <= A; k += 256) {
    paste_start[(int64_t)b * (A + 1) + k] = paste;
    if (k < A) accepted[(int64_t)b * A + k] = -1;
  }
  if (tid == 0) { n_accept[b] = n_acc; n_merged[b] = n_m + n_acc; status[b] = sh_status; }
}

// ---- P4: paste, global transforms, shuffle ------------------------------------------------------------------------------------------
// The draws of one frame turned into what preprocess.py:803-839, 771-788, 940-962 apply: the flips where the uniform is at least
// 1 - probability (np.random.choice's rule), the angle and the scale as low + (high - low) u in double, the matrix entries and the
// scale rounded to fp32 as an fp32 array meets them, the translation as a double (the reference adds a float64 row).
struct xform {
  int fx, fy;
  float cs, sn, ang, sc;
  double cs64, sn64, t[3];
};

__device__ __forceinline__ xform make_xform(const link_detaug_transform_cfg_t &c, const float *__restrict__ d) {
  xform x;
  x.fx = (double)d[0] >= 1.0 - c.flip_probability;
  x.fy = (double)d[1] >= 1.0 - c.flip_probability;
  const double a = c.rot_lo + (c.rot_hi - c.rot_lo) * (double)d[2];
  x.cs64 = cos(a); x.sn64 = sin(a);
  x.cs = (float)x.cs64; x.sn = (float)x.sn64; x.ang = (float)a;
  x.sc = (float)(c.scale_lo + (c.scale_hi - c.scale_lo) * (double)d[3]);
  x.t[0] = c.translate_std[0] * (double)d[4];
  x.t[1] = c.translate_std[1] * (double)d[5];
  x.t[2] = c.translate_std[0] * (double)d[6];                // preprocess.py:955: z is drawn with std[0]
  return x;
}

__device__ __forceinline__ void xform_xyz(const xform &x, float &px, float &py, float &pz) {
  if (x.fx) py = -py;
  if (x.fy) px = -px;
  const float rx = px * x.cs + py * x.sn, ry = px * (-x.sn) + py * x.cs;
  px = rx * x.sc; py = ry * x.sc; pz = pz * x.sc;
  px = (float)((double)px + x.t[0]); py = (float)((double)py + x.t[1]); pz = (float)((double)pz + x.t[2]);
}

// One lane per slot of the frame's [cap, F] buffer: slot r is a pasted point (the accepted objects in acceptance order, each
// object's points plus its box centre), then a scene point, then NaN; it is written to row perm[b, r].
__global__ __launch_bounds__(256) void k_detaug_points(link_detaug_transform_cfg_t cfg, const float *__restrict__ draws,
                                                       const float *__restrict__ pts, const int32_t *__restrict__ off, int64_t P, int F,
                                                       const float *__restrict__ db_pts, const long long *__restrict__ db_off,
                                                       const float *__restrict__ db_boxes, int L, const int32_t *__restrict__ accepted,
                                                       const int32_t *__restrict__ paste_start, const int32_t *__restrict__ n_accept, int A,
                                                       const int32_t *__restrict__ perm, float *__restrict__ out) {
  __shared__ xform X;
  const int b = blockIdx.y, cap = cfg.point_capacity;
  if (threadIdx.x == 0) X = make_xform(cfg, draws + 7 * b);
  __syncthreads();
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= cap) return;
  const int pv = perm[(int64_t)b * cap + r];
  if (pv < 0 || pv >= cap) return;             // not a permutation: nothing is written out of bounds
  float *o = out + ((int64_t)b * cap + pv) * F;
  int64_t lo = off[b], hi = off[b + 1];
  lo = lo < 0 ? 0 : (lo > P ? P : lo);
  hi = hi < lo ? lo : (hi > P ? P : hi);
  const int32_t *ps = paste_start + (int64_t)b * (A + 1);
  const int64_t pasted = ps[A];
  if (r >= pasted + (hi - lo)) {
    for (int f = 0; f < F; f++) o[f] = NAN;
    return;
  }
  const float *src;
  float x, y, z;
  if (r < pasted) {
    int k0 = 0, k1 = n_accept[b];              // the last k with ps[k] <= r
    while (k1 - k0 > 1) {
      const int mid = (k0 + k1) >> 1;
      if (ps[mid] <= r) k0 = mid; else k1 = mid;
    }
    const int d = accepted[(int64_t)b * A + k0];
    src = db_pts + ((int64_t)db_off[d] + (r - ps[k0])) * F;
    x = src[0] + db_boxes[(int64_t)d * L]; y = src[1] + db_boxes[(int64_t)d * L + 1]; z = src[2] + db_boxes[(int64_t)d * L + 2];
  } else {
    src = pts + (lo + (r - pasted)) * F;
    x = src[0]; y = src[1]; z = src[2];
  }
  xform_xyz(X, x, y, z);
  o[0] = x; o[1] = y; o[2] = z;
  for (int f = 3; f < F; f++) o[f] = src[f];
}

// The merged boxes of one frame per workgroup: transformed as preprocess.py does it to an fp32 [n, 7 | 9] array (the velocity pair
// is rotated in double: the reference stacks it with a float64 column), filtered by filter_gt_box_outside_range (a box stays when
// one BEV corner lies strictly inside the range) and compacted in order.
__global__ __launch_bounds__(256) void k_detaug_boxes(link_detaug_transform_cfg_t cfg, const float *__restrict__ draws,
                                                      const float *__restrict__ mboxes, const int32_t *__restrict__ mcls,
                                                      const int32_t *__restrict__ n_merged, int T, int L,
                                                      const int32_t *__restrict__ off, int64_t P, const int32_t *__restrict__ paste_start, int A,
                                                      float *__restrict__ out_boxes, int32_t *__restrict__ out_cls,
                                                      int32_t *__restrict__ n_boxes, int32_t *__restrict__ n_points, int32_t *__restrict__ status) {
  __shared__ xform X;
  __shared__ int wsum[4];
  const int b = blockIdx.x, tid = threadIdx.x, K = cfg.max_objs;
  if (tid == 0) X = make_xform(cfg, draws + 7 * b);
  __syncthreads();
  int n = n_merged[b];
  n = n < 0 ? 0 : (n > T ? T : n);
  int kept = 0;
  for (int t0 = 0; t0 < n; t0 += 256) {
    const int t = t0 + tid;
    float v[9];
    bool keep = false;
    if (t < n) {
      const float *row = mboxes + ((int64_t)b * T + t) * L;
      for (int f = 0; f < L; f++) v[f] = row[f];
      if (X.fx) { v[1] = -v[1]; v[L - 1] = -v[L - 1] + (float)M_PI; if (L == 9) v[7] = -v[7]; }
      if (X.fy) { v[0] = -v[0]; v[L - 1] = -v[L - 1] + (float)(2.0 * M_PI); if (L == 9) v[6] = -v[6]; }
      const float rx = v[0] * X.cs + v[1] * X.sn, ry = v[0] * (-X.sn) + v[1] * X.cs;
      v[0] = rx; v[1] = ry;
      if (L == 9) {
        const double vx = v[6], vy = v[7];
        v[6] = (float)(vx * X.cs64 + vy * X.sn64);
        v[7] = (float)(vx * (-X.sn64) + vy * X.cs64);
      }
      v[L - 1] = v[L - 1] + X.ang;
      for (int f = 0; f < L - 1; f++) v[f] = v[f] * X.sc;          // gt_boxes[:, :-1] *= s: the velocity is scaled too
      for (int f = 0; f < 3; f++) v[f] = (float)((double)v[f] + X.t[f]);
      float c8[8];
      box2d_corners(v[0], v[1], v[3], v[4], true, v[L - 1], 0.5f, c8);
      for (int k = 0; k < 4; k++)
        keep |= (double)c8[2 * k] > cfg.range[0] && (double)c8[2 * k] < cfg.range[2] && (double)c8[2 * k + 1] > cfg.range[1] &&
                (double)c8[2 * k + 1] < cfg.range[3];
    }
    int tot;
    const int pos = kept + block_rank(keep, wsum, tot);
    if (keep && pos < K) {
      float *o = out_boxes + ((int64_t)b * K + pos) * L;
      for (int f = 0; f < L; f++) o[f] = v[f];
      out_cls[(int64_t)b * K + pos] = mcls[(int64_t)b * T + t];
    }
    kept += tot;
  }
  const int used = kept < K ? kept : K;
  for (int k = used + tid; k < K; k += 256) {
    float *o = out_boxes + ((int64_t)b * K + k) * L;
    for (int f = 0; f < L; f++) o[f] = 0.f;
    out_cls[(int64_t)b * K + k] = 0;
  }
  if (tid == 0) {
    int64_t lo = off[b], hi = off[b + 1];
    lo = lo < 0 ? 0 : (lo > P ? P : lo);
    hi = hi < lo ? lo : (hi > P ? P : hi);
    const int64_t total = (int64_t)paste_start[(int64_t)b * (A + 1) + A] + (hi - lo);
    n_boxes[b] = used;
    n_points[b] = (int32_t)(total < cfg.point_capacity ? total : cfg.point_capacity);
    status[b] = status[b] | (kept > K ? LINK_DETAUG_STATUS_BOXES_CUT : 0) | (total > cfg.point_capacity ? LINK_DETAUG_STATUS_POINTS_CUT : 0);
  }
}

constexpr int64_t MAX_POINTS = (1LL << 31) - 256;            // int32 offsets; the grid's x extent
constexpr int64_t MAX_MASK = 1LL << 40;

}  // namespace

extern "C" int link_points_in_rbbox(const float *points, int32_t ndim, const int32_t *point_offsets, int32_t batch, int64_t n_points,
                                    const float *boxes, int64_t n_boxes, int32_t box_len, uint8_t *mask, int32_t *counts, void *stream) {
  if (ndim < 3 || ndim > 64 || box_len < 7 || box_len > 64 || batch < 1 || batch > 65535) return LINK_ERR_ARG;
  if (n_points < 0 || n_points > MAX_POINTS || n_boxes < 0 || n_boxes > (1 << 24)) return LINK_ERR_ARG;
  if (!point_offsets && batch != 1) return LINK_ERR_ARG;
  if (!mask && !counts) return LINK_ERR_ARG;
  if (mask && n_points * n_boxes > MAX_MASK) return LINK_ERR_ARG;
  if (n_boxes == 0) return LINK_OK;
  if (!boxes || (n_points > 0 && !points)) return LINK_ERR_ARG;
  if (counts) {
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)batch * (size_t)n_boxes, S(stream));
    if (e != hipSuccess) { set_error("link_points_in_rbbox", e); return LINK_ERR_LAUNCH; }
  }
  if (n_points == 0) return LINK_OK;
  const dim3 grid(blocks_for(n_points, 256), batch), block(256);
#define LINK_PIB(M, C) \
  hipLaunchKernelGGL((k_points_in_rbbox<M, C>), grid, block, 0, S(stream), points, (int)ndim, point_offsets, n_points, boxes, (int)n_boxes, \
                     (int)box_len, mask, counts)
  if (mask && counts) LINK_PIB(true, true);
  else if (mask) LINK_PIB(true, false);
  else LINK_PIB(false, true);
#undef LINK_PIB
  return check_launch("link_points_in_rbbox");
}

extern "C" int link_box2d_corners(const float *centers, const float *dims, const float *angles, int64_t n, float origin, float *out,
                                  void *stream) {
  if (n < 0 || n > MAX_POINTS || !isfinite(origin)) return LINK_ERR_ARG;
  if (n == 0) return LINK_OK;
  if (!centers || !dims || !out) return LINK_ERR_ARG;
  hipLaunchKernelGGL(k_box2d_corners, dim3(blocks_for(n, 256)), dim3(256), 0, S(stream), centers, dims, angles, n, origin, out);
  return check_launch("link_box2d_corners");
}

extern "C" int link_box_collision(const float *corners_a, int64_t n, const float *corners_b, int64_t k, int32_t clockwise, uint8_t *out,
                                  void *stream) {
  if (n < 0 || k < 0 || n > (1 << 20) || k > (1 << 20) || n * k > MAX_POINTS) return LINK_ERR_ARG;
  if (n == 0 || k == 0) return LINK_OK;
  if (!corners_a || !corners_b || !out) return LINK_ERR_ARG;
  hipLaunchKernelGGL(k_box_collision, dim3(blocks_for(n * k, 256)), dim3(256), 0, S(stream), corners_a, n, corners_b, k, (int)clockwise, out);
  return check_launch("link_box_collision");
}

extern "C" int link_detaug_sample(const link_detaug_sample_cfg_t *cfg, int32_t batch, const float *gt_boxes, const int32_t *gt_classes,
                                  const int32_t *gt_counts, const int32_t *candidates, const int32_t *cand_len, const float *db_boxes,
                                  const int32_t *db_classes, const int64_t *db_offsets, int64_t db_size, int32_t *accepted,
                                  int32_t *paste_start, int32_t *n_accept, float *merged_boxes, int32_t *merged_classes,
                                  int32_t *n_merged, int32_t *status, void *stream) {
  if (!cfg || batch < 0 || batch > 65535) return LINK_ERR_ARG;
  if (cfg->n_groups < 0 || cfg->n_groups > LINK_DETAUG_MAX_GROUPS || cfg->max_candidates < 0 ||
      cfg->max_candidates > LINK_DETAUG_MAX_CANDIDATES || cfg->max_gt < 0 || (cfg->box_len != 7 && cfg->box_len != 9))
    return LINK_ERR_ARG;
  if ((int64_t)cfg->max_gt + (int64_t)cfg->n_groups * cfg->max_candidates > LINK_DETAUG_MAX_BOXES) return LINK_ERR_ARG;
  if (!isfinite(cfg->rate) || cfg->rate < 0.0 || db_size < 0 || db_size > (1LL << 31) - 1) return LINK_ERR_ARG;
  for (int q = 0; q < cfg->n_groups; q++)
    if (cfg->group_class[q] < 1 || cfg->group_max[q] < 0 || cfg->group_max[q] > (1 << 20)) return LINK_ERR_ARG;
  if (batch == 0) return LINK_OK;
  const bool sampling = cfg->n_groups > 0 && cfg->max_candidates > 0;
  if (!paste_start || !n_accept || !n_merged || !status) return LINK_ERR_ARG;
  if (cfg->max_gt > 0 && (!gt_boxes || !gt_classes || (cfg->min_points > 0 && !gt_counts))) return LINK_ERR_ARG;
  if (cfg->max_gt + cfg->n_groups * cfg->max_candidates > 0 && (!merged_boxes || !merged_classes)) return LINK_ERR_ARG;
  if (sampling && (!candidates || !cand_len || !db_boxes || !db_classes || !db_offsets || !accepted)) return LINK_ERR_ARG;
  if (cfg->n_groups > 0 && !cand_len) return LINK_ERR_ARG;
  hipLaunchKernelGGL(k_detaug_sample, dim3(batch), dim3(256), 0, S(stream), *cfg, gt_boxes, gt_classes, gt_counts, candidates, cand_len,
                     db_boxes, db_classes, reinterpret_cast<const long long *>(db_offsets), (int)db_size, accepted, paste_start, n_accept,
                     merged_boxes, merged_classes, n_merged, status);
  return check_launch("link_detaug_sample");
}

extern "C" int link_detaug_transform(const link_detaug_transform_cfg_t *cfg, int32_t batch, const float *draws, const float *points,
                                     const int32_t *point_offsets, int64_t n_points, int32_t ndim, const float *db_points,
                                     const int64_t *db_offsets, const float *db_boxes, int32_t box_len, const int32_t *accepted,
                                     const int32_t *paste_start, const int32_t *n_accept, int32_t max_accept, const int32_t *perm,
                                     float *out_points, const float *merged_boxes, const int32_t *merged_classes, const int32_t *n_merged,
                                     int32_t max_merged, float *out_boxes, int32_t *out_classes, int32_t *n_boxes, int32_t *n_out_points,
                                     int32_t *status, void *stream) {
  if (!cfg || batch < 0 || batch > 65535 || ndim < 3 || ndim > 64 || (box_len != 7 && box_len != 9)) return LINK_ERR_ARG;
  if (cfg->max_objs < 0 || cfg->max_objs > (1 << 20) || cfg->point_capacity < 0 || cfg->point_capacity > (1 << 30)) return LINK_ERR_ARG;
  if (n_points < 0 || n_points > MAX_POINTS || max_accept < 0 || max_accept > LINK_DETAUG_MAX_BOXES || max_merged < 0 ||
      max_merged > 2 * LINK_DETAUG_MAX_BOXES)
    return LINK_ERR_ARG;
  const double fin[] = {cfg->rot_lo, cfg->rot_hi, cfg->scale_lo, cfg->scale_hi, cfg->translate_std[0], cfg->translate_std[1],
                        cfg->translate_std[2], cfg->flip_probability, cfg->range[0], cfg->range[1], cfg->range[2], cfg->range[3]};
  for (double v : fin)
    if (!isfinite(v)) return LINK_ERR_ARG;
  if (cfg->flip_probability < 0.0 || cfg->flip_probability > 1.0) return LINK_ERR_ARG;
  if (batch == 0) return LINK_OK;
  if (!draws || !point_offsets || !paste_start || !n_accept || !n_merged || !n_boxes || !n_out_points || !status) return LINK_ERR_ARG;
  if (n_points > 0 && !points) return LINK_ERR_ARG;
  if (max_accept > 0 && (!accepted || !db_points || !db_offsets || !db_boxes)) return LINK_ERR_ARG;
  if (cfg->point_capacity > 0 && (!perm || !out_points)) return LINK_ERR_ARG;
  if (max_merged > 0 && (!merged_boxes || !merged_classes)) return LINK_ERR_ARG;
  if (cfg->max_objs > 0 && (!out_boxes || !out_classes)) return LINK_ERR_ARG;
  if (cfg->point_capacity > 0) {
    hipLaunchKernelGGL(k_detaug_points, dim3(blocks_for(cfg->point_capacity, 256), batch), dim3(256), 0, S(stream), *cfg, draws, points,
                       point_offsets, n_points, (int)ndim, db_points, reinterpret_cast<const long long *>(db_offsets), db_boxes, (int)box_len,
                       accepted, paste_start, n_accept, (int)max_accept, perm, out_points);
    const int rc = check_launch("link_detaug_transform");
    if (rc != LINK_OK) return rc;
  }
  hipLaunchKernelGGL(k_detaug_boxes, dim3(batch), dim3(256), 0, S(stream), *cfg, draws, merged_boxes, merged_classes, n_merged,
                     (int)max_merged, (int)box_len, point_offsets, n_points, paste_start, (int)max_accept, out_boxes, out_classes, n_boxes,
                     n_out_points, status);
  return check_launch("link_detaug_transform");
}
