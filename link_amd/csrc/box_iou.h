// link_amd/csrc/box_iou.h -- the rotated BEV overlap of a box pair as device functions, shared by csrc/boxnms.hip (sections I) and
// csrc/dettta.hip (section N).  Semantics: detection/det3d/ops/iou3d_nms/src/iou3d_nms_kernel.cu:35-234; the implementation notes
// are at the head of boxnms.hip.  At its end: the geometry record and the count body the two CenterHead decoders share.
//
// The reference rounds every product and sum on its own and its strict inequalities decide which points exist, so contraction is
// off for every translation unit that includes this file (from here to its end).
#pragma once
#pragma clang fp contract(off)
#include <math.h>

#include "common.h"

namespace link {

constexpr float BOX_EPS = 1e-8f;      // iou3d_nms_kernel.cu:14
constexpr float BOX_MARGIN = 1e-2f;   // :53
constexpr int NPTS = 24;              // 16 crossings + 8 corners
constexpr int NF = 17;                // floats of a staged box

// a box as the pair routine wants it: centre, cos / sin of -heading, half extents + margin, area, extents, rotated corners
struct Rec {
  float x, y, cn, sn, hx, hy, area, dx, dy, cx[4], cy[4];
};

template <int N, bool FULL>
__device__ __forceinline__ void stage_box(const float *box, float (*s)[N], int slot) {
  const float x = box[0], y = box[1], dx = box[3], dy = box[4], h = box[6];
  s[0][slot] = x; s[1][slot] = y; s[6][slot] = dx * dy; s[7][slot] = dx; s[8][slot] = dy;
  if (!FULL) return;
  const float dxh = dx / 2, dyh = dy / 2;
  const float x1 = x - dxh, y1 = y - dyh, x2 = x + dxh, y2 = y + dyh;                       // :109-113
  // cos / sin through double, rounded once: correctly rounded floats, which is what the host libm of the CPU twin returns -- a
  // 1 ulp difference in a corner is 1 ulp of a 40 m^2 overlap, 4e-6.  Per box, not per pair: the cost is in the staging only.
  const float c = (float)cos((double)h), sn = (float)sin((double)h);                        // :137-138
  const float px[4] = {x1, x2, x2, x1}, py[4] = {y1, y1, y2, y2};                           // :125-128
#pragma unroll
  for (int k = 0; k < 4; k++) {                                                             // rotate_around_center, :94-98
    s[9 + k][slot] = (px[k] - x) * c + (py[k] - y) * (-sn) + x;
    s[13 + k][slot] = (px[k] - x) * sn + (py[k] - y) * c + y;
  }
  s[2][slot] = (float)cos((double)-h); s[3][slot] = (float)sin((double)-h);                 // check_in_box2d, :56
  s[4][slot] = dx / 2 + BOX_MARGIN; s[5][slot] = dy / 2 + BOX_MARGIN;                       // :60
}

// FULL = false: the fields the axis-aligned and centre-distance predicates read (the only ones their staging writes)
template <int N, bool FULL = true>
__device__ __forceinline__ Rec load_box(const float (*s)[N], int slot) {
  Rec r = {};
  r.x = s[0][slot]; r.y = s[1][slot]; r.area = s[6][slot]; r.dx = s[7][slot]; r.dy = s[8][slot];
  if (!FULL) return r;
  r.cn = s[2][slot]; r.sn = s[3][slot]; r.hx = s[4][slot]; r.hy = s[5][slot];
#pragma unroll
  for (int k = 0; k < 4; k++) { r.cx[k] = s[9 + k][slot]; r.cy[k] = s[13 + k][slot]; }
  return r;
}

// :39-41
__device__ __forceinline__ float cross3(float p1x, float p1y, float p2x, float p2y, float p0x, float p0y) {
  return (p1x - p0x) * (p2y - p0y) - (p2x - p0x) * (p1y - p0y);
}

// :63-92
__device__ __forceinline__ bool intersection(float p1x, float p1y, float p0x, float p0y, float q1x, float q1y, float q0x, float q0y,
                                             float &ax, float &ay) {
  const bool rect = fminf(p0x, p1x) <= fmaxf(q0x, q1x) && fminf(q0x, q1x) <= fmaxf(p0x, p1x) &&
                    fminf(p0y, p1y) <= fmaxf(q0y, q1y) && fminf(q0y, q1y) <= fmaxf(p0y, p1y);
  if (!rect) return false;
  const float s1 = cross3(q0x, q0y, p1x, p1y, p0x, p0y);
  const float s2 = cross3(p1x, p1y, q1x, q1y, p0x, p0y);
  const float s3 = cross3(p0x, p0y, q1x, q1y, q0x, q0y);
  const float s4 = cross3(q1x, q1y, p1x, p1y, q0x, q0y);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  const float s5 = cross3(q1x, q1y, p1x, p1y, p0x, p0y);
  if (fabsf(s5 - s1) > BOX_EPS) {
    ax = (s5 * q0x - s1 * q1x) / (s5 - s1);
    ay = (s5 * q0y - s1 * q1y) / (s5 - s1);
  } else {
    const float a0 = p0y - p1y, b0 = p1x - p0x, c0 = p0x * p1y - p1x * p0y;
    const float a1 = q0y - q1y, b1 = q1x - q0x, c1 = q0x * q1y - q1x * q0y;
    const float D = a0 * b1 - a1 * b0;
    ax = (b0 * c1 - b1 * c0) / D;
    ay = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

// :51-61
__device__ __forceinline__ bool in_box(const Rec &b, float px, float py) {
  const float rx = (px - b.x) * b.cn + (py - b.y) * (-b.sn);
  const float ry = (px - b.x) * b.sn + (py - b.y) * b.cn;
  return fabsf(rx) < b.hx && fabsf(ry) < b.hy;
}

// :104-225.  Slot i * 4 + j holds the crossing of a's edge i with b's edge j, slots 16 + 2k / 17 + 2k b's / a's corner k: the
// reference's order of insertion.  A slot that holds no point gets the key +inf; a stable sort by key (odd-even transposition:
// only neighbours are exchanged, and only on a strict >) then leaves the points in exactly the order the reference's bubble sort
// leaves them in, followed by the empty slots.
static __device__ float box_overlap(const Rec &A, const Rec &B) {
  float px[NPTS], py[NPTS], key[NPTS];
  unsigned valid = 0;
  float sx = 0.f, sy = 0.f;
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float ax = 0.f, ay = 0.f;
      const bool f = intersection(A.cx[(i + 1) & 3], A.cy[(i + 1) & 3], A.cx[i], A.cy[i], B.cx[(j + 1) & 3], B.cy[(j + 1) & 3],
                                  B.cx[j], B.cy[j], ax, ay);
      px[i * 4 + j] = ax; py[i * 4 + j] = ay;
      if (f) { sx = sx + ax; sy = sy + ay; cnt++; valid |= 1u << (i * 4 + j); }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    px[16 + 2 * k] = B.cx[k]; py[16 + 2 * k] = B.cy[k];
    if (in_box(A, B.cx[k], B.cy[k])) { sx = sx + B.cx[k]; sy = sy + B.cy[k]; cnt++; valid |= 1u << (16 + 2 * k); }
    px[17 + 2 * k] = A.cx[k]; py[17 + 2 * k] = A.cy[k];
    if (in_box(B, A.cx[k], A.cy[k])) { sx = sx + A.cx[k]; sy = sy + A.cy[k]; cnt++; valid |= 1u << (17 + 2 * k); }
  }
  if (cnt == 0) return 0.f;
  const float mx = sx / (float)cnt, my = sy / (float)cnt;
#pragma unroll
  for (int s = 0; s < NPTS; s++) key[s] = ((valid >> s) & 1u) ? atan2f(py[s] - my, px[s] - mx) : INFINITY;
#pragma unroll
  for (int round = 0; round < NPTS; round++) {
#pragma unroll
    for (int i = round & 1; i + 1 < NPTS; i += 2) {
      const bool sw = key[i] > key[i + 1];
      const float k0 = key[i], k1 = key[i + 1], x0 = px[i], x1 = px[i + 1], y0 = py[i], y1 = py[i + 1];
      key[i] = sw ? k1 : k0; key[i + 1] = sw ? k0 : k1;
      px[i] = sw ? x1 : x0; px[i + 1] = sw ? x0 : x1;
      py[i] = sw ? y1 : y0; py[i + 1] = sw ? y0 : y1;
    }
  }
  float area = 0.f;
#pragma unroll
  for (int k = 0; k + 1 < NPTS; k++) {
    const float t = (px[k] - px[0]) * (py[k + 1] - py[0]) - (py[k] - py[0]) * (px[k + 1] - px[0]);
    if (k + 1 < cnt) area = area + t;
  }
  return fabsf(area) / 2.f;
}

__device__ __forceinline__ float iou_from_overlap(const Rec &A, const Rec &B, float ov) {          // :227-234
  return ov / fmaxf(A.area + B.area - ov, BOX_EPS);
}

// the number of leading boxes that count: *n_dev clamped to [0, cap], or cap
__device__ __forceinline__ int device_count(const int32_t *n_dev, int cap) {
  if (!n_dev) return cap;
  const int n = *n_dev;
  return n < 0 ? 0 : (n > cap ? cap : n);
}

// ---- what the two CenterHead decoders (k_center_decode, k_center_decode_flip4) share ----
struct decode_geom {
  float osf, vx, vy, px, py, thr, lo[3], hi[3];
};

// unmasked cells per frame, the body of the kernel behind either decoder: one workgroup of 256 threads per frame, integer sums
// through LDS (no atomics)
__device__ __forceinline__ void center_count_frame(const float *scores, int hw, int32_t *counts) {
  __shared__ int part[4];
  const float *s = scores + (int64_t)blockIdx.x * hw;
  int c = 0;
  for (int i = threadIdx.x; i < hw; i += 256) c += s[i] > -INFINITY ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

}  // namespace link
