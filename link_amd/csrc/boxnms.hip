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

#include "common.h"

using namespace link;

namespace {

constexpr float BOX_EPS = 1e-8f;      // iou3d_nms_kernel.cu:14
constexpr float BOX_MARGIN = 1e-2f;   // :53
constexpr int NPTS = 24;              // 16 crossings + 8 corners
constexpr int NF = 17;                // floats of a staged box
constexpr int REDUCE_WORDS = 64;      // remv words the scan holds at a time: one per lane of a wave

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
__device__ float box_overlap(const Rec &A, const Rec &B) {
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

__device__ __forceinline__ int device_count(const int32_t *n_dev, int cap) {
  if (!n_dev) return cap;
  const int n = *n_dev;
  return n < 0 ? 0 : (n > cap ? cap : n);
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

struct decode_geom {
  float osf, vx, vy, px, py, thr, lo[3], hi[3];
};

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

// unmasked cells per frame: one workgroup per frame, integer sums through LDS (no atomics)
__global__ __launch_bounds__(256) void k_center_count(const float *__restrict__ scores, int hw, int32_t *__restrict__ counts) {
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
