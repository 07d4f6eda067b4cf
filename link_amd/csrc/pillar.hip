// link_amd/csrc/pillar.hip -- section S of include/link_amd.h: the PointPillars reader and its BEV scatter for gfx950.
// Reference: detection/det3d/models/readers/pillar_encoder.py (PFNLayer :15-55, PillarFeatureNet.forward :116-162,
// PointPillarsScatter.forward :182-218).  The reference writes the decorated [P, T, D+5] tensor, the [P, T, units] activations of
// every layer and the [P, C] rows to memory, then builds the canvas with one indexed assignment per sample.  Here
//
//   k_pillar_reader   one wave = one pillar at a time (PW = 4 waves per workgroup, a persistent grid striding over the live
//                     pillars).  The wave reads the pillar's `num` valid rows, decorates them into its own LDS slab, runs
//                     layer 1 with lane = output unit (the unit's weights in registers), BatchNorm as a per-channel affine after
//                     the dot product, ReLU and the running max; with a second layer the layer-1 rows stay in the slab and
//                     layer 2 runs RB = 4 rows at a time against the transposed weight in LDS (one weight read feeds RB fused
//                     multiply-adds; the rows are read as broadcast 16-byte words).  The [x, x_max] concatenation is never
//                     formed: the x_max half of the layer-2 product is the same for every row of a pillar and is computed once.
//                     Padded rows: the reference runs all T rows through both layers, and a padded row leaves layer 1 as
//                     relu(shift1) -- the same for every padded row of a pillar -- so ONE representative padded row is evaluated
//                     where num < T and none where num == T.  The result goes to [P, C] rows or straight to the canvas.
//   k_pillar_scatter  rows [P, C] -> canvas [B, C, ny, nx] (the canvas is zero-filled by the entry, hipMemsetAsync on the stream)
//   k_pillar_gather   its adjoint: rows [P, C] <- canvas, zero for inert rows
//   k_pillar_decorate [P, T, D] -> masked [P, T, D+5(+1)] for the training path
//
// Plain VALU fp32 throughout; fused multiply-adds as the compiler contracts them; one rounding at a 16-bit store.  No atomics:
// every output element has one writer, so two runs give the same bits, and the row form and the canvas form of the reader are
// the same instantiation up to the store.  Every index that addresses the canvas is range-checked against (batch, ny, nx) first: a
// pillar whose coordinate lies outside writes nothing.
#include "common.h"
#include "dispatch.h"
#include "row_io.h"

using namespace link;

namespace {

constexpr int PW = 4;            // waves, and so pillars in flight, per workgroup
constexpr int RB = 4;            // rows per tile of layer 2
constexpr int MAXK = LINK_PILLAR_MAX_D + 6;   // decorated width: D + 3 (cluster) + 2 (centre) + 1 (distance)

struct PillarArgs {
  const float *vox;
  const int32_t *num, *coors, *count;
  const float *w1, *g1, *b1, *m1, *v1, *w2, *g2, *b2, *m2, *v2;   // weight, gamma, beta, running mean, running variance
  float eps1, eps2;
  void *rows, *canvas;
  int64_t P;
  int32_t T, D, K1, dist, U1, U2, C;   // U1: units of layer 1; U2: units of layer 2 (0 with one layer); C: output channels
  int32_t B, ny, nx;
  float vx, vy, xo, yo;
  // LDS layout, in floats (every offset a multiple of 4: the row tiles are read as 16-byte words)
  int32_t o_w2, o_wave, wave_floats, o_dec, o_x1, pitch;
};

// the lanes of a wave exchange data through the wave's own LDS slab: writes land before any lane reads
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float relu1(float v) { return v < 0.f ? 0.f : v; }

// eval-mode BatchNorm of one channel as y = x scale + shift
__device__ __forceinline__ void bn_affine(const float *g, const float *b, const float *m, const float *v, float eps, int u, float &scale,
                                          float &shift) {
  scale = g[u] / sqrtf(v[u] + eps);
  shift = b[u] - m[u] * scale;
}

__device__ __forceinline__ int64_t live_rows(const int32_t *count, int64_t P) {
  if (!count) return P;
  const int64_t c = *count;
  return c < 0 ? 0 : (c < P ? c : P);
}

// cell of pillar p in a [B, C, ny, nx] canvas: the element index of channel 0, or -1 when the coordinate is outside
__device__ __forceinline__ int64_t cell_base(const int32_t *coors, int64_t p, int32_t B, int32_t C, int32_t ny, int32_t nx) {
  const int32_t b = coors[p * 4], y = coors[p * 4 + 2], x = coors[p * 4 + 3];
  if ((uint32_t)b >= (uint32_t)B || (uint32_t)y >= (uint32_t)ny || (uint32_t)x >= (uint32_t)nx) return -1;
  return ((int64_t)b * C * ny + y) * nx + x;
}

// mean of xyz over the rows t < num (num >= 1), as row 0 plus the mean offset from row 0: the same number as sum / num, but the
// offsets inside a pillar are small, so the sum does not lose the low bits of a coordinate 50 m from the origin
__device__ __forceinline__ void pillar_mean(const float *rows, int D, int num, float &mx, float &my, float &mz) {
  const float x0 = rows[0], y0 = rows[1], z0 = rows[2];
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int t = 1; t < num; ++t) {                   // row order
    sx += rows[t * D] - x0;
    sy += rows[t * D + 1] - y0;
    sz += rows[t * D + 2] - z0;
  }
  const float fn = (float)num;
  mx = x0 + sx / fn;
  my = y0 + sy / fn;
  mz = z0 + sz / fn;
}

__device__ __forceinline__ void decorate_row(const float *row, int D, bool dist, float mx, float my, float mz, float cx, float cy,
                                             float *out) {
  const float x = row[0], y = row[1], z = row[2];
  for (int d = 0; d < D; ++d) out[d] = row[d];
  out[D] = x - mx;
  out[D + 1] = y - my;
  out[D + 2] = z - mz;
  out[D + 3] = x - cx;
  out[D + 4] = y - cy;
  if (dist) out[D + 5] = sqrtf(x * x + y * y + z * z);
}

// ---------------------------------------------------------------------------------------------------------------------------
// NL layers; CPL output channels per lane in the last layer (lane, lane + 64)
template <int IO, bool CANVAS, int NL, int CPL>
__global__ void __launch_bounds__(PW * 64) k_pillar_reader(const PillarArgs a) {
  extern __shared__ __align__(16) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = a.T, D = a.D, K1 = a.K1, U1 = a.U1;
  // ---- once per workgroup: the transposed layer-2 weight w2t[c][o] ----
  if constexpr (NL == 2) {
    float *w2t = lds + a.o_w2;
    const int IN2 = 2 * U1, U2 = a.U2;
    for (int e = tid; e < IN2 * U2; e += PW * 64) {
      const int o = e / IN2, c = e - o * IN2;       // coalesced read of w2[o][c]
      w2t[c * U2 + o] = a.w2[e];
    }
  }
  // ---- once per wave: this lane's layer-1 weights and affines ----
  constexpr int CPL1 = NL == 1 ? CPL : 1;           // with two layers U1 <= 64
  float w1r[CPL1][MAXK], s1[CPL1], h1[CPL1];
  int u1[CPL1];
#pragma unroll
  for (int j = 0; j < CPL1; ++j) {
    const int u = lane + 64 * j;
    u1[j] = u < U1 ? u : U1 - 1;                    // a lane past the width repeats the last unit and stores nothing
    bn_affine(a.g1, a.b1, a.m1, a.v1, a.eps1, u1[j], s1[j], h1[j]);
#pragma unroll
    for (int k = 0; k < MAXK; ++k) w1r[j][k] = k < K1 ? a.w1[u1[j] * K1 + k] : 0.f;
  }
  float s2[CPL], h2[CPL];
  int u2[CPL];
  if constexpr (NL == 2) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int u = lane + 64 * j;
      u2[j] = u < a.U2 ? u : a.U2 - 1;
      bn_affine(a.g2, a.b2, a.m2, a.v2, a.eps2, u2[j], s2[j], h2[j]);
    }
  }
  __syncthreads();

  float *slab = lds + a.o_wave + wv * a.wave_floats;
  float *raw = slab, *dec = slab + a.o_dec, *x1 = slab + a.o_x1;      // x1: row 0 = the max row, rows 1.. = the layer-1 rows
  const int64_t live = live_rows(a.count, a.P);
  const int64_t stride = (int64_t)gridDim.x * PW;
  for (int64_t p = (int64_t)blockIdx.x * PW + wv; p < live; p += stride) {
    int num = a.num[p];
    num = num < 0 ? 0 : (num > T ? T : num);
    const int nrow = num + (num < T ? 1 : 0);       // valid rows + one representative padded row; >= 1
    // ---- the valid rows -> LDS; mean; decoration ----
    const float *src = a.vox + p * (int64_t)T * D;
    for (int e = lane; e < num * D; e += 64) raw[e] = src[e];
    wave_sync();
    float mx = 0.f, my = 0.f, mz = 0.f;
    if (num > 0) pillar_mean(raw, D, num, mx, my, mz);                // every lane the same sum
    const float cx = (float)a.coors[p * 4 + 3] * a.vx + a.xo, cy = (float)a.coors[p * 4 + 2] * a.vy + a.yo;
    if (lane < num) decorate_row(raw + lane * D, D, a.dist != 0, mx, my, mz, cx, cy, dec + lane * K1);
    wave_sync();
    // ---- layer 1 ----
    float best1[CPL1];
#pragma unroll
    for (int j = 0; j < CPL1; ++j) best1[j] = num < T ? relu1(h1[j]) : 0.f;    // the padded row: relu(BN(0 . w)) = relu(shift)
    for (int t = 0; t < num; ++t) {
      float acc[CPL1];
#pragma unroll
      for (int j = 0; j < CPL1; ++j) acc[j] = 0.f;
#pragma unroll
      for (int k = 0; k < MAXK; ++k) {
        if (k < K1) {
          const float v = dec[t * K1 + k];
#pragma unroll
          for (int j = 0; j < CPL1; ++j) acc[j] += w1r[j][k] * v;
        }
      }
#pragma unroll
      for (int j = 0; j < CPL1; ++j) {
        const float v = relu1(acc[j] * s1[j] + h1[j]);
        best1[j] = fmaxf(best1[j], v);
        if constexpr (NL == 2) {
          if (lane < U1) x1[(1 + t) * a.pitch + lane] = v;
        }
      }
    }
    float out[CPL];
    if constexpr (NL == 1) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) out[j] = best1[j];
    } else {
      if (lane < U1) {
        x1[lane] = best1[0];
        if (num < T) x1[(1 + num) * a.pitch + lane] = relu1(h1[0]);
      }
      wave_sync();
      // ---- layer 2: the x_max half once, then RB rows at a time ----
      const float *w2t = lds + a.o_w2;
      const int U2 = a.U2;
      float cst[CPL];
#pragma unroll
      for (int j = 0; j < CPL; ++j) cst[j] = 0.f;
      for (int c = 0; c < U1; c += 4) {
        const float4 m = *reinterpret_cast<const float4 *>(x1 + c);
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          const float *w = w2t + (U1 + c) * U2 + u2[j];
          cst[j] += w[0] * m.x;
          cst[j] += w[U2] * m.y;
          cst[j] += w[2 * U2] * m.z;
          cst[j] += w[3 * U2] * m.w;
        }
      }
#pragma unroll
      for (int j = 0; j < CPL; ++j) out[j] = 0.f;   // relu(...) >= 0 and nrow >= 1
      for (int t0 = 0; t0 < nrow; t0 += RB) {
        float acc[RB][CPL];
        const float *xr[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          const int t = t0 + r < nrow ? t0 + r : nrow - 1;             // the last tile repeats its last row
          xr[r] = x1 + (1 + t) * a.pitch;
#pragma unroll
          for (int j = 0; j < CPL; ++j) acc[r][j] = cst[j];
        }
        for (int c = 0; c < U1; c += 4) {
          float4 xv[RB];
#pragma unroll
          for (int r = 0; r < RB; ++r) xv[r] = *reinterpret_cast<const float4 *>(xr[r] + c);
#pragma unroll
          for (int j = 0; j < CPL; ++j) {
            const float *w = w2t + c * U2 + u2[j];
            const float wa = w[0], wb = w[U2], wc = w[2 * U2], wd = w[3 * U2];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
              acc[r][j] += wa * xv[r].x;
              acc[r][j] += wb * xv[r].y;
              acc[r][j] += wc * xv[r].z;
              acc[r][j] += wd * xv[r].w;
            }
          }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
          for (int j = 0; j < CPL; ++j) out[j] = fmaxf(out[j], relu1(acc[r][j] * s2[j] + h2[j]));
      }
    }
    // ---- store: one rounding ----
    int64_t base;
    if constexpr (CANVAS) base = cell_base(a.coors, p, a.B, a.C, a.ny, a.nx);
    else base = p * (int64_t)a.C;
    if (base >= 0) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const int o = lane + 64 * j;
        if (o < a.C) {
          if constexpr (CANVAS) row_st1<IO>(a.canvas, base + (int64_t)o * a.ny * a.nx, out[j]);
          else row_st1<IO>(a.rows, base + o, out[j]);
        }
      }
    }
    wave_sync();                                    // the slab is read to the end before the next pillar overwrites it
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// E: the element as raw bits (uint32_t or uint16_t) -- a copy in any of the three types
template <class E>
__global__ void __launch_bounds__(256) k_pillar_scatter(const E *__restrict__ rows, const int32_t *__restrict__ coors, int64_t P, int32_t C,
                                                        const int32_t *__restrict__ count, int32_t B, int32_t ny, int32_t nx,
                                                        E *__restrict__ canvas) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t live = live_rows(count, P);
  if (e >= live * C) return;
  const int64_t p = e / C;
  const int32_t c = (int32_t)(e - p * C);
  const int64_t base = cell_base(coors, p, B, C, ny, nx);
  if (base >= 0) canvas[base + (int64_t)c * ny * nx] = rows[e];
}

template <class E>
__global__ void __launch_bounds__(256) k_pillar_gather(const E *__restrict__ canvas, const int32_t *__restrict__ coors, int64_t P, int32_t C,
                                                       const int32_t *__restrict__ count, int32_t B, int32_t ny, int32_t nx,
                                                       E *__restrict__ rows) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= P * C) return;
  const int64_t p = e / C;
  const int32_t c = (int32_t)(e - p * C);
  E v = 0;                                          // +0 in all three types
  if (p < live_rows(count, P)) {
    const int64_t base = cell_base(coors, p, B, C, ny, nx);
    if (base >= 0) v = canvas[base + (int64_t)c * ny * nx];
  }
  rows[e] = v;
}

// one thread per (pillar, row)
__global__ void __launch_bounds__(256) k_pillar_decorate(const float *__restrict__ vox, const int32_t *__restrict__ num_,
                                                         const int32_t *__restrict__ coors, int64_t P, const int32_t *__restrict__ count,
                                                         int32_t T, int32_t D, int32_t dist, float vx, float vy, float xo, float yo,
                                                         float *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= P * T) return;
  const int64_t p = e / T;
  const int32_t t = (int32_t)(e - p * T);
  const int K1 = D + 5 + (dist ? 1 : 0);
  float *dst = out + e * K1;
  int num = 0;
  if (p < live_rows(count, P)) {
    num = num_[p];
    num = num < 0 ? 0 : (num > T ? T : num);
  }
  if (t >= num) {                                   // a padded row, or a row of an inert pillar
    for (int k = 0; k < K1; ++k) dst[k] = 0.f;
    return;
  }
  const float *src = vox + p * (int64_t)T * D;
  float mx, my, mz;
  pillar_mean(src, D, num, mx, my, mz);             // the reader's own order
  const float cx = (float)coors[p * 4 + 3] * vx + xo, cy = (float)coors[p * 4 + 2] * vy + yo;
  decorate_row(src + t * D, D, dist != 0, mx, my, mz, cx, cy, dst);
}

// ---------------------------------------------------------------------------------------------------------------------------
constexpr int64_t MAX_ELEMS = 1LL << 31;

bool geom_ok(const link_pillar_geom_t *g) { return g && g->struct_bytes == (int32_t)sizeof(link_pillar_geom_t); }

bool canvas_ok(const link_pillar_geom_t *g, int64_t C) {
  if (g->batch < 1 || g->ny < 1 || g->nx < 1 || C < 1 || !row_io_ok(g->io_dtype)) return false;
  if ((int64_t)g->ny * g->nx > MAX_ELEMS) return false;
  return (int64_t)g->batch * C <= (1LL << 40) / ((int64_t)g->ny * g->nx);
}

size_t canvas_bytes(const link_pillar_geom_t *g, int64_t C) {
  return (size_t)g->batch * (size_t)C * g->ny * g->nx * (g->io_dtype == LINK_IO_F32 ? 4 : 2);
}

int zero_canvas(const link_pillar_geom_t *g, int64_t C, void *canvas, hipStream_t st, const char *what) {
  const hipError_t e = hipMemsetAsync(canvas, 0, canvas_bytes(g, C), st);
  if (e != hipSuccess) {
    set_error(what, e);
    return LINK_ERR_LAUNCH;
  }
  return LINK_OK;
}

bool reader_ok(const link_pillar_geom_t *g) {
  if (!geom_ok(g)) return false;
  if (g->t < 1 || g->t > LINK_PILLAR_MAX_T || g->d < 3 || g->d > LINK_PILLAR_MAX_D) return false;
  if (g->layers < 1 || g->layers > 2) return false;
  for (int i = 0; i < g->layers; ++i)
    if (g->width[i] < 16 || g->width[i] > LINK_PILLAR_MAX_WIDTH || g->width[i] % 16) return false;
  return row_io_ok(g->io_dtype);
}

bool layer_ok(const link_pillar_layer_t *l) {
  return l && l->weight && l->gamma && l->beta && l->running_mean && l->running_var && l->eps >= 0.f;
}

int32_t up4(int32_t v) { return (v + 3) & ~3; }

// the one-thread-per-element kernels: n x per elements in 256-thread workgroups must fit one grid dimension
bool elems_ok(int64_t n, int64_t per) { return per >= 1 && n <= (1LL << 38) / per; }

}  // namespace

extern "C" int link_pillar_native(const link_pillar_geom_t *geom) { return reader_ok(geom) ? 1 : 0; }

extern "C" int link_pillar_reader(const link_pillar_geom_t *geom, const float *voxels, const int32_t *num_points, const int32_t *coors,
                                  int64_t n_pillars, const int32_t *count, const link_pillar_layer_t *layer1,
                                  const link_pillar_layer_t *layer2, void *rows, void *canvas, void *stream) {
  if (!reader_ok(geom) || n_pillars < 0 || !layer_ok(layer1) || (rows != nullptr) == (canvas != nullptr)) return LINK_ERR_ARG;
  const int NL = geom->layers;
  if (NL == 2 && !layer_ok(layer2)) return LINK_ERR_ARG;
  const int32_t C = geom->width[NL - 1];
  if (n_pillars * (int64_t)geom->t * geom->d > (1LL << 40) || n_pillars > MAX_ELEMS) return LINK_ERR_ARG;
  if (canvas && !canvas_ok(geom, C)) return LINK_ERR_ARG;
  if (n_pillars > 0 && (!voxels || !num_points || !coors)) return LINK_ERR_ARG;
  if (canvas) {
    const int rc = zero_canvas(geom, C, canvas, S(stream), "link_pillar_reader: hipMemsetAsync");
    if (rc != LINK_OK) return rc;
  }
  if (n_pillars == 0) return LINK_OK;
  PillarArgs a{};
  a.vox = voxels; a.num = num_points; a.coors = coors; a.count = count;
  a.w1 = layer1->weight; a.g1 = layer1->gamma; a.b1 = layer1->beta; a.m1 = layer1->running_mean; a.v1 = layer1->running_var;
  a.eps1 = layer1->eps;
  if (NL == 2) {
    a.w2 = layer2->weight; a.g2 = layer2->gamma; a.b2 = layer2->beta; a.m2 = layer2->running_mean; a.v2 = layer2->running_var;
    a.eps2 = layer2->eps;
  }
  a.rows = rows; a.canvas = canvas; a.P = n_pillars;
  a.T = geom->t; a.D = geom->d; a.dist = geom->with_distance ? 1 : 0; a.K1 = geom->d + 5 + a.dist;
  a.U1 = NL == 2 ? geom->width[0] / 2 : geom->width[0];
  a.U2 = NL == 2 ? geom->width[1] : 0;
  a.C = C;
  a.B = geom->batch; a.ny = geom->ny; a.nx = geom->nx;
  a.vx = geom->vx; a.vy = geom->vy; a.xo = geom->x_offset; a.yo = geom->y_offset;
  a.pitch = up4(a.U1);
  a.o_w2 = 0;
  a.o_wave = NL == 2 ? up4(2 * a.U1 * a.U2) : 0;
  a.o_dec = up4(a.T * a.D);
  a.o_x1 = a.o_dec + up4(a.T * a.K1);
  a.wave_floats = a.o_x1 + (NL == 2 ? (a.T + 2) * a.pitch : 0);
  const size_t lds = (size_t)(a.o_wave + PW * a.wave_floats) * sizeof(float);      // at most 64 KiB + 4 x 23 KiB
  // persistent grid: enough workgroups to fill the chip several times over, never more than the pillars need
  int64_t nb = (n_pillars + PW - 1) / PW;
  if (nb > 256 * 8) nb = 256 * 8;
  const dim3 grid((unsigned)nb), block(PW * 64);
  const bool cpl2 = C > 64;
  const bool ok = dispatch_row_io(geom->io_dtype, [&](auto io) {
    return dispatch_bool2(canvas != nullptr, cpl2, [&](auto cv, auto wide) {
      constexpr int IO = decltype(io)::value;
      constexpr bool CV = decltype(cv)::value;
      constexpr int CPL = decltype(wide)::value ? 2 : 1;
      if (NL == 1) launch_kernel_unchecked(k_pillar_reader<IO, CV, 1, CPL>, grid, block, lds, S(stream), a);
      else launch_kernel_unchecked(k_pillar_reader<IO, CV, 2, CPL>, grid, block, lds, S(stream), a);
    });
  });
  if (!ok) return LINK_ERR_ARG;
  return check_launch("link_pillar_reader");
}

extern "C" int link_pillar_scatter(const link_pillar_geom_t *geom, const void *rows, const int32_t *coors, int64_t n_pillars,
                                   int32_t channels, const int32_t *count, void *canvas, void *stream) {
  if (!geom_ok(geom) || !canvas || n_pillars < 0 || !canvas_ok(geom, channels) || n_pillars > MAX_ELEMS) return LINK_ERR_ARG;
  if (!elems_ok(n_pillars, channels)) return LINK_ERR_ARG;
  if (n_pillars > 0 && (!rows || !coors)) return LINK_ERR_ARG;
  const int rc = zero_canvas(geom, channels, canvas, S(stream), "link_pillar_scatter: hipMemsetAsync");
  if (rc != LINK_OK || n_pillars == 0) return rc;
  const dim3 grid(blocks_for(n_pillars * channels, 256));
  if (geom->io_dtype == LINK_IO_F32)
    hipLaunchKernelGGL(k_pillar_scatter<uint32_t>, grid, dim3(256), 0, S(stream), reinterpret_cast<const uint32_t *>(rows), coors, n_pillars,
                       channels, count, geom->batch, geom->ny, geom->nx, reinterpret_cast<uint32_t *>(canvas));
  else
    hipLaunchKernelGGL(k_pillar_scatter<uint16_t>, grid, dim3(256), 0, S(stream), reinterpret_cast<const uint16_t *>(rows), coors, n_pillars,
                       channels, count, geom->batch, geom->ny, geom->nx, reinterpret_cast<uint16_t *>(canvas));
  return check_launch("link_pillar_scatter");
}

extern "C" int link_pillar_gather(const link_pillar_geom_t *geom, const void *grad_canvas, const int32_t *coors, int64_t n_pillars,
                                  int32_t channels, const int32_t *count, void *grad_rows, void *stream) {
  if (!geom_ok(geom) || !grad_canvas || n_pillars < 0 || !canvas_ok(geom, channels) || n_pillars > MAX_ELEMS) return LINK_ERR_ARG;
  if (!elems_ok(n_pillars, channels)) return LINK_ERR_ARG;
  if (n_pillars == 0) return LINK_OK;
  if (!grad_rows || !coors) return LINK_ERR_ARG;
  const dim3 grid(blocks_for(n_pillars * channels, 256));
  if (geom->io_dtype == LINK_IO_F32)
    hipLaunchKernelGGL(k_pillar_gather<uint32_t>, grid, dim3(256), 0, S(stream), reinterpret_cast<const uint32_t *>(grad_canvas), coors,
                       n_pillars, channels, count, geom->batch, geom->ny, geom->nx, reinterpret_cast<uint32_t *>(grad_rows));
  else
    hipLaunchKernelGGL(k_pillar_gather<uint16_t>, grid, dim3(256), 0, S(stream), reinterpret_cast<const uint16_t *>(grad_canvas), coors,
                       n_pillars, channels, count, geom->batch, geom->ny, geom->nx, reinterpret_cast<uint16_t *>(grad_rows));
  return check_launch("link_pillar_gather");
}

extern "C" int link_pillar_decorate(const link_pillar_geom_t *geom, const float *voxels, const int32_t *num_points, const int32_t *coors,
                                    int64_t n_pillars, const int32_t *count, float *decorated, void *stream) {
  if (!geom_ok(geom) || n_pillars < 0 || n_pillars > MAX_ELEMS) return LINK_ERR_ARG;
  if (geom->t < 1 || geom->t > LINK_PILLAR_MAX_T || geom->d < 3 || geom->d > LINK_PILLAR_MAX_D) return LINK_ERR_ARG;
  if (!elems_ok(n_pillars, geom->t)) return LINK_ERR_ARG;
  if (n_pillars == 0) return LINK_OK;
  if (!voxels || !num_points || !coors || !decorated) return LINK_ERR_ARG;
  hipLaunchKernelGGL(k_pillar_decorate, dim3(blocks_for(n_pillars * geom->t, 256)), dim3(256), 0, S(stream), voxels, num_points, coors,
                     n_pillars, count, geom->t, geom->d, geom->with_distance ? 1 : 0, geom->vx, geom->vy, geom->x_offset, geom->y_offset,
                     decorated);
  return check_launch("link_pillar_decorate");
}
