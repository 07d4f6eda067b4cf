// link_amd/csrc/dcn.hip -- section R of include/link_amd.h: deformable convolution (DCN v1) for gfx950.
// Reference: detection/det3d/ops/dcn/src/deform_conv_cuda.cpp (deform_conv_forward_cuda, deform_conv_backward_input_cuda,
// deform_conv_backward_parameters_cuda) over deform_conv_cuda_kernel.cu (deformable_im2col, deformable_col2im,
// deformable_col2im_coord).  The reference writes the [C kh kw, B Ho Wo] column matrix to memory and calls a GEMM; here the
// columns are sampled into LDS, 16 channels at a time, and go straight into the exact f32-input matrix instruction
// (v_mfma_f32_16x16x4_f32), so no column matrix exists in global memory in any of the three kernels.
//
//   k_dcn_fwd         workgroup = 128 output pixels (4 waves x 32) x all O.  Per (deformable group, tap): two offset loads per
//                     pixel, then per 16-channel chunk: weight slice [O,16] -> LDS (shared by the waves), bilinear samples
//                     [16,32] -> the wave's LDS tile, 4 k-steps x 2 pixel tiles x O/16 MFMAs into fp32 accumulators.
//   k_dcn_bwd_data    workgroup = 64 pixels (4 waves x 16).  grad_out of the wave's pixels stays in registers as B fragments;
//                     per (group, tap, 16-channel chunk) grad_col = W^T grad_out on the matrix cores, consumed at once:
//                     grad_offset sums over the group's channels in registers (fixed order, plain stores), grad_input is
//                     scattered with no-return fp32 atomics (the only part that is not reproducible run to run).
//   k_dcn_bwd_weight  grid = (pixel splits, group x tap x channel chunk).  grad_out columns^T with the pixels as the contraction
//                     axis; every wave writes its partial [O,16] block into the workspace, k_dcn_reduce_weight adds the
//                     partials in a fixed order.
// 16-bit tensors (forward only) are widened on load and rounded once on store; coordinates, samples and sums are fp32.
// Range test on the float coordinate before any conversion to an index: a NaN, an infinity or a value no int holds fails it,
// contributes 0, gets a zero offset gradient and scatters nothing.
#include "common.h"
#include "row_io.h"

using namespace link;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int KC = 16;       // channels per chunk (4 k-steps of the 16x16x4 instruction)
constexpr int WLD = 17;      // LDS row pitch of the weight chunk [o][16]: odd, so the 16 rows of a fragment fall in different banks
constexpr int NTP = 288;     // floats between the two 16-pixel halves of a wave's column tile (256 + 32: the halves' banks differ)

struct DcnArgs {
  const void *in, *off, *w, *out_c, *gout;
  void *out, *gin, *goff, *part;
  int32_t B, C, H, W, O, kh, kw, Ho, Wo, sh, sw, ph, pw, dlh, dlw, dg, Cg, relu;
  int64_t npix;             // B * Ho * Wo
  int32_t tiles_per_split;  // k_dcn_bwd_weight: 16-pixel tiles per workgroup
};

template <int IO>
__device__ __forceinline__ float ld1(const void *base, int64_t e) {
  if constexpr (IO == LINK_IO_F32) {
    return reinterpret_cast<const float *>(base)[e];
  } else if constexpr (IO == LINK_IO_F16) {
    return (float)reinterpret_cast<const _Float16 *>(base)[e];
  } else {
    return __uint_as_float((unsigned)reinterpret_cast<const unsigned short *>(base)[e] << 16);
  }
}
template <int IO>
__device__ __forceinline__ void st1(void *base, int64_t e, float v) {
  if constexpr (IO == LINK_IO_F32) {
    reinterpret_cast<float *>(base)[e] = v;
  } else if constexpr (IO == LINK_IO_F16) {
    reinterpret_cast<_Float16 *>(base)[e] = (_Float16)v;
  } else {
    reinterpret_cast<unsigned short *>(base)[e] = (unsigned short)bf16_rne(v);
  }
}

// one output pixel of the flattened [B, Ho, Wo] axis
struct Pix {
  int32_t b, ho, wo, rem;   // rem = ho * Wo + wo
  bool valid;
};
__device__ __forceinline__ Pix pix_of(int64_t p, const DcnArgs &a) {
  Pix x;
  x.valid = p < a.npix;
  const uint32_t hw = (uint32_t)a.Ho * (uint32_t)a.Wo;
  const uint32_t pp = x.valid ? (uint32_t)p : 0u;          // npix <= 2^31
  x.b = (int32_t)(pp / hw);
  x.rem = (int32_t)(pp - (uint32_t)x.b * hw);
  x.ho = x.rem / a.Wo;
  x.wo = x.rem - x.ho * a.Wo;
  return x;
}

// one bilinear sample: corner indices inside the H x W plane (0 where the corner is outside, with weight 0)
struct Tap {
  float w1, w2, w3, w4;     // weights of (hl,wl) (hl,wh) (hh,wl) (hh,wh), 0 for a corner off the map
  float lh, lw;             // fractions
  int32_t i1, i2, i3, i4;
  uint32_t m;               // bit k: corner k+1 is on the map; 0 when the sample fails the range test
};
__device__ __forceinline__ Tap tap_zero() {
  Tap t;
  t.w1 = t.w2 = t.w3 = t.w4 = t.lh = t.lw = 0.f;
  t.i1 = t.i2 = t.i3 = t.i4 = 0;
  t.m = 0;
  return t;
}
__device__ __forceinline__ Tap tap_at(float h, float w, int32_t H, int32_t W) {
  Tap t = tap_zero();
  // on the float values: NaN fails every comparison, +-inf and 1e30 fail one of them
  if (!(h > -1.f && w > -1.f && h < (float)H && w < (float)W)) return t;
  const float fh = floorf(h), fw = floorf(w);
  const int32_t hl = (int32_t)fh, wl = (int32_t)fw;       // in [-1, H-1] x [-1, W-1]
  const int32_t hh = hl + 1, wh = wl + 1;
  t.lh = h - fh;
  t.lw = w - fw;
  const float uh = 1.f - t.lh, uw = 1.f - t.lw;
  const bool a = hl >= 0, b = hh <= H - 1, c = wl >= 0, d = wh <= W - 1;
  if (a && c) { t.m |= 1u; t.i1 = hl * W + wl; t.w1 = uh * uw; }
  if (a && d) { t.m |= 2u; t.i2 = hl * W + wh; t.w2 = uh * t.lw; }
  if (b && c) { t.m |= 4u; t.i3 = hh * W + wl; t.w3 = t.lh * uw; }
  if (b && d) { t.m |= 8u; t.i4 = hh * W + wh; t.w4 = t.lh * t.lw; }
  return t;
}

template <int IO>
__device__ __forceinline__ Tap tap_of(const DcnArgs &a, const Pix &x, int32_t g, int32_t tap) {
  if (!x.valid) return tap_zero();
  const int32_t K = a.kh * a.kw;
  const int64_t hw = (int64_t)a.Ho * a.Wo;
  const int64_t e = ((int64_t)x.b * a.dg * 2 * K + (int64_t)g * 2 * K + 2 * tap) * hw + x.rem;
  const float dh = ld1<IO>(a.off, e), dw = ld1<IO>(a.off, e + hw);
  const int32_t i = tap / a.kw, j = tap - i * a.kw;
  const float h = (float)((int64_t)x.ho * a.sh - a.ph + (int64_t)i * a.dlh) + dh;
  const float w = (float)((int64_t)x.wo * a.sw - a.pw + (int64_t)j * a.dlw) + dw;
  return tap_at(h, w, a.H, a.W);
}

template <int IO>
__device__ __forceinline__ float sample(const void *in, int64_t plane, const Tap &t) {
  if (!t.m) return 0.f;
  // corners off the map read element 0 of the plane with weight 0 (finite inputs assumed, as in the reference)
  const float v1 = (t.m & 1u) ? ld1<IO>(in, plane + t.i1) : 0.f, v2 = (t.m & 2u) ? ld1<IO>(in, plane + t.i2) : 0.f;
  const float v3 = (t.m & 4u) ? ld1<IO>(in, plane + t.i3) : 0.f, v4 = (t.m & 8u) ? ld1<IO>(in, plane + t.i4) : 0.f;
  return t.w1 * v1 + t.w2 * v2 + t.w3 * v3 + t.w4 * v4;
}

// weight chunk of (group g, tap, channels c0 .. c0+15) -> s_w[o][c], zero rows / columns past O / Cg.  All 256 threads.
template <int IO, int OTN>
__device__ __forceinline__ void stage_weight(float *s_w, const DcnArgs &a, int32_t g, int32_t tap, int32_t c0, int tid) {
  const int32_t K = a.kh * a.kw;
#pragma unroll 4
  for (int e = tid; e < OTN * 16 * KC; e += 256) {
    const int o = e >> 4, c = e & 15;
    float v = 0.f;
    if (o < a.O && c0 + c < a.Cg) v = ld1<IO>(a.w, ((int64_t)o * a.C + (int64_t)g * a.Cg + c0 + c) * K + tap);
    s_w[o * WLD + c] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
template <int IO, int OTN>
__global__ void __launch_bounds__(256) k_dcn_fwd(const DcnArgs a) {
  __shared__ float s_w[OTN * 16 * WLD];
  __shared__ float s_col[4][2 * NTP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t pix0 = (int64_t)blockIdx.x * 128 + wv * 32;
  const int32_t K = a.kh * a.kw;
  const int64_t HW = (int64_t)a.H * a.W;
  // sampling role: pixel lane & 31, channels (lane >> 5) + 2 i of the chunk
  const int sp = lane & 31;
  const Pix sx = pix_of(pix0 + sp, a);
  const int64_t in_img = (int64_t)sx.b * a.C * HW;
  float *col = s_col[wv];
  const int cs = (sp >> 4) * NTP + (sp & 15);
  f32x4 acc[OTN][2];
#pragma unroll
  for (int ot = 0; ot < OTN; ++ot) acc[ot][0] = acc[ot][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int32_t g = 0; g < a.dg; ++g) {
    for (int32_t tap = 0; tap < K; ++tap) {
      const Tap t = tap_of<IO>(a, sx, g, tap);
      for (int32_t c0 = 0; c0 < a.Cg; c0 += KC) {
        __syncthreads();                         // the last chunk's fragments are read
        stage_weight<IO, OTN>(s_w, a, g, tap, c0, tid);
#pragma unroll
        for (int i = 0; i < KC / 2; ++i) {
          const int c = (lane >> 5) + 2 * i;
          float v = 0.f;
          if (c0 + c < a.Cg) v = sample<IO>(a.in, in_img + ((int64_t)g * a.Cg + c0 + c) * HW, t);
          col[cs + c * 16] = v;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          // B[k = 4 ks + (lane >> 4)][pixel = lane & 15] = col[k * 16 + pixel] = col[64 ks + lane]
          const float b0 = col[ks * 64 + lane], b1 = col[NTP + ks * 64 + lane];
#pragma unroll
          for (int ot = 0; ot < OTN; ++ot) {
            const float aa = s_w[(ot * 16 + (lane & 15)) * WLD + 4 * ks + (lane >> 4)];
            acc[ot][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aa, b0, acc[ot][0], 0, 0, 0);
            acc[ot][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aa, b1, acc[ot][1], 0, 0, 0);
          }
        }
      }
    }
  }
  // D[o = 16 ot + 4 (lane >> 4) + r][pixel = lane & 15]
  const int64_t howo = (int64_t)a.Ho * a.Wo;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const Pix x = pix_of(pix0 + nt * 16 + (lane & 15), a);
    if (!x.valid) continue;
#pragma unroll
    for (int ot = 0; ot < OTN; ++ot) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = ot * 16 + 4 * (lane >> 4) + r;
        if (o < a.O) {
          float v = acc[ot][nt][r];
          if (a.relu) v = v < 0.f ? 0.f : v;     // a NaN stays a NaN, as in torch.relu
          st1<IO>(a.out, ((int64_t)x.b * a.O + o) * howo + x.rem, v);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
template <int OTN>
__global__ void __launch_bounds__(256) k_dcn_bwd_data(const DcnArgs a) {
  __shared__ float s_w[OTN * 16 * WLD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t K = a.kh * a.kw;
  const int64_t HW = (int64_t)a.H * a.W, howo = (int64_t)a.Ho * a.Wo;
  const Pix x = pix_of((int64_t)blockIdx.x * 64 + wv * 16 + (lane & 15), a);
  const int64_t in_img = (int64_t)x.b * a.C * HW;
  const float *gout = reinterpret_cast<const float *>(a.gout);
  const float *outc = reinterpret_cast<const float *>(a.out_c);
  float *gin = reinterpret_cast<float *>(a.gin);
  float *goff = reinterpret_cast<float *>(a.goff);
  // B[k = o = 4 ks + (lane >> 4)][pixel = lane & 15]: grad_out of the wave's 16 pixels, masked by the ReLU
  float bf[OTN * 4];
#pragma unroll
  for (int ks = 0; ks < OTN * 4; ++ks) {
    const int o = 4 * ks + (lane >> 4);
    float v = 0.f;
    if (x.valid && o < a.O) {
      const int64_t e = ((int64_t)x.b * a.O + o) * howo + x.rem;
      v = gout[e];
      if (a.relu && !(outc[e] > 0.f)) v = 0.f;
    }
    bf[ks] = v;
  }
  for (int32_t g = 0; g < a.dg; ++g) {
    for (int32_t tap = 0; tap < K; ++tap) {
      const Tap t = tap_of<LINK_IO_F32>(a, x, g, tap);
      const float uh = 1.f - t.lh, uw = 1.f - t.lw;
      float goh = 0.f, gow = 0.f;
      for (int32_t c0 = 0; c0 < a.Cg; c0 += KC) {
        __syncthreads();
        stage_weight<LINK_IO_F32, OTN>(s_w, a, g, tap, c0, tid);
        __syncthreads();
        // A[m = c = lane & 15][k = o = 4 ks + (lane >> 4)] = W[o][c]
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < OTN * 4; ++ks)
          d = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w[(4 * ks + (lane >> 4)) * WLD + (lane & 15)], bf[ks], d, 0, 0, 0);
        // D[c = 4 (lane >> 4) + r][pixel = lane & 15]: grad_col of four channels at this lane's pixel
        if (t.m) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = c0 + 4 * (lane >> 4) + r;
            if (c >= a.Cg) continue;
            const float gc = d[r];
            const int64_t plane = in_img + ((int64_t)g * a.Cg + c) * HW;
            if (goff) {
              const float *in = reinterpret_cast<const float *>(a.in) + plane;
              const float v1 = (t.m & 1u) ? in[t.i1] : 0.f, v2 = (t.m & 2u) ? in[t.i2] : 0.f;
              const float v3 = (t.m & 4u) ? in[t.i3] : 0.f, v4 = (t.m & 8u) ? in[t.i4] : 0.f;
              // d sample / dh and / dw (the reference's get_coordinate_weight)
              goh += gc * (uw * (v3 - v1) + t.lw * (v4 - v2));
              gow += gc * (uh * (v2 - v1) + t.lh * (v4 - v3));
            }
            if (gin) {
              float *gp = gin + plane;
              if (t.m & 1u) unsafeAtomicAdd(gp + t.i1, gc * t.w1);
              if (t.m & 2u) unsafeAtomicAdd(gp + t.i2, gc * t.w2);
              if (t.m & 4u) unsafeAtomicAdd(gp + t.i3, gc * t.w3);
              if (t.m & 8u) unsafeAtomicAdd(gp + t.i4, gc * t.w4);
            }
          }
        }
      }
      if (goff) {
        // the four lane groups hold disjoint channels of the same pixel: fixed-order sum, one store per pixel
        goh += __shfl_xor(goh, 16, 64);
        gow += __shfl_xor(gow, 16, 64);
        goh += __shfl_xor(goh, 32, 64);
        gow += __shfl_xor(gow, 32, 64);
        if (lane < 16 && x.valid) {
          const int64_t e = ((int64_t)x.b * a.dg * 2 * K + (int64_t)g * 2 * K + 2 * tap) * howo + x.rem;
          goff[e] = goh;
          goff[e + howo] = gow;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
template <int OTN>
__global__ void __launch_bounds__(256) k_dcn_bwd_weight(const DcnArgs a) {
  __shared__ float s_col[4][16 * WLD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t K = a.kh * a.kw;
  const int32_t nchunk = (a.Cg + KC - 1) / KC;
  const int32_t y = blockIdx.y;
  const int32_t c0 = (y % nchunk) * KC, gt = y / nchunk, tap = gt % K, g = gt / K;
  const int64_t HW = (int64_t)a.H * a.W, howo = (int64_t)a.Ho * a.Wo;
  const int64_t ntile = (a.npix + 15) / 16;
  const int64_t t_begin = (int64_t)blockIdx.x * a.tiles_per_split;
  int64_t t_end = t_begin + a.tiles_per_split;
  if (t_end > ntile) t_end = ntile;
  const float *gout = reinterpret_cast<const float *>(a.gout);
  const float *outc = reinterpret_cast<const float *>(a.out_c);
  float *col = s_col[wv];
  f32x4 acc[OTN];
#pragma unroll
  for (int ot = 0; ot < OTN; ++ot) acc[ot] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t tile = t_begin + wv; tile < t_end; tile += 4) {      // wave-local from here: no workgroup barrier in the loop
    const int64_t p0 = tile * 16;
    // columns of the tile: pixel lane & 15, channels c0 + (lane >> 4) + 4 j  ->  col[pixel][c]
    const Pix x = pix_of(p0 + (lane & 15), a);
    const Tap t = tap_of<LINK_IO_F32>(a, x, g, tap);
    const int64_t in_img = (int64_t)x.b * a.C * HW;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = (lane >> 4) + 4 * j;
      float v = 0.f;
      if (c0 + c < a.Cg) v = sample<LINK_IO_F32>(a.in, in_img + ((int64_t)g * a.Cg + c0 + c) * HW, t);
      col[(lane & 15) * WLD + c] = v;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): the wave's own LDS writes have landed
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      // B[k = pixel 4 ks + (lane >> 4)][n = c = lane & 15];  A[m = o = 16 ot + (lane & 15)][k = pixel 4 ks + (lane >> 4)]
      const float b = col[(4 * ks + (lane >> 4)) * WLD + (lane & 15)];
      const Pix xa = pix_of(p0 + 4 * ks + (lane >> 4), a);
#pragma unroll
      for (int ot = 0; ot < OTN; ++ot) {
        const int o = ot * 16 + (lane & 15);
        float v = 0.f;
        if (xa.valid && o < a.O) {
          const int64_t e = ((int64_t)xa.b * a.O + o) * howo + xa.rem;
          v = gout[e];
          if (a.relu && !(outc[e] > 0.f)) v = 0.f;
        }
        acc[ot] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, b, acc[ot], 0, 0, 0);
      }
    }
    __builtin_amdgcn_wave_barrier();             // the fragments are in registers before the next tile overwrites col
  }
  // partial [split][o][c][tap], split = 4 blockIdx.x + wave; D[o = 16 ot + 4 (lane >> 4) + r][c = lane & 15]
  float *part = reinterpret_cast<float *>(a.part) + ((int64_t)blockIdx.x * 4 + wv) * ((int64_t)a.O * a.C * K);
  const int c = c0 + (lane & 15);
  if (c < a.Cg) {
#pragma unroll
    for (int ot = 0; ot < OTN; ++ot) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = ot * 16 + 4 * (lane >> 4) + r;
        if (o < a.O) part[((int64_t)o * a.C + (int64_t)g * a.Cg + c) * K + tap] = acc[ot][r];
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_dcn_reduce_weight(const float *__restrict__ part, int32_t nsplit, int64_t n,
                                                           float *__restrict__ gw) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float s = 0.f;
  for (int32_t k = 0; k < nsplit; ++k) s += part[(int64_t)k * n + e];     // fixed order: reproducible
  gw[e] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------
constexpr int64_t MAX_ELEMS = 1LL << 31;

// shapes, envelope and sizes; fills the kernel arguments.  Host only.
bool dcn_args(const link_deform_conv_geom_t *q, DcnArgs *a) {
  if (!q) return false;
  if (q->batch < 1 || q->c < 1 || q->h < 1 || q->w < 1 || q->o < 1 || q->kh < 1 || q->kw < 1) return false;
  if (q->stride_h < 1 || q->stride_w < 1 || q->dil_h < 1 || q->dil_w < 1 || q->pad_h < 0 || q->pad_w < 0) return false;
  if (q->groups != 1 || q->deformable_groups < 1) return false;
  if ((int64_t)q->kh * q->kw > LINK_DCN_MAX_TAPS || q->c > LINK_DCN_MAX_CHANNELS || q->o > LINK_DCN_MAX_CHANNELS) return false;
  if (q->c % q->deformable_groups != 0) return false;
  const int32_t K = q->kh * q->kw;
  if (q->offset_channels != q->deformable_groups * 2 * K) return false;
  if (!row_io_ok(q->io_dtype) || (q->flags & ~LINK_DCN_RELU)) return false;
  const int64_t eh = (int64_t)q->h + 2LL * q->pad_h - ((int64_t)q->dil_h * (q->kh - 1) + 1);
  const int64_t ew = (int64_t)q->w + 2LL * q->pad_w - ((int64_t)q->dil_w * (q->kw - 1) + 1);
  if (eh < 0 || ew < 0) return false;
  const int64_t Ho = eh / q->stride_h + 1, Wo = ew / q->stride_w + 1;
  if (Ho > MAX_ELEMS || Wo > MAX_ELEMS || Ho * Wo > MAX_ELEMS) return false;
  const int64_t npix = (int64_t)q->batch * Ho * Wo;
  if (npix > MAX_ELEMS || npix * q->o > MAX_ELEMS || npix * q->offset_channels > MAX_ELEMS) return false;
  if ((int64_t)q->batch * q->c * q->h * q->w > MAX_ELEMS || (int64_t)q->h * q->w > MAX_ELEMS) return false;
  if ((int64_t)q->batch * q->c > MAX_ELEMS / ((int64_t)q->h * q->w)) return false;
  *a = DcnArgs{};
  a->B = q->batch; a->C = q->c; a->H = q->h; a->W = q->w; a->O = q->o; a->kh = q->kh; a->kw = q->kw;
  a->Ho = (int32_t)Ho; a->Wo = (int32_t)Wo; a->sh = q->stride_h; a->sw = q->stride_w; a->ph = q->pad_h; a->pw = q->pad_w;
  a->dlh = q->dil_h; a->dlw = q->dil_w; a->dg = q->deformable_groups; a->Cg = q->c / q->deformable_groups;
  a->relu = (q->flags & LINK_DCN_RELU) ? 1 : 0;
  a->npix = npix;
  return true;
}

// pixel splits of k_dcn_bwd_weight: enough workgroups to fill the chip a few times over, at most 64 (256 partials)
void weight_splits(const DcnArgs &a, int32_t *splits, int32_t *tiles_per_split) {
  const int64_t ntile = (a.npix + 15) / 16;
  const int64_t ny = (int64_t)a.dg * a.kh * a.kw * ((a.Cg + KC - 1) / KC);
  int64_t s = (1024 + ny - 1) / ny;
  if (s > 64) s = 64;
  const int64_t most = (ntile + 3) / 4;
  if (s > most) s = most;
  if (s < 1) s = 1;
  const int64_t tps = (ntile + s - 1) / s;
  *splits = (int32_t)((ntile + tps - 1) / tps);
  *tiles_per_split = (int32_t)tps;
}

template <int IO>
void launch_fwd(const DcnArgs &a, hipStream_t st) {
  const unsigned nb = (unsigned)((a.npix + 127) / 128);
  if (a.O <= 64) hipLaunchKernelGGL((k_dcn_fwd<IO, 4>), dim3(nb), dim3(256), 0, st, a);
  else if (a.O <= 128) hipLaunchKernelGGL((k_dcn_fwd<IO, 8>), dim3(nb), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_dcn_fwd<IO, 16>), dim3(nb), dim3(256), 0, st, a);
}

}  // namespace

extern "C" size_t link_deform_conv_workspace_bytes(const link_deform_conv_geom_t *geom) {
  DcnArgs a;
  if (!dcn_args(geom, &a)) return 0;
  int32_t splits, tps;
  weight_splits(a, &splits, &tps);
  return (size_t)splits * 4 * (size_t)a.O * a.C * a.kh * a.kw * sizeof(float);
}

extern "C" int link_deform_conv_forward(const link_deform_conv_geom_t *geom, const void *input, const void *offset,
                                        const void *weight, void *output, void *stream) {
  DcnArgs a;
  if (!input || !offset || !weight || !output || !dcn_args(geom, &a)) return LINK_ERR_ARG;
  a.in = input; a.off = offset; a.w = weight; a.out = output;
  if (geom->io_dtype == LINK_IO_F32) launch_fwd<LINK_IO_F32>(a, S(stream));
  else if (geom->io_dtype == LINK_IO_F16) launch_fwd<LINK_IO_F16>(a, S(stream));
  else launch_fwd<LINK_IO_BF16>(a, S(stream));
  return check_launch("link_deform_conv_forward");
}

extern "C" int link_deform_conv_backward_data(const link_deform_conv_geom_t *geom, const float *input, const float *offset,
                                              const float *weight, const float *output, const float *grad_out,
                                              float *grad_input, float *grad_offset, void *stream) {
  DcnArgs a;
  if (!input || !offset || !weight || !grad_out || (!grad_input && !grad_offset) || !dcn_args(geom, &a)) return LINK_ERR_ARG;
  if (geom->io_dtype != LINK_IO_F32 || (a.relu && !output)) return LINK_ERR_ARG;
  a.in = input; a.off = offset; a.w = weight; a.out_c = output; a.gout = grad_out; a.gin = grad_input; a.goff = grad_offset;
  if (grad_input) {
    const hipError_t e = hipMemsetAsync(grad_input, 0, (size_t)a.B * a.C * a.H * a.W * sizeof(float), S(stream));
    if (e != hipSuccess) {
      set_error("link_deform_conv_backward_data: hipMemsetAsync", e);
      return LINK_ERR_LAUNCH;
    }
  }
  const unsigned nb = (unsigned)((a.npix + 63) / 64);
  if (a.O <= 64) hipLaunchKernelGGL((k_dcn_bwd_data<4>), dim3(nb), dim3(256), 0, S(stream), a);
  else if (a.O <= 128) hipLaunchKernelGGL((k_dcn_bwd_data<8>), dim3(nb), dim3(256), 0, S(stream), a);
  else hipLaunchKernelGGL((k_dcn_bwd_data<16>), dim3(nb), dim3(256), 0, S(stream), a);
  return check_launch("link_deform_conv_backward_data");
}

extern "C" int link_deform_conv_backward_weight(const link_deform_conv_geom_t *geom, const float *input, const float *offset,
                                                const float *output, const float *grad_out, float *grad_weight, void *workspace,
                                                size_t workspace_bytes, void *stream) {
  DcnArgs a;
  if (!input || !offset || !grad_out || !grad_weight || !workspace || !dcn_args(geom, &a)) return LINK_ERR_ARG;
  if (geom->io_dtype != LINK_IO_F32 || (a.relu && !output)) return LINK_ERR_ARG;
  int32_t splits, tps;
  weight_splits(a, &splits, &tps);
  const int64_t n = (int64_t)a.O * a.C * a.kh * a.kw;
  if (workspace_bytes < (size_t)splits * 4 * (size_t)n * sizeof(float)) return LINK_ERR_WORKSPACE;
  a.in = input; a.off = offset; a.out_c = output; a.gout = grad_out; a.part = workspace; a.tiles_per_split = tps;
  const dim3 grid((unsigned)splits, (unsigned)(a.dg * a.kh * a.kw * ((a.Cg + KC - 1) / KC)));
  if (a.O <= 64) hipLaunchKernelGGL((k_dcn_bwd_weight<4>), grid, dim3(256), 0, S(stream), a);
  else if (a.O <= 128) hipLaunchKernelGGL((k_dcn_bwd_weight<8>), grid, dim3(256), 0, S(stream), a);
  else hipLaunchKernelGGL((k_dcn_bwd_weight<16>), grid, dim3(256), 0, S(stream), a);
  int rc = check_launch("link_deform_conv_backward_weight");
  if (rc != LINK_OK) return rc;
  hipLaunchKernelGGL(k_dcn_reduce_weight, dim3(blocks_for(n, 256)), dim3(256), 0, S(stream),
                     reinterpret_cast<const float *>(workspace), splits * 4, n, grad_weight);
  return check_launch("link_deform_conv_backward_weight (reduce)");
}
