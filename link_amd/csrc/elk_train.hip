// link_amd/csrc/elk_train.hip -- the training form of ELKBlock on the general layout (include/link_amd.h, sections C and D):
//
//   link_elk_mid_forward / _backward   the middle of R_core between pre_mix and self.norm.  The forward and two thirds of
//                                      the backward ARE the forward's kernels (elk.hip, through elk_host.h); k_voxel_bwd_g
//                                      is the voxel-level backward with the theta gradient.
//   link_elk_out_ln_backward           k_out_ln_bwd_g: backward of self.norm on the recomputed rows
//   link_premix_ln_backward[_io]       k_premix_ln_bwd: backward of pre_mix on the forward's MFMA schedule
//   link_ln_add_relu_*[_io]            k_ln_add_relu_fwd_g / _bwd_g: the block's tail, y = relu(addend + LayerNorm(x))
//   link_sum_partials                  the deterministic tail of every parameter gradient
//
// The _io entries take feature rows in fp16 / bf16 (autocast; row_io.h): feats / x read and g_feats / g_x written in
// io_dtype, everything else fp32 as in the fp32 entries, which are the same code with io_dtype = LINK_IO_F32.
#include "dispatch.h"
#include "elk_common.h"
#include "elk_host.h"
#include "row_io.h"

using namespace link;

// rows of every per-workgroup partial array = workgroups of the kernels that write them
extern "C" int32_t link_elk_mid_partial_rows(void) { return 1024; }

// ---------------------------------------------------------------------------------------------
// Training form of the middle of R_core:  new = demodulate(aggregate(modulate(fin, theta)), theta)
// (linkunet.py:151-176 between pre_mix and self.norm), forward and backward.  The two LayerNorms and
// the pre_mix Linear stay with the host framework's autograd (library GEMM + its LayerNorm).
//
// Backward, per part (v = A[block(i)], X = modulated features, g = grad(new)):
//   gA[m]   = (1/den[m]) * sum_{i in m} g_i * d(new)/d(v)          -> the forward's modulate+block-sum kernel
//             with the backward factors ([cos, sin] | [cos, -sin] | [cos, sin, 1]) and a row scale
//   gS[n]   = sum_{m : n in region(m)} gA[m]                       -> the forward's block gather, transposed
//             neighbourhood, no normalisation
//   g_fin_i = gS[block(i)] . d(X)/d(fin)  (+ the -theta*g term of cos_x), and the theta gradient folded
//             into per-workgroup partial sums of d/d(alpha) and d/d(pos_weight)  -> k_voxel_bwd_g
// ---------------------------------------------------------------------------------------------
template <int LPR, int OP>
__global__ void __launch_bounds__(256) k_voxel_bwd_g(
    const float *__restrict__ gS, const float *__restrict__ A_tab, const float *__restrict__ fin,
    const float *__restrict__ g_new, const int4 *__restrict__ vox_sorted, const int32_t *__restrict__ pos_blk,
    const float *__restrict__ w_pos, const float *__restrict__ alpha, const int32_t *__restrict__ hdr, int c,
    int cg, float coord_div, float *__restrict__ g_fin, float *__restrict__ partials) {
  constexpr int P = (OP == LINK_OP_COSX) ? 3 : 2;
  constexpr int G = 64 / LPR;
  __shared__ float red[4][16][LPR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & (LPR - 1);
  const int ch0 = 4 * li;
  const bool act = ch0 < c;
  const int cofs = act ? ch0 : 0;
  const int n = hdr[LINK_HDR_NVALID];
  const int ra = P * c;
  float w0[4], w1[4], w2[4], al[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    int tc = act ? (ch0 + e) % cg : 0;
    w0[e] = w_pos[3 * tc + 0]; w1[e] = w_pos[3 * tc + 1]; w2[e] = w_pos[3 * tc + 2];
    al[e] = alpha ? alpha[tc] : 1.0f;
  }
  float acc[4][4];                                 // [d alpha | d w.x | d w.y | d w.z][channel of the lane]
#pragma unroll
  for (int q = 0; q < 4; q++)
#pragma unroll
    for (int e = 0; e < 4; e++) acc[q][e] = 0.f;
  const int64_t ngroups = (int64_t)gridDim.x * 4 * G;
  for (int64_t p = ((int64_t)blockIdx.x * 4 + wave) * G + lane / LPR; p < n; p += ngroups) {
    const int4 rc = vox_sorted[p];
    const int b = pos_blk[p];
    float4 gx4[P], av4[P];
#pragma unroll
    for (int pp = 0; pp < P; pp++) {
      gx4[pp] = *reinterpret_cast<const float4 *>(&gS[(int64_t)b * ra + pp * c + cofs]);
      av4[pp] = *reinterpret_cast<const float4 *>(&A_tab[(int64_t)b * ra + pp * c + cofs]);
    }
    const float4 f4 = *reinterpret_cast<const float4 *>(&fin[(int64_t)rc.w * c + cofs]);
    const float4 g4 = *reinterpret_cast<const float4 *>(&g_new[(int64_t)rc.w * c + cofs]);
    float x = (float)rc.x, y = (float)rc.y, z = (float)rc.z;
    if (coord_div != 1.0f) { x = x / coord_div; y = y / coord_div; z = z / coord_div; }
    const float fv[4] = {f4.x, f4.y, f4.z, f4.w}, gv[4] = {g4.x, g4.y, g4.z, g4.w};
    const float gx0[4] = {gx4[0].x, gx4[0].y, gx4[0].z, gx4[0].w}, gx1[4] = {gx4[1].x, gx4[1].y, gx4[1].z, gx4[1].w};
    const float gx2[4] = {gx4[P - 1].x, gx4[P - 1].y, gx4[P - 1].z, gx4[P - 1].w};
    const float v0[4] = {av4[0].x, av4[0].y, av4[0].z, av4[0].w}, v1[4] = {av4[1].x, av4[1].y, av4[1].z, av4[1].w};
    float gf[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float t = fmaf(z, w2[e], fmaf(y, w1[e], x * w0[e]));
      const float th = t * al[e];
      float sn, cs;
      sincos_fast(th, sn, cs);
      float g_cs, g_sn, gth;
      if (OP == LINK_OP_SIN) {                     // new = v0 cos - v1 sin ; X = [f sin, f cos]
        gf[e] = gx0[e] * sn + gx1[e] * cs;
        g_cs = gv[e] * v0[e] + gx1[e] * fv[e];
        g_sn = gx0[e] * fv[e] - gv[e] * v1[e];
      } else {                                     // new = v0 cos + v1 sin (+ v2 - f theta) ; X = [f cos, f sin, (f theta)]
        gf[e] = gx0[e] * cs + gx1[e] * sn;
        g_cs = gv[e] * v0[e] + gx0[e] * fv[e];
        g_sn = gv[e] * v1[e] + gx1[e] * fv[e];
      }
      gth = cs * g_sn - sn * g_cs;
      if (OP == LINK_OP_COSX) {
        const float d = gx2[e] - gv[e];
        gf[e] = fmaf(d, th, gf[e]);
        gth = fmaf(d, fv[e], gth);
      }
      if (act) {
        acc[0][e] = fmaf(gth, t, acc[0][e]);
        const float ga = gth * al[e];
        acc[1][e] = fmaf(ga, x, acc[1][e]);
        acc[2][e] = fmaf(ga, y, acc[2][e]);
        acc[3][e] = fmaf(ga, z, acc[3][e]);
      }
    }
    if (act) *reinterpret_cast<float4 *>(&g_fin[(int64_t)rc.w * c + ch0]) = make_float4(gf[0], gf[1], gf[2], gf[3]);
  }
  // fixed reduction tree: groups of the wave, then the 4 waves through LDS -> one partial row per workgroup
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int e = 0; e < 4; e++) acc[q][e] += __shfl_xor(acc[q][e], o, 64);
  if (lane < LPR)
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int e = 0; e < 4; e++) red[wave][q * 4 + e][li] = acc[q][e];
  __syncthreads();
  if (wave == 0 && lane < LPR && act) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      float4 o;
      o.x = (red[0][q * 4 + 0][li] + red[1][q * 4 + 0][li]) + (red[2][q * 4 + 0][li] + red[3][q * 4 + 0][li]);
      o.y = (red[0][q * 4 + 1][li] + red[1][q * 4 + 1][li]) + (red[2][q * 4 + 1][li] + red[3][q * 4 + 1][li]);
      o.z = (red[0][q * 4 + 2][li] + red[1][q * 4 + 2][li]) + (red[2][q * 4 + 2][li] + red[3][q * 4 + 2][li]);
      o.w = (red[0][q * 4 + 3][li] + red[1][q * 4 + 3][li]) + (red[2][q * 4 + 3][li] + red[3][q * 4 + 3][li]);
      *reinterpret_cast<float4 *>(&partials[((int64_t)blockIdx.x * 4 + q) * c + ch0]) = o;
    }
  }
}

// Backward of self.norm fused with the recomputation of its input: new_i is rebuilt from the saved A
// row of the voxel's block exactly as the forward's voxel kernel builds it (same operation order), its
// LayerNorm statistics are recomputed, and g_new = rstd * (gy*w - mean(gy*w) - xhat * mean(gy*w*xhat)).
// Per-workgroup partial sums of d/d(norm.weight) = sum gy*xhat and d/d(norm.bias) = sum gy.
template <int LPR, int OP>
__global__ void __launch_bounds__(256) k_out_ln_bwd_g(
    const float *__restrict__ g_out, const float *__restrict__ A_tab, const float *__restrict__ fin,
    const int4 *__restrict__ vox_sorted, const int32_t *__restrict__ pos_blk, const float *__restrict__ w_pos,
    const float *__restrict__ alpha, const float *__restrict__ ln_w, const int32_t *__restrict__ hdr, int c,
    int cg, float coord_div, float eps, float *__restrict__ g_new, float *__restrict__ partials) {
  constexpr int P = (OP == LINK_OP_COSX) ? 3 : 2;
  constexpr int G = 64 / LPR;
  __shared__ float red[4][8][LPR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & (LPR - 1);
  const int ch0 = 4 * li;
  const bool act = ch0 < c;
  const int cofs = act ? ch0 : 0;
  const int n = hdr[LINK_HDR_NVALID];
  const int ra = P * c;
  const float inv_c = 1.0f / (float)c;
  float w0[4], w1[4], w2[4], al[4], gw[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    int ch = act ? ch0 + e : 0;
    int tc = ch % cg;
    w0[e] = w_pos[3 * tc + 0]; w1[e] = w_pos[3 * tc + 1]; w2[e] = w_pos[3 * tc + 2];
    al[e] = alpha ? alpha[tc] : 1.0f;
    gw[e] = ln_w[ch];
  }
  float aw[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t ngroups = (int64_t)gridDim.x * 4 * G;
  for (int64_t p = ((int64_t)blockIdx.x * 4 + wave) * G + lane / LPR; p < n; p += ngroups) {
    const int4 rc = vox_sorted[p];
    const int b = pos_blk[p];
    float4 av4[P];
#pragma unroll
    for (int pp = 0; pp < P; pp++) av4[pp] = *reinterpret_cast<const float4 *>(&A_tab[(int64_t)b * ra + pp * c + cofs]);
    float4 f4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (OP == LINK_OP_COSX) f4 = *reinterpret_cast<const float4 *>(&fin[(int64_t)rc.w * c + cofs]);
    const float4 g4 = *reinterpret_cast<const float4 *>(&g_out[(int64_t)rc.w * c + cofs]);
    float x = (float)rc.x, y = (float)rc.y, z = (float)rc.z;
    if (coord_div != 1.0f) { x = x / coord_div; y = y / coord_div; z = z / coord_div; }
    const float v0[4] = {av4[0].x, av4[0].y, av4[0].z, av4[0].w}, v1[4] = {av4[1].x, av4[1].y, av4[1].z, av4[1].w};
    const float v2[4] = {av4[P - 1].x, av4[P - 1].y, av4[P - 1].z, av4[P - 1].w};
    const float fv[4] = {f4.x, f4.y, f4.z, f4.w}, gy[4] = {g4.x, g4.y, g4.z, g4.w};
    float nv[4], sm = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float th = theta_of(x, y, z, w0[e], w1[e], w2[e], al[e]);
      float sn, cs;
      sincos_fast(th, sn, cs);
      float va;
      if (OP == LINK_OP_SIN) va = __fsub_rn(__fmul_rn(v0[e], cs), __fmul_rn(v1[e], sn));
      else va = __fadd_rn(__fmul_rn(v0[e], cs), __fmul_rn(v1[e], sn));
      if (OP == LINK_OP_COSX) va = __fadd_rn(va, __fsub_rn(v2[e], link_mul_rn(fv[e], th)));
      nv[e] = act ? va : 0.f;
      sm += nv[e];
    }
    const float mean = grp_sum<LPR>(sm) * inv_c;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) { const float d = act ? nv[e] - mean : 0.f; q += d * d; }
    const float rstd = 1.0f / sqrtf(grp_sum<LPR>(q) * inv_c + eps);
    float xh[4], gx[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      xh[e] = act ? (nv[e] - mean) * rstd : 0.f;
      gx[e] = act ? gy[e] * gw[e] : 0.f;
      s1 += gx[e];
      s2 = fmaf(gx[e], xh[e], s2);
      if (act) { aw[e] = fmaf(gy[e], xh[e], aw[e]); ab[e] += gy[e]; }
    }
    const float m1 = grp_sum<LPR>(s1) * inv_c, m2 = grp_sum<LPR>(s2) * inv_c;
    if (act) {
      float4 o;
      o.x = rstd * (gx[0] - m1 - xh[0] * m2);
      o.y = rstd * (gx[1] - m1 - xh[1] * m2);
      o.z = rstd * (gx[2] - m1 - xh[2] * m2);
      o.w = rstd * (gx[3] - m1 - xh[3] * m2);
      *reinterpret_cast<float4 *>(&g_new[(int64_t)rc.w * c + ch0]) = o;
    }
  }
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
    for (int e = 0; e < 4; e++) { aw[e] += __shfl_xor(aw[e], o, 64); ab[e] += __shfl_xor(ab[e], o, 64); }
  if (lane < LPR)
#pragma unroll
    for (int e = 0; e < 4; e++) { red[wave][e][li] = aw[e]; red[wave][4 + e][li] = ab[e]; }
  __syncthreads();
  if (wave == 0 && lane < LPR && act) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      float4 o;
      o.x = (red[0][q * 4 + 0][li] + red[1][q * 4 + 0][li]) + (red[2][q * 4 + 0][li] + red[3][q * 4 + 0][li]);
      o.y = (red[0][q * 4 + 1][li] + red[1][q * 4 + 1][li]) + (red[2][q * 4 + 1][li] + red[3][q * 4 + 1][li]);
      o.z = (red[0][q * 4 + 2][li] + red[1][q * 4 + 2][li]) + (red[2][q * 4 + 2][li] + red[3][q * 4 + 2][li]);
      o.w = (red[0][q * 4 + 3][li] + red[1][q * 4 + 3][li]) + (red[2][q * 4 + 3][li] + red[3][q * 4 + 3][li]);
      *reinterpret_cast<float4 *>(&partials[((int64_t)blockIdx.x * 2 + q) * c + ch0]) = o;
    }
  }
}

// Backward of pre_mix = LayerNorm(F @ Wpre^T): the pre-LayerNorm activations are RECOMPUTED with the
// forward's MFMA schedule (so the statistics are bit-identical to the forward's), the LayerNorm backward
// is applied in the accumulator layout (lane = 4 channels x 4 tiles of one voxel), and
// g_F = g_pre @ Wpre runs as a second MFMA pass whose B operand IS that accumulator layout and whose A
// operand is a transposed copy of W in LDS.  g_pre is also stored (the weight gradient
// g_pre^T @ F is a plain GEMM left to the library), and per-workgroup partial sums of
// d/d(pre_mix.1.weight) = sum g_fin*xhat and d/d(pre_mix.1.bias) = sum g_fin are written.
// IO (row_io.h): type of feats (read) and g_feats (written); g_fin, g_pre and the partials stay fp32.
template <int C, int IO = LINK_IO_F32>
__global__ void __launch_bounds__(256) k_premix_ln_bwd(const void *__restrict__ feats,
                                                       const float *__restrict__ w_pre,
                                                       const float *__restrict__ ln_w,
                                                       const float *__restrict__ g_fin, int64_t n, float eps,
                                                       float *__restrict__ g_pre, void *__restrict__ g_feats,
                                                       float *__restrict__ partials) {
  constexpr int T = C / 16;
  constexpr int LDW = C + 4;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float *w_lds = reinterpret_cast<float *>(smem_raw);          // W   [j][k]
  float *wt_lds = w_lds + C * LDW;                             // W^T [k][j]
  float *red = wt_lds + C * LDW;                               // [4 waves][2][C]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  for (int e = tid * 4; e < C * C; e += 256 * 4) {
    int r = e / C, col = e - r * C;
    const float4 w4 = *reinterpret_cast<const float4 *>(&w_pre[e]);
    *reinterpret_cast<float4 *>(&w_lds[r * LDW + col]) = w4;
    wt_lds[(col + 0) * LDW + r] = w4.x; wt_lds[(col + 1) * LDW + r] = w4.y;
    wt_lds[(col + 2) * LDW + r] = w4.z; wt_lds[(col + 3) * LDW + r] = w4.w;
  }
  __syncthreads();
  float lw[T][4];
#pragma unroll
  for (int tp = 0; tp < T; tp++) {
    const float4 l4 = *reinterpret_cast<const float4 *>(&ln_w[16 * tp + 4 * g]);
    lw[tp][0] = l4.x; lw[tp][1] = l4.y; lw[tp][2] = l4.z; lw[tp][3] = l4.w;
  }
  float pw[T][4], pb[T][4];
#pragma unroll
  for (int tp = 0; tp < T; tp++)
#pragma unroll
    for (int r = 0; r < 4; r++) pw[tp][r] = pb[tp][r] = 0.f;
  const int64_t tiles = (n + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t v = tile * 16 + li;
    const bool ok = v < n;
    const int64_t vl = ok ? v : n - 1;
    float4 f[T], gf4[T];
#pragma unroll
    for (int t = 0; t < T; t++) f[t] = row_ld4<IO>(feats, vl * C + 16 * t + 4 * g);
#pragma unroll
    for (int t = 0; t < T; t++) gf4[t] = *reinterpret_cast<const float4 *>(&g_fin[vl * C + 16 * t + 4 * g]);
    floatx4 acc[T];
#pragma unroll
    for (int tp = 0; tp < T; tp++) acc[tp] = (floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < T; t++) {
#pragma unroll
      for (int tp = 0; tp < T; tp++) {
        float4 a = *reinterpret_cast<const float4 *>(&w_lds[(16 * tp + li) * LDW + 16 * t + 4 * g]);
        acc[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, f[t].x, acc[tp], 0, 0, 0);
        acc[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, f[t].y, acc[tp], 0, 0, 0);
        acc[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, f[t].z, acc[tp], 0, 0, 0);
        acc[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, f[t].w, acc[tp], 0, 0, 0);
      }
    }
    float s = 0.f;
#pragma unroll
    for (int tp = 0; tp < T; tp++) s += (acc[tp][0] + acc[tp][1]) + (acc[tp][2] + acc[tp][3]);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    const float mean = s * (1.0f / C);
    float q = 0.f;
#pragma unroll
    for (int tp = 0; tp < T; tp++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float d = acc[tp][r] - mean;
        q += d * d;
      }
    q += __shfl_xor(q, 16, 64);
    q += __shfl_xor(q, 32, 64);
    const float rstd = 1.0f / sqrtf(q * (1.0f / C) + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int tp = 0; tp < T; tp++) {
      const float gv[4] = {gf4[tp].x, gf4[tp].y, gf4[tp].z, gf4[tp].w};
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float xh = (acc[tp][r] - mean) * rstd;
        const float gx = gv[r] * lw[tp][r];
        s1 += gx;
        s2 = fmaf(gx, xh, s2);
        if (ok) { pw[tp][r] = fmaf(gv[r], xh, pw[tp][r]); pb[tp][r] += gv[r]; }
        acc[tp][r] = xh;                            // keep xhat; gx is recomputed below (saves 16 VGPRs)
      }
    }
    s1 += __shfl_xor(s1, 16, 64); s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 16, 64); s2 += __shfl_xor(s2, 32, 64);
    const float m1 = s1 * (1.0f / C), m2 = s2 * (1.0f / C);
#pragma unroll
    for (int tp = 0; tp < T; tp++) {
      const float gv[4] = {gf4[tp].x, gf4[tp].y, gf4[tp].z, gf4[tp].w};
#pragma unroll
      for (int r = 0; r < 4; r++) acc[tp][r] = rstd * (gv[r] * lw[tp][r] - m1 - acc[tp][r] * m2);   // g_pre
      if (ok)
        *reinterpret_cast<float4 *>(&g_pre[v * C + 16 * tp + 4 * g]) = make_float4(acc[tp][0], acc[tp][1], acc[tp][2], acc[tp][3]);
    }
    // g_F[v][k] = sum_j g_pre[v][j] W[j][k]:  D2[k][v] = sum_j W^T[k][j] g_pre[v][j]
    floatx4 acc2[T];
#pragma unroll
    for (int tp = 0; tp < T; tp++) acc2[tp] = (floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < T; t++) {
#pragma unroll
      for (int tp = 0; tp < T; tp++) {
        float4 a = *reinterpret_cast<const float4 *>(&wt_lds[(16 * tp + li) * LDW + 16 * t + 4 * g]);
        acc2[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, acc[t][0], acc2[tp], 0, 0, 0);
        acc2[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, acc[t][1], acc2[tp], 0, 0, 0);
        acc2[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, acc[t][2], acc2[tp], 0, 0, 0);
        acc2[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, acc[t][3], acc2[tp], 0, 0, 0);
      }
    }
    if (ok) {
#pragma unroll
      for (int tp = 0; tp < T; tp++)
        row_st4<IO>(g_feats, v * C + 16 * tp + 4 * g, make_float4(acc2[tp][0], acc2[tp][1], acc2[tp][2], acc2[tp][3]));
    }
  }
  // LayerNorm parameter gradients: sum over the 16 voxel lanes of each quarter-wave, then over waves
#pragma unroll
  for (int tp = 0; tp < T; tp++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      pw[tp][r] = grp_sum<16>(pw[tp][r]);
      pb[tp][r] = grp_sum<16>(pb[tp][r]);
    }
  if (li == 0) {
#pragma unroll
    for (int tp = 0; tp < T; tp++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        red[(wave * 2 + 0) * C + 16 * tp + 4 * g + r] = pw[tp][r];
        red[(wave * 2 + 1) * C + 16 * tp + 4 * g + r] = pb[tp][r];
      }
  }
  __syncthreads();
  for (int e = tid; e < 2 * C; e += 256) {
    const int qq = e / C, ch = e - qq * C;
    partials[((int64_t)blockIdx.x * 2 + qq) * C + ch] =
        (red[(0 * 2 + qq) * C + ch] + red[(1 * 2 + qq) * C + ch]) + (red[(2 * 2 + qq) * C + ch] + red[(3 * 2 + qq) * C + ch]);
  }
}

template <int C, int IO = LINK_IO_F32>
static int launch_premix_bwd(const void *feats, const float *w_pre, const float *ln_w, const float *g_fin,
                             int64_t n, float eps, float *g_pre, void *g_feats, float *partials, int wgs,
                             hipStream_t st) {
  size_t lds = ((size_t)2 * C * (C + 4) + 8 * C) * sizeof(float);
  return launch_kernel(k_premix_ln_bwd<C, IO>, dim3((unsigned)wgs), dim3(256), lds, st, "link_premix_ln_backward", feats, w_pre, ln_w, g_fin, n, eps,
                       g_pre, g_feats, partials);
}

// the one place the width and the row type of the pre_mix backward are chosen; the callers have checked both
static int premix_ln_backward(const void *feats, int io_dtype, const float *w_pre, const float *ln_w, const float *g_fin,
                              int64_t n, int c, float eps, float *g_pre, void *g_feats, float *partials, void *stream) {
  if (!row_io_ok(io_dtype)) return LINK_ERR_ARG;
  if (n < 0 || c <= 0 || (c & 15) != 0 || c > 128) return LINK_ERR_ARG;     // MFMA path only; callers fall back
  if (n == 0) return LINK_OK;
  if (!feats || !w_pre || !ln_w || !g_fin || !g_pre || !g_feats || !partials) return LINK_ERR_ARG;
  int rc = LINK_ERR_ARG;
  dispatch_width(c, [&](auto w) {
    constexpr int C = decltype(w)::value;
    return dispatch_row_io(io_dtype, [&](auto io) {
      rc = launch_premix_bwd<C, decltype(io)::value>(feats, w_pre, ln_w, g_fin, n, eps, g_pre, g_feats, partials,
                                                     link_elk_mid_partial_rows(), S(stream));
    });
  });
  return rc;
}

extern "C" int link_premix_ln_backward(const float *feats, const float *w_pre, const float *ln_w,
                                       const float *g_fin, int64_t n, int32_t c, float eps, float *g_pre,
                                       float *g_feats, float *partials, void *stream) {
  return premix_ln_backward(feats, LINK_IO_F32, w_pre, ln_w, g_fin, n, c, eps, g_pre, g_feats, partials, stream);
}

extern "C" int link_premix_ln_backward_io(const void *feats, int32_t io_dtype, const float *w_pre, const float *ln_w,
                                          const float *g_fin, int64_t n, int32_t c, float eps, float *g_pre, void *g_feats,
                                          float *partials, void *stream) {
  return premix_ln_backward(feats, io_dtype, w_pre, ln_w, g_fin, n, c, eps, g_pre, g_feats, partials, stream);
}

extern "C" int link_elk_out_ln_backward(const float *g_out, const float *A, const float *fin,
                                        const int32_t *vox_sorted, const int32_t *pos_blk, const float *w_pos,
                                        const float *alpha, const float *ln_w, const int32_t *hdr,
                                        const link_elk_desc_t *desc, int64_t n, float *g_new, float *partials,
                                        void *stream) {
  if (check_desc(desc) != LINK_OK || n < 0 || (desc->c & 3) != 0) return LINK_ERR_ARG;
  if (n == 0) return LINK_OK;
  if (!g_out || !A || !vox_sorted || !pos_blk || !w_pos || !ln_w || !hdr || !g_new || !partials) return LINK_ERR_ARG;
  if (desc->op == LINK_OP_COSX && !fin) return LINK_ERR_ARG;
  const int4 *v4 = reinterpret_cast<const int4 *>(vox_sorted);
  hipStream_t st = S(stream);
  const link_elk_desc_t &d = *desc;
  const bool ok = dispatch_lpr(d.c, [&](auto lpr) {
    constexpr int LPR = decltype(lpr)::value;
    return dispatch_op(d.op, [&](auto op) {
      hipLaunchKernelGGL((k_out_ln_bwd_g<LPR, decltype(op)::value>), dim3(link_elk_mid_partial_rows()), dim3(256), 0, st, g_out, A,
                         fin, v4, pos_blk, w_pos, alpha, ln_w, hdr, d.c, d.cg, d.coord_div, d.eps, g_new, partials);
    });
  });
  if (!ok) return LINK_ERR_ARG;
  return check_launch("link_elk_out_ln_backward");
}

// ---------------------------------------------------------------------------------------------
// The block's tail for training (linkunet.py:183 / ts_elk.py:228): y = relu(addend + LayerNorm(x)),
// forward and backward, one 16-byte-per-lane group per row (persistent grid).  Inference fuses this
// tail into the convolution kernel instead (conv.hip, row N2).
// ---------------------------------------------------------------------------------------------
// IO (row_io.h): type of the x rows (the local_mix output; link_ln_add_relu_*_io); addend, y and g_y stay fp32.
template <int LPR, int IO = LINK_IO_F32>
__global__ void __launch_bounds__(256) k_ln_add_relu_fwd_g(const void *__restrict__ x,
                                                           const float *__restrict__ addend,
                                                           const float *__restrict__ ln_w,
                                                           const float *__restrict__ ln_b, int64_t n, int c,
                                                           float eps, float *__restrict__ y) {
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & (LPR - 1), ch0 = 4 * li;
  const bool act = ch0 < c;
  const int cofs = act ? ch0 : 0;
  const float inv_c = 1.0f / (float)c;
  const float4 w4 = *reinterpret_cast<const float4 *>(&ln_w[cofs]), b4 = *reinterpret_cast<const float4 *>(&ln_b[cofs]);
  const int64_t ngroups = (int64_t)gridDim.x * 4 * G;
  for (int64_t i = ((int64_t)blockIdx.x * 4 + wave) * G + lane / LPR; i < n; i += ngroups) {
    float4 v = row_ld4<IO>(x, i * c + cofs);
    const float4 a = *reinterpret_cast<const float4 *>(&addend[i * c + cofs]);
    if (!act) v = make_float4(0.f, 0.f, 0.f, 0.f);
    const float mean = grp_sum<LPR>((v.x + v.y) + (v.z + v.w)) * inv_c;
    const float dx = act ? v.x - mean : 0.f, dy = act ? v.y - mean : 0.f, dz = act ? v.z - mean : 0.f, dw = act ? v.w - mean : 0.f;
    const float rstd = 1.0f / sqrtf(grp_sum<LPR>((dx * dx + dy * dy) + (dz * dz + dw * dw)) * inv_c + eps);
    if (act) {
      float4 o;
      o.x = fmaxf(a.x + (dx * rstd * w4.x + b4.x), 0.f);
      o.y = fmaxf(a.y + (dy * rstd * w4.y + b4.y), 0.f);
      o.z = fmaxf(a.z + (dz * rstd * w4.z + b4.z), 0.f);
      o.w = fmaxf(a.w + (dw * rstd * w4.w + b4.w), 0.f);
      *reinterpret_cast<float4 *>(&y[i * c + ch0]) = o;
    }
  }
}

template <int LPR, int IO = LINK_IO_F32>
__global__ void __launch_bounds__(256) k_ln_add_relu_bwd_g(const float *__restrict__ g_y,
                                                           const float *__restrict__ y,
                                                           const void *__restrict__ x,
                                                           const float *__restrict__ ln_w, int64_t n, int c,
                                                           float eps, float *__restrict__ g_addend,
                                                           void *__restrict__ g_x, float *__restrict__ partials) {
  constexpr int G = 64 / LPR;
  __shared__ float red[4][8][LPR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & (LPR - 1), ch0 = 4 * li;
  const bool act = ch0 < c;
  const int cofs = act ? ch0 : 0;
  const float inv_c = 1.0f / (float)c;
  const float4 w4 = *reinterpret_cast<const float4 *>(&ln_w[cofs]);
  const float gw[4] = {w4.x, w4.y, w4.z, w4.w};
  float aw[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t ngroups = (int64_t)gridDim.x * 4 * G;
  for (int64_t i = ((int64_t)blockIdx.x * 4 + wave) * G + lane / LPR; i < n; i += ngroups) {
    const float4 v4 = row_ld4<IO>(x, i * c + cofs);
    const float4 y4 = *reinterpret_cast<const float4 *>(&y[i * c + cofs]);
    const float4 g4 = *reinterpret_cast<const float4 *>(&g_y[i * c + cofs]);
    const float xv[4] = {v4.x, v4.y, v4.z, v4.w}, yv[4] = {y4.x, y4.y, y4.z, y4.w}, gv[4] = {g4.x, g4.y, g4.z, g4.w};
    float sm = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) sm += act ? xv[e] : 0.f;
    const float mean = grp_sum<LPR>(sm) * inv_c;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) { const float d = act ? xv[e] - mean : 0.f; q += d * d; }
    const float rstd = 1.0f / sqrtf(grp_sum<LPR>(q) * inv_c + eps);
    float g[4], xh[4], gx[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      g[e] = (act && yv[e] > 0.f) ? gv[e] : 0.f;              // ReLU mask from the saved output
      xh[e] = act ? (xv[e] - mean) * rstd : 0.f;
      gx[e] = g[e] * gw[e];
      s1 += gx[e];
      s2 = fmaf(gx[e], xh[e], s2);
      aw[e] = fmaf(g[e], xh[e], aw[e]);
      ab[e] += g[e];
    }
    const float m1 = grp_sum<LPR>(s1) * inv_c, m2 = grp_sum<LPR>(s2) * inv_c;
    if (act) {
      *reinterpret_cast<float4 *>(&g_addend[i * c + ch0]) = make_float4(g[0], g[1], g[2], g[3]);
      row_st4<IO>(g_x, i * c + ch0,
                  make_float4(rstd * (gx[0] - m1 - xh[0] * m2), rstd * (gx[1] - m1 - xh[1] * m2),
                              rstd * (gx[2] - m1 - xh[2] * m2), rstd * (gx[3] - m1 - xh[3] * m2)));
    }
  }
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
    for (int e = 0; e < 4; e++) { aw[e] += __shfl_xor(aw[e], o, 64); ab[e] += __shfl_xor(ab[e], o, 64); }
  if (lane < LPR)
#pragma unroll
    for (int e = 0; e < 4; e++) { red[wave][e][li] = aw[e]; red[wave][4 + e][li] = ab[e]; }
  __syncthreads();
  if (wave == 0 && lane < LPR && act) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      float4 o;
      o.x = (red[0][q * 4 + 0][li] + red[1][q * 4 + 0][li]) + (red[2][q * 4 + 0][li] + red[3][q * 4 + 0][li]);
      o.y = (red[0][q * 4 + 1][li] + red[1][q * 4 + 1][li]) + (red[2][q * 4 + 1][li] + red[3][q * 4 + 1][li]);
      o.z = (red[0][q * 4 + 2][li] + red[1][q * 4 + 2][li]) + (red[2][q * 4 + 2][li] + red[3][q * 4 + 2][li]);
      o.w = (red[0][q * 4 + 3][li] + red[1][q * 4 + 3][li]) + (red[2][q * 4 + 3][li] + red[3][q * 4 + 3][li]);
      *reinterpret_cast<float4 *>(&partials[((int64_t)blockIdx.x * 2 + q) * c + ch0]) = o;
    }
  }
}

static int ln_add_relu_forward(const void *x, int io_dtype, const float *addend, const float *ln_w, const float *ln_b, int64_t n,
                               int32_t c, float eps, float *y, void *stream) {
  if (!row_io_ok(io_dtype)) return LINK_ERR_ARG;
  if (n < 0 || c <= 0 || (c & 3) != 0 || c > 256) return LINK_ERR_ARG;
  if (n == 0) return LINK_OK;
  if (!x || !addend || !ln_w || !ln_b || !y) return LINK_ERR_ARG;
  const bool ok = dispatch_lpr(c, [&](auto lpr) {
    constexpr int LPR = decltype(lpr)::value;
    return dispatch_row_io(io_dtype, [&](auto io) {
      hipLaunchKernelGGL((k_ln_add_relu_fwd_g<LPR, decltype(io)::value>), dim3(1024), dim3(256), 0, S(stream), x, addend, ln_w,
                         ln_b, n, (int)c, eps, y);
    });
  });
  return ok ? check_launch("link_ln_add_relu_forward") : LINK_ERR_ARG;
}

static int ln_add_relu_backward(const float *g_y, const float *y, const void *x, int io_dtype, const float *ln_w, int64_t n,
                                int32_t c, float eps, float *g_addend, void *g_x, float *partials, void *stream) {
  if (!row_io_ok(io_dtype)) return LINK_ERR_ARG;
  if (n < 0 || c <= 0 || (c & 3) != 0 || c > 256) return LINK_ERR_ARG;
  if (!partials) return LINK_ERR_ARG;
  if (n > 0 && (!g_y || !y || !x || !ln_w || !g_addend || !g_x)) return LINK_ERR_ARG;
  const bool ok = dispatch_lpr(c, [&](auto lpr) {
    constexpr int LPR = decltype(lpr)::value;
    return dispatch_row_io(io_dtype, [&](auto io) {
      hipLaunchKernelGGL((k_ln_add_relu_bwd_g<LPR, decltype(io)::value>), dim3(link_elk_mid_partial_rows()), dim3(256), 0,
                         S(stream), g_y, y, x, ln_w, n, (int)c, eps, g_addend, g_x, partials);
    });
  });
  return ok ? check_launch("link_ln_add_relu_backward") : LINK_ERR_ARG;
}

extern "C" int link_ln_add_relu_forward(const float *x, const float *addend, const float *ln_w,
                                        const float *ln_b, int64_t n, int32_t c, float eps, float *y,
                                        void *stream) {
  return ln_add_relu_forward(x, LINK_IO_F32, addend, ln_w, ln_b, n, c, eps, y, stream);
}

extern "C" int link_ln_add_relu_forward_io(const void *x, int32_t io_dtype, const float *addend, const float *ln_w,
                                           const float *ln_b, int64_t n, int32_t c, float eps, float *y, void *stream) {
  return ln_add_relu_forward(x, io_dtype, addend, ln_w, ln_b, n, c, eps, y, stream);
}

extern "C" int link_ln_add_relu_backward(const float *g_y, const float *y, const float *x, const float *ln_w,
                                         int64_t n, int32_t c, float eps, float *g_addend, float *g_x,
                                         float *partials, void *stream) {
  return ln_add_relu_backward(g_y, y, x, LINK_IO_F32, ln_w, n, c, eps, g_addend, g_x, partials, stream);
}

extern "C" int link_ln_add_relu_backward_io(const float *g_y, const float *y, const void *x, int32_t io_dtype, const float *ln_w,
                                            int64_t n, int32_t c, float eps, float *g_addend, void *g_x, float *partials,
                                            void *stream) {
  return ln_add_relu_backward(g_y, y, x, io_dtype, ln_w, n, c, eps, g_addend, g_x, partials, stream);
}

// Column sums of up to three per-workgroup partial arrays [rows, cols_k] in one launch, fixed order
// (row lanes ascending, then a fixed LDS tree): the deterministic tail of every parameter gradient.
__global__ void __launch_bounds__(256) k_sum_partials(const float *__restrict__ p0, int c0,
                                                      const float *__restrict__ p1, int c1,
                                                      const float *__restrict__ p2, int c2, int64_t rows,
                                                      float *__restrict__ out) {
  __shared__ float red[32][8];
  const int col = blockIdx.x * 8 + (threadIdx.x & 7), rl = threadIdx.x >> 3;
  const int total = c0 + c1 + c2;
  const float *src = nullptr;
  int stride = 0, off = 0;
  if (col < c0) { src = p0; stride = c0; off = col; }
  else if (col < c0 + c1) { src = p1; stride = c1; off = col - c0; }
  else if (col < total) { src = p2; stride = c2; off = col - c0 - c1; }
  float acc = 0.f;
  if (src)
    for (int64_t r = rl; r < rows; r += 32) acc += src[r * stride + off];
  red[rl][threadIdx.x & 7] = acc;
  __syncthreads();
  for (int h = 16; h >= 1; h >>= 1) {
    if (rl < h) red[rl][threadIdx.x & 7] += red[rl + h][threadIdx.x & 7];
    __syncthreads();
  }
  if (rl == 0 && col < total) out[col] = red[0][threadIdx.x & 7];
}

extern "C" int link_sum_partials(const float *p0, int32_t cols0, const float *p1, int32_t cols1,
                                 const float *p2, int32_t cols2, int64_t rows, float *out, void *stream) {
  if (cols0 < 0 || cols1 < 0 || cols2 < 0 || rows < 0 || !out) return LINK_ERR_ARG;
  if ((cols0 && !p0) || (cols1 && !p1) || (cols2 && !p2)) return LINK_ERR_ARG;
  const int total = cols0 + cols1 + cols2;
  if (total == 0) return LINK_OK;
  hipLaunchKernelGGL(k_sum_partials, dim3((total + 7) / 8), dim3(256), 0, S(stream), p0, (int)cols0, p1, (int)cols1,
                     p2, (int)cols2, rows, out);
  return check_launch("link_sum_partials");
}

static int train_args_ok(const link_elk_desc_t *desc, const link_grid_t *grid, int64_t n, int64_t m_cap) {
  if (check_desc(desc) != LINK_OK || !grid || n < 0 || m_cap < 0) return LINK_ERR_ARG;
  if ((desc->c & 3) != 0 || desc->r > 3) return LINK_ERR_ARG;      // group kernels only; callers fall back
  return LINK_OK;
}

extern "C" int link_elk_mid_forward(const float *fin, const int32_t *vox_sorted, const int32_t *pos_blk,
                                    const int32_t *blk_start, const int32_t *blk_coords,
                                    const int32_t *cell_blk, const link_grid_t *grid, const int32_t *hdr,
                                    const float *w_pos, const float *alpha, const link_elk_desc_t *desc,
                                    const float *ln_w, const float *ln_b, int64_t n, int64_t m_cap,
                                    float *S_, float *A, float *den, float *out, void *stream) {
  int rc = train_args_ok(desc, grid, n, m_cap);
  if (rc != LINK_OK) return rc;
  if (n == 0 || m_cap == 0) return LINK_OK;
  if (!fin || !vox_sorted || !pos_blk || !blk_start || !blk_coords || !cell_blk || !hdr || !w_pos || !S_ || !A ||
      !den || !out)
    return LINK_ERR_ARG;
  const int4 *v4 = reinterpret_cast<const int4 *>(vox_sorted);
  if (!modsum_group_path(desc, S(stream), fin, v4, w_pos, alpha, blk_start, hdr, S_, m_cap)) return LINK_ERR_ARG;
  rc = check_launch("link_elk_mid_forward");
  if (rc != LINK_OK) return rc;
  rc = block_gather_impl(S_, blk_coords, cell_blk, grid, hdr, desc, m_cap, A, 0, den, stream);
  if (rc != LINK_OK) return rc;
  if ((ln_w == nullptr) != (ln_b == nullptr)) return LINK_ERR_ARG;
  return voxel_demod_impl(A, fin, vox_sorted, pos_blk, w_pos, alpha, ln_w, ln_b, hdr, desc, n, out, stream);
}

extern "C" int link_elk_mid_backward(const float *g_out, const float *fin, const float *A, const float *den,
                                     const int32_t *vox_sorted, const int32_t *pos_blk,
                                     const int32_t *blk_start, const int32_t *blk_coords,
                                     const int32_t *cell_blk, const link_grid_t *grid, const int32_t *hdr,
                                     const float *w_pos, const float *alpha, const link_elk_desc_t *desc,
                                     int64_t n, int64_t m_cap, float *S_, float *gS, float *g_fin,
                                     float *partials, void *stream) {
  int rc = train_args_ok(desc, grid, n, m_cap);
  if (rc != LINK_OK) return rc;
  if (n == 0 || m_cap == 0) return LINK_OK;
  if (!g_out || !fin || !A || !den || !vox_sorted || !pos_blk || !blk_start || !blk_coords || !cell_blk || !hdr ||
      !w_pos || !S_ || !gS || !g_fin || !partials)
    return LINK_ERR_ARG;
  const int4 *v4 = reinterpret_cast<const int4 *>(vox_sorted);
  hipStream_t st = S(stream);
  const int bop = desc->op == LINK_OP_COS ? LINK_OP_COS : (desc->op == LINK_OP_SIN ? LINK_OPI_SIN_BWD : LINK_OPI_COSX_BWD);
  if (!modsum_group_path(desc, st, g_out, v4, w_pos, alpha, blk_start, hdr, S_, m_cap, bop, den)) return LINK_ERR_ARG;
  rc = check_launch("link_elk_mid_backward");
  if (rc != LINK_OK) return rc;
  rc = block_gather_impl(S_, blk_coords, cell_blk, grid, hdr, desc, m_cap, gS, 1 | 2, nullptr, stream);
  if (rc != LINK_OK) return rc;
  const link_elk_desc_t &d = *desc;
  const bool ok = dispatch_lpr(d.c, [&](auto lpr) {
    constexpr int LPR = decltype(lpr)::value;
    return dispatch_op(d.op, [&](auto op) {
      hipLaunchKernelGGL((k_voxel_bwd_g<LPR, decltype(op)::value>), dim3(link_elk_mid_partial_rows()), dim3(256), 0, st, gS, A, fin,
                         g_out, v4, pos_blk, w_pos, alpha, hdr, d.c, d.cg, d.coord_div, g_fin, partials);
    });
  });
  if (!ok) return LINK_ERR_ARG;
  return check_launch("link_elk_mid_backward");
}
