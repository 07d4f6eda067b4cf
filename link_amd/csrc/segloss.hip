// link_amd/csrc/segloss.hip -- section K of include/link_amd.h: the segmentation criterion of the reference's trainer on the device,
// cross-entropy + Lovasz-softmax (segmentation/core/trainers.py:64-73, core/builder.py:61-72, core/lovasz_losses.py:21-33,174-225)
// in one call, forward and the unit-upstream gradient, with no host read-back, no allocation and no float atomics.
//
// Every table in the workspace is CLASS-MAJOR with leading dimension n (P[c][row], unit[c][row], keys[c][pos], vals[c][pos]): the
// row kernels (one thread per row) then read and write a table coalesced, class by class, and the one uncoalesced step -- the
// scatter of +-g_k from sorted position back to (row, class) -- lands inside one class's n * 4-byte window (400 KB at n = 100 000,
// far below an XCD's 4 MiB L2) instead of touching one 128-byte line of a row-major [n, C] table per element.
//
//   k_rows      softmax of the widened row -> P, the CE partial of the workgroup (fixed-order tree), valid-row count of the
//               workgroup, foreground histogram and CE row count (integer atomics)
//   k_prefix    one workgroup: exclusive prefix of the valid counts (the packed position of every workgroup's first valid row),
//               the CE sum in workgroup order, the number of classes taken
//   k_keys      packed position of each valid row; per class the key 0x3F800000 - bits(error) (ascending key = descending error;
//               errors lie in [0, 1] so their bit patterns order as unsigned integers) and the payload row * 2 + foreground
//   k_hist / k_hist_scan / k_scatter   four 8-bit passes of a stable LSD radix sort over all C segments at once (segment c =
//               [c * n, c * n + n_valid)); ranks inside a tile come from wave ballots in position order, so equal keys keep
//               their row order
//   k_chunk_fg  foreground count of every 2048-element chunk of every sorted segment
//   k_grad      F_k by a block scan on top of the chunk prefix, g_k in closed form, the chunk's part of sum e g (fixed-order
//               tree), the scatter of +-g_k / n_taken into unit[c][row]
//   k_final     out[0..2] = total, CE, Lovasz: per class the chunk parts in chunk order, then the classes in class order
//   k_unit      per row: the softmax Jacobian applied to unit[., row] plus the CE term, in place (probabilities: d/dp as it is)
//   k_backward  grad_rows[row][c] = unit[c][row] * upstream (a device scalar), rounded once into the row type
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>

#include "block_prims.h"
#include "dispatch.h"
#include "radix_pass.h"
#include "row_io.h"

using namespace link;

namespace {

constexpr int T = 256;                    // threads per workgroup (4 waves), every kernel here
constexpr int ITEMS = 8;
constexpr int TILE = T * ITEMS;           // keys per sort tile and per finish chunk
constexpr uint32_t ONE_BITS = 0x3F800000u;
constexpr int HDR_WORDS_K = 64;           // 0 n_valid, 1 n_ce, 2 n_taken, 3 non-finite flag, 4 CE sum (float), 8..39 foreground histogram
enum { H_NV = 0, H_NCE = 1, H_TAKEN = 2, H_BAD = 3, H_CESUM = 4, H_HIST = 8 };

struct Layout {
  int64_t nrb, ntiles;
  size_t hdr, P, keys0, keys1, vals0, vals1, hist, rowcnt, cepart, cf, lpart, total;
};

inline bool shape_ok(int64_t n, int32_t c) {
  // n is bounded before the product is formed: n * c cannot overflow
  return n >= 0 && n < (1LL << 31) && c >= LINK_SEGLOSS_MIN_CLASSES && c <= LINK_SEGLOSS_MAX_CLASSES &&
         n * (int64_t)c < (1LL << 31) - TILE;
}

Layout layout_of(int64_t n, int32_t c) {
  Layout L;
  L.nrb = n > 0 ? (n + T - 1) / T : 1;
  L.ntiles = n > 0 ? (n + TILE - 1) / TILE : 1;
  const size_t nc = (size_t)(n > 0 ? n : 1) * (size_t)c * 4;
  size_t o = 0;
  L.hdr = o; o += up256(HDR_WORDS_K * 4);
  L.P = o; o += up256(nc);
  L.keys0 = o; o += up256(nc);
  L.keys1 = o; o += up256(nc);
  L.vals0 = o; o += up256(nc);
  L.vals1 = o; o += up256(nc);
  L.hist = o; o += up256((size_t)c * 256 * (size_t)L.ntiles * 4);
  L.rowcnt = o; o += up256((size_t)L.nrb * 4);
  L.cepart = o; o += up256((size_t)L.nrb * 4);
  L.cf = o; o += up256((size_t)c * (size_t)L.ntiles * 4);
  L.lpart = o; o += up256((size_t)c * (size_t)L.ntiles * 4);
  L.total = o;
  return L;
}

// ------------------------------------------------------------------------------------------------------------------ row pass
template <int IO>
__global__ void __launch_bounds__(T) k_rows(const void *__restrict__ rows, const int64_t *__restrict__ labels, int64_t n, int c,
                                            int probas, int64_t ce_ignore, int64_t lov_ignore, int use_lov_ignore,
                                            float *__restrict__ P, int *__restrict__ hdr, int *__restrict__ rowcnt,
                                            float *__restrict__ cepart) {
  __shared__ float fl[T];
  __shared__ int il[8];
  __shared__ int lh[LINK_SEGLOSS_MAX_CLASSES];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * T + t;
  const bool in = i < n;
  if (t < LINK_SEGLOSS_MAX_CLASSES) lh[t] = 0;
  __syncthreads();
  int64_t y = -1;
  float ce = 0.f;
  bool valid = false, ce_on = false;
  if (in) {
    y = labels[i];
    const bool in_range = y >= 0 && y < c;
    valid = !use_lov_ignore || y != lov_ignore;
    const int64_t r0 = i * c;
    if (probas) {
      for (int j = 0; j < c; ++j) P[(int64_t)j * n + i] = row_ld1<IO>(rows, r0 + j);
    } else {
      float m = -INFINITY;
      for (int j = 0; j < c; ++j) m = fmaxf(m, row_ld1<IO>(rows, r0 + j));
      float s = 0.f;
      for (int j = 0; j < c; ++j) s += expf(row_ld1<IO>(rows, r0 + j) - m);
      const float inv = 1.0f / s;
      for (int j = 0; j < c; ++j) P[(int64_t)j * n + i] = expf(row_ld1<IO>(rows, r0 + j) - m) * inv;
      ce_on = in_range && y != ce_ignore;
      if (ce_on) ce = logf(s) - (row_ld1<IO>(rows, r0 + y) - m);
    }
    if (valid && in_range) atomicAdd(&lh[(int)y], 1);
  }
  const float ce_blk = block_sum_fixed(ce, fl);
  int nvalid, nce;
  block_scan_excl(valid ? 1 : 0, il, nvalid);
  block_scan_excl(ce_on ? 1 : 0, il, nce);
  if (t == 0) {
    rowcnt[blockIdx.x] = nvalid;
    cepart[blockIdx.x] = ce_blk;
    if (nce) atomicAdd(&hdr[H_NCE], nce);
  }
  if (t < c && lh[t]) atomicAdd(&hdr[H_HIST + t], lh[t]);
}

__global__ void __launch_bounds__(T) k_prefix(int *__restrict__ hdr, int *__restrict__ rowcnt, const float *__restrict__ cepart,
                                              int64_t nrb, int c, int classes_all) {
  __shared__ float fl[T];
  __shared__ int il[8];
  const int t = threadIdx.x;
  int carry = 0;
  float ce = 0.f;
  for (int64_t b0 = 0; b0 < nrb; b0 += T) {
    const int64_t b = b0 + t;
    const int v = b < nrb ? rowcnt[b] : 0;
    int tot;
    const int ex = block_scan_excl(v, il, tot);
    if (b < nrb) rowcnt[b] = carry + ex;
    carry += tot;
    ce += block_sum_fixed(b < nrb ? cepart[b] : 0.f, fl);
  }
  if (t == 0) {
    hdr[H_NV] = carry;
    reinterpret_cast<float *>(hdr)[H_CESUM] = ce;
    int taken = 0;
    if (carry > 0) {
      if (classes_all) taken = c;
      else
        for (int j = 0; j < c; ++j) taken += hdr[H_HIST + j] > 0;
    }
    hdr[H_TAKEN] = taken;
  }
}

__global__ void __launch_bounds__(T) k_keys(const int64_t *__restrict__ labels, int64_t n, int c, int64_t lov_ignore, int use_lov_ignore,
                                            const float *__restrict__ P, int *__restrict__ hdr, const int *__restrict__ rowoff,
                                            uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  __shared__ int il[8];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * T + t;
  int64_t y = -1;
  bool valid = false;
  if (i < n) {
    y = labels[i];
    valid = !use_lov_ignore || y != lov_ignore;
  }
  int tot;
  const int rank = block_scan_excl(valid ? 1 : 0, il, tot);
  if (!valid) return;
  const int64_t pos = (int64_t)rowoff[blockIdx.x] + rank;      // < n_valid <= n
  bool bad = false;
  for (int j = 0; j < c; ++j) {
    const float p = P[(int64_t)j * n + i];
    const bool fg = y == j;
    const float e = fabsf((fg ? 1.0f : 0.0f) - p);
    bad |= !(e < INFINITY);                                      // NaN or inf: the total must come out non-finite
    uint32_t bits = __float_as_uint(e);
    bits = bits > ONE_BITS ? ONE_BITS : bits;                    // the key never leaves 30 bits, whatever the input holds
    keys[(int64_t)j * n + pos] = ONE_BITS - bits;
    vals[(int64_t)j * n + pos] = ((uint32_t)i << 1) | (fg ? 1u : 0u);
  }
  if (bad) atomicOr(&hdr[H_BAD], 1);
}

// ---------------------------------------------------------------------------------------------------------------- radix sort
// One pass of radix_pass.h over all C segments at once: grid (ntiles, C) for the tiles, grid C for the scan.  Segment c of the keys and
// values starts at c * n and holds n_valid pairs; its histogram words are hist[(c * ntiles + tile) * 256 + digit].
static_assert(T == RADIX_T && TILE == RADIX_TILE, "the sort tile is the finish chunk");

__global__ void __launch_bounds__(T) k_hist(const uint32_t *__restrict__ keys, int64_t n, int64_t ntiles, const int *__restrict__ hdr,
                                            int shift, uint32_t *__restrict__ hist) {
  const int cls = blockIdx.y;
  const int64_t tile = blockIdx.x;
  radix_tile_hist(keys + (int64_t)cls * n, (int64_t)hdr[H_NV], tile, shift, hist + ((int64_t)cls * ntiles + tile) * 256);
}

__global__ void __launch_bounds__(T) k_hist_scan(uint32_t *__restrict__ hist, int64_t ntiles) {
  radix_digit_scan(hist + (int64_t)blockIdx.x * ntiles * 256, ntiles);
}

__global__ void __launch_bounds__(T) k_scatter(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, int64_t n,
                                               int64_t ntiles, const int *__restrict__ hdr, int shift, const uint32_t *__restrict__ hist,
                                               uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out) {
  const int cls = blockIdx.y;
  const int64_t tile = blockIdx.x;
  const int64_t nv = hdr[H_NV];
  if (tile * TILE >= nv) return;                                 // uniform over the workgroup
  const int64_t seg = (int64_t)cls * n;
  radix_tile_scatter(keys + seg, vals + seg, nv, tile, shift, hist + ((int64_t)cls * ntiles + tile) * 256, keys_out + seg, vals_out + seg);
}

// ------------------------------------------------------------------------------------------------------------------- finish
__global__ void __launch_bounds__(T) k_chunk_fg(const uint32_t *__restrict__ vals, int64_t n, int64_t nchunks, const int *__restrict__ hdr,
                                                int *__restrict__ cf) {
  __shared__ int il[8];
  const int t = threadIdx.x, cls = blockIdx.y;
  const int64_t nv = hdr[H_NV];
  const int64_t p0 = (int64_t)blockIdx.x * TILE;
  const uint32_t *v = vals + (int64_t)cls * n;
  int f = 0;
#pragma unroll
  for (int r = 0; r < ITEMS; ++r) {
    const int64_t p = p0 + r * T + t;
    if (p < nv) f += (int)(v[p] & 1u);
  }
  int tot;
  block_scan_excl(f, il, tot);
  if (t == 0) cf[(int64_t)cls * nchunks + blockIdx.x] = tot;
}

__global__ void __launch_bounds__(T) k_grad(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, int64_t n,
                                            int64_t nchunks, const int *__restrict__ hdr, const int *__restrict__ cf, int classes_all,
                                            float *__restrict__ unit, float *__restrict__ lpart) {
  __shared__ float fl[T];
  __shared__ int il[8];
  const int t = threadIdx.x, cls = blockIdx.y;
  const int64_t chunk = blockIdx.x;
  const int64_t nv = hdr[H_NV];
  const int nc = hdr[H_HIST + cls];
  const int ntaken = hdr[H_TAKEN];
  const bool taken = nv > 0 && (classes_all || nc > 0);
  const float inv_taken = ntaken > 0 ? 1.0f / (float)ntaken : 0.f;
  const int64_t seg = (int64_t)cls * n;
  // foreground elements in front of this chunk
  int pre = 0;
  for (int64_t j = t; j < chunk; j += T) pre += cf[(int64_t)cls * nchunks + j];
  int before;
  block_scan_excl(pre, il, before);
  // eight consecutive positions per thread
  const int64_t q0 = chunk * TILE + (int64_t)t * ITEMS;
  uint32_t kk[ITEMS], vv[ITEMS];
  int f = 0;
#pragma unroll
  for (int r = 0; r < ITEMS; ++r) {
    const int64_t p = q0 + r;
    kk[r] = 0; vv[r] = 0;
    if (p < nv) {
      kk[r] = keys[seg + p];
      vv[r] = vals[seg + p];
      f += (int)(vv[r] & 1u);
    }
  }
  int tot;
  int F = before + block_scan_excl(f, il, tot);                  // foreground strictly before q0
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < ITEMS; ++r) {
    const int64_t p = q0 + r;
    if (p < nv) {
      const bool fg = vv[r] & 1u;
      F += fg ? 1 : 0;
      const int64_t k = p + 1;                                   // 1-based position
      const int64_t U = (int64_t)nc + (k - F);                   // n_c + B_k
      float g;
      if (fg) {
        g = 1.0f / (float)U;
      } else {
        const int64_t Up = U - 1;
        g = Up == 0 ? 1.0f : (float)(nc - F) / ((float)Up * (float)U);
      }
      const float e = __uint_as_float(ONE_BITS - kk[r]);
      float d = 0.f;
      if (taken) {
        acc += e * g;
        d = e == 0.f ? 0.f : (fg ? -g : g) * inv_taken;
      }
      const uint32_t row = vv[r] >> 1;
      if ((int64_t)row < n) unit[seg + row] = d;
    }
  }
  const float part = block_sum_fixed(acc, fl);
  if (t == 0) lpart[(int64_t)cls * nchunks + chunk] = part;
}

__global__ void __launch_bounds__(64) k_final(const int *__restrict__ hdr, const float *__restrict__ lpart, int64_t nchunks, int c,
                                              int probas, float *__restrict__ out) {
  __shared__ float cl[LINK_SEGLOSS_MAX_CLASSES];
  const int t = threadIdx.x;
  const int64_t nv = hdr[H_NV];
  const int64_t used = (nv + TILE - 1) / TILE;                   // chunks that k_grad filled with this call's data
  if (t < c) {
    float s = 0.f;
    for (int64_t j = 0; j < used; ++j) s += lpart[(int64_t)t * nchunks + j];
    cl[t] = s;
  }
  __syncthreads();
  if (t == 0) {
    float lov = 0.f;
    const int ntaken = hdr[H_TAKEN];
    if (ntaken > 0) {
      for (int j = 0; j < c; ++j) lov += cl[j];
      lov /= (float)ntaken;
    }
    if (hdr[H_BAD]) lov = NAN;
    const float ce = probas ? 0.f : reinterpret_cast<const float *>(hdr)[H_CESUM] / (float)hdr[H_NCE];    // 0 / 0 = NaN, as torch
    out[0] = ce + lov;
    out[1] = ce;
    out[2] = lov;
  }
}

__global__ void __launch_bounds__(T) k_unit(const int64_t *__restrict__ labels, int64_t n, int c, int probas, int64_t ce_ignore,
                                            int64_t lov_ignore, int use_lov_ignore, const float *__restrict__ P,
                                            const int *__restrict__ hdr, float *__restrict__ unit) {
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  if (i >= n) return;
  const int64_t y = labels[i];
  const bool valid = !use_lov_ignore || y != lov_ignore;
  if (probas) {
    if (!valid)
      for (int j = 0; j < c; ++j) unit[(int64_t)j * n + i] = 0.f;
    return;
  }
  const bool ce_on = y >= 0 && y < c && y != ce_ignore;
  const float inv_ce = ce_on ? 1.0f / (float)hdr[H_NCE] : 0.f;
  float dot = 0.f;
  if (valid)
    for (int j = 0; j < c; ++j) dot += unit[(int64_t)j * n + i] * P[(int64_t)j * n + i];
  for (int j = 0; j < c; ++j) {
    const float p = P[(int64_t)j * n + i];
    const float g = valid ? unit[(int64_t)j * n + i] : 0.f;
    float u = p * (g - dot);
    if (ce_on) u += (p - (y == j ? 1.0f : 0.0f)) * inv_ce;
    unit[(int64_t)j * n + i] = u;
  }
}

template <int IO>
__global__ void __launch_bounds__(T) k_backward(const float *__restrict__ unit, const float *__restrict__ upstream, int64_t n, int c,
                                                void *__restrict__ grad_rows) {
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  if (i >= n) return;
  const float s = upstream[0];
  for (int j = 0; j < c; ++j) row_st1<IO>(grad_rows, i * c + j, unit[(int64_t)j * n + i] * s);
}

}  // namespace

// ----------------------------------------------------------------------------------------------------------------- C entries
extern "C" size_t link_segloss_workspace_bytes(int64_t n, int32_t c) {
  if (!shape_ok(n, c)) return 0;
  return layout_of(n, c).total;
}

extern "C" int link_segloss_forward(const void *rows, int32_t io_dtype, int32_t input_kind, const int64_t *labels, int64_t n, int32_t c,
                                    int64_t ce_ignore, int64_t lov_ignore, int32_t use_lov_ignore, int32_t classes, void *workspace,
                                    size_t workspace_bytes, float *out, float *unit_grad, void *stream) {
  if (!rows || !labels || !workspace || !out || !unit_grad || !shape_ok(n, c) || !row_io_ok(io_dtype) ||
      (input_kind != LINK_SEGLOSS_LOGITS && input_kind != LINK_SEGLOSS_PROBAS) ||
      (classes != LINK_SEGLOSS_PRESENT && classes != LINK_SEGLOSS_ALL))
    return LINK_ERR_ARG;
  const Layout L = layout_of(n, c);
  if (workspace_bytes < L.total) return LINK_ERR_WORKSPACE;
  char *ws = reinterpret_cast<char *>(workspace);
  int *hdr = reinterpret_cast<int *>(ws + L.hdr);
  float *P = reinterpret_cast<float *>(ws + L.P);
  uint32_t *keys[2] = {reinterpret_cast<uint32_t *>(ws + L.keys0), reinterpret_cast<uint32_t *>(ws + L.keys1)};
  uint32_t *vals[2] = {reinterpret_cast<uint32_t *>(ws + L.vals0), reinterpret_cast<uint32_t *>(ws + L.vals1)};
  uint32_t *hist = reinterpret_cast<uint32_t *>(ws + L.hist);
  int *rowcnt = reinterpret_cast<int *>(ws + L.rowcnt);
  float *cepart = reinterpret_cast<float *>(ws + L.cepart);
  int *cf = reinterpret_cast<int *>(ws + L.cf);
  float *lpart = reinterpret_cast<float *>(ws + L.lpart);
  hipStream_t s = S(stream);
  const int probas = input_kind == LINK_SEGLOSS_PROBAS, all = classes == LINK_SEGLOSS_ALL, use_ign = use_lov_ignore != 0;
  const dim3 rb((unsigned)L.nrb), tb((unsigned)L.ntiles, (unsigned)c);

  const hipError_t me = hipMemsetAsync(hdr, 0, HDR_WORDS_K * 4, s);
  if (me != hipSuccess) {
    set_error("link_segloss_forward: memset", me);
    return LINK_ERR_LAUNCH;
  }
  dispatch_row_io(io_dtype, [&](auto io) {
    hipLaunchKernelGGL(k_rows<decltype(io)::value>, rb, dim3(T), 0, s, rows, labels, n, (int)c, probas, ce_ignore, lov_ignore, use_ign, P,
                       hdr, rowcnt, cepart);
  });
  hipLaunchKernelGGL(k_prefix, dim3(1), dim3(T), 0, s, hdr, rowcnt, cepart, L.nrb, (int)c, all);
  hipLaunchKernelGGL(k_keys, rb, dim3(T), 0, s, labels, n, (int)c, lov_ignore, use_ign, P, hdr, rowcnt, keys[0], vals[0]);
  for (int pass = 0; pass < 4; ++pass) {
    const int a = pass & 1, b = a ^ 1;
    hipLaunchKernelGGL(k_hist, tb, dim3(T), 0, s, keys[a], n, L.ntiles, hdr, pass * 8, hist);
    hipLaunchKernelGGL(k_hist_scan, dim3((unsigned)c), dim3(T), 0, s, hist, L.ntiles);
    hipLaunchKernelGGL(k_scatter, tb, dim3(T), 0, s, keys[a], vals[a], n, L.ntiles, hdr, pass * 8, hist, keys[b], vals[b]);
  }
  // four passes: the sorted segments are back in buffer 0
  hipLaunchKernelGGL(k_chunk_fg, tb, dim3(T), 0, s, vals[0], n, L.ntiles, hdr, cf);
  hipLaunchKernelGGL(k_grad, tb, dim3(T), 0, s, keys[0], vals[0], n, L.ntiles, hdr, cf, all, unit_grad, lpart);
  hipLaunchKernelGGL(k_final, dim3(1), dim3(64), 0, s, hdr, lpart, L.ntiles, (int)c, probas, out);
  hipLaunchKernelGGL(k_unit, rb, dim3(T), 0, s, labels, n, (int)c, probas, ce_ignore, lov_ignore, use_ign, P, hdr, unit_grad);
  return check_launch("link_segloss_forward");
}

extern "C" int link_segloss_backward(const float *unit_grad, const float *upstream, int64_t n, int32_t c, int32_t io_dtype,
                                     void *grad_rows, void *stream) {
  if (!unit_grad || !upstream || !grad_rows || !shape_ok(n, c) || !row_io_ok(io_dtype)) return LINK_ERR_ARG;
  const dim3 rb((unsigned)(n > 0 ? (n + T - 1) / T : 1));
  hipStream_t s = S(stream);
  dispatch_row_io(io_dtype, [&](auto io) {
    hipLaunchKernelGGL(k_backward<decltype(io)::value>, rb, dim3(T), 0, s, unit_grad, upstream, n, (int)c, grad_rows);
  });
  return check_launch("link_segloss_backward");
}
