// link_amd/csrc/row_io.h -- feature rows at a kernel boundary in fp32, fp16 or bf16, chosen at compile time (IO = LINK_IO_*).
// The 16-bit rows are widened on load and narrowed on store with round-to-nearest-even; everything in between stays fp32,
// so a kernel instantiated for IO = LINK_IO_F16 / LINK_IO_BF16 gives, bit for bit, what its fp32 instance gives on the rows
// widened to fp32, rounded once into the row type.  Non-finite values stay non-finite (no clamping: a GradScaler upstream
// has to see an overflow).  bf16_rne is shared with the dense-cell kernels (dense_io.h).
#pragma once
#include "common.h"

namespace link {

// fp32 -> bf16 bits, round to nearest even; NaN stays (quiet) NaN, +-inf and overflow to inf as the rounding gives them
__device__ __forceinline__ unsigned bf16_rne(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;      // NaN stays NaN
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

typedef _Float16 rio_h4 __attribute__((ext_vector_type(4)));
typedef unsigned short rio_us4 __attribute__((ext_vector_type(4)));
typedef __bf16 rio_b4 __attribute__((ext_vector_type(4)));

// four consecutive channels starting at element index e (a multiple of 4)
template <int IO>
__device__ __forceinline__ float4 row_ld4(const void *base, int64_t e) {
  static_assert(IO == LINK_IO_F32 || IO == LINK_IO_F16 || IO == LINK_IO_BF16, "row type");
  if constexpr (IO == LINK_IO_F32) {
    return *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(base) + e);
  } else if constexpr (IO == LINK_IO_F16) {
    const rio_h4 h = *reinterpret_cast<const rio_h4 *>(reinterpret_cast<const _Float16 *>(base) + e);
    return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
  } else {
    const rio_us4 u = *reinterpret_cast<const rio_us4 *>(reinterpret_cast<const unsigned short *>(base) + e);
    float4 v = make_float4(__uint_as_float((unsigned)u.x << 16), __uint_as_float((unsigned)u.y << 16),
                           __uint_as_float((unsigned)u.z << 16), __uint_as_float((unsigned)u.w << 16));
    // opaque to the optimiser (as the fp16 conversion is): the arithmetic that follows is scheduled and contracted exactly as in
    // the fp32 instance, whatever the compiler could derive from the zero low half -- the bit-for-bit contract with the fp32 path
    asm("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
    return v;
  }
}

template <int IO>
__device__ __forceinline__ void row_st4(void *base, int64_t e, float4 v) {
  static_assert(IO == LINK_IO_F32 || IO == LINK_IO_F16 || IO == LINK_IO_BF16, "row type");
  if constexpr (IO == LINK_IO_F32) {
    *reinterpret_cast<float4 *>(reinterpret_cast<float *>(base) + e) = v;
  } else if constexpr (IO == LINK_IO_F16) {
    const rio_h4 h = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};     // v_cvt_f16_f32: RNE, overflow -> inf
    *reinterpret_cast<rio_h4 *>(reinterpret_cast<_Float16 *>(base) + e) = h;
  } else {
    // gfx950's v_cvt_pk_bf16_f32 (round to nearest even, NaN kept) -- the same bits as bf16_rne.  Unlike the integer form it
    // leaves the arithmetic before the store as the compiler schedules it for fp32 rows (same contractions: bit-equal results)
    const rio_b4 h = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
    *reinterpret_cast<rio_b4 *>(reinterpret_cast<__bf16 *>(base) + e) = h;
  }
}

// one element of a row, for the kernels that walk a row a scalar at a time
template <int IO>
__device__ __forceinline__ float row_ld1(const void *base, int64_t e) {
  static_assert(IO == LINK_IO_F32 || IO == LINK_IO_F16 || IO == LINK_IO_BF16, "row type");
  if constexpr (IO == LINK_IO_F32) {
    return reinterpret_cast<const float *>(base)[e];
  } else if constexpr (IO == LINK_IO_F16) {
    return (float)reinterpret_cast<const _Float16 *>(base)[e];
  } else {
    return __uint_as_float((unsigned)reinterpret_cast<const unsigned short *>(base)[e] << 16);
  }
}

template <int IO>
__device__ __forceinline__ void row_st1(void *base, int64_t e, float v) {
  static_assert(IO == LINK_IO_F32 || IO == LINK_IO_F16 || IO == LINK_IO_BF16, "row type");
  if constexpr (IO == LINK_IO_F32) {
    reinterpret_cast<float *>(base)[e] = v;
  } else if constexpr (IO == LINK_IO_F16) {
    reinterpret_cast<_Float16 *>(base)[e] = (_Float16)v;
  } else {
    reinterpret_cast<unsigned short *>(base)[e] = (unsigned short)bf16_rne(v);
  }
}

inline bool row_io_ok(int32_t io_dtype) {
  return io_dtype == LINK_IO_F32 || io_dtype == LINK_IO_F16 || io_dtype == LINK_IO_BF16;
}

}  // namespace link
