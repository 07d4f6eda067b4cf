// link_amd/csrc/dispatch.h -- run-time int -> template argument: one helper, and one wrapper per template axis (host only).
//
//   if (!dispatch_lpr(c, [&](auto lpr) { launch<decltype(lpr)::value>(...); })) return LINK_ERR_ARG;
//
// The generic lambda is called with std::integral_constant<int, V> for the V of the axis' list that the run-time value
// selects.  A value outside the list calls nothing and gives false -- there is no default that guesses.  A lambda that
// returns bool (a nested dispatch) is passed through, so the axes compose.
#pragma once
#include <type_traits>

#include "common.h"

namespace link {

template <auto V, class F>
inline bool dispatch_call(F &f) {
  using arg = std::integral_constant<decltype(V), V>;
  if constexpr (std::is_void_v<decltype(f(arg{}))>) { f(arg{}); return true; }
  else return f(arg{});
}

template <int... Vs, class F>
inline bool dispatch_int(int v, F &&f) {
  bool ok = false;
  (void)((v == Vs && ((ok = dispatch_call<Vs>(f)), true)) || ...);
  return ok;
}

// a two-valued template argument: the lambda gets std::bool_constant
template <class F>
inline bool dispatch_bool(bool b, F &&f) { return b ? dispatch_call<true>(f) : dispatch_call<false>(f); }

// two of them: the lambda gets (a, b)
template <class F>
inline bool dispatch_bool2(bool a, bool b, F &&f) {
  return dispatch_bool(a, [&](auto ta) { return dispatch_bool(b, [&](auto tb) { return f(ta, tb); }); });
}

// lanes per feature row of the group kernels, 4 channels (16 B) a lane: pow2ceil(c / 4), at least 4 (narrower rows idle
// lanes).  Every caller has checked 0 < c <= 256, so the result is at most 64; a wider row is refused, not run as 64.
template <class F>
inline bool dispatch_lpr(int c, F &&f) {
  int need = (c + 3) / 4, l = 4;
  while (l < need) l <<= 1;
  return dispatch_int<4, 8, 16, 32, 64>(l, f);
}

// row width of the MFMA pre_mix kernels
template <class F>
inline bool dispatch_width(int c, F &&f) { return dispatch_int<16, 32, 48, 64, 80, 96, 112, 128>(c, f); }

// channels per lane of the lane = channel fallback kernels (0 < c <= 256 checked by the callers: 1..4 is the whole range)
template <class F>
inline bool dispatch_cpl(int c, F &&f) { return dispatch_int<1, 2, 3, 4>((c + 63) / 64, f); }

template <class F>
inline bool dispatch_op(int op, F &&f) { return dispatch_int<LINK_OP_COS, LINK_OP_SIN, LINK_OP_COSX>(op, f); }

// neighbourhood radius of the group kernels (callers have checked 0 < r <= 3)
template <class F>
inline bool dispatch_radius(int r, F &&f) { return dispatch_int<1, 2, 3>(r, f); }

// row type at a kernel boundary (row_io.h)
template <class F>
inline bool dispatch_row_io(int io_dtype, F &&f) { return dispatch_int<LINK_IO_F32, LINK_IO_F16, LINK_IO_BF16>(io_dtype, f); }

// ---- (cin, cout) width pairs of the sparse convolution ----
// A pair travels through dispatch_int as cin * 256 + cout; the lambda is called with two integral constants, (cin, cout).
// Each kernel family's list stands here once: its "supported" predicate is a dispatch with an empty lambda.
constexpr int wp(int cin, int cout) { return cin * 256 + cout; }

template <int... Ps, class F>
inline bool dispatch_pair(int cin, int cout, F &&f) {
  if (cin <= 0 || cin >= 256 || cout <= 0 || cout >= 256) return false;     // outside the packing's range
  return dispatch_int<Ps...>(wp(cin, cout), [&](auto p) {
    constexpr int P = decltype(p)::value;
    return f(std::integral_constant<int, P / 256>{}, std::integral_constant<int, P % 256>{});
  });
}

// pair-list form (conv_pairs.hip): gemm, centre-sum and weight-gradient kernels
template <class F>
inline bool dispatch_conv_pairs(int cin, int cout, F &&f) {
  return dispatch_pair<wp(16, 16), wp(32, 32), wp(64, 64), wp(128, 128), wp(16, 32), wp(32, 16), wp(32, 64), wp(64, 32),
                       wp(64, 128), wp(128, 64), wp(16, 64), wp(64, 16)>(cin, cout, f);
}

// table form (conv.hip, k_subm_conv_mfma): the square widths, then the channel changes of the reference encoders
// (cs = [32,32,64,128,256,256,128,96,96] x cr, linkunet.py:262)
template <class F>
inline bool dispatch_conv_table(int cin, int cout, F &&f) {
  return dispatch_pair<wp(16, 16), wp(32, 32), wp(48, 48), wp(64, 64), wp(80, 80), wp(96, 96), wp(112, 112), wp(128, 128),
                       wp(16, 32), wp(32, 16), wp(32, 64), wp(64, 32), wp(64, 128), wp(128, 64), wp(96, 128), wp(128, 96),
                       wp(64, 96), wp(96, 64), wp(32, 96), wp(96, 32), wp(16, 64), wp(64, 16), wp(32, 128), wp(128, 32)>(
      cin, cout, f);
}

// resident-weights kernels (conv.hip): every W_k of the layer fits in LDS
template <class F>
inline bool dispatch_conv_resident(int cin, int cout, F &&f) {
  return dispatch_pair<wp(16, 16), wp(32, 32), wp(16, 32), wp(32, 16)>(cin, cout, f);
}

}  // namespace link
