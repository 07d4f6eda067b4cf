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

template <int V, class F>
inline bool dispatch_call(F &f) {
  using arg = std::integral_constant<int, V>;
  if constexpr (std::is_void_v<decltype(f(arg{}))>) { f(arg{}); return true; }
  else return f(arg{});
}

template <int... Vs, class F>
inline bool dispatch_int(int v, F &&f) {
  bool ok = false;
  (void)((v == Vs && ((ok = dispatch_call<Vs>(f)), true)) || ...);
  return ok;
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

}  // namespace link
