// Run-time value -> template argument.  A launch site is a generic lambda that takes std::integral_constant / std::bool_constant
// tags:  with_block_size(bs_, [&](auto bs) { constexpr int BS = bs; hipLaunchKernelGGL((kernel<BS>), ...); });
// Included from common.h (ArgFailure).
#pragma once
#include <type_traits>

namespace g2ohip {

template <int... Vs, class F>
inline bool dispatch_value(int v, F&& f) {   // f(integral_constant<int, V>) for the V equal to v; false: none is
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
template <class F>
inline void with_block_size(int bs, F&& f) {
  if (!dispatch_value<3, 6, 7>(bs, f)) throw ArgFailure("SparseCholesky: unsupported block size (3, 6, 7)");
}
template <class F>
inline void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
template <int... Gs, class F>
inline void with_lane_group(int G, F&& f) {   // the first listed width >= G, the last one otherwise
  constexpr int gs[] = {Gs...}, last = gs[sizeof...(Gs) - 1];
  (void)((G <= Gs || Gs == last ? (f(std::integral_constant<int, Gs>{}), true) : false) || ...);
}
template <int... Vs, class F>
inline void for_each_value(F&& f) {
  (f(std::integral_constant<int, Vs>{}), ...);
}

}  // namespace g2ohip
