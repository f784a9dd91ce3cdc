// Runtime value -> compile-time constant: the host side picks a kernel instantiation by
// calling a generic lambda with a std::integral_constant, e.g.
//   return dispatch_nmsg(nmsg, [&](auto NM) {
//     return dispatch_bool(nseg > 1, [&](auto SEG) { return CHOCO_LAUNCH(..., (kernel<NM, SEG>), ...); });
//   });
// The lambda returns a status code.  A value outside the list is CHOCO_ERR_INVALID: nothing
// is launched and nothing reports success.
#pragma once

#include <type_traits>

#include "choco_common.h"

namespace choco {

template <int V>
using int_c = std::integral_constant<int, V>;

template <typename F>
int dispatch_bool(bool v, F&& f) {
  return v ? f(std::true_type{}) : f(std::false_type{});
}

template <int... Vs, typename F>
int dispatch_list(int v, const char* what, F&& f) {
  int rc = CHOCO_OK;
  const bool hit = ((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
  return hit ? rc : fail(CHOCO_ERR_INVALID, "%s = %d has no kernel", what, v);
}

// message counts 1..8 (kMaxMsg, kQMaxMsg)
template <typename F>
int dispatch_nmsg(int nmsg, F&& f) {
  return dispatch_list<1, 2, 3, 4, 5, 6, 7, 8>(nmsg, "nmsg", f);
}

// QSGD container widths in bits
template <typename F>
int dispatch_width(int cw, F&& f) {
  return dispatch_list<1, 2, 4, 8, 16>(cw, "container width", f);
}

}  // namespace choco
