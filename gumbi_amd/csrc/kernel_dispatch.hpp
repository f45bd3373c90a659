// kernel_dispatch.hpp -- which covariance kinds and which padded widths exist, and the template values they map to.
//
// Every covariance kernel is a template on <KIND, NC>: KIND the kernel kind as 0 .. 4, NC the padded number of continuous
// columns.  with_kind_nc is the one place that turns the run-time pair (kind, nc_pad) into that pair of constants; a launch site
// passes it a generic lambda whose body is the launch (with_kind and with_nc, its two halves, serve the one site that launches
// two kernels per kind).  pick_nc, which makes nc_pad, stands beside the list it has to agree with.
//
// No engine types and no HIP: tools/kernel_dispatch_check.cpp drives this very header with a recording functor.
#pragma once

#include <type_traits>

#include "../../include/gumbi_hip.h"

namespace gmb {

// the padded width of n continuous columns: the least of 1, 2, 4, 8, 16 that holds them (n <= GMB_MAX_DIMS = 16)
inline int pick_nc(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 16; }

// f(integral_constant<int, K>) for the kernel kind; false, and no call, for a kind that is none of the five
template <typename F>
bool with_kind(int kind, F&& f) {
  switch (kind) {
    case GMB_EXPQUAD: f(std::integral_constant<int, 0>{}); return true;
    case GMB_MATERN52: f(std::integral_constant<int, 1>{}); return true;
    case GMB_MATERN32: f(std::integral_constant<int, 2>{}); return true;
    case GMB_MATERN12: f(std::integral_constant<int, 3>{}); return true;
    case GMB_EXPONENTIAL: f(std::integral_constant<int, 4>{}); return true;
  }
  return false;
}

// f(integral_constant<int, NC>) for the width: 1, 2, 4, 8 as themselves, anything else as 16
template <typename F>
void with_nc(int nc_pad, F&& f) {
  switch (nc_pad) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
  }
}

// f(integral_constant<int, K>, integral_constant<int, NC>) for the pair; false, and no call, for an unknown kind
template <typename F>
bool with_kind_nc(int kind, int nc_pad, F&& f) {
  return with_kind(kind, [&](auto k) { with_nc(nc_pad, [&](auto nc) { f(k, nc); }); });
}

}  // namespace gmb
