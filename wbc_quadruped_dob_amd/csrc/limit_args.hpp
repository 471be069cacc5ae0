// Plain-data arguments of the torque-limit post-pass (limit.hip.hpp): shared by the kernel unit and the host side.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace wbc {

// the device list of states whose GRF QP is re-solved: list[0] = count (zeroed on the stream in front of the scan), indices from list[LIMIT_LIST_HEAD]
constexpr int LIMIT_LIST_HEAD = 4;
// the limited QP at its largest: four stance feet, 12 forces, 24 friction / normal-force rows + 24 torque rows
constexpr int LIMIT_QP_N = 12, LIMIT_QP_M = 48;
constexpr int LIMIT_QP_WPB = 4;   // wavefronts (= QPs in flight) per workgroup of limit_qp_kernel

template <class T> struct LimitArgs {
  size_t N;
  const T* Jc;        // [216][N] the tick's contact Jacobians: lever arms (base-angular columns) and own-leg blocks (joint columns)
  const T* wdes;      // [6][N]
  const T* rhat;      // [18][N] the observer estimate as the tick left it, or null (observer off: zero)
  const T* normals; const T* mu; const int* mask;
  T* tau; T* f; int* status; int* iters; int* limited;   // the tick's outputs, rewritten in place; iters / limited may be null
  int* list;
  unsigned long long jpack;   // caller's joint index of leg l joint k in nibble 3 l + k (pack_jidx)
  double lim[12];             // tau_max in LEG-MAJOR order (entry 3 l + k), +inf = none
  double S[6], alpha, fn_min, fn_max, mu_scale, tol;   // wbc_params, unrounded: the limited QP runs in fp64 for both scalar types
  int max_iter;
};

}  // namespace wbc
