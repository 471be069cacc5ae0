// Shared by every host translation unit of the library, the HIP-free ones (error.cpp, tick_plan.cpp, api_model.cpp) included: the thread-local error
// string, the model handle, the argument checks that touch no device.  What needs the HIP runtime is in solver.hpp.
#pragma once
#include <cmath>
#include <cstddef>
#include <initializer_list>
#include <string>
#include "../../include/wbc_hip.h"
#include "model.hpp"

struct wbc_model { wbc::FlatModel fm; };

namespace wbc {
int fail(int code, const std::string& msg);   // records msg for wbc_last_error(), returns code (error.cpp)
// the argument checks of wbc_step_batch (rollout = true: those of wbc_rollout_batch), without touching the device
int check_step_args(const wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out,
                    const wbc_observer_state* obs, bool rollout);
int check_params_public(const wbc_params* p);   // wbc_solver_set_params' checks, no side effect

// the preamble of the wbc_solver_set_*_params calls: the caller's struct is at least this build's; these fields are finite and >= 0.  `msg` is the
// whole error text (tests read it through wbc_last_error)
template <class P> int check_struct_size(const P* p, const char* msg) { return p->struct_size < sizeof(P) ? fail(WBC_E_INVALID, msg) : WBC_OK; }
inline int check_finite_nonneg(std::initializer_list<double> fields, const char* msg) {
  for (double x : fields)
    if (!(x >= 0) || !std::isfinite(x)) return fail(WBC_E_INVALID, msg);
  return WBC_OK;
}
}
