// The scoring kernels that run beside the rollouts: one tick's cost per state, and the per-group selection (score.hip.hpp).
#include "k_common.hip.hpp"
#include "score.hip.hpp"

namespace wbc {

template <>
hipError_t k_score_tick<Scalar>(const LaunchCtx& L, const ScoreArgs<Scalar>& sc, const Scalar* q, const Scalar* v, const Scalar* tau, const Scalar* f,
                                const int* status, int is_last) {
  WBC_KLAUNCH(L, (score_tick_kernel<Scalar>), dim3((unsigned)((sc.N + 255) / 256)), dim3(256), sc, q, v, tau, f, status, is_last);
  return hipGetLastError();
}

template <>
hipError_t k_rollout_select<Scalar>(hipStream_t st, size_t n_groups, size_t group, const Scalar* cost, Scalar lambda, int* best, Scalar* best_cost,
                                    Scalar* weights) {
  if (group <= 64)
    hipLaunchKernelGGL((rollout_select_kernel<Scalar, 64>), dim3((unsigned)n_groups), dim3(64), 0, st, cost, (unsigned)group, lambda, best, best_cost, weights);
  else
    hipLaunchKernelGGL((rollout_select_kernel<Scalar, 256>), dim3((unsigned)n_groups), dim3(256), 0, st, cost, (unsigned)group, lambda, best, best_cost, weights);
  return hipGetLastError();
}

}  // namespace wbc
