// The torque-limit post-pass (limit.hip.hpp): the scan of a tick's torques and the on-chip re-solve of the listed states' GRF QPs.
#include "k_common.hip.hpp"
#include "limit.hip.hpp"

namespace wbc {

template <>
hipError_t k_limit_scan<Scalar>(const LaunchCtx& L, const LimitArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (limit_scan_kernel<Scalar>), dim3((unsigned)((a.N + 255) / 256)), dim3(256), a);
  return hipGetLastError();
}

// (grid: limit_qp_grid, launch.hpp)
template <>
hipError_t k_limit_qp<Scalar>(const LaunchCtx& L, const LimitArgs<Scalar>& a, int workgroups) {
  const int per_qp = qpg_lds_scalars(LIMIT_QP_N, LIMIT_QP_M);
  const size_t bytes = (size_t)LIMIT_QP_WPB * per_qp * sizeof(double);
  WBC_KLAUNCH_SMEM(L, (limit_qp_kernel<Scalar>), dim3((unsigned)workgroups), dim3(64 * LIMIT_QP_WPB), bytes, a, per_qp);
  return hipGetLastError();
}

}  // namespace wbc
