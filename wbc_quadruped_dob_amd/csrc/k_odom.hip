// Base state from leg odometry (wbc_base_estimate_batch, wbc_gait_estimated_odom_batch): a unit of its own, so that no other unit's device code
// changes -- k_contact's kernels are the forms that read the plant's base rows, untouched.
#include "k_common.hip.hpp"
#include "odom.hip.hpp"

namespace wbc {

template <>
hipError_t k_base_estimate<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const OdomArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (base_estimate_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

template <>
hipError_t k_gait_estimated_odom<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const GaitEstimatedOdomArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (gait_estimated_odom_kernel<Scalar>), dim3((unsigned)((a.e.g.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

}  // namespace wbc
