// Contact sensing from the observer's residual (wbc_contact_estimate_batch, wbc_gait_estimated_batch): a unit of its own, so that no other unit's
// device code changes.
#include "k_common.hip.hpp"
#include "contact_est.hip.hpp"

namespace wbc {

template <>
hipError_t k_contact_estimate<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const ContactArgs<Scalar>& a) {
  (void)model;
  WBC_KLAUNCH(L, (contact_estimate_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), a);
  return hipGetLastError();
}

template <>
hipError_t k_gait_estimated<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const GaitEstimatedArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (gait_estimated_kernel<Scalar>), dim3((unsigned)((a.g.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

}  // namespace wbc
