// Stiction on the ground plant (wbc_ground_stick_force_batch, wbc_integrate_ground_stick_batch): a unit of its own, so that no other unit's device
// code changes.
#include "k_common.hip.hpp"
#include "stick.hip.hpp"

namespace wbc {

template <>
hipError_t k_stick_force<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const StickArgs<Scalar>& a) {
  (void)model;
  WBC_KLAUNCH(L, (stick_force_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), a);
  return hipGetLastError();
}

template <>
hipError_t k_stick_integrate<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const StickIntegrateArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (stick_integrate_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

}  // namespace wbc
