// Ground-contact plant (wbc_ground_force_batch, wbc_integrate_ground_batch): a unit of its own, so that no other unit's device code changes.
#include "k_common.hip.hpp"
#include "ground.hip.hpp"

namespace wbc {

template <>
hipError_t k_ground_force<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const GroundArgs<Scalar>& a) {
  (void)model;
  WBC_KLAUNCH(L, (ground_force_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), a);
  return hipGetLastError();
}

template <>
hipError_t k_ground_integrate<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const GroundIntegrateArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (ground_integrate_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

}  // namespace wbc
