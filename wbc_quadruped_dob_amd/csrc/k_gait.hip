// Gait scheduler (wbc_gait_batch): a unit of its own, so that no other unit's device code changes.
#include "k_common.hip.hpp"
#include "gait.hip.hpp"

namespace wbc {

template <>
hipError_t k_gait<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const GaitArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (gait_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

}  // namespace wbc
