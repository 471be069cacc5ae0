// Trunk reference from the velocity command (wbc_reference_cmd_batch, wbc_reference_cmd_swing_batch): a unit of its own, so that no other unit's
// device code changes -- k_misc's and k_swing's reference kernels are the plan-driven forms, untouched.
#include "k_common.hip.hpp"
#include "cmd_ref.hip.hpp"

namespace wbc {

template <>
hipError_t k_reference_cmd<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const DevRefParams<Scalar>* G, const CmdRefArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (cmd_reference_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), model, G, a);
  return hipGetLastError();
}

template <>
hipError_t k_reference_cmd_swing<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const DevRefParams<Scalar>* G, const CmdRefArgs<Scalar>& a,
                                         const SwingArgs<Scalar>& sa) {
  WBC_KLAUNCH(L, (cmd_swing_reference_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), model, G, a, sa);
  return hipGetLastError();
}

}  // namespace wbc
