// Swing-foot references: the stand-alone kernel (wbc_swing_reference_batch) and the CoM reference generator with the swing law fused in
// (wbc_reference_swing_batch).
#include "k_common.hip.hpp"
#include "swing_ref.hip.hpp"

namespace wbc {

template <>
hipError_t k_swing_reference<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const SwingRefArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (swing_reference_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

template <>
hipError_t k_reference_swing<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const DevRefParams<Scalar>* G, const RefArgs<Scalar>& a,
                                     const SwingArgs<Scalar>& sa) {
  WBC_KLAUNCH(L, (com_swing_reference_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), model, G, a, sa);
  return hipGetLastError();
}

}  // namespace wbc
