// Foothold selection (wbc_terrain_cost_batch, wbc_foothold_select_batch, wbc_gait_terrain_select_batch, wbc_gait_estimated_terrain_select_batch): a
// unit of its own, so that no other unit's device code changes -- k_terrain's kernels are the "selection off" forms, untouched.
#include "k_common.hip.hpp"
#include "foothold.hip.hpp"

namespace wbc {

template <>
hipError_t k_terrain_cost<Scalar>(const LaunchCtx& L, const TerrainCostArgs<Scalar>& a, unsigned n_tiles) {
  WBC_KLAUNCH(L, (terrain_cost_kernel<Scalar>), dim3(a.nbx * a.nby * n_tiles), dim3(COST_TX * COST_TY), a);
  return hipGetLastError();
}

template <>
hipError_t k_foothold_select<Scalar>(const LaunchCtx& L, const FootholdSelectArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (foothold_select_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), a);
  return hipGetLastError();
}

template <>
hipError_t k_gait_terrain_select<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const GaitTerrainSelectArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (gait_terrain_select_kernel<Scalar>), dim3((unsigned)((a.g.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

template <>
hipError_t k_gait_estimated_terrain_select<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const GaitEstimatedTerrainSelectArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (gait_estimated_terrain_select_kernel<Scalar>), dim3((unsigned)((a.e.g.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

}  // namespace wbc
