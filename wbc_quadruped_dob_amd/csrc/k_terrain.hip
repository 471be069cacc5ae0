// Terrain heightfield (wbc_terrain_sample_batch, wbc_terrain_feet_batch, wbc_gait_terrain_batch, wbc_gait_estimated_terrain_batch): a unit of its own,
// so that no other unit's device code changes.
#include "k_common.hip.hpp"
#include "terrain.hip.hpp"

namespace wbc {

template <>
hipError_t k_terrain_sample<Scalar>(const LaunchCtx& L, const TerrainSampleArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (terrain_sample_kernel<Scalar>), dim3((unsigned)((a.M + 63) / 64)), dim3(64), a);
  return hipGetLastError();
}

template <>
hipError_t k_terrain_feet<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const TerrainFeetArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (terrain_feet_kernel<Scalar>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

template <>
hipError_t k_gait_terrain<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const GaitTerrainArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (gait_terrain_kernel<Scalar>), dim3((unsigned)((a.g.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

template <>
hipError_t k_gait_estimated_terrain<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const GaitEstimatedTerrainArgs<Scalar>& a) {
  WBC_KLAUNCH(L, (gait_estimated_terrain_kernel<Scalar>), dim3((unsigned)((a.e.g.N + 15) / 16)), dim3(64), model, a);
  return hipGetLastError();
}

}  // namespace wbc
