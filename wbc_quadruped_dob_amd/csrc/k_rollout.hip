// rollout_kernel launches: a whole horizon of dependent ticks incl. forward dynamics as one launch (fused_tick.hip.hpp).
// The file compiles once per subset of three flags (csrc/Makefile, ROLLOUT_UNITS), and each compilation defines the ONE rollout_launch<Scalar, TRACK,
// PAYLOAD, SCORE> its flags name:
//   -DWBC_ROLLOUT_TRACK=1    the planner in the loop
//   -DWBC_ROLLOUT_PAYLOAD=1  the plant carries a payload (rollout_kernel<..., PAYLOAD = true>; without the other two flags also integrate_kernel<T, true>)
//   -DWBC_ROLLOUT_SCORE=1    the scored siblings, rollout_scored_kernel<T, OBSERVER, TRACK, SPW, PAYLOAD>, and nothing else -- so that the unscored units
//                            emit exactly the kernels they emitted before the score existed.
#include "k_common.hip.hpp"
#include "fused_tick.hip.hpp"

namespace wbc {

#ifndef WBC_ROLLOUT_TRACK
#define WBC_ROLLOUT_TRACK 0
#endif
#ifndef WBC_ROLLOUT_PAYLOAD
#define WBC_ROLLOUT_PAYLOAD 0
#endif
#ifndef WBC_ROLLOUT_SCORE
#define WBC_ROLLOUT_SCORE 0
#endif
constexpr bool UNIT_TRACK = WBC_ROLLOUT_TRACK != 0, UNIT_PAYLOAD = WBC_ROLLOUT_PAYLOAD != 0, UNIT_SCORE = WBC_ROLLOUT_SCORE != 0;

// the integrator's arguments as the kernels take them: with the payload behind them where the plant carries one
template <bool PAYLOAD> static IntegrateArgsP<Scalar, PAYLOAD> integrate_args(const IntegrateArgs<Scalar>& ia, const Scalar* payload) {
  IntegrateArgsP<Scalar, PAYLOAD> p;
  static_cast<IntegrateArgs<Scalar>&>(p) = ia;
  if constexpr (PAYLOAD) p.payload = payload;
  return p;
}

// one (OBSERVER, SPW) form of a variant: its cold and its warm rollout_kernel, or its (always warm) rollout_scored_kernel
// (4-state workgroups are four wavefronts since round 5: WBC_RO_MERGE, fused_tick.hip.hpp)
template <bool TRACK, bool PAYLOAD, bool SCORE, bool OB, int SPW>
static void launch_form(const LaunchCtx& L, const RolloutLaunch<Scalar>& r, const IntegrateArgsP<Scalar, PAYLOAD>& ia) {
  using T = Scalar;
  const dim3 grid((unsigned)((r.a.N + SPW - 1) / SPW)), block(rollout_threads(OB, SPW));
  if constexpr (SCORE)
    WBC_KLAUNCH(L, (rollout_scored_kernel<T, OB, TRACK, SPW, PAYLOAD>), grid, block, r.model, r.prm, r.a, r.qa, r.jmap, ia, r.horizon, r.G, r.ra, *r.score);
  else if (r.warm)
    WBC_KLAUNCH(L, (rollout_kernel<T, OB, TRACK, SPW, true, PAYLOAD>), grid, block, r.model, r.prm, r.a, r.qa, r.jmap, ia, r.horizon, r.G, r.ra);
  else
    WBC_KLAUNCH(L, (rollout_kernel<T, OB, TRACK, SPW, false, PAYLOAD>), grid, block, r.model, r.prm, r.a, r.qa, r.jmap, ia, r.horizon, r.G, r.ra);
}

template <>
hipError_t rollout_launch<Scalar, UNIT_TRACK, UNIT_PAYLOAD, UNIT_SCORE>(const LaunchCtx& L, const RolloutLaunch<Scalar>& r) {
  const auto ia = integrate_args<UNIT_PAYLOAD>(r.ia, r.payload);
  if (r.spw == 4) {
    if (r.observer) launch_form<UNIT_TRACK, UNIT_PAYLOAD, UNIT_SCORE, true, 4>(L, r, ia);
    else launch_form<UNIT_TRACK, UNIT_PAYLOAD, UNIT_SCORE, false, 4>(L, r, ia);
  } else {
    if (r.observer) launch_form<UNIT_TRACK, UNIT_PAYLOAD, UNIT_SCORE, true, 16>(L, r, ia);
    else launch_form<UNIT_TRACK, UNIT_PAYLOAD, UNIT_SCORE, false, 16>(L, r, ia);
  }
  return hipGetLastError();
}

#if !WBC_ROLLOUT_TRACK && !WBC_ROLLOUT_PAYLOAD && !WBC_ROLLOUT_SCORE
// the family's dispatcher: the variant is what the call carries (a plan, a payload, a score)
template <>
hipError_t k_rollout<Scalar>(const LaunchCtx& L, const RolloutLaunch<Scalar>& r) {
  using T = Scalar;
  using Fn = hipError_t(const LaunchCtx&, const RolloutLaunch<T>&);
  static Fn* const variant[8] = {   // index: TRACK + 2 PAYLOAD + 4 SCORE
      rollout_launch<T, false, false, false>, rollout_launch<T, true, false, false>, rollout_launch<T, false, true, false>, rollout_launch<T, true, true, false>,
      rollout_launch<T, false, false, true>,  rollout_launch<T, true, false, true>,  rollout_launch<T, false, true, true>,  rollout_launch<T, true, true, true>};
  return variant[(r.ra.plan ? 1 : 0) + (r.payload ? 2 : 0) + (r.score ? 4 : 0)](L, r);
}
#endif

#if WBC_ROLLOUT_PAYLOAD && !WBC_ROLLOUT_TRACK && !WBC_ROLLOUT_SCORE
// the per-tick forward dynamics of a plant with a payload (wbc_integrate_plant_batch; the plant rollouts' per-tick launches)
template <>
hipError_t k_integrate_plant<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const IntegrateArgs<Scalar>& a, const Scalar* payload) {
  WBC_KLAUNCH(L, (integrate_kernel<Scalar, true>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), model, integrate_args<true>(a, payload));
  return hipGetLastError();
}
#endif

}  // namespace wbc
