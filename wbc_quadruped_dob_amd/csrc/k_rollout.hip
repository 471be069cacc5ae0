// rollout_kernel launches: a whole horizon of dependent ticks incl. forward dynamics as one launch (fused_tick.hip.hpp).
// The planner-in-the-loop instantiations (-DWBC_ROLLOUT_TRACK=1) compile as their own unit, and so do the instantiations whose plant
// carries a payload (-DWBC_ROLLOUT_PAYLOAD=1: rollout_kernel<..., PAYLOAD = true> and integrate_kernel<T, true>).
// -DWBC_ROLLOUT_SCORE=1 (with either, both or none of the two): the scored siblings, rollout_scored_kernel<T, OBSERVER, TRACK, SPW, PAYLOAD>, and nothing else --
// units of their own (k_rollout_sc*), so that the units above emit exactly the kernels they emitted before the score existed.
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
#define WBC_ROLLOUT_ARGS const LaunchCtx& L, bool observer, int spw, const DevModel<Scalar>* model, const DevParams<Scalar>& prm,            \
                         const SweepArgs<Scalar>& a, const QpArgs<Scalar>& qa, const QpJidx& jmap, const IntegrateArgs<Scalar>& ia, int horizon, \
                         const DevRefParams<Scalar>* G, const RefArgs<Scalar>& ra, bool warm
hipError_t rollout_plain(WBC_ROLLOUT_ARGS);
hipError_t rollout_track(WBC_ROLLOUT_ARGS);
hipError_t rollout_plain_payload(WBC_ROLLOUT_ARGS, const Scalar* payload);
hipError_t rollout_track_payload(WBC_ROLLOUT_ARGS, const Scalar* payload);
hipError_t rollout_plain_scored(WBC_ROLLOUT_ARGS, const ScoreArgs<Scalar>& sc);
hipError_t rollout_track_scored(WBC_ROLLOUT_ARGS, const ScoreArgs<Scalar>& sc);
hipError_t rollout_plain_payload_scored(WBC_ROLLOUT_ARGS, const Scalar* payload, const ScoreArgs<Scalar>& sc);
hipError_t rollout_track_payload_scored(WBC_ROLLOUT_ARGS, const Scalar* payload, const ScoreArgs<Scalar>& sc);

// (4-state workgroups are four wavefronts since round 5: WBC_RO_MERGE, fused_tick.hip.hpp)
#define WBC_ROLLOUT_THREADS(OB_, SPW_) rollout_threads(OB_, SPW_)
#if WBC_ROLLOUT_SCORE
#define WBC_ROLLOUT(OB_, SPW_) \
  WBC_KLAUNCH(L, (rollout_scored_kernel<T, OB_, (WBC_ROLLOUT_TRACK != 0), SPW_ WBC_ROLLOUT_PL>), grid, dim3(WBC_ROLLOUT_THREADS(OB_, SPW_)), model, prm, a, qa, jmap, WBC_ROLLOUT_IA, horizon, G, ra, sc)
#define WBC_ROLLOUT_FN(name_) name_##_scored
#define WBC_ROLLOUT_SC , const ScoreArgs<Scalar>& sc
#else
#define WBC_ROLLOUT_FN(name_) name_
#define WBC_ROLLOUT_SC
#define WBC_ROLLOUT(OB_, SPW_) \
  do { if (warm) WBC_KLAUNCH(L, (rollout_kernel<T, OB_, (WBC_ROLLOUT_TRACK != 0), SPW_, true WBC_ROLLOUT_PL>), grid, dim3(WBC_ROLLOUT_THREADS(OB_, SPW_)), model, prm, a, qa, jmap, WBC_ROLLOUT_IA, horizon, G, ra); \
       else WBC_KLAUNCH(L, (rollout_kernel<T, OB_, (WBC_ROLLOUT_TRACK != 0), SPW_, false WBC_ROLLOUT_PL>), grid, dim3(WBC_ROLLOUT_THREADS(OB_, SPW_)), model, prm, a, qa, jmap, WBC_ROLLOUT_IA, horizon, G, ra); } while (0)
#endif

#if WBC_ROLLOUT_PAYLOAD
#define WBC_ROLLOUT_PL , true
#define WBC_ROLLOUT_IA pia
#if WBC_ROLLOUT_TRACK
hipError_t WBC_ROLLOUT_FN(rollout_track_payload)(WBC_ROLLOUT_ARGS, const Scalar* payload WBC_ROLLOUT_SC) {
#else
hipError_t WBC_ROLLOUT_FN(rollout_plain_payload)(WBC_ROLLOUT_ARGS, const Scalar* payload WBC_ROLLOUT_SC) {
#endif
  PlantIntegrateArgs<Scalar> pia;
  static_cast<IntegrateArgs<Scalar>&>(pia) = ia;
  pia.payload = payload;
#else
#define WBC_ROLLOUT_PL
#define WBC_ROLLOUT_IA ia
#if WBC_ROLLOUT_TRACK
hipError_t WBC_ROLLOUT_FN(rollout_track)(WBC_ROLLOUT_ARGS WBC_ROLLOUT_SC) {
#else
hipError_t WBC_ROLLOUT_FN(rollout_plain)(WBC_ROLLOUT_ARGS WBC_ROLLOUT_SC) {
#endif
#endif
  using T = Scalar;
  const dim3 grid((unsigned)((a.N + spw - 1) / spw));
  if (spw == 4) { if (observer) WBC_ROLLOUT(true, 4); else WBC_ROLLOUT(false, 4); }
  else { if (observer) WBC_ROLLOUT(true, 16); else WBC_ROLLOUT(false, 16); }
  return hipGetLastError();
}

#if !WBC_ROLLOUT_TRACK && !WBC_ROLLOUT_PAYLOAD && WBC_ROLLOUT_SCORE
template <>
hipError_t k_rollout_scored<Scalar>(const LaunchCtx& L, bool observer, bool track, int spw, const DevModel<Scalar>* model, const DevParams<Scalar>& prm,
                                    const SweepArgs<Scalar>& a, const QpArgs<Scalar>& qa, const QpJidx& jmap, const IntegrateArgs<Scalar>& ia, int horizon,
                                    const DevRefParams<Scalar>* G, const RefArgs<Scalar>& ra, const Scalar* payload, const ScoreArgs<Scalar>& sc) {
  const bool warm = true;
  if (payload)
    return track ? rollout_track_payload_scored(L, observer, spw, model, prm, a, qa, jmap, ia, horizon, G, ra, warm, payload, sc)
                 : rollout_plain_payload_scored(L, observer, spw, model, prm, a, qa, jmap, ia, horizon, G, ra, warm, payload, sc);
  return track ? rollout_track_scored(L, observer, spw, model, prm, a, qa, jmap, ia, horizon, G, ra, warm, sc)
               : rollout_plain_scored(L, observer, spw, model, prm, a, qa, jmap, ia, horizon, G, ra, warm, sc);
}
#endif

#if !WBC_ROLLOUT_TRACK && !WBC_ROLLOUT_PAYLOAD && !WBC_ROLLOUT_SCORE
template <>
hipError_t k_rollout<Scalar>(const LaunchCtx& L, bool observer, bool track, int spw, const DevModel<Scalar>* model, const DevParams<Scalar>& prm,
                             const SweepArgs<Scalar>& a, const QpArgs<Scalar>& qa, const QpJidx& jmap, const IntegrateArgs<Scalar>& ia, int horizon,
                             const DevRefParams<Scalar>* G, const RefArgs<Scalar>& ra, bool warm, const Scalar* payload) {
  if (payload)
    return track ? rollout_track_payload(L, observer, spw, model, prm, a, qa, jmap, ia, horizon, G, ra, warm, payload)
                 : rollout_plain_payload(L, observer, spw, model, prm, a, qa, jmap, ia, horizon, G, ra, warm, payload);
  return track ? rollout_track(L, observer, spw, model, prm, a, qa, jmap, ia, horizon, G, ra, warm)
               : rollout_plain(L, observer, spw, model, prm, a, qa, jmap, ia, horizon, G, ra, warm);
}
#endif

#if WBC_ROLLOUT_PAYLOAD && !WBC_ROLLOUT_TRACK && !WBC_ROLLOUT_SCORE
// the per-tick forward dynamics of a plant with a payload (wbc_integrate_plant_batch; the plant rollouts' per-tick launches)
template <>
hipError_t k_integrate_plant<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const IntegrateArgs<Scalar>& a, const Scalar* payload) {
  PlantIntegrateArgs<Scalar> pa;
  static_cast<IntegrateArgs<Scalar>&>(pa) = a;
  pa.payload = payload;
  WBC_KLAUNCH(L, (integrate_kernel<Scalar, true>), dim3((unsigned)((a.N + 15) / 16)), dim3(64), model, pa);
  return hipGetLastError();
}
#endif

}  // namespace wbc
