// fused_tick_kernel launches: the whole tick of a small batch as one launch of wavefront roles (fused_tick.hip.hpp).
#include "k_common.hip.hpp"
#include "fused_tick.hip.hpp"

namespace wbc {

// One instantiation's launch.  Observer off: the kernel's leading arguments (fused_tick.hip.hpp, LEAD) are the first-use fields of the two structs, passed from
// the structs themselves, so both places always hold the same values; observer on: the structs alone.
template <class T, bool OBSERVER, bool MATS, bool WARM>
static void launch_fused_tick(const LaunchCtx& L, const DevModel<T>* model, const DevParams<T>& prm, const SweepArgs<T>& a, const QpArgs<T>& qa, const QpJidx& jmap) {
  const dim3 grid((unsigned)((a.N + 15) / 16)), block((unsigned)fused_threads<T, OBSERVER, MATS, WARM>());
  if constexpr (OBSERVER) {
    WBC_KLAUNCH(L, (fused_tick_kernel<T, true, MATS, WARM>), grid, block, model, prm, a, qa, jmap);
  } else {
    using P = const T*;
    WBC_KLAUNCH(L, (fused_tick_kernel<T, false, MATS, WARM, P, P, size_t, unsigned long long, P, P, const int*, P, P>), grid, block,
                model, a.q, a.v, a.N, a.jpack, a.vdot_des, a.w_des, qa.mask, qa.normals, qa.mu, prm, a, qa, jmap);
  }
}

template <>
hipError_t k_fused_tick<Scalar>(const LaunchCtx& L, bool observer, bool mats, const DevModel<Scalar>* model, const DevParams<Scalar>& prm,
                                const SweepArgs<Scalar>& a, const QpArgs<Scalar>& qa, const QpJidx& jmap, bool warm) {
  using T = Scalar;
  if (qa.N != a.N || qa.jpack != a.jpack) return hipErrorInvalidValue;   // (the kernel takes one N and one jpack for both structs)
  if (warm) {
    if (observer && mats) launch_fused_tick<T, true, true, true>(L, model, prm, a, qa, jmap);
    else if (observer) launch_fused_tick<T, true, false, true>(L, model, prm, a, qa, jmap);
    else if (mats) launch_fused_tick<T, false, true, true>(L, model, prm, a, qa, jmap);
    else launch_fused_tick<T, false, false, true>(L, model, prm, a, qa, jmap);
    return hipGetLastError();
  }
  if (observer && mats) launch_fused_tick<T, true, true, false>(L, model, prm, a, qa, jmap);
  else if (observer) launch_fused_tick<T, true, false, false>(L, model, prm, a, qa, jmap);
  else if (mats) launch_fused_tick<T, false, true, false>(L, model, prm, a, qa, jmap);
  else launch_fused_tick<T, false, false, false>(L, model, prm, a, qa, jmap);
  return hipGetLastError();
}

// fused_pair_kernel: N >= 64, observer off, M / h / Jc wanted, cold
template <>
hipError_t k_fused_pair<Scalar>(const LaunchCtx& L, const DevModel<Scalar>* model, const DevParams<Scalar>& prm, const SweepArgs<Scalar>& a, const QpArgs<Scalar>& qa,
                                const QpJidx& jmap) {
  using T = Scalar;
  if (a.N < 64) return hipErrorInvalidValue;
  WBC_KLAUNCH(L, (fused_pair_kernel<T>), dim3((unsigned)((a.N + 31) / 32)), dim3((unsigned)FUSED_PAIR_THREADS), model, prm, a, qa, jmap);
  return hipGetLastError();
}

}  // namespace wbc
