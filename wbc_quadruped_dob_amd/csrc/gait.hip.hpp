// Gait scheduler: contact masks, footholds and swing plans on the device (include/wbc_hip.h at wbc_gait_batch).  The front of the per-tick loop
// gait -> reference_swing -> step -> integrate: a phase clock per robot, the foot schedule with late lift-off / early touchdown rules, and the
// nine plan words of every lifted foot (p0 latched at lift-off, the Raibert foothold p1, hgt, T, t0) written where wbc_swing_reference_batch reads them.
//   phi' = phi + dphi (wrapped);  phi_k = phi' + offset[k] (wrapped);  sched_k = phi_k < duty[k];  u_k = (phi_k - duty[k]) inv_sw[k]
//   bit_k = sched_k ? 1 : (prev_k ? u_k >= late : (contact_k && u_k >= late))
// Same lane mapping as the swing kernel (lane = 16*leg + state, one wavefront per workgroup): every lane runs the POSITION part of its leg's chain
// (restated from swing_leg_cmd: no velocities, no Jacobian) to get p_f, decides its foot's bit and writes its foot's plan words.  The four lanes of a
// state combine their bits with one wave64 ballot each for mask, lift-off and touchdown; the owner lane (leg 0) stores phase, mask and events.  Every
// lane has loaded phase and mask before that store: the stored values depend on those loads and a workgroup is exactly one wavefront, so the call is
// safe in place.
// Out of scope: the rollout kernels and wbc_rollout_*, wbc_multi_*, late touchdown (the schedule says stance and no contact is sensed), terrain-normal
// footholds, fusing this into com_swing_reference_kernel (its fp64 instantiation sits at 256 VGPRs).
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "dyn_sweep.hip.hpp"

namespace wbc {

// a[leg] of a kernel-argument array without a dynamically indexed copy (that would live in scratch)
template <class T> WBC_DEV T gait_sel(const T (&a)[4], int leg) { return leg == 0 ? a[0] : (leg == 1 ? a[1] : (leg == 2 ? a[2] : a[3])); }

// bits s, 16 + s, 32 + s, 48 + s of a ballot -> the state's four-bit word
WBC_DEV int gait_gather(unsigned long long b, unsigned s) {
  return (int)(((b >> s) & 1ull) | (((b >> (16 + s)) & 1ull) << 1) | (((b >> (32 + s)) & 1ull) << 2) | (((b >> (48 + s)) & 1ull) << 3));
}

template <class T>
__global__ __launch_bounds__(64) void gait_kernel(const DevModel<T>* __restrict__ model, GaitArgs<T> a) {
#define GAIT_SENSED_WORD (a.contact ? a.contact[s32] : 0)
#include "gait_body.inc.hpp"
#undef GAIT_SENSED_WORD
}

}  // namespace wbc
