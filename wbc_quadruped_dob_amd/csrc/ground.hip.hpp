// Ground-contact plant (include/wbc_hip.h at wbc_ground_force_batch): the terrain's reaction force on every foot and the sensed contact bits -- the
// producer of wbc_gait_batch's `contact` input and the last link of the walking tick gait -> reference_swing -> step -> integrate_ground.
// A stateless penalty law, each foot on its own.  The terrain under foot k is the plane n_k . x = d_k (n_k = the foot's rows of `normals`, d_k = its row of
// `height`); with the foot's lever arm and own-leg Jacobian block taken from this tick's Jc exactly as integrate_body phase 1 takes them:
//   p_f = p_b + lever,   v_f = pdot_b + omega x lever + J_leg qdot_leg
//   phi = n . p_f - d    (the gap; negative = penetration)      v_n = n . v_f      v_t = v_f - v_n n
//   f_n = phi < 0 ? max(0, -k_n phi - c_n v_n) : 0
//   g   = -c_t v_t;   f_t = g scaled back onto the cone |f_t| <= mu f_n (mu UNSCALED: mu_scale belongs to the QP's pyramid);  |g| = 0 -> f_t = 0
//   f_gr = f_n n + f_t,   contact bit = f_n > f_touch
// The force acts on EVERY foot whatever the controller's mask says; the commanded f is no input.  Viscous friction has no stiction: a foot under a
// tangential load F creeps at F / c_t (the anchor spring that holds it: stick.hip.hpp, wbc_ground_stick_force_batch).
// Same lane mapping as the gait and integrate kernels (lane = 16*leg + state, one wavefront per workgroup): a lane evaluates its foot and stores its three
// rows of f_gr and its gap; the four lanes of a state combine their bits with one wave64 ballot (gait_gather) and the leg-0 lane stores contact.  Lanes
// beyond the batch recompute its last state and store nothing.
// ground_integrate_kernel: the law, then integrate_body<.., GROUND> with the lane's force in registers -- f_gr is stored for the caller, never read back.
// q, v advance in place: every lane has loaded what the law reads before any lane of its wavefront stores the new state, and a state's four lanes share
// a wavefront.
// Out of scope: the payload plant, the rollout kernels and wbc_rollout_*, wbc_multi_*, late touchdown in the gait rule, terrain-normal footholds.
// (Stiction is stick.hip.hpp's.)
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "dyn_sweep.hip.hpp"
#include "gait.hip.hpp"
#include "integrate.hip.hpp"

namespace wbc {

WBC_DEV double ground_sqrt(double x) { return sqrt(x); }
WBC_DEV float ground_sqrt(float x) { return sqrtf(x); }

// one lane's foot: returns f_gr, leaves the gap in `phi` and the bit in `touch`.  s32 = the state the lane computes, N32 = the batch size.
template <class T>
WBC_DEV V3<T> ground_law(const T* __restrict__ q, const T* __restrict__ v, const T* __restrict__ Jc, const GroundIO<T>& g, unsigned long long jpack,
                         int leg, unsigned s32, unsigned N32, T& phi, bool& touch) {
  const LaneRows A(leg, s32, N32);   // (indices, not words: the loads stay on the __restrict__ pointers)
  int jx[3];
  jidx_of_leg((const DevModel<T>*)nullptr, jpack, leg, jx);
  // the words integrate_body phase 1 loads: the lever arm from the base-angular block -[d]x of my foot's rows, the own-leg Jacobian block
  const V3<T> dl = mk<T>(Jc[A.leg_idx(18 * 1 + 5, 54)], Jc[A.leg_idx(18 * 2 + 3, 54)], Jc[A.leg_idx(18 * 0 + 4, 54)]);
  T jcl[3][3], qd[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int col = 6 + jx[k];
    jcl[0][k] = Jc[A.leg_idx(0 + col, 54)]; jcl[1][k] = Jc[A.leg_idx(18 + col, 54)]; jcl[2][k] = Jc[A.leg_idx(36 + col, 54)];
    qd[k] = v[A.idx(col)];
  }
  const V3<T> pb = mk<T>(q[A.idx(0)], q[A.idx(1)], q[A.idx(2)]);
  const V3<T> vb = mk<T>(v[A.idx(0)], v[A.idx(1)], v[A.idx(2)]), om = mk<T>(v[A.idx(3)], v[A.idx(4)], v[A.idx(5)]);
  const V3<T> n = mk<T>(g.normals[A.leg_idx(0, 3)], g.normals[A.leg_idx(1, 3)], g.normals[A.leg_idx(2, 3)]);
  const T d = g.height[A.leg_idx(0, 1)], mu = g.mu[A.leg_idx(0, 1)];
  const V3<T> pf = pb + dl;
  const V3<T> vf = vb + cross(om, dl) + mk<T>(jcl[0][0] * qd[0] + jcl[0][1] * qd[1] + jcl[0][2] * qd[2],
                                              jcl[1][0] * qd[0] + jcl[1][1] * qd[1] + jcl[1][2] * qd[2],
                                              jcl[2][0] * qd[0] + jcl[2][1] * qd[1] + jcl[2][2] * qd[2]);
  phi = dot(n, pf) - d;
  const T vn = dot(n, vf);
  const V3<T> vt = vf - n * vn;
  const T raw = -g.P.k_n * phi - g.P.c_n * vn;
  const T fn = (phi < (T)0 && raw > (T)0) ? raw : (T)0;
  const V3<T> gt = vt * (-g.P.c_t);
  const T gn = ground_sqrt(dot(gt, gt));
  const T cone = mu * fn;
  const T s = gn > cone ? cone / gn : (T)1;   // (gn > cone >= 0 implies gn > 0: no 0/0; gn = 0 gives s = 1 and f_t = g = 0)
  touch = fn > g.P.f_touch;
  return n * fn + gt * s;
}

// the lane's stores: three rows of f_gr, its gap, and (leg-0 lane) the state's four bits
template <class T>
WBC_DEV void ground_store(const GroundIO<T>& g, int leg, unsigned st, unsigned s32, unsigned N32, bool live, V3<T> f, T phi, bool touch) {
  const size_t N = N32;
  const unsigned long long bc = __ballot(touch);
  if (live) {
    T* const fo = g.f_gr + (size_t)(3 * leg) * N + s32;
    fo[0] = f.x; fo[N] = f.y; fo[2 * N] = f.z;
    if (g.gap) g.gap[(size_t)leg * N + s32] = phi;
    if (leg == 0 && g.contact) g.contact[s32] = gait_gather(bc, st);
  }
}

// the four kernels' lane mapping: lane = 16 * leg + state, one wavefront per workgroup.  Lanes beyond the batch recompute its last state (the state
// integrate_body gives the same lane) and store nothing.
WBC_DEV LegLane foot_lane(size_t N) {
  WBC_LAUNDERED_TID(tx);
  return leg_lane<16>(tx, N);
}

template <class T>
__global__ __launch_bounds__(64) void ground_force_kernel(GroundArgs<T> a) {
  const LegLane l = foot_lane(a.N);
  T phi; bool touch;
  const V3<T> f = ground_law<T>(a.q, a.v, a.Jc, a.g, a.jpack, l.leg, l.s32, (unsigned)a.N, phi, touch);
  ground_store<T>(a.g, l.leg, l.st, l.s32, (unsigned)a.N, l.live, f, phi, touch);
}

template <class T>
__global__ __launch_bounds__(64) void ground_integrate_kernel(const DevModel<T>* __restrict__ model, GroundIntegrateArgs<T> a) {
  const LegLane l = foot_lane(a.N);
  T phi; bool touch;
  const V3<T> f = ground_law<T>(a.q, a.v, a.Jc, a.g, a.jpack, l.leg, l.s32, (unsigned)a.N, phi, touch);
  ground_store<T>(a.g, l.leg, l.st, l.s32, (unsigned)a.N, l.live, f, phi, touch);
  integrate_body<T, 16, IntegrateNoWait, 0, false, false, false, IntegrateNoWait, false, false, false, true>(
      model, a, IntegrateNoWait(), nullptr, nullptr, nullptr, IntegrateNoWait(), nullptr, nullptr, f);
}

}  // namespace wbc
