// Base state from leg odometry (include/wbc_hip.h at wbc_base_estimate_batch): the trunk's world position and linear velocity estimated from the joint
// encoders, the attitude, the gyro and the contact word -- the controller-side producer of rows 0-2 of q and v, which every launch of the walking tick
// otherwise takes from the plant.  A loaded stance foot does not move: it measures the trunk's velocity through its leg's Jacobian and the trunk's
// position through its leg's forward kinematics from the point it stands on.  Per foot k, from the chain and velocity recursion swing_leg_cmd runs
// (d and vf with zero base linear velocity, om0 = R^T omega):
//   lever_k = R d_k            u_k = R vf_k            S_k = contact bit k && mask bit k           cnt = |S|           inv[c] = 1 / c
//   cnt > 0:   vm = -((u_0 + u_1) + (u_2 + u_3)) inv[cnt]  (untrusted terms exactly 0),   v^ += a_v (vm - v^)
//   p_pred = p^ + dt v^;   A = S && odo's in-bits;   A != {}:  pm = ((x_0 + x_1) + (x_2 + x_3)) inv[|A|],  x_k = anchor_k - lever_k,
//   p^ = p_pred + a_p (pm - p_pred);   A == {}:  p^ = p_pred
//   k in S \ A:  x = p^ + lever_k;  planes given: x -= n_k (n_k . x - height_k);  anchor_k = x, bit k = 1, bit 4+k = 1.   k not in S: bit k = 0
// Same lane mapping as the gait and contact kernels (lane = 16*leg + state, one wavefront per workgroup, the constant table in LDS): a lane runs its
// leg's chain once and has lever and u.  The four lanes of a state sum across the rows of 16 with a two-step butterfly (xor 16, then xor 32): with the
// summation order above every lane ends with the same bits, so all four hold p^ and v^ in registers -- gait_estimated_odom_kernel runs the gait
// scheduler's body on them and no value goes to memory and back inside the launch.  The words S, A and the new odo word need no cross-lane step: every
// lane loads the state's contact, mask and odo words whole.  The leg-0 lane stores base, odo and rows 0-2 of the estimates; a lane stores its own
// foot's anchor; the copy rows (3 .. of q_est and v_est, unless the outputs are the inputs) are dealt over the four lanes.  Lanes beyond the batch
// recompute its last state and store nothing.  In place: every lane has loaded base, odo and its anchor before the stores that depend on them, and a
// state's four lanes share a wavefront.
// Out of scope: an accelerometer or a Kalman covariance, attitude estimation, compensating the penetration bias from f_est, the terrain and
// foothold-select fused variants, the rollout kernels and wbc_rollout_*, wbc_multi_*.
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "dyn_sweep.hip.hpp"
#include "contact_est.hip.hpp"

namespace wbc {

constexpr int ODOM_NQ = 19, ODOM_NV = 18;   // the rows of q and v (a floating base and twelve joints, as everywhere in the walking tick)

// x summed over the four lanes of a state, as (x_0 + x_1) + (x_2 + x_3): the same bits in all four (addition commutes)
template <class T> WBC_DEV T odom_sum4(T x) {
  x = x + __shfl_xor(x, 16, 64);
  return x + __shfl_xor(x, 32, 64);
}
template <class T> WBC_DEV V3<T> odom_sum4(V3<T> x) { return mk<T>(odom_sum4(x.x), odom_sum4(x.y), odom_sum4(x.z)); }
// 1 / c for c = 0 .. 4 (0 for c = 0: nobody reads it), the quotients rounded at compile time
template <class T> WBC_DEV T odom_inv(int c) { return c == 1 ? (T)1 : (c == 2 ? (T)0.5 : (c == 3 ? (T)1 / (T)3 : (c == 4 ? (T)0.25 : (T)0))); }

// One lane's share of the law.  cst: the constant table (LDS); q, v: the sensor state (rows 0-2 are not read); cw, mw: the state's contact and mask
// words as loaded.  Leaves p^ and v^ (the new ones) in ph, vh in every lane and has stored everything the law stores.
template <class T>
WBC_DEV void odom_law(const OdomIO<T>& o, const T* cst, const T* q, const T* v, unsigned long long jpack, int leg, unsigned s32, size_t N, bool live,
                      int cw, int mw, T (&ph)[3], T (&vh)[3]) {
  const unsigned N32 = (unsigned)N;
  T qa[4], om[3];
#pragma unroll
  for (int c = 0; c < 4; ++c) qa[c] = ROWI(q, 3 + c);
#pragma unroll
  for (int c = 0; c < 3; ++c) om[c] = ROWI(v, 3 + c);
  int jx[3];
  jidx_of_leg((const DevModel<T>*)nullptr, jpack, leg, jx);
  T ql[3], vl[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { ql[k] = ROWI(q, 7 + jx[k]); vl[k] = ROWI(v, 6 + jx[k]); }
  const int in = o.odo[s32] & 15;
  T pin[3], vin[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { pin[c] = ROWI(o.base, c); vin[c] = ROWI(o.base, 3 + c); }
  const int S = cw & mw & 15, A4 = S & in;
  const bool mine = ((S >> leg) & 1) != 0, had = ((A4 >> leg) & 1) != 0;
  T* const anc = o.anchor + (size_t)(3 * leg) * N + s32;
  V3<T> av = mk<T>((T)0, (T)0, (T)0);
  if (had) av = mk<T>(anc[0], anc[N], anc[2 * N]);

  M3<T> R;
  {
    const T n = rsqrt_t(qa[0] * qa[0] + qa[1] * qa[1] + qa[2] * qa[2] + qa[3] * qa[3]);
    const T x = qa[0] * n, y = qa[1] * n, z = qa[2] * n, w = qa[3] * n;
    R.a[0] = 1 - 2 * (y * y + z * z); R.a[1] = 2 * (x * y - z * w);     R.a[2] = 2 * (x * z + y * w);
    R.a[3] = 2 * (x * y + z * w);     R.a[4] = 1 - 2 * (x * x + z * z); R.a[5] = 2 * (y * z - x * w);
    R.a[6] = 2 * (x * z - y * w);     R.a[7] = 2 * (y * z + x * w);     R.a[8] = 1 - 2 * (x * x + y * y);
  }
  // the leg's chain in base coordinates with the base origin at rest: origins, the foot point d, and the foot's velocity vf (the position and
  // velocity parts of swing_leg_cmd's recursion: no accelerations, no Jacobian)
  V3<T> og = mk<T>((T)0, (T)0, (T)0), vo = og;
  V3<T> Om = tmul(R, mk<T>(om[0], om[1], om[2]));
  M3<T> A;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int ok = JOINT_WORDS * k;
    T sn, cs;
    sincos_t(ql[k], &sn, &cs);
    M3<T> E;
#pragma unroll
    for (int e = 0; e < 9; ++e) E.a[e] = CS(ok + e) + cs * CS(ok + 9 + e) + sn * CS(ok + 18 + e);
    const V3<T> r = mk<T>(CS(ok + 27), CS(ok + 28), CS(ok + 29));
    const V3<T> ax = mk<T>(CS(ok + 30), CS(ok + 31), CS(ok + 32));
    const V3<T> l = k == 0 ? r : mul(A, r);
    vo = vo + cross(Om, l);
    og = og + l;
    if (k == 0) {
      A = E;
    } else {
      M3<T> B;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B.a[3 * i + j] = A.a[3 * i] * E.a[j] + A.a[3 * i + 1] * E.a[3 + j] + A.a[3 * i + 2] * E.a[6 + j];
      A = B;
    }
    Om = Om + mul(A, ax) * vl[k];
  }
  const V3<T> lf = mul(A, mk<T>(CS(3 * JOINT_WORDS), CS(3 * JOINT_WORDS + 1), CS(3 * JOINT_WORDS + 2)));
  const V3<T> lever = mul(R, og + lf);
  const V3<T> u = mul(R, vo + cross(Om, lf));

  // velocity: the trusted feet's mean (selected, not multiplied: an untrusted foot's NaN stays out), then the blend
  const V3<T> zero = mk<T>((T)0, (T)0, (T)0);
  const V3<T> su = odom_sum4(mine ? u : zero);
  const int cnt = __popc((unsigned)S), na = __popc((unsigned)A4);
  const T ic = odom_inv<T>(cnt), ia = odom_inv<T>(na);
  const T sux[3] = {su.x, su.y, su.z};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const T vm = -sux[c] * ic;
    vh[c] = cnt > 0 ? vin[c] + o.a_v * (vm - vin[c]) : vin[c];
  }
  // position: predict, then blend with the mean of the anchored trusted feet
  const V3<T> sx = odom_sum4(had ? av - lever : zero);
  const T sxx[3] = {sx.x, sx.y, sx.z};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const T pp = pin[c] + o.dt * vh[c];
    const T pm = sxx[c] * ia;
    ph[c] = na > 0 ? pp + o.a_p * (pm - pp) : pp;
  }
  // a trusted foot without an anchor takes one where it stands, dropped onto its plane
  if (mine && !had) {
    V3<T> x = mk<T>(ph[0], ph[1], ph[2]) + lever;
    if (o.height) {
      const V3<T> n = mk<T>(ROWI(o.normals, 3 * leg), ROWI(o.normals, 3 * leg + 1), ROWI(o.normals, 3 * leg + 2));
      x = x - n * (dot(n, x) - ROWI(o.height, leg));
    }
    if (live) { anc[0] = x.x; anc[N] = x.y; anc[2 * N] = x.z; }
  }
  if (live) {
    if (leg == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        ROWI(o.base, c) = ph[c]; ROWI(o.base, 3 + c) = vh[c];
        ROWI(o.q_est, c) = ph[c]; ROWI(o.v_est, c) = vh[c];
      }
      o.odo[s32] = S | ((S & ~in) << 4);
    }
    // the copy rows, dealt over the state's four lanes (32-bit element offsets: every array is below 4 GiB)
    if (o.q_est != q)
      for (unsigned r = 3 + (unsigned)leg; r < (unsigned)ODOM_NQ; r += 4) o.q_est[r * N32 + s32] = q[r * N32 + s32];
    if (o.v_est != v)
      for (unsigned r = 3 + (unsigned)leg; r < (unsigned)ODOM_NV; r += 4) o.v_est[r * N32 + s32] = v[r * N32 + s32];
  }
}

template <class T>
__global__ __launch_bounds__(64) void base_estimate_kernel(const DevModel<T>* __restrict__ model, OdomArgs<T> a) {
  __shared__ T cst[CST_WORDS];
  for (int i = threadIdx.x; i < CST_WORDS; i += blockDim.x) cst[i] = model->cst[i];
  __syncthreads();
  WBC_LAUNDERED_TID(tx);
  const LegLane l = leg_lane<16>(tx, a.N);
  T ph[3], vh[3];
  odom_law<T>(a.o, cst, a.q, a.v, a.jpack, l.leg, l.s32, a.N, l.live, a.o.contact[l.s32], a.o.mask[l.s32], ph, vh);
}

// the law on the words as loaded (the previous tick's contact and mask), the contact law, then the gait scheduler's body on the estimated base rows
template <class T>
__global__ __launch_bounds__(64) void gait_estimated_odom_kernel(const DevModel<T>* __restrict__ model, GaitEstimatedOdomArgs<T> xa) {
  __shared__ T cst[CST_WORDS];
  for (int i = threadIdx.x; i < CST_WORDS; i += blockDim.x) cst[i] = model->cst[i];
  __syncthreads();
  int word;
  T p_hat[3], v_hat[3];
  {
    WBC_LAUNDERED_TID(tx);
    const GaitEstimatedArgs<T>& ea = xa.e;
    const LegLane l = leg_lane<16>(tx, ea.g.N);
    T fn; bool bit, sing; int prev;
    const V3<T> f = contact_law<T>(ea.c, ea.g.jpack, l.leg, l.s32, (unsigned)ea.g.N, fn, bit, sing, prev);   // (loads and arithmetic: nothing is stored yet)
    odom_law<T>(xa.o, cst, ea.g.q, ea.g.v, ea.g.jpack, l.leg, l.s32, ea.g.N, l.live, prev, ea.g.mask[l.s32], p_hat, v_hat);
    word = contact_store<T>(ea.c, l.leg, l.st, l.s32, (unsigned)ea.g.N, l.live, f, fn, bit, sing, prev);
  }
  const GaitArgs<T>& a = xa.e.g;
#define GAIT_SENSED_WORD word
#define GAIT_CST_STAGED 1
#define GAIT_BASE_Q(c) ((c) < 3 ? p_hat[(c) < 3 ? (c) : 0] : ROWI(a.q, c))
#define GAIT_BASE_V(c) v_hat[c]
#include "gait_body.inc.hpp"
#undef GAIT_BASE_V
#undef GAIT_BASE_Q
#undef GAIT_CST_STAGED
#undef GAIT_SENSED_WORD
}

}  // namespace wbc
