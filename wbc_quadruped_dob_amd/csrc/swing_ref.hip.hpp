// Swing-foot references: Cartesian foot tracking for the legs whose mask bit is clear (include/wbc_hip.h at wbc_swing_reference_batch).
// The CoM reference generator asks a lifted leg only for a joint posture; this maps a foot trajectory to the leg's joint accelerations:
//   swing [36][N]: per foot k rows 9 k ...: p0 (3) lift-off, p1 (3) touchdown (world), hgt apex clearance, T duration, t0 elapsed
//   u = clamp((t0 + t) / T, 0, 1);  p_ref = p0 + s0 d + hgt b z,  s0 the rest-to-rest quintic of com_ref.hip.hpp,  b = 64 u^3 (1 - u)^3
//   a_cmd = pdd_ref + kp (p_ref - p_f) + kd (pd_ref - J_k v)
//   (J_kl J_kl^T + damping 1) y = a_cmd - Jdot_k v - J_kb vdot_des[0..5],   vdot_des[6 + j] = (J_kl^T y)_j
// Same lane mapping as the reference generator (lane = 16*leg + state): every lane runs the kinematics of ITS leg in base coordinates --
// joint axes z_j, link origins o_j, the foot point d -- and with them the foot's velocity and its acceleration at vdot = 0 (the velocity-product
// recursion: angular velocity Om, angular acceleration al, origin acceleration ao, leaf-ward).  J_kl = R C with C_j = z_j x (d - o_j), so the 3x3
// system is solved in base coordinates, (C C^T + damping 1) y_b = R^T rhs, by cofactors in registers.  No cross-lane traffic.
// Out of scope: the one-launch rollout kernels and wbc_rollout_*, wbc_multi_*, contact schedules and touchdown detection, an apex direction
// aligned with the terrain normal (the clearance is along world z).
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "dyn_sweep.hip.hpp"
#include "com_ref.hip.hpp"

namespace wbc {

// One leg.  cst: the constant table (LDS); R: base -> world; pb, vlin: base position / linear velocity (world); om0: base angular velocity in BASE
// coordinates; E[k]: the leg's joint rotations (child -> parent); vl: its joint rates; bacc: vdot_des[0..5]; sw: the foot's nine plan words.
// Out: qdd (the leg's joint accelerations, base to foot), pf, jv (foot position and velocity J_k v, world).
template <class T>
WBC_DEV void swing_leg_cmd(const T* cst, int leg, const M3<T>& R, V3<T> pb, V3<T> vlin, V3<T> om0, const M3<T> (&E)[3], const T (&vl)[3],
                           const T (&bacc)[6], const T (&sw)[9], T t, const DevSwingParams<T>& P, T (&qdd)[3], V3<T>& pf, V3<T>& jv) {
  M3<T> A = E[0];                       // link k -> base
  V3<T> o = mk<T>((T)0, (T)0, (T)0);    // origin of link k, base coordinates
  V3<T> z[3], oj[3];
  V3<T> Om = om0, al = o, ao = o, vo = o;   // of the link the loop has reached: angular velocity / acceleration, its origin's acceleration and velocity (relative to the base origin's)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int ok = JOINT_WORDS * k;
    const V3<T> r = mk<T>(CS(ok + 27), CS(ok + 28), CS(ok + 29));
    const V3<T> ax = mk<T>(CS(ok + 30), CS(ok + 31), CS(ok + 32));
    const V3<T> l = k == 0 ? r : mul(A, r);   // o_k - o_(k-1)
    ao = ao + cross(al, l) + cross(Om, cross(Om, l));
    vo = vo + cross(Om, l);
    o = o + l;
    if (k > 0) {
      M3<T> B;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B.a[3 * i + j] = A.a[3 * i] * E[k].a[j] + A.a[3 * i + 1] * E[k].a[3 + j] + A.a[3 * i + 2] * E[k].a[6 + j];
      A = B;
    }
    const V3<T> zk = mul(A, ax);
    al = al + cross(Om, zk) * vl[k];
    Om = Om + zk * vl[k];
    z[k] = zk; oj[k] = o;
  }
  const V3<T> lf = mul(A, mk<T>(CS(3 * JOINT_WORDS), CS(3 * JOINT_WORDS + 1), CS(3 * JOINT_WORDS + 2)));
  const V3<T> d = o + lf;                                                   // foot relative to the base origin
  const V3<T> af = ao + cross(al, lf) + cross(Om, cross(Om, lf));           // Jdot_k v, base coordinates
  const V3<T> vf = vo + cross(Om, lf);
  V3<T> C[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) C[k] = cross(z[k], d - oj[k]);
  const V3<T> dw = mul(R, d);
  pf = pb + dw;
  jv = vlin + mul(R, vf);

  // time law
  const T Tp = sw[7];
  const bool hasT = Tp > (T)0;
  const T iT = hasT ? (T)1 / Tp : (T)0;
  T u = hasT ? (sw[8] + t) * iT : (T)1;
  u = u < (T)0 ? (T)0 : (u > (T)1 ? (T)1 : u);
  const T u2 = u * u, u3 = u2 * u;
  const T s0 = u3 * (10 + u * (-15 + 6 * u));
  const T s1 = u2 * (30 + u * (-60 + 30 * u)) * iT;
  const T s2 = u * (60 + u * (-180 + 120 * u)) * iT * iT;
  const T w = u * ((T)1 - u), w2 = w * w;
  const T b0 = sw[6] * ((T)64 * w2 * w);
  const T b1 = sw[6] * ((T)192 * w2 * ((T)1 - 2 * u)) * iT;
  const T b2 = sw[6] * ((T)384 * w * ((T)1 + u * (-5 + 5 * u))) * iT * iT;
  const T pfv[3] = {pf.x, pf.y, pf.z}, jvv[3] = {jv.x, jv.y, jv.z};
  T ac[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const T dd = sw[3 + i] - sw[i];
    T pr = sw[i] + s0 * dd, vr = s1 * dd, ar = s2 * dd;
    if (i == 2) { pr += b0; vr += b1; ar += b2; }
    ac[i] = ar + P.kp[i] * (pr - pfv[i]) + P.kd[i] * (vr - jvv[i]);
  }
  const V3<T> jb = mk<T>(bacc[0], bacc[1], bacc[2]) + cross(mk<T>(bacc[3], bacc[4], bacc[5]), dw);   // J_kb vdot_des[0..5]
  const V3<T> rhs = tmul(R, mk<T>(ac[0], ac[1], ac[2]) - jb) - af;
  // G = C C^T + damping 1 (SPD), y = G^-1 rhs by cofactors
  const T lam = P.damping;
  const T g00 = C[0].x * C[0].x + C[1].x * C[1].x + C[2].x * C[2].x + lam;
  const T g01 = C[0].x * C[0].y + C[1].x * C[1].y + C[2].x * C[2].y;
  const T g02 = C[0].x * C[0].z + C[1].x * C[1].z + C[2].x * C[2].z;
  const T g11 = C[0].y * C[0].y + C[1].y * C[1].y + C[2].y * C[2].y + lam;
  const T g12 = C[0].y * C[0].z + C[1].y * C[1].z + C[2].y * C[2].z;
  const T g22 = C[0].z * C[0].z + C[1].z * C[1].z + C[2].z * C[2].z + lam;
  const T c00 = g11 * g22 - g12 * g12;
  const T c01 = g02 * g12 - g01 * g22;
  const T c02 = g01 * g12 - g02 * g11;
  const T c11 = g00 * g22 - g02 * g02;
  const T c12 = g01 * g02 - g00 * g12;
  const T c22 = g00 * g11 - g01 * g01;
  const T idet = (T)1 / (g00 * c00 + g01 * c01 + g02 * c02);
  const V3<T> y = mk<T>((c00 * rhs.x + c01 * rhs.y + c02 * rhs.z) * idet, (c01 * rhs.x + c11 * rhs.y + c12 * rhs.z) * idet,
                        (c02 * rhs.x + c12 * rhs.y + c22 * rhs.z) * idet);
#pragma unroll
  for (int k = 0; k < 3; ++k) qdd[k] = dot(C[k], y);
}

// the plan words and mask bit of the lane's leg, the command, the foot rows (by their owner lane); swing legs' qdd replace adj
template <class T>
WBC_DEV void swing_apply(const SwingArgs<T>& sa, const T* cst, int leg, size_t N, unsigned s32, bool live, const M3<T>& R, const T (&qb)[7],
                         const T (&vb)[6], V3<T> om0, const M3<T> (&E)[3], const T (&vl)[3], const T (&bacc)[6], T t, T (&adj)[3]) {
  T sw[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) sw[c] = sa.swing[((size_t)(9 * leg + c)) * N + s32];
  const bool lifted = ((sa.mask[s32] >> leg) & 1) == 0;
  T qdd[3];
  V3<T> pf, jv;
  swing_leg_cmd<T>(cst, leg, R, mk<T>(qb[0], qb[1], qb[2]), mk<T>(vb[0], vb[1], vb[2]), om0, E, vl, bacc, sw, t, sa.P, qdd, pf, jv);
#pragma unroll
  for (int k = 0; k < 3; ++k) adj[k] = lifted ? qdd[k] : adj[k];
  if (sa.foot && live) {
    T* const f = sa.foot + (size_t)(6 * leg) * N + s32;
    f[0] = pf.x; f[N] = pf.y; f[2 * N] = pf.z; f[3 * N] = jv.x; f[4 * N] = jv.y; f[5 * N] = jv.z;
  }
}

// SWING functor of com_reference_body: the fused kernel (wbc_reference_swing_batch)
template <class T> struct RefSwing {
  static constexpr bool on = true;
  const SwingArgs<T>* sa;
  WBC_DEV void operator()(const T* cst, int leg, size_t N, unsigned s32, bool live, const M3<T>& R, const T (&qb)[7], const T (&vb)[6], V3<T> om0,
                          const M3<T> (&E)[3], const T (&vl)[3], const T (&acmd)[3], const T (&alcmd)[3], T t, T (&adj)[3]) const {
    const T bacc[6] = {acmd[0], acmd[1], acmd[2], alcmd[0], alcmd[1], alcmd[2]};
    swing_apply<T>(*sa, cst, leg, N, s32, live, R, qb, vb, om0, E, vl, bacc, t, adj);
  }
};

template <class T>
__global__ __launch_bounds__(64) void com_swing_reference_kernel(const DevModel<T>* __restrict__ model, const DevRefParams<T>* __restrict__ G,
                                                                 RefArgs<T> a, SwingArgs<T> sa) {
  com_reference_body<T, false, 16, false, RefSwing<T>>(model, G, a, nullptr, RefSwing<T>{&sa});
}

// the stand-alone kernel (wbc_swing_reference_batch): the base rows of vdot_des are read as they stand, the swing legs' joint rows are written
template <class T>
__global__ __launch_bounds__(64) void swing_reference_kernel(const DevModel<T>* __restrict__ model, SwingRefArgs<T> a) {
  __shared__ T cst[CST_WORDS];
  for (int i = threadIdx.x; i < CST_WORDS; i += blockDim.x) cst[i] = model->cst[i];
  __syncthreads();
  WBC_LAUNDERED_TID(tx);
  const size_t N = a.N;
  WBC_LEG_LANE(16, 1, WBC_SRAW_A(16))   // lanes beyond the batch recompute its last state and store nothing.  (The macro form: through leg_lane() this kernel's device code moved)
  T qb[7], vb[6], bacc[6];
#pragma unroll
  for (int c = 0; c < 7; ++c) qb[c] = ROWI(a.q, c);
#pragma unroll
  for (int c = 0; c < 6; ++c) { vb[c] = ROWI(a.v, c); bacc[c] = ROWI(a.vdot_des, c); }
  int jx[3];
  jidx_of_leg(model, a.jpack, leg, jx);
  T ql[3], vl[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { ql[k] = ROWI(a.q, 7 + jx[k]); vl[k] = ROWI(a.v, 6 + jx[k]); }
  M3<T> R;
  {
    const T n = rsqrt_t(qb[3] * qb[3] + qb[4] * qb[4] + qb[5] * qb[5] + qb[6] * qb[6]);
    const T x = qb[3] * n, y = qb[4] * n, z = qb[5] * n, w = qb[6] * n;
    R.a[0] = 1 - 2 * (y * y + z * z); R.a[1] = 2 * (x * y - z * w);     R.a[2] = 2 * (x * z + y * w);
    R.a[3] = 2 * (x * y + z * w);     R.a[4] = 1 - 2 * (x * x + z * z); R.a[5] = 2 * (y * z - x * w);
    R.a[6] = 2 * (x * z - y * w);     R.a[7] = 2 * (y * z + x * w);     R.a[8] = 1 - 2 * (x * x + y * y);
  }
  const V3<T> om0 = tmul(R, mk<T>(vb[3], vb[4], vb[5]));
  M3<T> E[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int o = JOINT_WORDS * k;
    T sn, cs;
    sincos_t(ql[k], &sn, &cs);
#pragma unroll
    for (int e = 0; e < 9; ++e) E[k].a[e] = CS(o + e) + cs * CS(o + 9 + e) + sn * CS(o + 18 + e);
  }
  T adj[3] = {(T)0, (T)0, (T)0};
  swing_apply<T>(a.s, cst, leg, N, s32, live, R, qb, vb, om0, E, vl, bacc, a.t, adj);
  if (live && ((a.s.mask[s32] >> leg) & 1) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) ROWI(a.vdot_des, 6 + jx[k]) = adj[k];
  }
}

}  // namespace wbc
