// Trunk reference from the velocity command (include/wbc_hip.h at wbc_reference_cmd_batch): the reference generator of the walking tick without a
// host-written plan.  Where com_reference_kernel tracks plan [12][N] -- a quintic from c0 to c1 and one fixed quat_des -- these kernels form the CoM
// reference and the desired attitude from the cmd buffer the gait call reads and from the foot planes the terrain call writes, and advance a small
// per-robot state trunk [6][N] in place:  (x, y) the reference CoM, psi the reference heading, z_s / s_x / s_y the support plane under the four feet.
//   1 heading   psi+ = psi + wz dt unless that moves it further than yaw_leash from the trunk's heading h_r (then held and w_des_z = 0), wrapped
//   2 position  (x, y) += Rz(psi+)(vx, vy) dt, pulled back to within `leash` of the CoM
//   3 support   least-squares plane through the surface points under the feet whose plane has n_z >= nz_min, blended with a_s
//   4 reference c_ref = (x, y, z_s + height), cd_ref = (v_w, slope . v_w)       5 attitude  quat_des = q_tilt (e_z -> the leaned normal) * q_yaw(psi+)
//   6 outputs   the PD laws, F, w_des and the joint posture rows of com_reference_body
// Same lane mapping as com_reference_kernel (lane = 16*leg + state, 64 threads, the constant table in LDS).  The body below RESTATES
// com_reference_body's chain (stand-alone form: !EXT, !SIMG) so that no existing unit's device code moves; the plan policy is what differs.  A lane
// runs its leg's chain once: the CoM moments as there, and p_f of its foot (the position chain of the gait call: origins down the leg in base
// coordinates).  It loads its own foot's plane (3 + 1 words) and contributes its terms of step 3; the four legs are combined with xrow_sum, after
// which every lane of a state holds the same bits, so the law runs redundantly in all four and the leg-0 lane stores trunk (the leg-1 lane ref).
// Everything behind the chain -- p_f, the law, the PD laws, F and Mo -- is written with contraction OFF: no product of it is fused, in either
// instantiation, so cmd_reference_kernel and cmd_swing_reference_kernel cannot round it differently.  (The chain keeps com_reference_body's text.)
// In place: every lane has loaded the state's trunk words before the store that depends on them, and a state's four lanes share a wavefront.
// Registers: the fused kernel stores trunk, ref, w_des, com and the base rows BEFORE the swing functor runs; a_cmd, alpha_cmd, the posture rows, R,
// E and the base state are what stays live across it.
// Out of scope: the rollout kernels and wbc_rollout_*, wbc_multi_*, a pitch/roll-rate feed-forward, a convex-MPC force plan, CoM references shaped
// by the gait phase.
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "dyn_sweep.hip.hpp"
#include "com_ref.hip.hpp"
#include "swing_ref.hip.hpp"

namespace wbc {

WBC_DEV double atan2_t(double y, double x) { return atan2(y, x); }
WBC_DEV float atan2_t(float y, float x) { return atan2f(y, x); }

// M v and A B with every product rounded on its own (see the head of this file)
template <class T> WBC_DEV V3<T> nc_mul(const M3<T>& m, V3<T> v) {
#pragma clang fp contract(off)
  return mk<T>(m.a[0] * v.x + m.a[1] * v.y + m.a[2] * v.z, m.a[3] * v.x + m.a[4] * v.y + m.a[5] * v.z, m.a[6] * v.x + m.a[7] * v.y + m.a[8] * v.z);
}
template <class T> WBC_DEV V3<T> nc_tmul(const M3<T>& m, V3<T> v) {
#pragma clang fp contract(off)
  return mk<T>(m.a[0] * v.x + m.a[3] * v.y + m.a[6] * v.z, m.a[1] * v.x + m.a[4] * v.y + m.a[7] * v.z, m.a[2] * v.x + m.a[5] * v.y + m.a[8] * v.z);
}
template <class T> WBC_DEV M3<T> nc_mm(const M3<T>& A, const M3<T>& B) {
#pragma clang fp contract(off)
  M3<T> C;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C.a[3 * i + j] = A.a[3 * i] * B.a[j] + A.a[3 * i + 1] * B.a[3 + j] + A.a[3 * i + 2] * B.a[6 + j];
  return C;
}
template <class T> WBC_DEV V3<T> nc_add(V3<T> a, V3<T> b) { return mk<T>(a.x + b.x, a.y + b.y, a.z + b.z); }

// Steps 0-5 of the law for one state, run alike by its four lanes.  In: the CoM c, the trunk's heading (hx, hy), the command, the lane's own foot
// point pf and plane (n, d), reset.  tr: the state's six words, advanced.  Out: w_des_z, v_w, and quat_des (x, y, z, w).
template <class T>
WBC_DEV void trunk_law(const DevTrunkParams<T>& P, bool rs, T cx, T cy, T hx, T hy, T vx, T vy, T wz, V3<T> pf, V3<T> n, T dpl, T (&tr)[TRUNK_WORDS],
                       T& wdz, T (&vw)[2], T (&qd)[4]) {
#pragma clang fp contract(off)
  const T zero = (T)0, one = (T)1;
  // 0 reset
  T x = rs ? cx : tr[0], y = rs ? cy : tr[1];
  const T psi = rs ? atan2_t(hy, hx) : tr[2];
  // 1 heading
  T psn = psi + wz * P.dt;
  T s0, c0, s1, c1;
  sincos_t(psi, &s0, &c0);
  sincos_t(psn, &s1, &c1);
  const T g0 = hx * c0 + hy * s0, g1 = hx * c1 + hy * s1;
  const bool adv = g1 >= P.cos_yl || g1 >= g0;
  psn = adv ? psn : psi;
  wdz = adv ? wz : zero;
  psn = psn > P.pi ? psn - P.two_pi : (psn <= -P.pi ? psn + P.two_pi : psn);
  // 2 position
  T sp, cp;
  sincos_t(psn, &sp, &cp);
  const T vwx = cp * vx - sp * vy, vwy = sp * vx + cp * vy;
  T xn = x + vwx * P.dt, yn = y + vwy * P.dt;
  {
    const T ex = xn - cx, ey = yn - cy, e2 = ex * ex + ey * ey;
    const T sc = P.leash * rsqrt_t(e2);
    const bool pull = e2 > P.leash * P.leash;
    xn = pull ? cx + ex * sc : xn;
    yn = pull ? cy + ey * sc : yn;
  }
  // 3 support plane
  const bool w = n.z >= P.nz_min;
  const T zk = (dpl - n.x * pf.x - n.y * pf.y) / n.z;
  const T m = xrow_sum(w ? one : zero);
  const T im = m > zero ? one / m : zero;
  const T xb = xrow_sum(w ? pf.x : zero) * im, yb = xrow_sum(w ? pf.y : zero) * im, zb = xrow_sum(w ? zk : zero) * im;
  const T dx = w ? pf.x - xb : zero, dy = w ? pf.y - yb : zero, dz = w ? zk - zb : zero;
  const T Sxx = xrow_sum(dx * dx), Sxy = xrow_sum(dx * dy), Syy = xrow_sum(dy * dy), Sxz = xrow_sum(dx * dz), Syz = xrow_sum(dy * dz);
  const T det = Sxx * Syy - Sxy * Sxy;
  const bool fit = m >= (T)3 && det > P.det_min;
  const T b = fit ? (Syy * Sxz - Sxy * Syz) / det : zero, c = fit ? (Sxx * Syz - Sxy * Sxz) / det : zero;
  const T sx0 = (rs && !fit) ? zero : tr[4], sy0 = (rs && !fit) ? zero : tr[5];
  // (a reset ASSIGNS: a_s = 1 without the rounding of z + (z* - z), and without reading words the caller may not have initialised)
  const T sxn = fit ? (rs ? b : sx0 + P.a_s * (b - sx0)) : sx0, syn = fit ? (rs ? c : sy0 + P.a_s * (c - sy0)) : sy0;
  const T zst = zb + (fit ? b : sx0) * (xn - xb) + (fit ? c : sy0) * (yn - yb);
  const T zsn = m > zero ? (rs ? zst : tr[3] + P.a_s * (zst - tr[3])) : tr[3];
  // 5 desired attitude
  {
    const T tx = -(P.tilt * sxn), ty = -(P.tilt * syn);
    const T nn = rsqrt_t(tx * tx + ty * ty + one);
    const T nx = tx * nn, ny = ty * nn, nz = nn;
    const T w1 = one + nz;
    const T qn = rsqrt_t(ny * ny + nx * nx + w1 * w1);
    const T x1 = -ny * qn, y1 = nx * qn, ww = w1 * qn;
    T sh, ch;
    sincos_t((T)0.5 * psn, &sh, &ch);
    qd[0] = x1 * ch + y1 * sh; qd[1] = y1 * ch - x1 * sh; qd[2] = ww * sh; qd[3] = ww * ch;
  }
  tr[0] = xn; tr[1] = yn; tr[2] = psn; tr[3] = zsn; tr[4] = sxn; tr[5] = syn;
  vw[0] = vwx; vw[1] = vwy;
}

template <class T, class SWING = RefNoSwing>
WBC_DEV void cmd_reference_body(const DevModel<T>* __restrict__ model, const DevRefParams<T>* __restrict__ G, const CmdRefArgs<T>& a,
                                const SWING& swing = SWING()) {
  __shared__ T cst[CST_WORDS];
  for (int i = threadIdx.x; i < CST_WORDS; i += blockDim.x) cst[i] = model->cst[i];
  __syncthreads();
  WBC_LAUNDERED_TID(tx);
  const size_t N = a.N;
  WBC_LEG_LANE(16, 1, WBC_SRAW_A(16))
  using RowV = T;
  T qb[7], vb[6];
#pragma unroll
  for (int c = 0; c < 7; ++c) qb[c] = LDU(a.q, c);
#pragma unroll
  for (int c = 0; c < 6; ++c) vb[c] = LDU(a.v, c);
  int jx[3];
  jidx_of_leg(model, a.jpack, leg, jx);
  T ql[3], vl[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ql[k] = LDV(a.q, 7 + jx[k]);
    vl[k] = LDV(a.v, 6 + jx[k]);
  }
  T tr[TRUNK_WORDS];
#pragma unroll
  for (int c = 0; c < TRUNK_WORDS; ++c) tr[c] = LDU(a.trunk, c);
  const T cvx = LDU(a.cmd, 0), cvy = LDU(a.cmd, 1), cwz = LDU(a.cmd, 2);
  const bool rs = a.reset ? a.reset[s32] != 0 : false;
  T qx, qy, qz, qw;
  {
    const T n = rsqrt_t(qb[3] * qb[3] + qb[4] * qb[4] + qb[5] * qb[5] + qb[6] * qb[6]);
    qx = qb[3] * n; qy = qb[4] * n; qz = qb[5] * n; qw = qb[6] * n;
  }
  M3<T> R;
  {
    const T x = qx, y = qy, z = qz, w = qw;
    R.a[0] = 1 - 2 * (y * y + z * z); R.a[1] = 2 * (x * y - z * w);     R.a[2] = 2 * (x * z + y * w);
    R.a[3] = 2 * (x * y + z * w);     R.a[4] = 1 - 2 * (x * x + z * z); R.a[5] = 2 * (y * z - x * w);
    R.a[6] = 2 * (x * z - y * w);     R.a[7] = 2 * (y * z + x * w);     R.a[8] = 1 - 2 * (x * x + y * y);
  }
  const V3<T> om0 = tmul(R, mk<T>(vb[3], vb[4], vb[5]));
  const V3<T> v0 = tmul(R, mk<T>(vb[0], vb[1], vb[2]));

  // forward sweep down the leg (com_reference_body's, stand-alone form)
  M3<T> E[3];
  V3<T> pk[3];
  V3<T> omp = om0, vp = v0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int o = JOINT_WORDS * k;
    T sn, cs;
    sincos_t(ql[k], &sn, &cs);
#pragma unroll
    for (int e = 0; e < 9; ++e) E[k].a[e] = CS(o + e) + cs * CS(o + 9 + e) + sn * CS(o + 18 + e);
    const V3<T> r = mk<T>(CS(o + 27), CS(o + 28), CS(o + 29));
    const V3<T> ax = mk<T>(CS(o + 30), CS(o + 31), CS(o + 32));
    const V3<T> h = mk<T>(CS(o + 34), CS(o + 35), CS(o + 36));
    V3<T> om;
    {
#pragma clang fp contract(off)
      const M3<T>& e = E[k];
      om = mk<T>(fma_w(ax.x, vl[k], fma_w(e.a[6], omp.z, fma_w(e.a[0], omp.x, e.a[3] * omp.y))),
                 fma_w(ax.y, vl[k], fma_w(e.a[7], omp.z, fma_w(e.a[1], omp.x, e.a[4] * omp.y))),
                 fma_w(ax.z, vl[k], fma_w(e.a[8], omp.z, fma_w(e.a[2], omp.x, e.a[5] * omp.y))));
    }
    const V3<T> vv = tmul(E[k], vp + cross(omp, r));
    pk[k] = vv * CS(o + 33) + cross(om, h);
    omp = om; vp = vv;
  }
  // return sweep: first moment (cm, ch) and linear momentum P of the leg, expressed in the base frame at the end
  T cm = CS(2 * JOINT_WORDS + 33);
  V3<T> ch = mk<T>(CS(2 * JOINT_WORDS + 34), CS(2 * JOINT_WORDS + 35), CS(2 * JOINT_WORDS + 36));
  V3<T> P = pk[2];
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    const int o = JOINT_WORDS * k;
    const V3<T> r = mk<T>(CS(o + 27), CS(o + 28), CS(o + 29));
    ch = mul(E[k], ch) + r * cm;
    P = mul(E[k], P);
    if (k > 0) {
      const int op = JOINT_WORDS * (k - 1);
      cm += CS(op + 33);
      ch = ch + mk<T>(CS(op + 34), CS(op + 35), CS(op + 36));
      P = P + pk[k - 1];
    }
  }
  const T bm = model->base_m;
  const V3<T> bh = mk<T>(model->base_h[0], model->base_h[1], model->base_h[2]);
  const T mtot = xrow_sum(cm) + bm;
  const V3<T> hb = xrow_sum(ch) + bh;
  const V3<T> Pb = xrow_sum(P) + v0 * bm + cross(om0, bh);
  const T im = (T)1 / mtot;
  const V3<T> crel = mul(R, hb) * im;
  const V3<T> c = crel + mk<T>(qb[0], qb[1], qb[2]);
  const V3<T> cd = mul(R, Pb) * im;

  // the lane's foot point: the gait call's position chain (origins down the leg in base coordinates), and its plane
  V3<T> pf;
  {
    const V3<T> r0 = mk<T>(CS(27), CS(28), CS(29));
    const V3<T> r1 = mk<T>(CS(JOINT_WORDS + 27), CS(JOINT_WORDS + 28), CS(JOINT_WORDS + 29));
    const V3<T> r2 = mk<T>(CS(2 * JOINT_WORDS + 27), CS(2 * JOINT_WORDS + 28), CS(2 * JOINT_WORDS + 29));
    V3<T> o = nc_add(r0, nc_mul(E[0], r1));
    M3<T> A = nc_mm(E[0], E[1]);
    o = nc_add(o, nc_mul(A, r2));
    A = nc_mm(A, E[2]);
    const V3<T> d = nc_add(o, nc_mul(A, mk<T>(CS(3 * JOINT_WORDS), CS(3 * JOINT_WORDS + 1), CS(3 * JOINT_WORDS + 2))));
    pf = nc_add(mk<T>(qb[0], qb[1], qb[2]), nc_mul(R, d));
  }
  const V3<T> pn = mk<T>(LDL(a.normals, 0, 3), LDL(a.normals, 1, 3), LDL(a.normals, 2, 3));
  const T pd = LDL(a.height, 0, 1);

  T acmd[3], alcmd[3], Fv[3], Mv[3], wdz, vw[2], qd[4];
  {
#pragma clang fp contract(off)
    const T hn = rsqrt_t(R.a[0] * R.a[0] + R.a[3] * R.a[3]);
    trunk_law<T>(a.P, rs, c.x, c.y, R.a[0] * hn, R.a[3] * hn, cvx, cvy, cwz, pf, pn, pd, tr, wdz, vw, qd);
    // 4 reference, 6 outputs
    const T cref[3] = {tr[0], tr[1], tr[3] + a.P.height}, cdref[3] = {vw[0], vw[1], tr[4] * vw[0] + tr[5] * vw[1]};
    const T cc[3] = {c.x, c.y, c.z}, cdv[3] = {cd.x, cd.y, cd.z};
#pragma unroll
    for (int i = 0; i < 3; ++i) acmd[i] = G->kp_com[i] * (cref[i] - cc[i]) + G->kd_com[i] * (cdref[i] - cdv[i]);
    {
      const T dn = rsqrt_t(qd[0] * qd[0] + qd[1] * qd[1] + qd[2] * qd[2] + qd[3] * qd[3]);
      const T dx = qd[0] * dn, dy = qd[1] * dn, dz = qd[2] * dn, dw = qd[3] * dn;
      const T x = -qx, y = -qy, z = -qz, w = qw;
      const T ex = dw * x + dx * w + dy * z - dz * y;
      const T ey = dw * y - dx * z + dy * w + dz * x;
      const T ez = dw * z + dx * y - dy * x + dz * w;
      const T ew = dw * w - dx * x - dy * y - dz * z;
      const T sg = ew < (T)0 ? (T)-2 : (T)2;
      alcmd[0] = G->kp_rot[0] * (sg * ex) + G->kd_rot[0] * ((T)0 - vb[3]);
      alcmd[1] = G->kp_rot[1] * (sg * ey) + G->kd_rot[1] * ((T)0 - vb[4]);
      alcmd[2] = G->kp_rot[2] * (sg * ez) + G->kd_rot[2] * (wdz - vb[5]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) Fv[i] = (acmd[i] - model->grav[i]) * mtot;
    const V3<T> lb = nc_tmul(R, mk<T>(alcmd[0], alcmd[1], alcmd[2]));
    const V3<T> Il = nc_mul(R, mk<T>(G->inertia_nom[0] * lb.x, G->inertia_nom[1] * lb.y, G->inertia_nom[2] * lb.z));
    Mv[0] = (crel.y * Fv[2] - crel.z * Fv[1]) + Il.x;
    Mv[1] = (crel.z * Fv[0] - crel.x * Fv[2]) + Il.y;
    Mv[2] = (crel.x * Fv[1] - crel.y * Fv[0]) + Il.z;
    if (live && leg == 0) {
#pragma unroll
      for (int i = 0; i < TRUNK_WORDS; ++i) ROWU(a.trunk, i) = tr[i];
    }
    if (a.ref && live && leg == 1) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { ROWU(a.ref, i) = cref[i]; ROWU(a.ref, 3 + i) = cdref[i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i) ROWU(a.ref, 6 + i) = qd[i];
    }
  }
  // outputs: dealt over the four leg rows as com_reference_body deals them; everything but the posture rows before the swing functor
  if (live) ROWV(a.w_des, sel4<int>(leg, 0, 1, 2, 3)) = sel4<T>(leg, Fv[0], Fv[1], Fv[2], Mv[0]);
  if (leg < 2) if (live) ROWV(a.w_des, 4 + leg) = leg == 0 ? Mv[1] : Mv[2];
  if (live) ROWV(a.vdot_des, sel4<int>(leg, 0, 1, 2, 3)) = sel4<T>(leg, acmd[0], acmd[1], acmd[2], alcmd[0]);
  if (leg >= 2) if (live) ROWV(a.vdot_des, 2 + leg) = leg == 2 ? alcmd[1] : alcmd[2];
  if (a.com) {
    if (live) ROWV(a.com, sel4<int>(leg, 0, 1, 2, 3)) = sel4<T>(leg, c.x, c.y, c.z, cd.x);
    if (leg < 2) if (live) ROWV(a.com, 4 + leg) = leg == 0 ? cd.y : cd.z;
  }
  T adj[3];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) adj[k] = G->kp_joint * (G->q_nom[jx[k]] - ql[k]) - G->kd_joint * vl[k];
  }
  if constexpr (SWING::on) swing(cst, leg, N, s32, live, R, qb, vb, om0, E, vl, acmd, alcmd, (T)0, adj);
#pragma unroll
  for (int k = 0; k < 3; ++k) if (live) ROWV(a.vdot_des, 6 + jx[k]) = adj[k];
}

template <class T>
__global__ __launch_bounds__(64) void cmd_reference_kernel(const DevModel<T>* __restrict__ model, const DevRefParams<T>* __restrict__ G,
                                                           CmdRefArgs<T> a) {
  cmd_reference_body<T>(model, G, a);
}

template <class T>
__global__ __launch_bounds__(64) void cmd_swing_reference_kernel(const DevModel<T>* __restrict__ model, const DevRefParams<T>* __restrict__ G,
                                                                 CmdRefArgs<T> a, SwingArgs<T> sa) {
  cmd_reference_body<T, RefSwing<T>>(model, G, a, RefSwing<T>{&sa});
}

}  // namespace wbc
