// Momentum-observer update as its own kernel (unit a5/a6 without the rest of the sweep) for LARGE observer-on batches.
// The all-in-one observer sweep (dyn_sweep_kernel<.., SW_OBS>) needs 370 VGPRs and 28 kB of LDS per wavefront, i.e. one
// wave per SIMD; without the observer passes the sweep runs at two.  Here the observer is a light kernel -- per leg only
// the kinematics, body momenta, gravity terms and the own-leg Jacobian -- that runs in front of dyn_sweep<M, h, Jc + step>.
// It reads q, v, tau_prev, f_prev and the observer state, writes the new state and rhat (18 words at WS_RHAT of the step
// workspace); the QP kernel completes b = w_des - rhat_base and tau_partial - rhat_joint itself (RHAT of the QP bodies, qp_struct16.hip.hpp).
// Round 1 measured this kernel at 236 us (N = 262 144, fp64: 255 VGPRs + a 324-byte spill), as long as the sweep it was
// meant to relieve.  What held the registers was not the algorithm but two things the compiler did with it (found by a
// liveness scan of the ISA, round 2): (1) the sweep's results only feed stores guarded by `live`, so the arithmetic was sunk
// into that guarded region and the ~160 LDS reads of the whole return sweep were left in one row in front of it; (2) in a
// 256-thread workgroup the constant table sat behind a 68 kB array in LDS, out of reach of the 16-bit ds_read offset.  With
// the carried values pinned per joint, one LDS object (table first) and the forward sweep's per-joint state parked in LDS:
// 170 VGPRs, no scratch, 112 us fp64 / 57 us fp32 -- default for fp64 observer-on batches from 65 536 states on
// (fp32: 98 304); see plan_consts.hpp for the A/B.
// Same lane mapping as the sweep (lane = 16*leg + state), same formulas as the observer role of the fused tick
// (rnea_step_body<RS_OBS | RS_OBSW>): beta = C^T v - g from the momentum recursion, see docs/DESIGN_R04.md section 3.
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include <type_traits>
#include "dyn_sweep.hip.hpp"

namespace wbc {

// observer_body: the observer ROLE of the fused tick / persistent rollout kernels, EXT = 1 / 2 (EXT = 0 also compiles: the
// form the stand-alone kernel had in round 1; the kernel itself is observer_park_body below)
// (fused_tick.hip.hpp): one wavefront of a larger workgroup that owns 16 states, constant table staged by other wavefronts
// (EXT = 2: this body joins the workgroup barrier after issuing its state loads), rhat goes to the LDS image wsl.
// PART (roles only): 0 = the whole update; 1 = base rows only (momentum / gravity sums over the legs, rhat_base: what the QP's
// target wrench b waits for); 2 = joint rows only (rhat_joint, needed in the torque map).  Two wavefronts running parts 1
// and 2 side by side share the sweeps' arithmetic but each drops the other's projections and update.
// `before_store()` (roles) runs right before the base rows of {integ, r} are stored: the fused kernels wait there until the QP wavefronts
// have read r_prev (QpSync::rp_ack) -- normally long past by then.
// `after_base(stage)` (PART 0 as the ONE observer wavefront of a 4-state rollout workgroup, round 5): called with 0 as soon as rhat_base is in the LDS image
// -- the QP waits for nothing else of this role until its torque map and starts ~1.2 us earlier than behind the whole body -- and with 1 when rhat_joint is;
// the new observer state goes to memory behind both.  With the hook the observer state {f_prev, r, integ, tau_prev} is requested at the head of the body, with q and v (24
// values more in flight across the sweeps: the four-wavefront rollout kernel has the registers), instead of where the update needs it.
struct ObsNoWait { WBC_DEV void operator()() const {} WBC_DEV void operator()(int) const {} };
template <class T, int BLOCK, int EXT, int PART = 0, int SPW = 16, class BeforeStore = ObsNoWait, class AfterBase = ObsNoWait>
WBC_DEV void observer_body(const DevModel<T>* __restrict__ model, const DevParams<T> prm, const SweepArgs<T>& a, const T* cst_ext, T* wsl,
                           BeforeStore before_store = BeforeStore(), AfterBase after_base = AfterBase()) {
  static_assert(EXT == 0 || BLOCK == 64, "one wavefront");
  static_assert(PART == 0 || EXT != 0, "split parts exist only as roles");
  constexpr bool BASE = PART != 2, JOINTS = PART != 1;
  constexpr bool EARLY_BASE = !std::is_same<AfterBase, ObsNoWait>::value;
  static_assert(!EARLY_BASE || (PART == 0 && EXT != 0), "the early hand-over of rhat_base: whole update, as a role");
  __shared__ T cst_own[EXT ? 1 : CST_WORDS];
  const T* cst = EXT ? cst_ext : cst_own;
  WBC_LAUNDERED_TID(tx);
  const size_t N = a.N;
  WBC_LEG_LANE(SPW, 1, EXT ? WBC_SRAW_A(SPW) : WBC_SRAW_W(BLOCK, 1, blockIdx.x))   // (roles: SPW <= 16 states per workgroup, lane_rows.hip.hpp)
  using RowV = T;
  // rhat: HBM workspace (stand-alone kernel) or the workgroup's LDS image (role)
#define ORHAT(comp, val) do { if constexpr (EXT != 0) wsl[(comp) * 16 + (int)(tx & 15)] = (val); else { if (live) ROWV(a.ws, comp) = (val); } } while (0)
  // state loads first, table staging while they are in flight (4-state rollout workgroups: the state is in LDS, see WBC_STATE_MACROS in dyn_split.hip.hpp)
  constexpr bool SIMG = EXT == 3;
  const T* const si_ = SIMG ? a.simg + (int)(s32 - (unsigned)((size_t)blockIdx.x * SPW)) : nullptr;
  T qq[4], vb[6];
#pragma unroll
  for (int c = 0; c < 4; ++c) qq[c] = SIMG ? si_[(3 + c) * 16] : LDU(a.q, 3 + c);
#pragma unroll
  for (int c = 0; c < 6; ++c) vb[c] = SIMG ? si_[(SIMG_V + c) * 16] : LDU(a.v, c);
  int jx[3];
  // (the role keeps the table load: its joint-state loads are not on the tick's critical path -- the QP starts on r_prev -- and with the indices in
  // hand two cycles after entry the fp64 observer-on fused tick, which sits at 255 registers, spills a value)
#pragma unroll
  for (int k = 0; k < 3; ++k) jx[k] = model->jidx[leg][k];
  T ql[3], vl[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ql[k] = SIMG ? si_[(7 + jx[k]) * 16] : LDV(a.q, 7 + jx[k]);
    vl[k] = SIMG ? si_[(SIMG_V + 6 + jx[k]) * 16] : LDV(a.v, 6 + jx[k]);
  }
  T pre_k1[3] = {0, 0, 0}, pre_k2[3] = {0, 0, 0};
  T pre_fp[3] = {0, 0, 0}, pre_rb[6] = {0, 0, 0, 0, 0, 0}, pre_igb[6] = {0, 0, 0, 0, 0, 0}, pre_rj[3] = {0, 0, 0}, pre_igj[3] = {0, 0, 0}, pre_tp[3] = {0, 0, 0};
  if constexpr (EARLY_BASE) {
    if (prm.observer_order > 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) pre_fp[c] = SIMG ? a.resimg[(RES_F + 3 * leg + c) * 16 + (si_ - a.simg)] : LDV(a.f_prev, 3 * leg + c);
#pragma unroll
      for (int c = 0; c < 6; ++c) { pre_rb[c] = LDU(a.obs_r, c); pre_igb[c] = LDU(a.obs_integ, c); }
#pragma unroll
      for (int k = 0; k < 3; ++k) { pre_rj[k] = LDV(a.obs_r, 6 + jx[k]); pre_igj[k] = LDV(a.obs_integ, 6 + jx[k]); pre_tp[k] = SIMG ? a.resimg[(RES_TAU + jx[k]) * 16 + (si_ - a.simg)] : LDV(a.tau_prev, jx[k]); }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {   // gains of my joint rows by a select (no run-time index into the kernel arguments), while those loads are in flight
      pre_k1[k] = prm.K1[6]; pre_k2[k] = prm.K2[6];
#pragma unroll
      for (int j = 1; j < 12; ++j) { pre_k1[k] = (jx[k] == j) ? prm.K1[6 + j] : pre_k1[k]; pre_k2[k] = (jx[k] == j) ? prm.K2[6 + j] : pre_k2[k]; }
    }
  }
  if constexpr (EXT == 0) {
    // branch-free (clamped index, the tail lanes rewrite the last word): with a divergent staging loop here hipcc 7.2 put
    // VGPR spill stores of the fp64 build into the loop's exit block BEFORE exec is restored, i.e. with no lane enabled
    // (found by parity: rhat garbage in every state; tools/spill_lint.py now scans the ISA for that pattern)
#pragma unroll
    for (int i0 = 0; i0 < CST_WORDS; i0 += BLOCK) {
      const int i = min(i0 + (int)tx, CST_WORDS - 1);
      cst_own[i] = model->cst[i];
    }
    __syncthreads();
  }
  if constexpr (EXT == 2) __syncthreads();

  T qx, qy, qz, qw;
  {
    const T n = rsqrt_sel<SIMG>(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
    qx = qq[0] * n; qy = qq[1] * n; qz = qq[2] * n; qw = qq[3] * n;
  }
  M3<T> R;
  {
    const T x = qx, y = qy, z = qz, w = qw;
    R.a[0] = 1 - 2 * (y * y + z * z); R.a[1] = 2 * (x * y - z * w);     R.a[2] = 2 * (x * z + y * w);
    R.a[3] = 2 * (x * y + z * w);     R.a[4] = 1 - 2 * (x * x + z * z); R.a[5] = 2 * (y * z - x * w);
    R.a[6] = 2 * (x * z - y * w);     R.a[7] = 2 * (y * z + x * w);     R.a[8] = 1 - 2 * (x * x + y * y);
  }
  const T bm = model->base_m;
  const V3<T> bh = mk<T>(model->base_h[0], model->base_h[1], model->base_h[2]);
  S3<T> bI;
  bI.xx = model->base_Io[0]; bI.xy = model->base_Io[1]; bI.xz = model->base_Io[2];
  bI.yy = model->base_Io[3]; bI.yz = model->base_Io[4]; bI.zz = model->base_Io[5];
  const V3<T> om0 = tmul(R, mk<T>(vb[3], vb[4], vb[5]));
  const V3<T> v0 = tmul(R, mk<T>(vb[0], vb[1], vb[2]));
  const V3<T> gneg = tmul(R, mk<T>(-model->grav[0], -model->grav[1], -model->grav[2]));   // R^T (-g)

  // ---- forward sweep down the leg: joint rotations, body velocities, body momenta, weights (all kept in registers)
  M3<T> E[3];
  V3<T> om[3], vv[3], gL[3];   // body momenta / weights are re-formed from these in the return sweep (fewer live registers)
  {
    V3<T> omp = om0, vp = v0, gp = gneg;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int o = JOINT_WORDS * k;
      T sn, cs;
      sincos_t(ql[k], &sn, &cs);
#pragma unroll
      for (int e = 0; e < 9; ++e) E[k].a[e] = CS(o + e) + cs * CS(o + 9 + e) + sn * CS(o + 18 + e);
      const V3<T> r = mk<T>(CS(o + 27), CS(o + 28), CS(o + 29));
      const V3<T> ax = mk<T>(CS(o + 30), CS(o + 31), CS(o + 32));
      om[k] = tmul(E[k], omp) + ax * vl[k];
      vv[k] = tmul(E[k], vp + cross(omp, r));
      gL[k] = tmul(E[k], gp);
      omp = om[k]; vp = vv[k]; gp = gL[k];
    }
  }
  // ---- return sweep: subtree momentum / weight, their projections on the joint axes, foot geometry
  T p_leg[3], beta_l[3];
  V3<T> dft = mk<T>(CS(129), CS(130), CS(131));
  V3<T> jc[3];
  SF<T> macc, gacc;
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    const int o = JOINT_WORDS * k;
    const V3<T> r = mk<T>(CS(o + 27), CS(o + 28), CS(o + 29));
    const V3<T> ax = mk<T>(CS(o + 30), CS(o + 31), CS(o + 32));
    const T m = CS(o + 33);
    const V3<T> h = mk<T>(CS(o + 34), CS(o + 35), CS(o + 36));
    S3<T> Io;
    Io.xx = CS(o + 37); Io.xy = CS(o + 38); Io.xz = CS(o + 39); Io.yy = CS(o + 40); Io.yz = CS(o + 41); Io.zz = CS(o + 42);
    SF<T> mk_ = inertia_mul(m, h, Io, om[k], vv[k]), gk;
    gk.n = cross(h, gL[k]);
    gk.f = gL[k] * m;
    if (k < 2) { mk_.n = mk_.n + macc.n; mk_.f = mk_.f + macc.f; gk.n = gk.n + gacc.n; gk.f = gk.f + gacc.f; }
    p_leg[k] = dot(ax, mk_.n);
    beta_l[k] = -dot(ax, cross(om[k], mk_.n) + cross(vv[k], mk_.f)) - dot(ax, gk.n);   // (C^T v)_k - g_k
    jc[k] = cross(ax, dft);
    dft = r + mul(E[k], dft);
#pragma unroll
    for (int j = k; j < 3; ++j) jc[j] = mul(E[k], jc[j]);
    macc = to_parent(E[k], r, mk_);
    gacc = to_parent(E[k], r, gk);
  }
  const V3<T> dw = mul(R, dft);
  V3<T> jw[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) jw[k] = mul(R, jc[k]);

  // ---- base rows: the four legs + the base body itself
  T p_b[6] = {0, 0, 0, 0, 0, 0}, beta_b[6] = {0, 0, 0, 0, 0, 0};
  if constexpr (BASE) {
    const SF<T> Iv0 = inertia_mul(bm, bh, bI, om0, v0);
    T xb[12] = {macc.n.x, macc.n.y, macc.n.z, macc.f.x, macc.f.y, macc.f.z, gacc.n.x, gacc.n.y, gacc.n.z, gacc.f.x, gacc.f.y, gacc.f.z};
    xrow_sum_k<T, 12>(xb);
    const V3<T> m0n = mk<T>(xb[0], xb[1], xb[2]) + Iv0.n, m0f = mk<T>(xb[3], xb[4], xb[5]) + Iv0.f;
    const V3<T> g0n = mk<T>(xb[6], xb[7], xb[8]) + cross(bh, gneg), g0f = mk<T>(xb[9], xb[10], xb[11]) + gneg * bm;
    const V3<T> Pl = mul(R, m0f), Pa = mul(R, m0n);
    const V3<T> gl = mul(R, g0f), ga = mul(R, g0n);
    const V3<T> cx = cross(mk<T>(vb[0], vb[1], vb[2]), Pl);
    p_b[0] = Pl.x; p_b[1] = Pl.y; p_b[2] = Pl.z; p_b[3] = Pa.x; p_b[4] = Pa.y; p_b[5] = Pa.z;
    beta_b[0] = -gl.x; beta_b[1] = -gl.y; beta_b[2] = -gl.z;
    beta_b[3] = -cx.x - ga.x; beta_b[4] = -cx.y - ga.y; beta_b[5] = -cx.z - ga.z;
  }
  // ---- observer update (order 1 or 2) and rhat for the QP kernel
  T rb[6] = {0, 0, 0, 0, 0, 0}, rl[3] = {0, 0, 0};
  if constexpr (EARLY_BASE) {
    // the one-wavefront form: everything the QP waits for goes to the LDS image first -- rhat_base, hook(0), rhat_joint, hook(1) -- and only then the new
    // observer state to memory (14 store instructions of a lone wavefront, ~0.1 us each with their guards)
    T igj[3] = {0, 0, 0};
    if (prm.observer_order > 0) {
      const V3<T> fp = mk<T>(pre_fp[0], pre_fp[1], pre_fp[2]);
      const T dt = prm.dt;
      const bool o1 = prm.observer_order == 1;
      const V3<T> dxf = cross(dw, fp);
      T ub[6] = {fp.x, fp.y, fp.z, dxf.x, dxf.y, dxf.z};
      xrow_sum_k<T, 6>(ub);
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const T r0 = pre_rb[c];
        const T ig = pre_igb[c] + dt * (ub[c] + beta_b[c] + r0);
        const T e = p_b[c] - ig;
        rb[c] = o1 ? prm.K1[c] * e : r0 + dt * prm.K2[c] * (prm.K1[c] * e - r0);
        p_b[c] = ig;
      }
      ORHAT(sel4<int>(leg, WS_RHAT + 0, WS_RHAT + 1, WS_RHAT + 2, WS_RHAT + 3), sel4<T>(leg, rb[0], rb[1], rb[2], rb[3]));
      if (leg < 2) ORHAT(WS_RHAT + 4 + leg, leg == 0 ? rb[4] : rb[5]);
      after_base(0);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const T r0 = pre_rj[k];
        const T u = pre_tp[k] + dot(jw[k], fp);
        igj[k] = pre_igj[k] + dt * (u + beta_l[k] + r0);
        const T e = p_leg[k] - igj[k];
        rl[k] = o1 ? pre_k1[k] * e : r0 + dt * pre_k2[k] * (pre_k1[k] * e - r0);
        ORHAT(WS_RHAT + 6 + 3 * leg + k, rl[k]);
      }
      after_base(1);
      before_store();
      if (live) ROWV4(a.obs_integ, leg, 0, 1, 2, 3) = sel4<T>(leg, p_b[0], p_b[1], p_b[2], p_b[3]);
      if (leg < 2) if (live) ROWV(a.obs_integ, 4 + leg) = leg == 0 ? p_b[4] : p_b[5];
      if (live) ROWV4(a.obs_r, leg, 0, 1, 2, 3) = sel4<T>(leg, rb[0], rb[1], rb[2], rb[3]);
      if (leg < 2) if (live) ROWV(a.obs_r, 4 + leg) = leg == 0 ? rb[4] : rb[5];
#pragma unroll
      for (int k = 0; k < 3; ++k) { if (live) ROWV(a.obs_integ, 6 + jx[k]) = igj[k]; if (live) ROWV(a.obs_r, 6 + jx[k]) = rl[k]; }
    } else {   // (observer off in an observer kernel: not launched that way, but the QP must not wait for ever)
      ORHAT(sel4<int>(leg, WS_RHAT + 0, WS_RHAT + 1, WS_RHAT + 2, WS_RHAT + 3), (T)0);
      if (leg < 2) ORHAT(WS_RHAT + 4 + leg, (T)0);
      after_base(0);
#pragma unroll
      for (int k = 0; k < 3; ++k) ORHAT(WS_RHAT + 6 + 3 * leg + k, (T)0);
      after_base(1);
    }
  } else {
  if (prm.observer_order > 0) {
    // (SIMG: tau_prev, f_prev are the rows the previous tick's QP left in the workgroup's result image -- nothing of them is in memory before the last tick)
    const T* const rimg = SIMG ? a.resimg + (si_ - a.simg) : nullptr;
    const V3<T> fp = SIMG ? mk<T>(rimg[(RES_F + 3 * leg + 0) * 16], rimg[(RES_F + 3 * leg + 1) * 16], rimg[(RES_F + 3 * leg + 2) * 16])
                          : mk<T>(LDV(a.f_prev, 3 * leg + 0), LDV(a.f_prev, 3 * leg + 1), LDV(a.f_prev, 3 * leg + 2));
    const T dt = prm.dt;
    const bool o1 = prm.observer_order == 1;
    if constexpr (BASE) {
      const V3<T> dxf = cross(dw, fp);
      T ub[6] = {fp.x, fp.y, fp.z, dxf.x, dxf.y, dxf.z};
      xrow_sum_k<T, 6>(ub);
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const T r0 = LDU(a.obs_r, c);
        const T ig = LDU(a.obs_integ, c) + dt * (ub[c] + beta_b[c] + r0);
        const T e = p_b[c] - ig;
        rb[c] = o1 ? prm.K1[c] * e : r0 + dt * prm.K2[c] * (prm.K1[c] * e - r0);
        p_b[c] = ig;
      }
      // every lane's loads of the replicated rows feed its own store values: all loads of a row have returned in every lane
      // of the wave before any lane stores to it
      before_store();
      if (live) ROWV4(a.obs_integ, leg, 0, 1, 2, 3) = sel4<T>(leg, p_b[0], p_b[1], p_b[2], p_b[3]);
      if (leg < 2) if (live) ROWV(a.obs_integ, 4 + leg) = leg == 0 ? p_b[4] : p_b[5];
      if (live) ROWV4(a.obs_r, leg, 0, 1, 2, 3) = sel4<T>(leg, rb[0], rb[1], rb[2], rb[3]);
      if (leg < 2) if (live) ROWV(a.obs_r, 4 + leg) = leg == 0 ? rb[4] : rb[5];
    }
#pragma unroll
    for (int k = 0; k < (JOINTS ? 3 : 0); ++k) {
      const int c = 6 + jx[k];
      const T r0 = LDV(a.obs_r, c);
      const T u = (SIMG ? rimg[(RES_TAU + jx[k]) * 16] : LDV(a.tau_prev, jx[k])) + dot(jw[k], fp);
      const T ig = LDV(a.obs_integ, c) + dt * (u + beta_l[k] + r0);
      const T e = p_leg[k] - ig;
      T k1 = prm.K1[6], k2 = prm.K2[6];   // gains of joint row c by a select (no run-time index into the kernel arguments)
#pragma unroll
      for (int j = 1; j < 12; ++j) { k1 = (jx[k] == j) ? prm.K1[6 + j] : k1; k2 = (jx[k] == j) ? prm.K2[6 + j] : k2; }
      rl[k] = o1 ? k1 * e : r0 + dt * k2 * (k1 * e - r0);
      if (live) ROWV(a.obs_integ, c) = ig;
      if (live) ROWV(a.obs_r, c) = rl[k];
    }
  }
  if constexpr (BASE) {
    ORHAT(sel4<int>(leg, WS_RHAT + 0, WS_RHAT + 1, WS_RHAT + 2, WS_RHAT + 3), sel4<T>(leg, rb[0], rb[1], rb[2], rb[3]));
    if (leg < 2) ORHAT(WS_RHAT + 4 + leg, leg == 0 ? rb[4] : rb[5]);
  }
  if constexpr (JOINTS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) ORHAT(WS_RHAT + 6 + 3 * leg + k, rl[k]);
  }
  }
#undef ORHAT
}

// ======================================================================================================================
// The stand-alone kernel: the same recursion with the forward sweep's per-joint state parked in LDS (see the file header).
// Round 5: written against the lane value type V of the sweep (dyn_sweep.hip.hpp) -- T itself, or with W = 2 a packed pair of fp32 states per lane
// (whole 128-byte lines per 16-lane row, v_pk_* arithmetic, half the wavefronts) -- and with its LDS handed in by the kernel, so that it can run
// as one of the two roles of sweep_obs_kernel (below).
// ======================================================================================================================
constexpr int OBS_PKW = 11;   // parked words per joint: sin, cos, body angular / linear velocity, gravity direction
template <class T, int BLOCK, int W, bool XR = false> struct ObsLds {   // one LDS object, constant table first (see dyn_sweep.hip.hpp; XR: the table is the workgroup's, SweepLds)
  using V = typename LaneT<T, W>::type;
  T cst[XR ? 4 : CST_WORDS]; T kgain[36]; V park[3 * OBS_PKW][BLOCK];
};
template <class T, int BLOCK, int W = 1, bool XR = false>
WBC_DEV void observer_park_body(const DevModel<T>* __restrict__ model, const DevParams<T> prm, const SweepArgs<T>& a, ObsLds<T, BLOCK, W, XR>& lds, const unsigned blk,
                                const RoleShare<T> xr = RoleShare<T>()) {
  using V = typename LaneT<T, W>::type;
  constexpr int PKW = OBS_PKW;
  static_assert(!XR || BLOCK == 64, "a shared role is one wavefront");
  decltype(auto) cst = role_cst<XR>(lds, xr.cst);
  T (&kgain)[36] = lds.kgain;
  V (&park)[3 * PKW][BLOCK] = lds.park;
  unsigned tx = threadIdx.x & (unsigned)(BLOCK - 1);   // (thread within the BLOCK threads that run this body)
  asm volatile("" : "+v"(tx));   // see WBC_LAUNDERED_TID (lane_rows.hip.hpp)
  const size_t N = a.N;
  WBC_LEG_LANE(16, W, WBC_SRAW_W(BLOCK, W, blk))
  using RowV = V;
  // state loads first, table staging while they are in flight
  V qq[4], vb[6];
#pragma unroll
  for (int c = 0; c < 4; ++c) qq[c] = LDU(a.q, 3 + c);
#pragma unroll
  for (int c = 0; c < 6; ++c) vb[c] = LDU(a.v, c);
  int jx[3];
  jidx_of_leg(model, a.jpack, leg, jx);
  V ql[3], vl[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ql[k] = LDV(a.q, 7 + jx[k]);
    vl[k] = LDV(a.v, 6 + jx[k]);
  }
  // branch-free staging (clamped index, the tail lanes rewrite the last word): with a divergent staging loop here hipcc 7.2 put
  // VGPR spill stores of the fp64 build into the loop's exit block BEFORE exec is restored, i.e. with no lane enabled
  // (found by parity: rhat garbage in every state; tools/spill_lint.py scans the ISA for that pattern)
  if constexpr (XR) {
    for (int i0 = 0; i0 < CST_WORDS; i0 += xr.stage_threads) {
      const int i = min(i0 + (int)threadIdx.x, CST_WORDS - 1);
      cst[i] = model->cst[i];
    }
  } else {
#pragma unroll
    for (int i0 = 0; i0 < CST_WORDS; i0 += BLOCK) {
      const int i = min(i0 + (int)tx, CST_WORDS - 1);
      cst[i] = model->cst[i];
    }
  }
  // the gains are read from LDS: those of the joint rows are indexed by a run-time joint number, and 72 SGPRs of gains held to
  // the end of a kernel are SGPR spills
  if (tx == 0) {
#pragma unroll
    for (int i = 0; i < 18; ++i) { kgain[i] = prm.K1[i]; kgain[18 + i] = prm.K2[i]; }  // static indices only
  }
  __syncthreads();
  const int hcol = xr.col0 + (int)(tx & 15) * W;   // (XR) my first state's column of the tile
  (void)hcol;
#define ORH(comp, val) do { if constexpr (XR) *(V*)(xr.hand + ((comp) - WS_RHAT + HAND_RHAT) * xr.hs + hcol) = (val); else { if (live) ROWV(a.ws, comp) = (val); } } while (0)   /* rhat for the QP stage */

  V qx, qy, qz, qw;
  {
    const V n = rsqrt_t(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
    qx = qq[0] * n; qy = qq[1] * n; qz = qq[2] * n; qw = qq[3] * n;
  }
  // base rotation, base body inertia, base velocity / gravity in base coordinates: formed twice -- here for the forward sweep
  // and again after the return sweep, from the (laundered) quaternion and a second read of v -- so that 34 values do not live
  // through both sweeps
  auto base_state = [&](const V* vbx, M3<V>& R, V& bm, V3<V>& bh, S3<V>& bI, V3<V>& om0, V3<V>& v0, V3<V>& gneg) __attribute__((always_inline)) {
    const V x = qx, y = qy, z = qz, w = qw;
    R.a[0] = 1 - 2 * (y * y + z * z); R.a[1] = 2 * (x * y - z * w);     R.a[2] = 2 * (x * z + y * w);
    R.a[3] = 2 * (x * y + z * w);     R.a[4] = 1 - 2 * (x * x + z * z); R.a[5] = 2 * (y * z - x * w);
    R.a[6] = 2 * (x * z - y * w);     R.a[7] = 2 * (y * z + x * w);     R.a[8] = 1 - 2 * (x * x + y * y);
    bm = model->base_m;
    bh = mk<V>(model->base_h[0], model->base_h[1], model->base_h[2]);
    bI.xx = model->base_Io[0]; bI.xy = model->base_Io[1]; bI.xz = model->base_Io[2];
    bI.yy = model->base_Io[3]; bI.yz = model->base_Io[4]; bI.zz = model->base_Io[5];
    om0 = tmul(R, mk<V>(vbx[3], vbx[4], vbx[5]));
    v0 = tmul(R, mk<V>(vbx[0], vbx[1], vbx[2]));
    gneg = tmul(R, mk<V>(-model->grav[0], -model->grav[1], -model->grav[2]));   // R^T (-g)
  };
  M3<V> R;
  V bm;
  V3<V> bh, om0, v0, gneg;
  S3<V> bI;
  base_state(vb, R, bm, bh, bI, om0, v0, gneg);

  // ---- forward sweep down the leg: joint rotations, body velocities, weights.  What the return sweep needs is PARKED in LDS
  // ([word][lane], conflict-free): sin / cos of the joint angle (E is rebuilt from them: 18 FMAs on constants that are read from
  // LDS anyway) and the body's velocity and gravity direction -- 11 words per joint instead of 54 live values through both sweeps.
  auto joint_E = [&](int k, V sn, V cs, M3<V>& Ek) __attribute__((always_inline)) {
    const int o = JOINT_WORDS * k;
#pragma unroll
    for (int e = 0; e < 9; ++e) Ek.a[e] = CS(o + e) + cs * CS(o + 9 + e) + sn * CS(o + 18 + e);
  };
  {
    V3<V> omp = om0, vp = v0, gp = gneg;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int o = JOINT_WORDS * k;
      V sn, cs;
      sincos_t(ql[k], &sn, &cs);
      M3<V> Ek;
      joint_E(k, sn, cs, Ek);
      const V3<V> r = mk<V>(CS(o + 27), CS(o + 28), CS(o + 29));
      const V3<V> ax = mk<V>(CS(o + 30), CS(o + 31), CS(o + 32));
      const V3<V> omk = tmul(Ek, omp) + ax * vl[k];
      const V3<V> vvk = tmul(Ek, vp + cross(omp, r));
      const V3<V> gk = tmul(Ek, gp);
      V* pk = &park[PKW * k][tx];
      pk[0] = sn; pk[BLOCK] = cs;
      pk[BLOCK * 2] = omk.x; pk[BLOCK * 3] = omk.y; pk[BLOCK * 4] = omk.z;
      pk[BLOCK * 5] = vvk.x; pk[BLOCK * 6] = vvk.y; pk[BLOCK * 7] = vvk.z;
      pk[BLOCK * 8] = gk.x; pk[BLOCK * 9] = gk.y; pk[BLOCK * 10] = gk.z;
      omp = omk; vp = vvk; gp = gk;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // (without this the compiler keeps the forward sweep's table words in registers for the return sweep instead of reading
  // them from LDS again)
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  // The inputs of the update -- previous forces and torques, the observer state -- are requested HERE, so that they arrive
  // during the return sweep: loaded where they are used, after it, each exposed a memory latency (two wavefronts per SIMD).
  const bool obs_on = prm.observer_order > 0;
  V3<V> fp = mk<V>(0, 0, 0);
  V in_r[3] = {0, 0, 0}, in_ig[3] = {0, 0, 0}, in_tp[3] = {0, 0, 0}, in_rb[6] = {0, 0, 0, 0, 0, 0}, in_igb[6] = {0, 0, 0, 0, 0, 0};
  if (obs_on) {
    fp = mk<V>(LDV(a.f_prev, 3 * leg + 0), LDV(a.f_prev, 3 * leg + 1), LDV(a.f_prev, 3 * leg + 2));
#pragma unroll
    for (int k = 0; k < 3; ++k) { in_r[k] = LDV(a.obs_r, 6 + jx[k]); in_ig[k] = LDV(a.obs_integ, 6 + jx[k]); in_tp[k] = LDV(a.tau_prev, jx[k]); }
#pragma unroll
    for (int c = 0; c < 6; ++c) { in_rb[c] = LDU(a.obs_r, c); in_igb[c] = LDU(a.obs_integ, c); }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) vb[c] = LDU(a.v, c);   // the base velocity again, for base_state after the sweep
  // ---- return sweep: subtree momentum / weight, their projections on the joint axes, foot geometry
  V p_leg[3], beta_l[3];
  V3<V> dft = mk<V>(CS(129), CS(130), CS(131));
  V3<V> jc[3];
  SF<V> macc, gacc;
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    const int o = JOINT_WORDS * k;
    const V3<V> r = mk<V>(CS(o + 27), CS(o + 28), CS(o + 29));
    const V3<V> ax = mk<V>(CS(o + 30), CS(o + 31), CS(o + 32));
    const V m = CS(o + 33);
    const V3<V> h = mk<V>(CS(o + 34), CS(o + 35), CS(o + 36));
    S3<V> Io;
    Io.xx = CS(o + 37); Io.xy = CS(o + 38); Io.xz = CS(o + 39); Io.yy = CS(o + 40); Io.yz = CS(o + 41); Io.zz = CS(o + 42);
    const V* pk = &park[PKW * k][tx];
    M3<V> Ek;
    joint_E(k, pk[0], pk[BLOCK], Ek);
    const V3<V> omk = mk<V>(pk[BLOCK * 2], pk[BLOCK * 3], pk[BLOCK * 4]);
    const V3<V> vvk = mk<V>(pk[BLOCK * 5], pk[BLOCK * 6], pk[BLOCK * 7]);
    const V3<V> glk = mk<V>(pk[BLOCK * 8], pk[BLOCK * 9], pk[BLOCK * 10]);
    SF<V> mk_ = inertia_mul(m, h, Io, omk, vvk), gk;
    gk.n = cross(h, glk);
    gk.f = glk * m;
    if (k < 2) { mk_.n = mk_.n + macc.n; mk_.f = mk_.f + macc.f; gk.n = gk.n + gacc.n; gk.f = gk.f + gacc.f; }
    p_leg[k] = dot(ax, mk_.n);
    beta_l[k] = -dot(ax, cross(omk, mk_.n) + cross(vvk, mk_.f)) - dot(ax, gk.n);   // (C^T v)_k - g_k
    jc[k] = cross(ax, dft);
    dft = r + mul(Ek, dft);
#pragma unroll
    for (int j = k; j < 3; ++j) jc[j] = mul(Ek, jc[j]);
    macc = to_parent(Ek, r, mk_);
    gacc = to_parent(Ek, r, gk);
    // One joint at a time.  The results of the sweep only feed stores guarded by `live`, so the compiler sinks the whole
    // arithmetic into that guarded region and leaves the LDS reads of all three iterations (~160 doubles: table words and
    // parked values) in a row in front of it.  Passing the carried values through an empty asm statement pins each
    // iteration's arithmetic where it is written.
    pin(macc.n); pin(macc.f); pin(gacc.n); pin(gacc.f);
    pin(dft); pin(p_leg[k]); pin(beta_l[k]);
#pragma unroll
    for (int j = k; j < 3; ++j) pin(jc[j]);
    __builtin_amdgcn_sched_barrier(0);
  }
  // base quantities again (see base_state)
  pin(qx); pin(qy); pin(qz); pin(qw);
#pragma unroll
  for (int c = 0; c < 6; ++c) pin(vb[c]);
  base_state(vb, R, bm, bh, bI, om0, v0, gneg);

  // ---- observer update (order 1 or 2) and rhat for the QP kernel (18 words at WS_RHAT of the step workspace), in two phases:
  // the joint rows first (their inputs -- Jacobian columns, leg momenta -- die there), the base rows afterwards
  const T dt = prm.dt;
  const bool o1 = prm.observer_order == 1;
  // (pins: the loads above stay where they are issued)
  pin(fp);
#pragma unroll
  for (int k = 0; k < 3; ++k) { pin(in_r[k]); pin(in_ig[k]); pin(in_tp[k]); }
#pragma unroll
  for (int c = 0; c < 6; ++c) { pin(in_rb[c]); pin(in_igb[c]); }
  {
    V rl[3] = {0, 0, 0};
    if (obs_on) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int c = 6 + jx[k];
        const V r0 = in_r[k];
        const V u = in_tp[k] + dot(mul(R, jc[k]), fp);
        const V ig = in_ig[k] + dt * (u + beta_l[k] + r0);
        const V e = p_leg[k] - ig;
        const T k1 = kgain[c], k2 = kgain[18 + c];
        rl[k] = o1 ? k1 * e : r0 + dt * k2 * (k1 * e - r0);
        if (live) ROWV(a.obs_integ, c) = ig;
        if (live) ROWV(a.obs_r, c) = rl[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) ORH(WS_RHAT + 6 + 3 * leg + k, rl[k]);
  }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  {
    // the four legs + the base body itself
    V p_b[6], beta_b[6];
    {
      const SF<V> Iv0 = inertia_mul(bm, bh, bI, om0, v0);
      V xb[12] = {macc.n.x, macc.n.y, macc.n.z, macc.f.x, macc.f.y, macc.f.z, gacc.n.x, gacc.n.y, gacc.n.z, gacc.f.x, gacc.f.y, gacc.f.z};
      xrow_sum_k<V, 12>(xb);
      const V3<V> m0n = mk<V>(xb[0], xb[1], xb[2]) + Iv0.n, m0f = mk<V>(xb[3], xb[4], xb[5]) + Iv0.f;
      const V3<V> g0n = mk<V>(xb[6], xb[7], xb[8]) + cross(bh, gneg), g0f = mk<V>(xb[9], xb[10], xb[11]) + gneg * bm;
      const V3<V> Pl = mul(R, m0f), Pa = mul(R, m0n);
      const V3<V> gl = mul(R, g0f), ga = mul(R, g0n);
      const V3<V> cx = cross(mk<V>(vb[0], vb[1], vb[2]), Pl);
      p_b[0] = Pl.x; p_b[1] = Pl.y; p_b[2] = Pl.z; p_b[3] = Pa.x; p_b[4] = Pa.y; p_b[5] = Pa.z;
      beta_b[0] = -gl.x; beta_b[1] = -gl.y; beta_b[2] = -gl.z;
      beta_b[3] = -cx.x - ga.x; beta_b[4] = -cx.y - ga.y; beta_b[5] = -cx.z - ga.z;
    }
    V rb[6] = {0, 0, 0, 0, 0, 0};
    if (obs_on) {
      const V3<V> dxf = cross(mul(R, dft), fp);
      V ub[6] = {fp.x, fp.y, fp.z, dxf.x, dxf.y, dxf.z};
      xrow_sum_k<V, 6>(ub);
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const V r0 = in_rb[c];
        const V ig = in_igb[c] + dt * (ub[c] + beta_b[c] + r0);
        const V e = p_b[c] - ig;
        rb[c] = o1 ? kgain[c] * e : r0 + dt * kgain[18 + c] * (kgain[c] * e - r0);
        p_b[c] = ig;
      }
      // (the replicated rows were read by every lane of the wave long before any lane stores to them)
      if (live) ROWV4(a.obs_integ, leg, 0, 1, 2, 3) = sel4<V>(leg, p_b[0], p_b[1], p_b[2], p_b[3]);
      if (leg < 2) if (live) ROWV(a.obs_integ, 4 + leg) = leg == 0 ? p_b[4] : p_b[5];
      if (live) ROWV4(a.obs_r, leg, 0, 1, 2, 3) = sel4<V>(leg, rb[0], rb[1], rb[2], rb[3]);
      if (leg < 2) if (live) ROWV(a.obs_r, 4 + leg) = leg == 0 ? rb[4] : rb[5];
    }
    ORH(sel4<int>(leg, WS_RHAT + 0, WS_RHAT + 1, WS_RHAT + 2, WS_RHAT + 3), sel4<V>(leg, rb[0], rb[1], rb[2], rb[3]));
    if (leg < 2) ORH(WS_RHAT + 4 + leg, leg == 0 ? rb[4] : rb[5]);
  }
#undef ORH
}

constexpr int WBC_OBS_WAVES = 2;
template <class T, int BLOCK, int W = 1>
__global__ __launch_bounds__(BLOCK, WBC_OBS_WAVES) void observer_kernel(const DevModel<T>* __restrict__ model, DevParams<T> prm, SweepArgs<T> a) {
  __shared__ ObsLds<T, BLOCK, W> lds;
  observer_park_body<T, BLOCK, W>(model, prm, a, lds, blockIdx.x);
}

// ======================================================================================================================
// sweep_obs_kernel (round 5): the observer update and the observer-free dynamics sweep as the TWO ROLES OF ONE LAUNCH -- the first
// `nsweep` workgroups run dyn_sweep_body<SW_MATS | SW_STEP | SW_NOB>, the rest observer_park_body, on the same states.
// Why: BASELINE.json's configs[3] puts 32 768 fp32 states on each GPU.  At that size the all-in-one observer sweep is ONE packed
// wavefront per SIMD (430 registers) running a 23 us dependent chain -- 0.31 of HBM on the stage's 443 words, against north_star's 0.40 --
// and its two halves as two kernels one after the other (the large-batch form) each pay their own latency-bound round.  As roles of one
// launch both halves are resident together -- 1 024 + 1 024 packed wavefronts = two per SIMD at <= 256 registers -- and the launch lasts
// about as long as the longer of the two chains.  Only worth it while BOTH fit one round of resident wavefronts (the host picks: plan_tick).
// One-wavefront workgroups, LDS overlaid (a workgroup runs one role).
// ======================================================================================================================
template <class T, int W>
__global__ __launch_bounds__(64, 2) void sweep_obs_kernel(const DevModel<T>* __restrict__ model, DevParams<T> prm, SweepArgs<T> a, unsigned nsweep) {
  constexpr int MODE = SW_MATS | SW_STEP | SW_NOB;
  union Lds {
    SweepLds<T, MODE, 64, W> sw;
    ObsLds<T, 64, W> ob;
    __device__ Lds() {}
  };
  __shared__ Lds lds;
  if (a.qp_todo && blockIdx.x == 0 && threadIdx.x == 0) a.qp_todo[0] = 0;
#ifdef WBC_SO_STAMP   // diagnostic build (tools/so_stamp.py): role, 100 MHz wall clock at entry / exit and the hardware slot of every workgroup, in place of pf
  unsigned* const so_stamp = (unsigned*)a.pf;
  a.pf = nullptr;
  const long long so_t0 = wall_clock64();
#endif
  // -DWBC_SWEEP_OBS_PRIO=1: the sweep role (the longer chain: ~16 us alone against ~12) at a higher issue priority than the observer role it shares SIMDs with
  if (blockIdx.x < nsweep) {
    dyn_sweep_body<T, MODE, 64, W>(model, prm, a, lds.sw, blockIdx.x);
  } else observer_park_body<T, 64, W>(model, prm, a, lds.ob, blockIdx.x - nsweep);
#ifdef WBC_SO_STAMP
  if (so_stamp && threadIdx.x == 0) {
    const long long so_t1 = wall_clock64();
    unsigned* o = so_stamp + (size_t)blockIdx.x * 8;
    o[0] = blockIdx.x < nsweep ? 0u : 1u; o[1] = (unsigned)so_t0; o[2] = (unsigned)so_t1;
    o[3] = __builtin_amdgcn_s_getreg((31 << 11) | 4);      // HW_ID
    o[4] = __builtin_amdgcn_s_getreg((31 << 11) | 20);     // XCC_ID
  }
#endif
}

}  // namespace wbc
