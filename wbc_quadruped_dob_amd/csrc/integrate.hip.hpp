// Forward dynamics with the planned GRFs + semi-implicit Euler: SURVEY.md 8(f)-1, the step Gazebo performs in the
// reference loop (/root/reference/README.md:58), restated as the simplest model that closes the loop for rollouts:
//     vdot = M^-1 (S^T tau + Jc^T f + tau_ext - h),   v += dt vdot,   q <- q (+) dt v   (world-frame omega)
//
// Same lane mapping as the dynamics sweep (lane = 16*leg + state; one leg per 16-lane row).  The quadruped's mass
// matrix is an arrow: a 6x6 base block, four 6x3 base-leg blocks and four independent 3x3 leg blocks.  Each lane
// inverts ITS leg block in closed form, forms its part of the base Schur complement (21 + 6 words summed across
// the four rows with v_permlane16/32_swap), every lane solves the 6x6 base system redundantly in registers, and
// back-substitutes its own leg.  M, h, Jc come from the buffers the sweep wrote (foot lever arms = the base-angular
// columns of Jc, own-leg Jacobian blocks = its joint columns).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "device_types.hpp"
#include "dyn_sweep.hip.hpp"
#include "score.hip.hpp"

namespace wbc {

// (SCORE, scored persistent rollout) what phase 2 needs to add this tick's cost: the call's ScoreArgs (a kernel argument) and the workgroup's LDS words --
// the weights, goals [GOAL_WORDS][16], the running cost and failed ticks per lane of the integrator wavefront, this tick's status per state
// where the sums go behind the last tick, parked in LDS by the kernel's prologue: held as kernel arguments they stay live through every role of every tick
template <class T> struct ScoreOut { T* cost; int* fail; int accumulate; };
template <class T> struct ScoreTick {
  const ScoreOut<T>* out;
  const DevScoreW<T>* w;   // the weights, in LDS
  const T* goal; T* run; int* nfail; const int* stat;
  bool first, last;   // tick 0 / the launch's last tick (wavefront-uniform)
};

// ---- plant payload (wbc_integrate_plant_batch, wbc_rollout_plant_batch, wbc_rollout_tracking_plant_batch)
// A rigid body fixed to the trunk: p = [m, c (3, base frame), I about c (6, base axes: xx yy zz xy xz yz)], [PAYLOAD_WORDS][N] in memory.
// It moves with the base and with no joint, so it changes only the 6x6 base block of M and the 6 base rows of h -- exactly.  In the mixed
// representation (v = [pdot world, omega world, qdot]; base rows = force in world, moment about the base origin in world), with r = R c,
// I_w = R I R^T and g the model's gravity:
//   dM_bb = [[m 1, -m[r]x], [m[r]x, I_w - m[r]x[r]x]]
//   dh_b  = [f; r x f + w x (I_w w)],   f = m w x (w x r) - m g
// dM: upper triangle of the 6x6 block, row-major (21 words); dh: 6 words.  Unused outputs cost nothing (the body is inlined).
constexpr int PAYLOAD_WORDS = 10;
template <class T>
WBC_DEV void payload_terms(const T (&R)[9], V3<T> om, const T (&p)[PAYLOAD_WORDS], const T* __restrict__ grav, T (&dM)[21], T (&dh)[6]) {
  const T m = p[0];
  const V3<T> r = mk<T>(R[0] * p[1] + R[1] * p[2] + R[2] * p[3], R[3] * p[1] + R[4] * p[2] + R[5] * p[3], R[6] * p[1] + R[7] * p[2] + R[8] * p[3]);
  // I_w = R I R^T: B = R I (I symmetric), then I_w[i][j] = B[i] . R[j]
  const T Ib[9] = {p[4], p[7], p[8], p[7], p[5], p[9], p[8], p[9], p[6]};
  T B[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) B[3 * i + j] = R[3 * i] * Ib[j] + R[3 * i + 1] * Ib[3 + j] + R[3 * i + 2] * Ib[6 + j];
  auto iw = [&](int i, int j) { return B[3 * i] * R[3 * j] + B[3 * i + 1] * R[3 * j + 1] + B[3 * i + 2] * R[3 * j + 2]; };
  const T Wxx = iw(0, 0), Wxy = iw(0, 1), Wxz = iw(0, 2), Wyy = iw(1, 1), Wyz = iw(1, 2), Wzz = iw(2, 2);
  const V3<T> h = r * m;   // first moment about the base origin
  const T Z = (T)0;
  // rows 0 .. 2: [m 1, -[h]x]
  dM[0] = m; dM[1] = Z; dM[2] = Z; dM[3] = Z;    dM[4] = h.z;  dM[5] = -h.y;
  dM[6] = m; dM[7] = Z; dM[8] = -h.z;            dM[9] = Z;    dM[10] = h.x;
  dM[11] = m; dM[12] = h.y; dM[13] = -h.x;       dM[14] = Z;
  // rows 3 .. 5: I_w - m[r]x[r]x = I_w + m (|r|^2 1 - r r^T)
  dM[15] = Wxx + (h.y * r.y + h.z * r.z); dM[16] = Wxy - h.x * r.y; dM[17] = Wxz - h.x * r.z;
  dM[18] = Wyy + (h.x * r.x + h.z * r.z); dM[19] = Wyz - h.y * r.z;
  dM[20] = Wzz + (h.x * r.x + h.y * r.y);
  const V3<T> f = cross(om, cross(om, r)) * m - mk<T>(grav[0], grav[1], grav[2]) * m;
  const V3<T> Lw = mk<T>(Wxx * om.x + Wxy * om.y + Wxz * om.z, Wxy * om.x + Wyy * om.y + Wyz * om.z, Wxz * om.x + Wyz * om.y + Wzz * om.z);
  const V3<T> n = cross(r, f) + cross(om, Lw);
  dh[0] = f.x; dh[1] = f.y; dh[2] = f.z; dh[3] = n.x; dh[4] = n.y; dh[5] = n.z;
}
// R of a unit quaternion (x, y, z, w), row-major (as MAKE_R, dyn_sweep.hip.hpp)
template <class T> WBC_DEV void quat_to_R(T x, T y, T z, T w, T (&R)[9]) {
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
}
// the argument struct of the payload kernels: IntegrateArgs + the payload (the kernels without it keep their argument layout)
template <class T> struct PlantIntegrateArgs : IntegrateArgs<T> { const T* payload; };
template <class T, bool PAYLOAD> using IntegrateArgsP = typename std::conditional<PAYLOAD, PlantIntegrateArgs<T>, IntegrateArgs<T>>::type;

// (also called as one wavefront of the persistent rollout kernel, fused_tick.hip.hpp: same mapping, no LDS.)
// Two phases.  Phase 1 needs only M and Jc: the leg blocks' inverses, the base Schur complement and its Cholesky factor.
// `between()` runs after it (nothing in the stand-alone kernel; the tick barrier in the rollout kernel, where phase 1
// overlaps the QP).  Phase 2 needs tau, f, h, q, v: right-hand sides, the two triangular solves, the state update.
struct IntegrateNoWait { WBC_DEV void operator()() const {} };
// `hand` (persistent rollout): M's leg / base-leg / base blocks, the own-leg Jacobian block and the lever arm come from the LDS image
// the mass_jac role left (dyn_split.hip.hpp, MJ_HAND_WORDS) instead of from the M / Jc buffers through L2 -- same numbers, so the
// results are bit-identical; what changes is when phase 1 can start and how long its operands take to arrive.
// `res` (persistent rollout, round 5): this tick's tau (rows 0 .. 11), f (12 .. 23), h (24 .. 41) in an LDS image [42][16] written by the QP wavefronts and
// the rnea role: phase 2 starts behind an LDS-only barrier instead of behind the acknowledgement of their global stores and a trip through L2.
// PHASE (persistent rollout, round 5): 0 = both phases on this wavefront.  1 = phase 1 ONLY, run by the mass_jac wavefront itself right behind its
// image (no flag, no second wavefront waiting for it), leaving the leg block's inverse (6 words) and the base factor (21) in the LDS image
// fact[27][64]; 2 = phase 2 only, on the integrator wavefront: state loads, the tick barrier, then M's blocks from `hand` and the factors from `fact`.
// The integrator wavefront used to run the observer's joint rows, THEN phase 1, and arrived last at the tick barrier (+10.3 us; profiles/r05f_*).
constexpr int INT_FACT_WORDS = 27;
// UNGUARD (persistent rollout): the state stores carry no `if (live)`.  Lanes beyond the batch or beyond the workgroup's states recompute a state of THEIR OWN
// wavefront (the workgroup's first, or the batch's last, which the last workgroup owns), in lockstep with the lane that owns it: what they store is a
// bit-identical duplicate at the same address, and every one of the 22 guards was an exec region of ~45 cycles in the one phase of a rollout tick during
// which nothing else runs (knock-out analysis: profiles/r05h_ro_knock.log).  Not for the stand-alone kernel: there a dead lane may sit in another wavefront.
// WBC_INT_SINV: 1 = phase 1 (which runs beside the QP: hidden) ends with the explicit inverse of the base Schur complement, and phase 2 multiplies by it --
// 36 independent multiply-adds instead of two triangular solves of 54 dependent operations at 13 cycles each for a lone wavefront; 0 (default) = the solves.
// measured (profiles/r05i_ab_rollout_phase2_*.log): 12.05 -> 12.22 us per tick in fp64, and the fp32 inverse loses the accuracy the
// fp32 rollout tests ask for (NaN on stiff states): not kept
// HAND / RESI: `hand` / `res` are given (template parameters, not null tests: a pointer that may be an LDS image or null turns every load behind it into a
// flat_load -- 39 of them in the round-4 rollout kernels, 30 in phase 2 -- where the image wants a ds_read).
// `after_state()` (4-state rollout workgroups): called when the new state is complete in the LDS image and before anything goes to memory -- the kernel
// can put the tick's barrier there, so that the next tick's roles start while this wavefront (the next tick's QP, idle until the lever arms are out)
// still issues its stores.  Measured (profiles/r05q_ab_rollout_early_barrier.log): 9.39-9.47 -> 9.48-9.52 us per tick at 1 024 robots, cold 15.71 -> 15.97:
// not kept (-DWBC_RO_EARLY_BARRIER=1).
// PAYLOAD (plant model mismatch, `payload` = [PAYLOAD_WORDS][N]): phase 1 adds dM_bb to the base block (with HAND: one more body in the composite
// (m, R h, R I R^T) before the block is rebuilt), phase 2 subtracts dh_b from the base right-hand side.  false: the code of rounds 1-6, unchanged.
// GROUND (ground-contact plant, ground.hip.hpp): this lane's foot force is `fground`, a register value the caller has just computed from the contact law,
// instead of rows 3 leg .. 3 leg + 2 of a.f, which is not read.  false: the code as it was.
template <class T, int SPW = 16, class Between = IntegrateNoWait, int PHASE = 0, bool UNGUARD = false, bool HAND = false, bool RESI = false,
          class AfterState = IntegrateNoWait, bool SIMG_ = false, bool PAYLOAD = false, bool SCORE = false, bool GROUND = false>
WBC_DEV void integrate_body(const DevModel<T>* __restrict__ model, const IntegrateArgs<T>& a, Between between = Between(), const T* hand_ = nullptr,
                            const T* res_ = nullptr, T* fact = nullptr, AfterState after_state = AfterState(), const T* payload = nullptr,
                            const ScoreTick<T>* sc = nullptr, V3<T> fground = V3<T>()) {
  static_assert(PHASE == 0 || PHASE == 1 || PHASE == 2, "phase");
  static_assert(!GROUND || (PHASE == 0 && !RESI), "the ground plant is the stand-alone kernel");
  static_assert(!SCORE || (PHASE == 2 && RESI && SIMG_), "the cost is accumulated in phase 2 of the persistent rollout");
  static_assert(PHASE == 0 || HAND, "the split phases hand M's blocks over in LDS");
  constexpr bool FASTR = PHASE != 0 && SIMG_;   // (rollout workgroups with the state image) rsqrt_fast, see dyn_sweep.hip.hpp
  const T* const hand = HAND ? hand_ : nullptr;
  const T* const res = RESI ? res_ : nullptr;
  const size_t N = a.N;
  WBC_LAUNDERED_TID(tx);
  WBC_LEG_LANE(SPW, 1, WBC_SRAW_A(SPW))   // (SPW <= 16 states per workgroup: lane_rows.hip.hpp)
  using RowV = T;
  int jx[3];
  jidx_of_leg(model, a.jpack, leg, jx);
#ifdef WBC_FUSED_STAMP
#define ISTAMP(slot) do { if (a.istamp && SPW < 16 && (tx & 63) == 0) a.istamp[(size_t)(slot) * a.istampN + (size_t)blockIdx.x * SPW + 1] = (double)wall_clock64(); } while (0)
#else
#define ISTAMP(slot) do {} while (0)
#endif
  ISTAMP(0);

  // ================================================================== phase 1: M, Jc only
  const T* hl = HAND ? hand + (int)(tx & 63) : nullptr;
  T* const fl_ = PHASE != 0 ? fact + (int)(tx & 63) : nullptr;
  V3<T> dl;
  T jcl[3][3];   // own-leg Jacobian block: jcl[m][k] = d pf_m / d q_(leg, k)
  T Mb[6][3];    // base-leg block (6x3) of M
  T A[3][3];     // inverse of the leg block
  T L[6][6];     // Cholesky factor of the base Schur complement (L[j][j] holds 1 / L_jj)
  auto load_blocks = [&]() __attribute__((always_inline)) {
    // foot position relative to the base origin from the base-angular block of my foot's Jacobian rows, -[d]x
    dl = HAND ? mk<T>(hl[33 * 64], hl[34 * 64], hl[35 * 64])
              : mk<T>(LDL(a.Jc, 18 * 1 + 5, 54), LDL(a.Jc, 18 * 2 + 3, 54), LDL(a.Jc, 18 * 0 + 4, 54));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const unsigned jo = (unsigned)(6 + jx[k]) * N32;   // column of joint (leg, k) in rows 3*leg + m of Jc
      if constexpr (HAND) { jcl[0][k] = hl[(24 + k) * 64]; jcl[1][k] = hl[(27 + k) * 64]; jcl[2][k] = hl[(30 + k) * 64]; }
      else { jcl[0][k] = LDLX(a.Jc, 0, 54, jo); jcl[1][k] = LDLX(a.Jc, 18, 54, jo); jcl[2][k] = LDLX(a.Jc, 36, 54, jo); }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) Mb[r][k] = HAND ? hl[(6 + 3 * r + k) * 64] : LDV(a.M, midx18(r, r) + (6 + jx[k] - r));
  };
  T dhp[6];   // (PAYLOAD) dh_b; the stand-alone kernel (PHASE 0) forms it in phase 1 beside dM_bb from the same loads and rotation (one payload_terms
              // per state, not one per phase); the split phases of the persistent rollout form it in phase 2
  if constexpr (PHASE != 2) {
  load_blocks();
  // leg block (symmetric 3x3) of M
  auto mi = [](int i, int j) { if (i > j) { const int t = i; i = j; j = t; } return i * 18 - i * (i - 1) / 2 + (j - i); };
  T Ml[3][3];
#pragma unroll
  for (int k1 = 0; k1 < 3; ++k1)
#pragma unroll
    for (int k2 = k1; k2 < 3; ++k2) {
      Ml[k1][k2] = HAND ? hl[(k1 * 3 - k1 * (k1 - 1) / 2 + (k2 - k1)) * 64] : LDV(a.M, mi(6 + jx[k1], 6 + jx[k2]));
      Ml[k2][k1] = Ml[k1][k2];
    }
  // base block of M (upper triangle): from the buffer, or rebuilt from (m, R h, R I R^T) of the hand-over image
  T Mbb[6][6];
  if constexpr (!HAND) {
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) Mbb[r][c] = LDU(a.M, midx18(r, c));
  }
  // (PAYLOAD) the payload's share of the base block, dM_bb, from the state's attitude: the unit quaternion from the state image (persistent rollout)
  // or from memory, the payload's 10 words from memory (L2: the whole array is 80 bytes per state)
  T dM[21];
  if constexpr (PAYLOAD) {
    T pw[PAYLOAD_WORDS];
#pragma unroll
    for (int k = 0; k < PAYLOAD_WORDS; ++k) pw[k] = LDU(payload, k);
    const T* const sq = SIMG_ ? a.simg + (int)(s32 - (unsigned)((size_t)blockIdx.x * SPW)) : nullptr;
    T qx, qy, qz, qw;
    if constexpr (SIMG_) { qx = sq[3 * 16]; qy = sq[4 * 16]; qz = sq[5 * 16]; qw = sq[6 * 16]; }
    else { qx = LDU(a.q, 3); qy = LDU(a.q, 4); qz = LDU(a.q, 5); qw = LDU(a.q, 6); }
    const T n = rsqrt_sel<FASTR>(qx * qx + qy * qy + qz * qz + qw * qw);
    T R[9], dh[6];
    quat_to_R<T>(qx * n, qy * n, qz * n, qw * n, R);
    const V3<T> om = PHASE == 0 ? mk<T>(LDU(a.v, 3), LDU(a.v, 4), LDU(a.v, 5)) : mk<T>((T)0, (T)0, (T)0);
    payload_terms<T>(R, om, pw, model->grav, dM, PHASE == 0 ? dhp : dh);
  }
  if constexpr (HAND) {
    T tm = hl[36 * 64], hx = hl[37 * 64], hy = hl[38 * 64], hz = hl[39 * 64];
    T I33 = hl[40 * 64], I34 = hl[41 * 64], I35 = hl[42 * 64], I44 = hl[43 * 64], I45 = hl[44 * 64], I55 = hl[45 * 64];
    if constexpr (PAYLOAD) {   // one more rigid body in the composite (m, R h, R I R^T)
      tm += dM[0]; hx += dM[10]; hy += dM[12]; hz += dM[4];
      I33 += dM[15]; I34 += dM[16]; I35 += dM[17]; I44 += dM[18]; I45 += dM[19]; I55 += dM[20];
    }
    const T Z = (T)0;
    Mbb[0][0] = tm; Mbb[0][1] = Z; Mbb[0][2] = Z; Mbb[0][3] = Z; Mbb[0][4] = hz; Mbb[0][5] = -hy;
    Mbb[1][1] = tm; Mbb[1][2] = Z; Mbb[1][3] = -hz; Mbb[1][4] = Z; Mbb[1][5] = hx;
    Mbb[2][2] = tm; Mbb[2][3] = hy; Mbb[2][4] = -hx; Mbb[2][5] = Z;
    Mbb[3][3] = I33; Mbb[3][4] = I34; Mbb[3][5] = I35; Mbb[4][4] = I44; Mbb[4][5] = I45; Mbb[5][5] = I55;
  } else if constexpr (PAYLOAD) {
#pragma unroll
    for (int r = 0, i = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c, ++i) Mbb[r][c] += dM[i];
  }
  ISTAMP(1);   // image read requested
  // A = Ml^-1 by cofactors (SPD 3x3)
  {
    const T c00 = Ml[1][1] * Ml[2][2] - Ml[1][2] * Ml[1][2];
    const T c01 = Ml[0][2] * Ml[1][2] - Ml[0][1] * Ml[2][2];
    const T c02 = Ml[0][1] * Ml[1][2] - Ml[0][2] * Ml[1][1];
    const T c11 = Ml[0][0] * Ml[2][2] - Ml[0][2] * Ml[0][2];
    const T c12 = Ml[0][1] * Ml[0][2] - Ml[0][0] * Ml[1][2];
    const T c22 = Ml[0][0] * Ml[1][1] - Ml[0][1] * Ml[0][1];
    const T idet = (T)1 / (Ml[0][0] * c00 + Ml[0][1] * c01 + Ml[0][2] * c02);
    A[0][0] = c00 * idet; A[0][1] = A[1][0] = c01 * idet; A[0][2] = A[2][0] = c02 * idet;
    A[1][1] = c11 * idet; A[1][2] = A[2][1] = c12 * idet; A[2][2] = c22 * idet;
  }
  ISTAMP(2);   // leg block inverted
  // base Schur complement S = Mbb - sum_legs W Mb^T with W = Mb A (6x3), one row of W at a time
  T S[6][6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    T Wr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) Wr[k] = Mb[r][0] * A[0][k] + Mb[r][1] * A[1][k] + Mb[r][2] * A[2][k];
#pragma unroll
    for (int c = r; c < 6; ++c) {
      const T sc = Wr[0] * Mb[c][0] + Wr[1] * Mb[c][1] + Wr[2] * Mb[c][2];
      S[r][c] = Mbb[r][c] - xrow_sum(sc);
    }
  }
  ISTAMP(3);   // Schur complement summed over the legs
  // Cholesky of S (L[j][j] holds 1 / L_jj), in registers
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    T d = S[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    const T inv = rsqrt_sel<FASTR>(d);
    L[j][j] = inv;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      T sij = S[j][i];
#pragma unroll
      for (int k = 0; k < j; ++k) sij -= L[i][k] * L[j][k];
      L[i][j] = sij * inv;
    }
  }

  if constexpr (PHASE == 1) {   // hand the factors to the integrator wavefront (which reads them behind the tick barrier) and return
    fl_[0 * 64] = A[0][0]; fl_[1 * 64] = A[0][1]; fl_[2 * 64] = A[0][2]; fl_[3 * 64] = A[1][1]; fl_[4 * 64] = A[1][2]; fl_[5 * 64] = A[2][2];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) fl_[(6 + i * (i + 1) / 2 + j) * 64] = L[i][j];
    return;
  }
  }   // PHASE != 2
  ISTAMP(4);   // Cholesky done
  // the state of this tick (q, v: inputs of the tick, untouched until the stores at the end) is requested BEFORE the tick barrier: the loads
  // complete while the wavefront waits there instead of after it
  // (4-state rollout workgroups, WBC_RO_MERGE: the state lives in the workgroup's LDS image -- device_types.hpp, SIMG_* -- and the new one goes to both)
  constexpr bool SIMG = PHASE == 2 && SIMG_;
  T* const si_ = SIMG ? a.simg + (int)(s32 - (unsigned)((size_t)blockIdx.x * SPW)) : nullptr;
#define STS(comp, val) do { if constexpr (SIMG) si_[(comp) * 16] = (val); } while (0)
  constexpr bool DEFER = SIMG && !std::is_same<AfterState, IntegrateNoWait>::value;   // (see after_state)
  const bool to_mem = !(SIMG && a.skip_state != 0);   // (wavefront-uniform: a kernel argument) the state in memory is read by nobody before the launch ends
  T ql[3], vl[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { ql[k] = SIMG ? si_[(7 + jx[k]) * 16] : LDV(a.q, 7 + jx[k]); vl[k] = SIMG ? si_[(SIMG_V + 6 + jx[k]) * 16] : LDV(a.v, 6 + jx[k]); }
  T vb0[6], qb[7];
#pragma unroll
  for (int c = 0; c < 6; ++c) vb0[c] = SIMG ? si_[(SIMG_V + c) * 16] : LDU(a.v, c);
#pragma unroll
  for (int c = 0; c < 7; ++c) qb[c] = SIMG ? si_[c * 16] : LDU(a.q, c);

  // (so is the unit quaternion of the state: a square root and a division of ~0.2 us for a lone wavefront, which used to sit behind the barrier)
  // Three shortenings of phase 2 (round 5), each 1 = fp32 only (default), 2 = both scalar types, 0 = off.  Measured at 1 024 rollouts
  // (profiles/r05n_ab_rollout_phase2.log): fp32 10.08 -> 9.82 us per tick with all three; fp64 11.57 -> 11.75 / 11.68 / 11.88 as they are added -- the fp64
  // rollout kernel sits at its 256 registers and each of them moves spill code INTO this phase (ISA: 11 scratch loads behind the barrier), so fp64 keeps
  // the forms of rounds 1-4.
// W rl = Mb (A rl) instead of forming W = Mb A again behind the barrier
// the quaternion increment from its power series (below)
// the state's unit quaternion (a square root and a division) in front of the barrier
  constexpr bool ARL = (sizeof(T) == 4);
  constexpr bool QUAT_SERIES = (sizeof(T) == 4);
  constexpr bool QNORM_EARLY = (sizeof(T) == 4);
  T ux, uy, uz, uw;
  if constexpr (QNORM_EARLY) {
    const T n = rsqrt_sel<FASTR>(qb[3] * qb[3] + qb[4] * qb[4] + qb[5] * qb[5] + qb[6] * qb[6]);
    ux = qb[3] * n; uy = qb[4] * n; uz = qb[5] * n; uw = qb[6] * n;
  }

  between();
  if constexpr (!QNORM_EARLY) {
    const T n = rsqrt_sel<FASTR>(qb[3] * qb[3] + qb[4] * qb[4] + qb[5] * qb[5] + qb[6] * qb[6]);
    ux = qb[3] * n; uy = qb[4] * n; uz = qb[5] * n; uw = qb[6] * n;
  }
  ISTAMP(5);   // barrier passed
  // (the image is indexed by the slot of the state a lane COMPUTES: a lane beyond the workgroup's states duplicates state s32, and with UNGUARD it stores)
  const T* rs = RESI ? res + (int)(s32 - (unsigned)((size_t)blockIdx.x * SPW)) : nullptr;
  if constexpr (PHASE == 2) {   // M's blocks from the mass_jac role's image, the factors from the image phase 1 left (both complete behind the barrier)
    load_blocks();
    A[0][0] = fl_[0 * 64]; A[0][1] = A[1][0] = fl_[1 * 64]; A[0][2] = A[2][0] = fl_[2 * 64]; A[1][1] = fl_[3 * 64]; A[1][2] = A[2][1] = fl_[4 * 64]; A[2][2] = fl_[5 * 64];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) L[i][j] = fl_[(6 + i * (i + 1) / 2 + j) * 64];
  }
  // the external torques: rows RES_WORDS .. RES_WORDS + 17 of the image hold them for the whole launch (parked once by the rollout kernel: fetched per
  // tick in front of the barrier they cost 18 registers across it -- and scratch), or the caller's buffer
  auto text = [&](int comp) __attribute__((always_inline)) -> T { if constexpr (RESI) return rs[(42 + comp) * 16]; else return a.tau_ext ? LDV(a.tau_ext, comp) : (T)0; };

  // ================================================================== phase 2: tau, f, h, q, v
  // ---- my leg: rhs_l = tau_l + JcL^T f_l + tau_ext_l - h_l
  const V3<T> fl = GROUND ? fground
                 : RESI ? mk<T>(rs[(12 + 3 * leg + 0) * 16], rs[(12 + 3 * leg + 1) * 16], rs[(12 + 3 * leg + 2) * 16])
                        : mk<T>(LDL(a.f, 0, 3), LDL(a.f, 1, 3), LDL(a.f, 2, 3));
  T rl[3], taul[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    taul[k] = RESI ? rs[jx[k] * 16] : LDV(a.tau, jx[k]);
    const T hl_k = RESI ? rs[(24 + 6 + jx[k]) * 16] : LDV(a.h, 6 + jx[k]);
    rl[k] = taul[k] + jcl[0][k] * fl.x + jcl[1][k] * fl.y + jcl[2][k] * fl.z - hl_k + text(6 + jx[k]);
  }
  ISTAMP(6);   // tau, f, h arrived: leg right-hand side
  // ---- base right-hand side rb = rhs_b - sum_legs W rl  (PAYLOAD: - dh_b at the state's attitude and angular velocity)
  if constexpr (PAYLOAD && PHASE != 0) {
    T pw2[PAYLOAD_WORDS];
#pragma unroll
    for (int k = 0; k < PAYLOAD_WORDS; ++k) pw2[k] = LDU(payload, k);
    T R[9], dMp[21];
    quat_to_R<T>(ux, uy, uz, uw, R);
    payload_terms<T>(R, mk<T>(vb0[3], vb0[4], vb0[5]), pw2, model->grav, dMp, dhp);
  }
  T rb[6];
  {
    const V3<T> mo = cross(dl, fl);
    const T own[6] = {fl.x, fl.y, fl.z, mo.x, mo.y, mo.z};
    T ul[3];   // W rl = Mb (A rl): 27 multiply-adds behind the barrier instead of the 72 of forming W = Mb A again
#pragma unroll
    for (int k = 0; k < 3; ++k) ul[k] = A[k][0] * rl[0] + A[k][1] * rl[1] + A[k][2] * rl[2];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      T part;
      if constexpr (ARL) part = own[r] - (Mb[r][0] * ul[0] + Mb[r][1] * ul[1] + Mb[r][2] * ul[2]);
      else {
        T Wr[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) Wr[k] = Mb[r][0] * A[0][k] + Mb[r][1] * A[1][k] + Mb[r][2] * A[2][k];
        part = own[r] - (Wr[0] * rl[0] + Wr[1] * rl[1] + Wr[2] * rl[2]);
      }
      rb[r] = xrow_sum(part) - (RESI ? rs[(24 + r) * 16] : LDU(a.h, r)) + text(r);
      if constexpr (PAYLOAD) rb[r] -= dhp[r];
    }
  }
  ISTAMP(7);   // base right-hand side summed
  // ---- base accelerations: S vb = rb
  T vb[6];
  {
    T y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      T sy = rb[i];
#pragma unroll
      for (int k = 0; k < i; ++k) sy -= L[i][k] * y[k];
      y[i] = sy * L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      T sx = y[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) sx -= L[k][i] * vb[k];
      vb[i] = sx * L[i][i];
    }
  }
  ISTAMP(8);   // solves done
  // ---- leg accelerations: vdl = A (rl - Mb^T vb)
  T tl[3], vdl[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    T t = rl[k];
#pragma unroll
    for (int r = 0; r < 6; ++r) t -= Mb[r][k] * vb[r];
    tl[k] = t;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) vdl[k] = A[k][0] * tl[0] + A[k][1] * tl[1] + A[k][2] * tl[2];

  // ---- semi-implicit Euler
  const T dt = a.dt;
  T vjn[3], qjn[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    vjn[k] = vl[k] + dt * vdl[k];
    qjn[k] = ql[k] + dt * vjn[k];
    STS(SIMG_V + 6 + jx[k], vjn[k]);
    STS(7 + jx[k], qjn[k]);
    if constexpr (!DEFER) {
      if (to_mem) {
        if (UNGUARD || live) ROWV(a.v, 6 + jx[k]) = vjn[k];
        if (UNGUARD || live) ROWV(a.q, 7 + jx[k]) = qjn[k];
      }
      if (a.tau_traj) if (UNGUARD || live) ROWV(a.tau_traj, jx[k]) = taul[k];
    }
  }
  ISTAMP(9);   // joint rows stored
  T vbn[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) vbn[c] = vb0[c] + dt * vb[c];
  T qn[7];
#pragma unroll
  for (int c = 0; c < 3; ++c) qn[c] = qb[c] + dt * vbn[c];
  {
    // q <- dq(omega dt) * q with dq = [sin(th/2) / th * w ; cos(th/2)], w = omega dt, th = |w|.  Both factors are even power series in th: with
    // u = th^2 / 4 <= 1/16 (half a radian per step) seven terms carry them to below 1e-19 -- no square root, no division, no argument reduction, which
    // together were ~1 us of the 3 us a rollout tick spends in this phase alone (profiles/r05g_rollout_timeline_spw4.txt).  Beyond that the closed form,
    // selected per lane: what a state gets does not depend on its neighbours.
    const T wx = vbn[3] * dt, wy = vbn[4] * dt, wz = vbn[5] * dt;
    const T th2 = wx * wx + wy * wy + wz * wz;
    const T u = th2 * (T)0.25;
    T sc = (T)(1.0 / 6227020800.0), dw = (T)(1.0 / 479001600.0);
    sc = sc * u - (T)(1.0 / 39916800.0); dw = dw * u - (T)(1.0 / 3628800.0);
    sc = sc * u + (T)(1.0 / 362880.0);   dw = dw * u + (T)(1.0 / 40320.0);
    sc = sc * u - (T)(1.0 / 5040.0);     dw = dw * u - (T)(1.0 / 720.0);
    sc = sc * u + (T)(1.0 / 120.0);      dw = dw * u + (T)(1.0 / 24.0);
    sc = sc * u - (T)(1.0 / 6.0);        dw = dw * u - (T)0.5;
    sc = sc * u + (T)1;                  dw = dw * u + (T)1;
    sc = sc * (T)0.5;
    const bool big = QUAT_SERIES ? !(u <= (T)0.0625) : true;
    if (!QUAT_SERIES || __ballot(big) != 0) {   // the closed form (with its own two-term series next to th = 0, as in rounds 1-4)
      const T th = th2 > (T)0 ? th2 * rsqrt_sel<FASTR>(th2) : (T)0;
      T sn, cs;
      sincos_t(th * (T)0.5, &sn, &cs);
      const bool small = th <= (T)1e-8;
      const T sc_c = small ? (T)0.5 - th2 * (T)(1.0 / 48.0) : sn / (small ? (T)1 : th);
      const T dw_c = small ? (T)1 - th2 * (T)0.125 : cs;
      sc = big ? sc_c : sc;
      dw = big ? dw_c : dw;
    }
    const T dx = sc * wx, dy = sc * wy, dz = sc * wz;
    const T x = ux, y = uy, z = uz, w = uw;
    qn[3] = dw * x + dx * w + dy * z - dz * y;
    qn[4] = dw * y - dx * z + dy * w + dz * x;
    qn[5] = dw * z + dx * y - dy * x + dz * w;
    qn[6] = dw * w - dx * x - dy * y - dz * z;
  }
  // the 13 base words are replicated over the four leg rows: every row stores its share.  All rows have read
  // q/v base rows above (their values feed these stores), so no lane can store before every lane has loaded.
  ISTAMP(10);   // quaternion advanced
  if constexpr (SIMG) {   // (every row holds all 13 base words: row `leg` writes its share, as to memory)
    STS(SIMG_V + sel4<int>(leg, 0, 1, 2, 3), sel4<T>(leg, vbn[0], vbn[1], vbn[2], vbn[3]));
    if (leg < 2) STS(SIMG_V + 4 + leg, leg == 0 ? vbn[4] : vbn[5]);
    STS(sel4<int>(leg, 0, 1, 2, 3), sel4<T>(leg, qn[0], qn[1], qn[2], qn[3]));
    if (leg < 3) STS(4 + leg, sel4<T>(leg, qn[4], qn[5], qn[6], qn[6]));
  }
  if constexpr (DEFER) {
    after_state();   // the image is complete: memory comes behind
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (to_mem) {
        if (UNGUARD || live) ROWV(a.v, 6 + jx[k]) = vjn[k];
        if (UNGUARD || live) ROWV(a.q, 7 + jx[k]) = qjn[k];
      }
      if (a.tau_traj) if (UNGUARD || live) ROWV(a.tau_traj, jx[k]) = taul[k];
    }
  }
  if (to_mem) {
    if (UNGUARD || live) ROWV(a.v, sel4<int>(leg, 0, 1, 2, 3)) = sel4<T>(leg, vbn[0], vbn[1], vbn[2], vbn[3]);
    if (leg < 2) if (UNGUARD || live) ROWV(a.v, 4 + leg) = leg == 0 ? vbn[4] : vbn[5];
    if (UNGUARD || live) ROWV(a.q, sel4<int>(leg, 0, 1, 2, 3)) = sel4<T>(leg, qn[0], qn[1], qn[2], qn[3]);
    if (leg < 3) if (UNGUARD || live) ROWV(a.q, 4 + leg) = sel4<T>(leg, qn[4], qn[5], qn[6], qn[6]);
  }
  ISTAMP(11);   // base rows stored
  // SCORE: this tick's cost, on the state the tick ends in -- behind the state's stores, where nothing of the integrator is live any more.  A state is spread
  // over its four leg rows: each row adds its own three joints' tau, qj, qdj and its foot's f, READ BACK from the result image (the QP wavefronts' words,
  // acquired above) and from the state image (this lane's own words of a moment ago: one wavefront's LDS traffic is in program order) so that they occupy no
  // register through the solves; row 0 also adds the base terms and the status.  The running sum is an LDS word per lane; the rows are summed behind the
  // LAST tick.  (lanes beyond the workgroup's states duplicate a live state in lockstep -- UNGUARD -- and only the live row-0 lane stores)
  if constexpr (SCORE) {
    // (the weights never change after the prologue: read at a fixed LDS address they are loop-invariant, and the compiler lifts all ~30 reads out of the
    //  horizon loop, where they sit in registers -- and in scratch -- through every role of every tick.  A zero it cannot see through keeps them here:
    //  tx went through an empty asm above and is below 2^31)
    const int z = (int)(tx >> 31);
    const DevScoreW<T>& wt = *(sc->w + z);
    const int slot = (int)(s32 - (unsigned)((size_t)blockIdx.x * SPW));
    const int ln = (int)(tx & 63);
    T g[GOAL_WORDS];
#pragma unroll
    for (int c = 0; c < GOAL_WORDS; ++c) g[c] = sc->goal[c * 16 + slot];
    const int st = sc->stat[slot];
    T t3[3], f3[3], q3[3], qd3[3], qn3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t3[k] = rs[jx[k] * 16]; f3[k] = rs[(12 + 3 * leg + k) * 16];
      q3[k] = si_[(7 + jx[k]) * 16]; qd3[k] = si_[(SIMG_V + 6 + jx[k]) * 16]; qn3[k] = wt.q_nom[jx[k]];
    }
    const T lk = score_stage<T>(wt, sc->last ? wt.terminal : (T)1, t3, f3, q3, qd3, qn3, leg == 0, qn, vbn, g, st);
    const T run = (sc->first ? (T)0 : sc->run[ln]) + lk;
    const int nf = (sc->first ? 0 : sc->nfail[ln]) + (st != 0 ? 1 : 0);
    if (!sc->last) { sc->run[ln] = run; sc->nfail[ln] = nf; }
    else {
      const T total = xrow_sum(run);
      if (live && leg == 0) {
        const bool acc = sc->out->accumulate != 0;
        T* const cp = (T*)((char*)sc->out->cost + (size_t)(s32 * (unsigned)sizeof(T)));
        *cp = acc ? *cp + total : total;
        int* const fl0 = sc->out->fail;
        if (fl0) { int* const fp = fl0 + s32; *fp = (acc ? *fp : 0) + nf; }
      }
    }
  }
#undef ISTAMP
#undef STS
}

// PAYLOAD: the plant carries a payload on its trunk (wbc_integrate_plant_batch, and the per-tick launches of the plant rollouts)
// (fp32: 195 registers with the payload against 160 without -- two wavefronts per SIMD instead of three.  Held to three (amdgpu_waves_per_eu) it
//  spills 53 scratch instructions; measured cost of the two: DESIGN.md 4.7)
template <class T, bool PAYLOAD = false>
__global__ __launch_bounds__(64) void integrate_kernel(const DevModel<T>* __restrict__ model, IntegrateArgsP<T, PAYLOAD> a) {
  if constexpr (PAYLOAD)
    integrate_body<T, 16, IntegrateNoWait, 0, false, false, false, IntegrateNoWait, false, true>(model, a, IntegrateNoWait(), nullptr, nullptr, nullptr,
                                                                                                 IntegrateNoWait(), a.payload);
  else
    integrate_body<T>(model, a);
}

}  // namespace wbc
