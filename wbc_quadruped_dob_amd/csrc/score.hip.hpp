// Scored rollouts (wbc_rollout_scored_batch, wbc_score_batch, wbc_rollout_select): a running quadratic cost of a rollout's state path and
// the choice of the best of K candidates per group.  Per state, for tick k, on the state (q, v) the tick ENDS in and the tau, f, status it produced:
//   l_k = w_tau |tau|^2 + w_f |f|^2 + w_fail [status != 0]
//       + s_k ( sum_c w_pos[c] (p_c - g_p[c])^2 + sum_c w_rot[c] e_c^2 + sum_c w_vel[c] (v_c - g_v[c])^2 + sum_c w_omega[c] om_c^2
//               + w_q sum_j (qj_j - q_nom_j)^2 + w_qd sum_j qdj_j^2 ),      s_k = 1, the launch's last tick: `terminal`
// e = the attitude error e_R of the CoM planner (com_ref.hip.hpp) with quat_des := g_quat.  goal [GOAL_WORDS][N]: g_p (3), g_quat (x, y, z, w), g_v (3).
// The formula exists ONCE, as score_stage = score_combine(score_effort, score_joints, score_base): the share of three joints and one foot, plus the base terms
// where `base` is set.  The per-tick kernel below calls it four times per state; the persistent rollout kernel once per leg row, at the end of phase 2 of the
// integrator (integrate.hip.hpp, SCORE).
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "dyn_sweep.hip.hpp"

namespace wbc {

// the three parts of l_k: the torque / force terms of three joints and one foot; the joint posture / velocity terms of three joints; the base terms
template <class T> WBC_DEV T score_effort(const DevScoreW<T>& w, const T (&tau)[3], const T (&f)[3]) {
  return w.w_tau * (tau[0] * tau[0] + tau[1] * tau[1] + tau[2] * tau[2]) + w.w_f * (f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
}
template <class T> WBC_DEV T score_joints(const DevScoreW<T>& w, const T (&qj)[3], const T (&qdj)[3], const T (&qnom)[3]) {
  const T d0 = qj[0] - qnom[0], d1 = qj[1] - qnom[1], d2 = qj[2] - qnom[2];
  return w.w_q * (d0 * d0 + d1 * d1 + d2 * d2) + w.w_qd * (qdj[0] * qdj[0] + qdj[1] * qdj[1] + qdj[2] * qdj[2]);
}
template <class T> WBC_DEV T score_base(const DevScoreW<T>& w, const T (&qb)[7], const T (&vb)[6], const T (&g)[GOAL_WORDS]) {
  T b = (T)0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const T dp = qb[c] - g[c], dv = vb[c] - g[7 + c];
    b += w.w_pos[c] * (dp * dp) + w.w_vel[c] * (dv * dv) + w.w_omega[c] * (vb[3 + c] * vb[3 + c]);
  }
  // e = 2 sign(ew) vec(g_quat (x) quat^-1), both normalised (as com_reference_body forms it)
  const T n = rsqrt_fast(qb[3] * qb[3] + qb[4] * qb[4] + qb[5] * qb[5] + qb[6] * qb[6]);
  const T dn = rsqrt_fast(g[3] * g[3] + g[4] * g[4] + g[5] * g[5] + g[6] * g[6]);
  const T x = -qb[3] * n, y = -qb[4] * n, z = -qb[5] * n, qw = qb[6] * n;
  const T dx = g[3] * dn, dy = g[4] * dn, dz = g[5] * dn, dw = g[6] * dn;
  const T ex = dw * x + dx * qw + dy * z - dz * y;
  const T ey = dw * y - dx * z + dy * qw + dz * x;
  const T ez = dw * z + dx * y - dy * x + dz * qw;
  // (the sign of the scalar part selects +2 or -2: squared, both give 4)
  return b + (T)4 * (w.w_rot[0] * (ex * ex) + w.w_rot[1] * (ey * ey) + w.w_rot[2] * (ez * ez));
}
// l_k from the parts: `base` = this share counts the base terms and the status (one share per state does)
template <class T> WBC_DEV T score_combine(const DevScoreW<T>& w, T s_k, T effort, T joints, T base_terms, bool base, int status) {
  const T st = joints + (base ? base_terms : (T)0);
  const T l = effort + ((base && status != 0) ? w.w_fail : (T)0);
  return l + s_k * st;
}
template <class T>
WBC_DEV T score_stage(const DevScoreW<T>& w, T s_k, const T (&tau)[3], const T (&f)[3], const T (&qj)[3], const T (&qdj)[3], const T (&qnom)[3], bool base,
                      const T (&qb)[7], const T (&vb)[6], const T (&g)[GOAL_WORDS], int status) {
  return score_combine<T>(w, s_k, score_effort<T>(w, tau, f), score_joints<T>(w, qj, qdj, qnom), score_base<T>(w, qb, vb, g), base, status);
}

// The per-tick path (larger batches, rollout_persistent = 0, wbc_score_batch): one state per lane behind the tick's integrate launch; every load is one
// component row at consecutive states.  accumulate = 0: cost = l_k (the first tick of a sum that starts at zero), else cost += l_k; fail likewise.
template <class T>
__global__ __launch_bounds__(256) void score_tick_kernel(ScoreArgs<T> a, const T* __restrict__ q, const T* __restrict__ v, const T* __restrict__ tau,
                                                         const T* __restrict__ f, const int* __restrict__ status, int is_last) {
  const size_t N = a.N;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  T qb[7], vb[6], g[GOAL_WORDS];
#pragma unroll
  for (int c = 0; c < 7; ++c) qb[c] = q[(size_t)c * N + i];
#pragma unroll
  for (int c = 0; c < 6; ++c) vb[c] = v[(size_t)c * N + i];
#pragma unroll
  for (int c = 0; c < GOAL_WORDS; ++c) g[c] = a.goal[(size_t)c * N + i];
  const int st = status[i];
  const T s_k = is_last ? a.w.terminal : (T)1;
  T part[4];
#pragma unroll
  for (int l = 0; l < 4; ++l) {   // joints 3 l .. 3 l + 2 in the caller's order with foot l: the sums run over all twelve, whichever leg they belong to
    T t3[3], f3[3], q3[3], qd3[3], qn3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int j = 3 * l + k;
      t3[k] = tau[(size_t)j * N + i]; f3[k] = f[(size_t)j * N + i];
      q3[k] = q[(size_t)(7 + j) * N + i]; qd3[k] = v[(size_t)(6 + j) * N + i]; qn3[k] = a.w.q_nom[j];
    }
    part[l] = score_stage<T>(a.w, s_k, t3, f3, q3, qd3, qn3, l == 0, qb, vb, g, st);
  }
  const T lk = (part[0] + part[1]) + (part[2] + part[3]);
  a.cost[i] = a.accumulate ? a.cost[i] + lk : lk;
  if (a.fail) a.fail[i] = (a.accumulate ? a.fail[i] : 0) + (st != 0 ? 1 : 0);
}

// ---- per-group selection: group g = costs [g * group, (g + 1) * group).  One workgroup per group; every reduction is a fixed tree (xor shuffles inside a
// wavefront, then the wavefronts' partial results from LDS in index order), so the results are bit-identical from run to run.
template <class T> WBC_DEV T select_inf();
template <> WBC_DEV double select_inf<double>() { return __builtin_huge_val(); }
template <> WBC_DEV float select_inf<float>() { return __builtin_huge_valf(); }
WBC_DEV double select_exp(double x) { return exp(x); }
WBC_DEV float select_exp(float x) { return expf(x); }

template <class T, int BLOCK>
__global__ __launch_bounds__(BLOCK) void rollout_select_kernel(const T* __restrict__ cost, unsigned group, T lambda, int* __restrict__ best,
                                                                T* __restrict__ best_cost, T* __restrict__ weights) {
  static_assert(BLOCK % 64 == 0 && BLOCK <= 256, "one to four wavefronts");
  constexpr int WAVES = BLOCK / 64;
  __shared__ T m_sh[WAVES];
  __shared__ int i_sh[WAVES];
  __shared__ T s_sh[WAVES];
  const T INF = select_inf<T>();
  constexpr int NONE = 0x7fffffff;
  const T* const c0 = cost + (size_t)blockIdx.x * group;
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  auto clean = [INF](T c) { return c == c ? c : INF; };   // NaN counts as +inf
  // pass 1: the smallest cost and the lowest index that holds it
  T m = INF;
  int mi = NONE;
  for (unsigned i = (unsigned)tid; i < group; i += BLOCK) {
    const T c = clean(c0[i]);
    if (c < m) { m = c; mi = (int)i; }   // (indices ascend within a thread: strict < keeps the lowest)
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T om = __shfl_xor(m, off, 64);
    const int oi = __shfl_xor(mi, off, 64);
    if (om < m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  if constexpr (WAVES > 1) {
    if ((tid & 63) == 0) { m_sh[wave] = m; i_sh[wave] = mi; }
    __syncthreads();
    m = m_sh[0]; mi = i_sh[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
      const T om = m_sh[w];
      const int oi = i_sh[w];
      if (om < m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
  }
  const bool none = mi == NONE;   // every cost of the group is +inf or NaN
  if (tid == 0) {
    best[blockIdx.x] = none ? -1 : mi;
    if (best_cost) best_cost[blockIdx.x] = m;
  }
  if (!weights) return;
  T* const w0 = weights + (size_t)blockIdx.x * group;
  if (none || !(lambda > (T)0)) {   // all-zero weights / one-hot on best
    for (unsigned i = (unsigned)tid; i < group; i += BLOCK) w0[i] = (!none && (int)i == mi) ? (T)1 : (T)0;
    return;
  }
  // pass 2: the sum of exp(-(c - c_min) / lambda); pass 3: the normalised weights
  const T il = (T)1 / lambda;
  T sum = (T)0;
  for (unsigned i = (unsigned)tid; i < group; i += BLOCK) sum += select_exp(-(clean(c0[i]) - m) * il);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) sum += __shfl_xor(sum, off, 64);
  if constexpr (WAVES > 1) {
    if ((tid & 63) == 0) s_sh[wave] = sum;
    __syncthreads();
    sum = s_sh[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) sum += s_sh[w];
  }
  const T is = (T)1 / sum;
  for (unsigned i = (unsigned)tid; i < group; i += BLOCK) w0[i] = select_exp(-(clean(c0[i]) - m) * il) * is;
}

}  // namespace wbc
