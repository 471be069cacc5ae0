// Joint torque limits behind a tick: the states whose stance-leg torques exceed their actuators' limits get their GRF QP solved again with the
// limits as rows, on chip.  Two kernels on the caller's stream behind ANY tick (wbc_limit_torques_batch):
//
//   limit_scan_kernel   one lane per state reads the tick's tau (12 component-major rows) and mask.  A SWING-leg joint beyond its limit is clipped
//                       (no contact force can change it); a state with a STANCE-leg joint beyond its limit is appended to a device list -- one ballot and
//                       one atomicAdd per wavefront.  limited[s] = 2 where a swing joint was clipped, else 0.
//   limit_qp_kernel     a fixed grid of wavefronts walks that list with a grid stride (the count is read from memory: no host read-back).  Per entry a
//                       wavefront builds the tick's own GRF QP
//                           min 1/2 (A f - b)^T S (A f - b) + alpha/2 |f|^2,   friction pyramid + normal-force box          (the QP of every tick: DESIGN.md section 2)
//                       PLUS, for every stance foot and each joint j of its leg with a finite limit, the two rows
//                           a_j^T f >= tau0_j - lim_j,     -a_j^T f >= -lim_j - tau0_j                                       (|tau0_j - a_j^T f| <= lim_j)
//                       directly in the LDS layout of the general Goldfarb-Idnani body (qpg_solve, qp_general.hip.hpp) -- the dense problem never exists in
//                       memory -- runs that body, and stores f, tau = tau0 - a^T f, status = 0, iters, limited = 1.  When the limited QP does not reach
//                       status 0 the tick's f and status stay and every tau_j is clipped to its limit (limited = 2).
//
// Everything comes from the tick's own outputs: tau0_j = tau_j + a_j^T f is the force-free torque (no M, vdot_des or joint residual needed), a_j = column 6 + j
// of Jc over the foot's three force components (the other feet's entries are structural zeros), A's lever arms are Jc's base-angular columns as
// integrate.hip.hpp reads them, b = w_des - rhat_base with rhat = the observer state the tick left.  The limited QP runs in fp64 for both scalar types, like
// the structured QP kernels; T is the type of the batch arrays only.  A state's result depends on that state alone: the order of the list does not matter.
// A clipped torque is the limit rounded to T (to nearest): for a limit that fp32 cannot represent (0.05, say) the stored magnitude can lie one rounding
// above the fp64 limit, and a second post-pass over the same buffers would call that joint "over" again and clip it to the same value.
#pragma once
#include <hip/hip_runtime.h>
#include "limit_args.hpp"
#include "qp_general.hip.hpp"

namespace wbc {

__device__ __forceinline__ double limit_pick12(const double (&v)[12], int i) {   // v[i] of a kernel-argument array without indexing it by a register
  double r = v[0];
#pragma unroll
  for (int k = 1; k < 12; ++k) r = (i == k) ? v[k] : r;
  return r;
}

template <class T>
__global__ __launch_bounds__(256) void limit_scan_kernel(LimitArgs<T> a) {
  const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = s < a.N;
  bool stance_over = false, swing_over = false;
  if (live) {
    const int mask = a.mask[s];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const bool stance = (mask >> l) & 1;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const size_t j = (size_t)((a.jpack >> (4 * (3 * l + k))) & 15);
        const double lim = a.lim[3 * l + k];
        const T t = a.tau[j * a.N + s];
        if (fabs((double)t) > lim) {
          if (stance) stance_over = true;
          else { swing_over = true; a.tau[j * a.N + s] = (T)(t > 0 ? lim : -lim); }
        }
      }
    }
    if (a.limited) a.limited[s] = swing_over ? 2 : 0;
  }
  const unsigned long long b = __ballot(stance_over);
  if (b != 0) {   // (wavefront-uniform)
    const int lane = threadIdx.x & 63, first = __ffsll((long long)b) - 1;
    int base = 0;
    if (lane == first) base = atomicAdd(&a.list[0], __popcll(b));
    base = __builtin_amdgcn_readlane(base, __builtin_amdgcn_readfirstlane(first));
    const size_t slot = (size_t)base + __popcll(b & ((1ull << lane) - 1ull));
    if (stance_over && slot < a.N) a.list[LIMIT_LIST_HEAD + slot] = (int)s;   // (slot < N whenever the counter started at zero: the list holds max_batch entries)
  }
}

// one listed state on one wavefront; S = the wavefront's LDS slice of qpg_lds_scalars(LIMIT_QP_N, LIMIT_QP_M) doubles
template <class T>
__device__ __forceinline__ void limit_qp_state(const LimitArgs<T>& a, double* S, int lane, size_t s) {
  const size_t N = a.N;
  const int mask = __builtin_amdgcn_readfirstlane(a.mask[s]) & 15;
  const int ns = __popc(mask);
  if (ns == 0) return;   // (never listed: a state is listed for a stance-leg joint)
  const int n = 3 * ns, ld = qpg_ld(n);
  auto foot_of_slot = [&](int slot) {   // the slot-th stance foot
    int mm = mask;
#pragma unroll
    for (int i = 0; i < 3; ++i) if (i < slot) mm &= mm - 1;
    return __ffs(mm) - 1;
  };
  // lane t < n is force variable t = (stance slot sv, axis av) AND joint av of that foot's leg
  const bool isvar = lane < n;
  const int sv = isvar ? lane / 3 : 0, av = isvar ? lane - 3 * sv : 0;
  const int kv = foot_of_slot(sv);
  const int lj = 3 * kv + av;                                  // leg-major joint
  const size_t j = (size_t)((a.jpack >> (4 * lj)) & 15);       // caller's joint
  const double lim = limit_pick12(a.lim, lj);
  auto ld_ = [&](const T* p, size_t row) { return (double)p[row * N + s]; };
  double Acol[6] = {0, 0, 0, 0, 0, 0}, aj[3] = {0, 0, 0}, tau0 = 0;
  if (isvar) {
    const double dx = ld_(a.Jc, JC_LEVER_WORD_((size_t), kv, 0)), dy = ld_(a.Jc, JC_LEVER_WORD_((size_t), kv, 1)), dz = ld_(a.Jc, JC_LEVER_WORD_((size_t), kv, 2));
    Acol[av] = 1;   // A = [1 ; [d]x] per foot: column av
    Acol[3] = av == 0 ? 0 : (av == 1 ? -dz : dy);
    Acol[4] = av == 0 ? dz : (av == 1 ? 0 : -dx);
    Acol[5] = av == 0 ? -dy : (av == 1 ? dx : 0);
    tau0 = ld_(a.tau, j);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      aj[c] = ld_(a.Jc, JC_LEG_WORD_((size_t), kv, c, j));
      tau0 += aj[c] * ld_(a.f, (size_t)(3 * kv + c));
    }
  }
  double b[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) b[r] = qpg_rl(ld_(a.wdes, r) - (a.rhat ? ld_(a.rhat, r) : 0.0), 0);   // (the same word in every lane: kept in scalar registers)
  const bool fin = isvar && lim < QpgLim<double>::big;
  const unsigned long long finb = __ballot(fin);
  const int m = 6 * ns + 2 * __popcll(finb);
  const QpgLds<double> L = qpg_carve(S, n, m, ld);

  // ---- H = alpha 1 + A^T S A, g = -A^T S b: A's columns through the (still unused) vector area, 6 n <= 7 (n + 1) scalars
  double* const As = L.xs;
  if (isvar) {
#pragma unroll
    for (int r = 0; r < 6; ++r) As[r * n + lane] = Acol[r];
  }
  for (int e = lane; e < m * ld; e += 64) L.Cm[e] = 0;
  if (lane <= m) L.lam[lane] = 0;
  QPG_WSYNC();
  for (int e = lane; e < n * n; e += 64) {
    const int i = e / n, c = e - i * n;
    double h = (i == c) ? a.alpha : 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) h += As[r * n + i] * a.S[r] * As[r * n + c];
    L.R[i * ld + c] = h;
  }
  double g_i = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) g_i -= Acol[r] * a.S[r] * b[r];
  // ---- rows.  Lane c < 6 ns: row c % 6 of stance slot c / 6 (mu~ n - t1, mu~ n + t1, mu~ n - t2, mu~ n + t2, n, -n)
  double d_i = 0;
  if (lane < 6 * ns) {
    const int sc = lane / 6, cc = lane - 6 * sc, kc = foot_of_slot(sc);
    const double nx = ld_(a.normals, (size_t)3 * kc), ny = ld_(a.normals, (size_t)3 * kc + 1), nz = ld_(a.normals, (size_t)3 * kc + 2);
    const double il = 1 / sqrt(nx * nx + ny * ny + nz * nz);
    const double n0 = nx * il, n1 = ny * il, n2 = nz * il;
    const bool rx = fabs(n0) < 0.9;
    const double r0 = rx ? 1.0 : 0.0, r1 = rx ? 0.0 : 1.0;
    const double rn = r0 * n0 + r1 * n1;
    const double u0 = r0 - n0 * rn, u1 = r1 - n1 * rn, u2 = -n2 * rn;
    const double iu = 1 / sqrt(u0 * u0 + u1 * u1 + u2 * u2);
    const double t10 = u0 * iu, t11 = u1 * iu, t12 = u2 * iu;
    const double t20 = n1 * t12 - n2 * t11, t21 = n2 * t10 - n0 * t12, t22 = n0 * t11 - n1 * t10;
    const double mt = ld_(a.mu, (size_t)kc) * a.mu_scale;
    double c0, c1, c2;
    if (cc < 4) {
      const double sg = (cc & 1) ? 1.0 : -1.0;
      const double w0 = cc < 2 ? t10 : t20, w1 = cc < 2 ? t11 : t21, w2 = cc < 2 ? t12 : t22;
      c0 = n0 * mt + sg * w0; c1 = n1 * mt + sg * w1; c2 = n2 * mt + sg * w2;
    } else {
      const double sg = cc == 4 ? 1.0 : -1.0;
      c0 = sg * n0; c1 = sg * n1; c2 = sg * n2;
      d_i = cc == 4 ? a.fn_min : -a.fn_max;
    }
    double* const row = L.Cm + lane * ld + 3 * sc;
    row[0] = c0; row[1] = c1; row[2] = c2;
  }
  // the torque rows of joint `lane`: rows 6 ns + 2 rank, + 1 (rank among the joints with a finite limit); their right-hand sides travel through lam
  if (fin) {
    const int c0 = 6 * ns + 2 * __popcll(finb & ((1ull << lane) - 1ull));
    double* const rp = L.Cm + c0 * ld + 3 * sv;
    double* const rm = rp + ld;
#pragma unroll
    for (int c = 0; c < 3; ++c) { rp[c] = aj[c]; rm[c] = -aj[c]; }
    L.lam[c0] = tau0 - lim;
    L.lam[c0 + 1] = -lim - tau0;
  }
  QPG_WSYNC();
  const bool trow = lane >= 6 * ns && lane < m;
  if (trow) d_i = L.lam[lane];
  QPG_WSYNC();
  if (trow) L.lam[lane] = 0;
  QPG_WSYNC();

  double x_i; int status, iter;
  qpg_solve<double>(L, lane, n, m, 0, ld, g_i, d_i, a.tol, a.max_iter, x_i, status, iter);

  if (status == 0) {   // (wavefront-uniform)
    if (isvar) {
      double t = tau0;
#pragma unroll
      for (int c = 0; c < 3; ++c) t -= aj[c] * L.xs[3 * sv + c];
      a.f[(size_t)lj * N + s] = (T)x_i;
      a.tau[j * N + s] = (T)t;
    }
    if (lane == 0) {
      a.status[s] = 0;
      if (a.iters) a.iters[s] = iter;
      if (a.limited && a.limited[s] != 2) a.limited[s] = 1;   // (2: the scan clipped a swing joint of this state)
    }
  } else {             // the limits cannot be met by any admissible force: the tick's f and status stay, every torque is clipped
    if (lane < 12) {
      const size_t jc = (size_t)((a.jpack >> (4 * lane)) & 15);
      const double lc = limit_pick12(a.lim, lane);
      const T t = a.tau[jc * N + s];
      if (fabs((double)t) > lc) a.tau[jc * N + s] = (T)(t > 0 ? lc : -lc);
    }
    if (lane == 0 && a.limited) a.limited[s] = 2;
  }
}

// Grid: see k_limit.hip (one resident round of wavefronts).  lds_per_qp = qpg_lds_scalars(LIMIT_QP_N, LIMIT_QP_M) doubles per wavefront.
template <class T>
__global__ __launch_bounds__(64 * LIMIT_QP_WPB) __attribute__((amdgpu_waves_per_eu(4, 4))) void limit_qp_kernel(LimitArgs<T> a, int lds_per_qp) {
  extern __shared__ __align__(16) unsigned char limit_lds_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  double* const S = (double*)limit_lds_raw + (size_t)wave * lds_per_qp;
  int count = __builtin_amdgcn_readfirstlane(a.list[0]);
  count = count < 0 ? 0 : (count > (int)a.N ? (int)a.N : count);   // never walk past what the scan can have written
  const int nw = (int)gridDim.x * wpb;
  for (int e = (int)blockIdx.x * wpb + wave; e < count; e += nw) {   // (whole wavefronts: no workgroup barrier anywhere)
    const size_t s = (size_t)__builtin_amdgcn_readfirstlane(a.list[LIMIT_LIST_HEAD + e]);
    if (s < a.N) limit_qp_state<T>(a, S, lane, s);
    QPG_WSYNC();
  }
}

}  // namespace wbc
