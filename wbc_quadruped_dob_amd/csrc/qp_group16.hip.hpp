// The orthogonal-factor ("dense") GRF-QP body in fp32 arithmetic: what large fp32 tiles run, and nothing else.
//
// Every other QP kernel of the library -- stand-alone, listed, staged tiles, the one-launch tick, the rollouts -- runs the structured
// wrench-space body (qp_struct16.hip.hpp), which computes in fp64 for both scalar types.  This body survives for ONE caller,
// qp_tile_kernel<float, RHAT, TILE, /*DENSE*/true> (qp_kernels.hip.hpp): tiles of 64 ... 128 fp32 states, from WBC_F32_DENSE_TILE_MIN
// states on.  At 117 VGPRs four of its workgroups share a CU where the structured body's 183 allow two: from ~49 152 fp32 states on
// (more than two tiles of 64 per CU) it wins (65 536: 38 vs 46 us, 131 072: 72 vs 92 us), below it loses (32 768: 26.0 vs 23.4 us;
// measured, MI355X).  It is TILED (the four rows of the wavefront solve the states `who` names), four wavefronts per workgroup, reads
// its inputs from memory and writes f, tau, status, iters there: the fused tick's LDS workspace, its producer flags and result images
// are the structured body's business alone.
//
// Mapping: ONE QP PER 16-LANE DPP ROW, four QPs per wavefront (qp_row16.hip.hpp).  The 12x12 factors of the Goldfarb-Idnani method
// live entirely in VGPRs:
//   lane 4f+a (a<3) of a row owns variable (foot f, axis a); lane 4f+3 is a spare that carries constraints
//   Jc[12] = column `me` of J,  Jr[12] = row `me` of J,  Rr[12] = row `me` of R   (static register indices)
// Products with J^T use the column copy, products with J use the row copy, the rank-one Householder update
// of an added constraint touches both; every cross-lane operand is a row broadcast (2 DPP movs per double).
// All four feet are always variables (swing feet decouple: H_ii = alpha, g_i = 0 => f = 0), so there is no
// per-QP dimension and no dynamic register index; per-QP control flow is predication, wave-level control
// flow is a ballot.  Dropping a constraint (rare) restores J from a copy of J0 = L^-T kept in LDS and
// re-adds the remaining active constraints -- no Givens chain.  LDS is used only for that copy and for the
// one transposition that derives the row copy of J0 from the column copy.
// The active-set factor is kept as U = R^-1 (row `me` of U per variable lane, in the LDS image that held R).  The dual step
// r = R^-1 d1 is then a matrix-vector product -- twelve broadcasts and FMAs in three independent chains -- instead of a
// back-substitution whose iq steps each wait for the one before (round 2 stamps: 610 of the ~3 200 cycles of an iteration).
// Appending a constraint needs nothing new: with r = R^-1 d1 at hand the new column of U is [-r / delta ; 1 / delta],
// delta = the new diagonal entry of R.
//
// Same algorithm and tolerances as the CPU oracle (dual active set; "no primal step" and "new diagonal"
// share |d2|); iterates differ from the oracle's only by orthogonal transformations of the free columns.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "device_types.hpp"
#include "qp_row16.hip.hpp"

namespace wbc {

// per wave: four 12x12 images of J0 ([i*12 + c]) and four images of R ([position*12 + variable]: row `me` of R is
// addressed by a run-time position, which LDS allows and a register array does not)
// ... and the 32 constraint rows (3 coefficients each) so that a candidate's normal is three broadcast reads
template <class T> struct G16Lds { T J0[4][144]; T R[4][12 * 12]; T C[4][32 * 3]; };

// RHAT: the observer kernel left rhat in the memory workspace; b and tau_partial are completed here (b -= rhat_base, tau_partial -= rhat_joint).
template <class T, bool RHAT>
WBC_DEV void qp_group16_body(const DevParams<T>& prm, const QpArgs<T>& a, const QpWho who) {
  using RowS = T;
  using RowA = T;
  __shared__ G16Lds<T> lds_all[4];   // one per wavefront of the workgroup
  WBC_QP_ROW_PROLOGUE
  T* J0 = lds_all[tx >> 6].J0[grp];
  T* Rl = lds_all[tx >> 6].R[grp] + v;  // my row of R: Rl[12 * position] (spare lanes alias a variable lane; they never write)
  T* Cl = lds_all[tx >> 6].C[grp];        // constraint rows by id
  const size_t N = a.N;
  const unsigned N32 = (unsigned)N;
  const size_t qp_raw = who.state;
  bool live = who.live;
  unsigned s32 = (unsigned)(live ? qp_raw : N - 1);
  const T INF = Lim<T>::inf, EPS = Lim<T>::eps;
#define WSLD(comp) GLD(a.ws, comp)
  // target wrench: the caller's w_des (two-kernel ticks whose front half does not change it) or the workspace
#define BLD(c) (a.wdes ? GLD(a.wdes, c) : GLD(a.ws, WS_B + (c)))

#ifdef WBC_QP_STAMP
  const long long st_t0 = __builtin_readcyclecounter();
#endif
  // ------------------------------------------------------------------ inputs
  int mask = a.mask[s32] & 0xF;
  bool on = (mask >> f) & 1;
  const bool geom_jc = a.Jc != nullptr;   // uniform: lever arms / own-leg blocks from Jc (see QpArgs)
  const T n_ld = isvar ? GLD(a.normals, v) : (T)0;
  const T mu_f = GLD(a.mu, f);
  T d_me = 0;
  if (geom_jc) {
    const int comp = JC_LEVER_WORD(f, c3);
    if (isvar) d_me = GLD(a.Jc, comp);
  } else if (isvar) d_me = WSLD(WS_D + v);
  // ------------------------------------------------------------------ a square root of H^-1 (a7), from the structure of H
  // H = alpha I + B^T B,  B = S^(1/2) A (6 x 12),  A = [I ; [d_f]x] per stance foot (zero columns for swing feet).
  // The dual active-set method needs ANY J with J J^T = H^-1 -- it only ever applies orthogonal transformations to the
  // columns of J -- so the dense 12x12 Cholesky factor and its inverse are not needed.  With the 6x6 matrix
  //     G = alpha I + B B^T = L L^T                         (B B^T = S^(1/2) [nc I, -[sd]x ; [sd]x, sum(|d|^2 I - d d^T)] S^(1/2))
  //     J = (I - B^T K B) / sqrt(alpha),   K = (G + sqrt(alpha) L^T)^-1 = L^-T (L + sqrt(alpha) I)^-1
  // because J J^T = (I - B^T (K + K^T - K (G - alpha I) K^T) B) / alpha and K + K^T - K (G - alpha I) K^T = G^-1 (Woodbury).
  // Every lane forms G and its factor redundantly from the twelve broadcast lever-arm components -- no cross-lane step,
  // six pivots instead of twelve -- then applies K and K^T to ITS column b_v of B; entries of J are three FMAs each.
  // Accuracy: the alpha-dominated directions are handled analytically, which in fp32 is ~100x closer to H^-1 than the
  // 12x12 Cholesky route (cond(H) ~ 1e4).
  const T dqx = dppx<0x00>(d_me), dqy = dppx<0x55>(d_me), dqz = dppx<0xAA>(d_me);  // quad_perm [0000],[1111],[2222]: my foot's lever arm
  const T onv = (on && isvar) ? (T)1 : (T)0;
  T u0, u1, u2;  // column c3 of [d_f]x for my own foot: [[0,-dz,dy],[dz,0,-dx],[-dy,dx,0]]
  u0 = (c3 == 0) ? (T)0 : (c3 == 1 ? -dqz : dqy);
  u1 = (c3 == 0) ? dqz : (c3 == 1 ? (T)0 : -dqx);
  u2 = (c3 == 0) ? -dqy : (c3 == 1 ? dqx : (T)0);
  // (the weights pass through an empty asm: they are kernel-uniform, so inside the tile loop every product of two of them would
  // otherwise be hoisted out of the loop and held in registers for the whole kernel)
  T s0 = prm.sS[0], s1 = prm.sS[1], s2 = prm.sS[2], s3 = prm.sS[3], s4 = prm.sS[4], s5 = prm.sS[5];
  T alpha_l = prm.alpha, sqa = prm.sqrt_alpha, rsa = prm.rsqrt_alpha;
  asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3), "+v"(s4), "+v"(s5), "+v"(alpha_l), "+v"(sqa), "+v"(rsa));
  // my column of B: bf on the force rows (one non-zero, at row c3), bm on the moment rows
  const T bfs = onv * (c3 == 0 ? s0 : (c3 == 1 ? s1 : s2));
  const T bm0 = onv * s3 * u0, bm1 = onv * s4 * u1, bm2 = onv * s5 * u2;
  T Dx[4], Dy[4], Dz[4], Of[4];   // lever arms of the four feet, zeroed for swing feet; stance flags
  sfor<0, 4>([&](auto fc) __attribute__((always_inline)) {
    constexpr int fj = decltype(fc)::value;
    const bool onj = (mask >> fj) & 1;
    Of[fj] = onj ? (T)1 : (T)0;
    Dx[fj] = onj ? gbc<3 * fj>(d_me) : (T)0; Dy[fj] = onj ? gbc<3 * fj + 1>(d_me) : (T)0; Dz[fj] = onj ? gbc<3 * fj + 2>(d_me) : (T)0;
  });
  // G and its lower factor L (qp_row16.hip.hpp); ld = L_kk beside il = 1 / L_kk
  const T nc = (Of[0] + Of[1]) + (Of[2] + Of[3]);
  const T sx = (Dx[0] + Dx[1]) + (Dx[2] + Dx[3]), sy = (Dy[0] + Dy[1]) + (Dy[2] + Dy[3]), sz = (Dz[0] + Dz[1]) + (Dz[2] + Dz[3]);
  T Pxx = 0, Pxy = 0, Pxz = 0, Pyy = 0, Pyz = 0, Pzz = 0;
  sfor<0, 4>([&](auto fc) __attribute__((always_inline)) {
    constexpr int fj = decltype(fc)::value;
    Pxx += Dx[fj] * Dx[fj]; Pxy += Dx[fj] * Dy[fj]; Pxz += Dx[fj] * Dz[fj];
    Pyy += Dy[fj] * Dy[fj]; Pyz += Dy[fj] * Dz[fj]; Pzz += Dz[fj] * Dz[fj];
  });
  WBC_QP_G_FACTOR(T, rsqrt_nr, alpha_l)
  const T ld[6] = {g00 * il[0], g11 * il[1], g22 * il[2], c00 * il[3], t11 * il[4], t22 * il[5]};
  const T bf0 = (c3 == 0) ? bfs : (T)0, bf1 = (c3 == 1) ? bfs : (T)0, bf2 = (c3 == 2) ? bfs : (T)0;
  // ------------------------------------------------------------------ unconstrained minimum x0 = -H^-1 g = B^T G^-1 S^(1/2) b
  // (b = w_des - rhat_base): one 6x6 solve with the factor at hand
  T x_me = 0;
  {
    const T b_ld = (l16 < 6) ? BLD(l16) - (RHAT ? WSLD(WS_RHAT + l16) : (T)0) : (T)0;
    T w[6], z[6];
    const T r0 = s0 * dppx<0x150 + 0>(b_ld), r1 = s1 * dppx<0x150 + 1>(b_ld), r2 = s2 * dppx<0x150 + 2>(b_ld), r3 = s3 * dppx<0x150 + 3>(b_ld),
            r4 = s4 * dppx<0x150 + 4>(b_ld), r5 = s5 * dppx<0x150 + 5>(b_ld);
    WBC_QP_FWD(il, r0, r1, r2, r3, r4, r5, w);
    WBC_QP_BWD(il, w, z);
    x_me = (bf0 * z[0] + bf1 * z[1] + bf2 * z[2]) + (bm0 * z[3] + bm1 * z[4] + bm2 * z[5]);
  }
  // ------------------------------------------------------------------ my column and my row of J
  // (J is built only when some row of the wavefront has a violated constraint at x0: a wavefront whose four unconstrained
  // minima are feasible -- common once tiles are dealt by predicted work -- is done after the 6x6 solve)
  T Jc[12], Jr[12];
  auto build_J = [&]() __attribute__((always_inline)) {
    T ia[6];   // 1 / (L_kk + sqrt(alpha))
    sfor<0, 6>([&](auto kc) __attribute__((always_inline)) { constexpr int k = decltype(kc)::value; ia[k] = rcp_nr(ld[k] + sqa); });
    T w[6], y[6], yt[6];
    WBC_QP_FWD(ia, bf0, bf1, bf2, bm0, bm1, bm2, w);   // y = K b_v = L^-T (L + sqrt(alpha) I)^-1 b_v
    WBC_QP_BWD(il, w, y);
    WBC_QP_FWD(il, bf0, bf1, bf2, bm0, bm1, bm2, w);   // yt = K^T b_v = (L + sqrt(alpha) I)^-T L^-1 b_v
    WBC_QP_BWD(ia, w, yt);
    const T yf[3] = {s0 * rsa * y[0], s1 * rsa * y[1], s2 * rsa * y[2]}, ym[3] = {s3 * rsa * y[3], s4 * rsa * y[4], s5 * rsa * y[5]};
    const T tf[3] = {s0 * rsa * yt[0], s1 * rsa * yt[1], s2 * rsa * yt[2]}, tm[3] = {s3 * rsa * yt[3], s4 * rsa * yt[4], s5 * rsa * yt[5]};
    sfor<0, 12>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      constexpr int fi = i / 3, ai = i % 3;
      const T dlt = (isvar && v == i) ? rsa : (T)0;
      // b_i . y with b_i = on_i [s_ai e_ai ; s_(3..5) * column ai of [d_i]x]   (Dx.. are already zero for swing feet)
      T cj = dlt - Of[fi] * yf[ai], rj = dlt - Of[fi] * tf[ai];
      if (ai == 0) { cj = cj - Dz[fi] * ym[1] + Dy[fi] * ym[2]; rj = rj - Dz[fi] * tm[1] + Dy[fi] * tm[2]; }
      else if (ai == 1) { cj = cj + Dz[fi] * ym[0] - Dx[fi] * ym[2]; rj = rj + Dz[fi] * tm[0] - Dx[fi] * tm[2]; }
      else { cj = cj - Dy[fi] * ym[0] + Dx[fi] * ym[1]; rj = rj - Dy[fi] * tm[0] + Dx[fi] * tm[1]; }
      Jc[i] = cj;   // J[i][v]
      Jr[i] = rj;   // J[v][i]
    });
    // keep the initial J in LDS: dropping a constraint (rare) restores it from there
    if (isvar) sfor<0, 12>([&](auto ic) __attribute__((always_inline)) { constexpr int i = decltype(ic)::value; J0[i * 12 + v] = Jc[i]; });
  };

  // ------------------------------------------------------------------ my constraints (friction pyramid, force box)
  T cAx, cAy, cAz, rA, cBx = 0, cBy = 0, cBz = 0;
  const bool hasB = c3 < 2;
  WBC_QP_FORM_ROWS;

  {
    T* c = Cl + 3 * (2 * l16);
    c[0] = cAx; c[1] = cAy; c[2] = cAz; c[3] = cBx; c[4] = cBy; c[5] = cBz;
    // the image of U starts at zero for EVERY QP: columns beyond the active set enter the dual step multiplied by a masked
    // zero, so whatever they hold must be finite -- a NaN left by an earlier state of this row slot (tiles, rollouts) must not leak
    if (isvar) sfor<0, 12>([&](auto kc) __attribute__((always_inline)) { constexpr int k = decltype(kc)::value; Rl[12 * k] = (T)0; });
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");   // (LDS hand-over inside the wavefront: no global traffic to wait for)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
  }

  // ------------------------------------------------------------------ dual active-set iterations (a8)
  int iq = 0, ip = -1, status = 0, iter = 0;
  bool done = !live;
  bool actA = false, actB = false;
  T sip = 0, Rnorm = 1, u_me = 0;
  T u_c = 0;  // multiplier of the candidate constraint (row-uniform; it has no position until it is added)
  int Aid = -1;

  // slack of my constraints at the current x
  auto slacks = [&](T& sA, T& sB) __attribute__((always_inline)) {
    const T xq0 = dppx<0x00>(x_me), xq1 = dppx<0x55>(x_me), xq2 = dppx<0xAA>(x_me);
    sA = cAx * xq0 + cAy * xq1 + cAz * xq2 - rA;
    sB = cBx * xq0 + cBy * xq1 + cBz * xq2;
  };
  // step 1 for rows that need a new candidate: most violated inactive constraint
  auto pick = [&]() __attribute__((always_inline)) {
    T sA, sB;
    slacks(sA, sB);
    T val = KeyT<T>::BIG;
    int id = 2 * l16;
    if (on && !actA && sA < -prm.qp_tol) { val = sA; }
    if (on && hasB && !actB && sB < -prm.qp_tol && sB < val) { val = sB; id = 2 * l16 + 1; }
    const bool found = gargmin(val, id);
    const T sw = val;  // winner's slack, exact to 2^-46
    const bool need = !done && ip < 0;
    if (need) {
      if (found) {
        ip = id; sip = sw; u_c = 0;
      } else done = true;
    }
  };
  // add constraint with normal (np0,np1,np2) on foot fp at position `pos` for rows where `doit`;
  // dd = J^T np of my column (valid when isvar), dn2 = |dd[pos..)|^2.  Householder on J[:, pos..12).
  auto add_column = [&](bool doit, int pos, T dd, T dn2, T& nr_out, T r_in) __attribute__((always_inline)) {
    const T a0 = gsum((isvar && v == pos) ? dd : (T)0);  // d[pos]: row sum of a one-hot, no LDS round trip
    const T inr = rsqrt_nr(dn2 > 0 ? dn2 : (T)1);
    const T nr = dn2 * inr;  // |d2| = dn2 / sqrt(dn2)
    const T sg = (a0 >= 0) ? (T)1 : (T)-1;
    const T beta = rcp_nr(nr * (nr + fabs_t(a0)));
    T w_me = 0;
    if (doit && isvar) w_me = (v == pos) ? a0 + sg * nr : (v > pos ? dd : (T)0);
    T ya[3] = {0, 0, 0};
    sfor<0, 12>([&](auto jc) __attribute__((always_inline)) { constexpr int j = decltype(jc)::value; ya[j % 3] += Jr[j] * gbc<j>(w_me); });
    T y_me = (ya[0] + ya[1]) + ya[2];
    y_me = doit ? y_me * beta : (T)0;
    sfor<0, 12>([&](auto jc) __attribute__((always_inline)) { constexpr int j = decltype(jc)::value; Jr[j] -= y_me * gbc<j>(w_me); });
    sfor<0, 12>([&](auto ic) __attribute__((always_inline)) { constexpr int i = decltype(ic)::value; Jc[i] -= gbc<i>(y_me) * w_me; });
    const T rdn = -sg * inr;   // 1 / (new diagonal entry of R)
    if (doit && isvar) Rl[12 * pos] = (v < pos) ? -r_in * rdn : (v == pos ? rdn : (T)0);   // column `pos` of U = R^-1, every row
    nr_out = nr;
  };
  // d = J^T np for my column, np = (n0,n1,n2) on the variables of foot fp
  auto jt_np = [&](int fp, T n0, T n1, T n2) __attribute__((always_inline)) -> T {
    // foot selection by 0/1 weights, not by a select chain: clang turns `fp==0 ? Jc[0] : fp==1 ? Jc[3] ...` into a
    // run-time index, which forces the whole register array into scratch memory
    const T m0 = fp == 0 ? (T)1 : (T)0, m1 = fp == 1 ? (T)1 : (T)0, m2 = fp == 2 ? (T)1 : (T)0, m3 = fp == 3 ? (T)1 : (T)0;
    const T j0 = m0 * Jc[0] + m1 * Jc[3] + m2 * Jc[6] + m3 * Jc[9];
    const T j1 = m0 * Jc[1] + m1 * Jc[4] + m2 * Jc[7] + m3 * Jc[10];
    const T j2 = m0 * Jc[2] + m1 * Jc[5] + m2 * Jc[8] + m3 * Jc[11];
    return isvar ? j0 * n0 + j1 * n1 + j2 * n2 : (T)0;
  };
  // r = U d1 (U = R^-1 by rows, d1 = d[0 .. q)); kmax = wave-uniform bound on q
  auto dual_step = [&](T dd, int q, int kmax) __attribute__((always_inline)) -> T {
    T Urow[12];
    sfor<0, 12>([&](auto kc) __attribute__((always_inline)) { constexpr int k = decltype(kc)::value; Urow[k] = Rl[12 * k]; });
    const T ddm = (isvar && v < q) ? dd : (T)0;   // masked at the source lane: columns >= q of the image are stale
    T ra[3] = {0, 0, 0};
    sfor<0, 12>([&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value;
      if (k < kmax) ra[k % 3] += Urow[k] * gbc<k>(ddm);
    });
    return (isvar && v < q) ? (ra[0] + ra[1]) + ra[2] : (T)0;
  };
  // normal of constraint id: its three coefficients live in lane (id >> 1)
  auto normal_of = [&](int id, T& n0, T& n1, T& n2) __attribute__((always_inline)) {
    const T* c = Cl + 3 * (id & 31);
    n0 = c[0]; n1 = c[1]; n2 = c[2];
  };

#ifdef WBC_QP_STAMP
  const long long st_t1 = __builtin_readcyclecounter();
#endif
  pick();
  if (__ballot(!done && ip >= 0) != 0ull) build_J();
  int guard = 0;
#ifdef WBC_QP_STAMP
  long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long st_last = __builtin_readcyclecounter();
#endif
  while (__ballot(!done && ip >= 0) != 0ull) {
    if (++guard > 4 * prm.max_iter + 8) break;  // hard stop; per-row limits are enforced below
    bool go = !done && ip >= 0;
    if (go && ++iter > prm.max_iter) { status = 1; done = true; go = false; }
    const int ipc = ip < 0 ? 0 : ip;
    const int lp = (ipc >> 1) & 15, fp = lp >> 2;
    T np0, np1, np2;
    normal_of(ipc, np0, np1, np2);
    const T dd = jt_np(fp, np0, np1, np2);
    const T dn2 = gsum((isvar && v >= iq) ? dd * dd : (T)0);
    SEG(0);
    // z = J2 d2 (row copy, d broadcast and masked below iq)
    T z_me;
    {
      T za[3] = {0, 0, 0};  // three independent chains instead of one 12-deep FMA chain
      const T ddz = (isvar && v >= iq) ? dd : (T)0;  // mask at the source lane: one select instead of twelve
      sfor<0, 12>([&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        za[j % 3] += Jr[j] * gbc<j>(ddz);
      });
      z_me = (za[0] + za[1]) + za[2];
    }
    SEG(1);
    // r = R^-1 d1 : column-oriented back-substitution, row k of R lives in variable lane k
    T r_me = 0;
    {
      const int iqg = go ? iq : 0;
      int iqmax = __builtin_amdgcn_readlane(iqg, 0);
      { const int b1 = __builtin_amdgcn_readlane(iqg, 16), b2 = __builtin_amdgcn_readlane(iqg, 32), b3 = __builtin_amdgcn_readlane(iqg, 48);
        iqmax = iqmax > b1 ? iqmax : b1; iqmax = iqmax > b2 ? iqmax : b2; iqmax = iqmax > b3 ? iqmax : b3; }
      r_me = dual_step(dd, iq, iqmax);
    }
    SEG(2);
    // step lengths
    T t1 = INF;
    int kmin = isvar ? v : 15;
    {
      T t1k = KeyT<T>::BIG;
      if (isvar && v < iq && r_me > 0) t1k = u_me * rcp_nr(r_me);
      const bool found = gargmin(t1k, kmin);
      if (found) t1 = t1k;
    }
    T t2 = INF;
    if (dn2 > (EPS * Rnorm) * (EPS * Rnorm)) t2 = -sip * rcp_nr(dn2);  // z.np = |d2|^2
    if (go && !(t1 < INF) && !(t2 < INF)) { status = 2; done = true; go = false; }
    const bool dual_only = !(t2 < INF);
    const bool full = !dual_only && !(t1 < t2);
    const T t = full ? t2 : t1;
    if (go) {
      if (!dual_only) x_me += t * z_me;
      if (isvar && v < iq) u_me -= t * r_me;
      u_c += t;
    }
    SEG(3);
    // ---- full step: the candidate joins the active set
    // Executed unconditionally (predicated per row) and followed directly by the search for the next candidate, so
    // that the factor update and the independent slack/argmin chain share one basic block and interleave.
    const bool addg = go && full;
    {
      T nr;
      add_column(addg, iq, dd, dn2, nr, r_me);
      if (addg) {
        Rnorm = (nr > Rnorm) ? nr : Rnorm;
        if (l16 == lp) { if (ipc & 1) actB = true; else actA = true; }
        if (isvar && v == iq) { u_me = u_c; Aid = ipc; }
        ++iq;
        ip = -1;
      }
    }
    // rows that just added look for their next candidate now (rows that drop keep theirs: ip >= 0 there)
    pick();
    SEG(4);
    // ---- partial / dual-only step: the blocking constraint leaves, factors are rebuilt
    const bool dropg = go && !full;
    if (__ballot(dropg) != 0ull) {
      const int kq = dropg ? kmin : 0;
      const int cid = gread(Aid, (kq + kq / 3) & 15, rowbase);
      if (dropg && l16 == ((cid >> 1) & 15)) { if (cid & 1) actB = false; else actA = false; }
      // shift multipliers and ids down over the hole (positions kq+1..iq-1 move to kq..iq-2)
      {
        const int nxt = v + 1;
        const T un = gread(u_me, (nxt + nxt / 3) & 15, rowbase);
        const int An = gread(Aid, (nxt + nxt / 3) & 15, rowbase);
        if (dropg && isvar && v >= kq && v < iq - 1) { u_me = un; Aid = An; }
        if (dropg && isvar && v == iq - 1) { u_me = 0; Aid = -1; }
      }
      if (dropg) --iq;
      // restore J0 and re-add the remaining active constraints in order
      if (dropg) {
        if (isvar) {
          sfor<0, 12>([&](auto ic) __attribute__((always_inline)) { constexpr int i = decltype(ic)::value; Jc[i] = J0[i * 12 + v]; });
          sfor<0, 12>([&](auto cc) __attribute__((always_inline)) { constexpr int c = decltype(cc)::value; Jr[c] = J0[v * 12 + c]; });
        }
        Rnorm = 1;
      }
      for (int p = 0; p < 11; ++p) {
        const bool rg = dropg && p < iq;
        if (__ballot(rg) == 0ull) break;
        const int idp = gread(Aid, (p + p / 3) & 15, rowbase);
        const int idc = rg ? idp : 0;
        T m0, m1, m2;
        normal_of(idc, m0, m1, m2);
        const T dp = jt_np(((idc >> 1) & 15) >> 2, m0, m1, m2);
        const T dp2 = gsum((isvar && v >= p) ? dp * dp : (T)0);
        T nr;
        const T rp = dual_step(dp, rg ? p : 0, p);
        add_column(rg, p, dp, dp2, nr, rp);
        if (rg) Rnorm = (nr > Rnorm) ? nr : Rnorm;
      }
      {  // a partial step moved x: refresh the candidate's slack (cross-lane ops stay unconditional)
        T sA, sB;
        slacks(sA, sB);
        const T sv = gread((ipc & 1) ? sB : sA, lp, rowbase);
        if (dropg && !dual_only) sip = sv;
      }
    }
    SEG(5);
  }

  // ------------------------------------------------------------------ outputs: f, tau (a9), status
  if (live) {
    T taup = 0, jl0 = 0, jl1 = 0, jl2 = 0;  // own-leg Jacobian entries d pf_m / d q_(f,c3)
    int jm = 0;   // caller's index of my joint (leg f, joint c3)
    jm = (int)((unsigned)(a.jpack >> (4 * (v & 15))) & 15u);
    if (isvar) {
      taup = WSLD(WS_TAUP + v) - (RHAT ? WSLD(WS_RHAT + 6 + v) : (T)0);
      if (geom_jc) {
        jl0 = GLD(a.Jc, JC_LEG_WORD(f, 0, jm)); jl1 = GLD(a.Jc, JC_LEG_WORD(f, 1, jm)); jl2 = GLD(a.Jc, JC_LEG_WORD(f, 2, jm));
      } else {
        jl0 = WSLD(WS_JCL + 9 * f + 0 + c3); jl1 = WSLD(WS_JCL + 9 * f + 3 + c3); jl2 = WSLD(WS_JCL + 9 * f + 6 + c3);
      }
    }
    const T xq0 = dppx<0x00>(x_me), xq1 = dppx<0x55>(x_me), xq2 = dppx<0xAA>(x_me);
    if (isvar) {
      const T fx = on ? xq0 : (T)0, fy = on ? xq1 : (T)0, fz = on ? xq2 : (T)0;
      GST(a.f, v, on ? x_me : (T)0);
      GST(a.tau, jm, taup - (jl0 * fx + jl1 * fy + jl2 * fz));
    }
    if (l16 == 0) {
      a.status[s32] = status;
      GST_ITERS(iter);
    }
  }
#undef WSLD
#undef BLD
}

}  // namespace wbc
