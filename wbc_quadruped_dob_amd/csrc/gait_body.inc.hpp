// The body of the gait scheduler (gait.hip.hpp), as text: included by gait_kernel and by gait_estimated_kernel (contact_est.hip.hpp), which forms the
// sensed word in the same launch.  As a function template over "the word is given" the body moved gait_kernel's register allocation; as text,
// gait_kernel assembles as before.  The includer provides `model` (const DevModel<T>*), `a` (GaitArgs<T>, or a reference to one) and the macro
// GAIT_SENSED_WORD: the expression for the four sensed bits of state s32 (gait_kernel: a.contact ? a.contact[s32] : 0).
// Optional hooks of the same kind, for an includer that holds the base state in registers (gait_estimated_odom_kernel, odom.hip.hpp); left
// undefined they are today's text:  GAIT_BASE_Q(c) row c of q for c = 0 .. 6,  GAIT_BASE_V(c) row c of v for c = 0, 1,  GAIT_CST_STAGED the
// includer has declared and staged `cst` itself.
#ifndef GAIT_BASE_Q
#define GAIT_BASE_Q(c) ROWI(a.q, c)
#define GAIT_BASE_Q_DEFAULTED_
#endif
#ifndef GAIT_BASE_V
#define GAIT_BASE_V(c) ROWI(a.v, c)
#define GAIT_BASE_V_DEFAULTED_
#endif
#ifndef GAIT_CST_STAGED
  __shared__ T cst[CST_WORDS];
  for (int i = threadIdx.x; i < CST_WORDS; i += blockDim.x) cst[i] = model->cst[i];
  __syncthreads();
#endif
  WBC_LAUNDERED_TID(tx);
  const size_t N = a.N;
  const LegLane lane_ = leg_lane<16>(tx, N);   // lanes beyond the batch recompute its last state and store nothing
  const int leg = lane_.leg;
  const unsigned st = lane_.st;
  const bool live = lane_.live;
  const unsigned s32 = lane_.s32;
  const T phase = a.phase[s32];
  const int prev = a.mask[s32];
  const int sensed = GAIT_SENSED_WORD;
  T qb[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) qb[c] = GAIT_BASE_Q(c);
  const T vx = GAIT_BASE_V(0), vy = GAIT_BASE_V(1);
  const T cvx = ROWI(a.cmd, 0), cvy = ROWI(a.cmd, 1), wz = ROWI(a.cmd, 2), zg = ROWI(a.cmd, 3);
  int jx[3];
  jidx_of_leg(model, a.jpack, leg, jx);
  T ql[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) ql[k] = ROWI(a.q, 7 + jx[k]);
  M3<T> R;
  {
    const T n = rsqrt_t(qb[3] * qb[3] + qb[4] * qb[4] + qb[5] * qb[5] + qb[6] * qb[6]);
    const T x = qb[3] * n, y = qb[4] * n, z = qb[5] * n, w = qb[6] * n;
    R.a[0] = 1 - 2 * (y * y + z * z); R.a[1] = 2 * (x * y - z * w);     R.a[2] = 2 * (x * z + y * w);
    R.a[3] = 2 * (x * y + z * w);     R.a[4] = 1 - 2 * (x * x + z * z); R.a[5] = 2 * (y * z - x * w);
    R.a[6] = 2 * (x * z - y * w);     R.a[7] = 2 * (y * z + x * w);     R.a[8] = 1 - 2 * (x * x + y * y);
  }
  // the foot point: origins down the leg in base coordinates (the position part of swing_leg_cmd)
  V3<T> o = mk<T>((T)0, (T)0, (T)0);
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
    if (k == 0) {
      o = r;
      A = E;
    } else {
      o = o + mul(A, r);
      M3<T> B;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B.a[3 * i + j] = A.a[3 * i] * E.a[j] + A.a[3 * i + 1] * E.a[3 + j] + A.a[3 * i + 2] * E.a[6 + j];
      A = B;
    }
  }
  const V3<T> d = o + mul(A, mk<T>(CS(3 * JOINT_WORDS), CS(3 * JOINT_WORDS + 1), CS(3 * JOINT_WORDS + 2)));
  const V3<T> pf = mk<T>(qb[0], qb[1], qb[2]) + mul(R, d);

  // the clock and the schedule: additions, subtractions, comparisons and the one rounded product u
  const DevGaitParams<T>& P = a.P;
  const T duty = gait_sel(P.duty, leg), Tsw = gait_sel(P.T_sw, leg);
  T ph = phase + P.dphi;
  if (ph >= (T)1) ph -= (T)1;
  T pk = ph + gait_sel(P.offset, leg);
  if (pk >= (T)1) pk -= (T)1;
  const bool sched = pk < duty;
  const T u = (pk - duty) * gait_sel(P.inv_sw, leg);
  const bool was = ((prev >> leg) & 1) != 0;
  const bool lateu = u >= P.late;
  const bool bit = sched || (lateu && (was || ((sensed >> leg) & 1) != 0));
  const bool lift = was && !bit, touch = !was && bit;
  const unsigned long long bm = __ballot(bit), bl = __ballot(lift), bt = __ballot(touch);

  if (live && !bit) {
    T* const sw = a.swing + (size_t)(9 * leg) * N + s32;
    if (lift) {
      sw[0] = pf.x; sw[N] = pf.y; sw[2 * N] = pf.z;
      sw[6 * N] = P.clearance; sw[7 * N] = Tsw;
    }
    sw[8 * N] = u * Tsw;
    if (lift || P.retarget) {
      // Raibert foothold in the heading frame h = (R00, R10) / |.|
      const T hn = rsqrt_t(R.a[0] * R.a[0] + R.a[3] * R.a[3]);
      const T hx = R.a[0] * hn, hy = R.a[3] * hn;
      const T nx = gait_sel(P.bx, leg), ny = gait_sel(P.by, leg);
      const T bx = hx * nx - hy * ny, by = hy * nx + hx * ny;
      const T cx = hx * cvx - hy * cvy, cy = hy * cvx + hx * cvy;
      const T Trem = ((T)1 - u) * Tsw;
      const T hst = (T)0.5 * (duty * P.period);
      sw[3 * N] = qb[0] + bx + vx * Trem + hst * cx + P.k_v * (vx - cx) + hst * wz * (-by);
      sw[4 * N] = qb[1] + by + vy * Trem + hst * cy + P.k_v * (vy - cy) + hst * wz * bx;
      sw[5 * N] = zg;
    }
  }
  if (live && leg == 0) {
    a.phase[s32] = ph;
    a.mask[s32] = gait_gather(bm, st);
    if (a.events) a.events[s32] = gait_gather(bl, st) | (gait_gather(bt, st) << 4);
  }
#ifdef GAIT_BASE_Q_DEFAULTED_
#undef GAIT_BASE_Q
#undef GAIT_BASE_Q_DEFAULTED_
#endif
#ifdef GAIT_BASE_V_DEFAULTED_
#undef GAIT_BASE_V
#undef GAIT_BASE_V_DEFAULTED_
#endif
