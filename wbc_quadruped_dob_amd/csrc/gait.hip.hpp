// Gait scheduler: contact masks, footholds and swing plans on the device (include/wbc_hip.h at wbc_gait_batch).  The front of the per-tick loop
// gait -> reference_swing -> step -> integrate: a phase clock per robot, the foot schedule with late lift-off / early touchdown rules, and the
// nine plan words of every lifted foot (p0 latched at lift-off, the Raibert foothold p1, hgt, T, t0) written where wbc_swing_reference_batch reads them.
//   phi' = phi + dphi (wrapped);  phi_k = phi' + offset[k] (wrapped);  sched_k = phi_k < duty[k];  u_k = (phi_k - duty[k]) inv_sw[k]
//   bit_k = sched_k ? 1 : (prev_k ? u_k >= late : (contact_k && u_k >= late))
// Same lane mapping as the swing kernel (lane = 16*leg + state, one wavefront per workgroup): every lane runs the POSITION part of its leg's chain
// (restated from swing_leg_cmd: no velocities, no Jacobian) to get p_f, decides its foot's bit and writes its foot's plan words.  The four lanes of a
// state combine their bits with one wave64 ballot each for mask, lift-off and touchdown; the owner lane (leg 0) stores phase, mask and events.  Every
// lane has loaded phase and mask before that store: the stored values depend on those loads and a workgroup is exactly one wavefront, so the call is
// safe in place.
// Out of scope: the rollout kernels and wbc_rollout_*, wbc_multi_*, late touchdown (the schedule says stance and no contact is sensed), terrain-normal
// footholds, fusing this into com_swing_reference_kernel (its fp64 instantiation sits at 256 VGPRs).
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "dyn_sweep.hip.hpp"

namespace wbc {

// a[leg] of a kernel-argument array without a dynamically indexed copy (that would live in scratch)
template <class T> WBC_DEV T gait_sel(const T (&a)[4], int leg) { return leg == 0 ? a[0] : (leg == 1 ? a[1] : (leg == 2 ? a[2] : a[3])); }

// bits s, 16 + s, 32 + s, 48 + s of a ballot -> the state's four-bit word
WBC_DEV int gait_gather(unsigned long long b, unsigned s) {
  return (int)(((b >> s) & 1ull) | (((b >> (16 + s)) & 1ull) << 1) | (((b >> (32 + s)) & 1ull) << 2) | (((b >> (48 + s)) & 1ull) << 3));
}

template <class T>
__global__ __launch_bounds__(64) void gait_kernel(const DevModel<T>* __restrict__ model, GaitArgs<T> a) {
  __shared__ T cst[CST_WORDS];
  for (int i = threadIdx.x; i < CST_WORDS; i += blockDim.x) cst[i] = model->cst[i];
  __syncthreads();
  WBC_LAUNDERED_TID(tx);
  const size_t N = a.N;
  const LegLane lane_ = leg_lane<16>(tx, N);   // lanes beyond the batch recompute its last state and store nothing
  const int leg = lane_.leg;
  const unsigned st = lane_.st;
  const bool live = lane_.live;
  const unsigned s32 = lane_.s32;
  const T phase = a.phase[s32];
  const int prev = a.mask[s32];
  const int sensed = a.contact ? a.contact[s32] : 0;
  T qb[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) qb[c] = ROWI(a.q, c);
  const T vx = ROWI(a.v, 0), vy = ROWI(a.v, 1);
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
}

}  // namespace wbc
