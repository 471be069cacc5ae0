// Contact sensing from the disturbance observer (include/wbc_hip.h at wbc_contact_estimate_batch): foot forces estimated from the momentum observer's
// residual r, and a contact word with hysteresis formed from them -- the controller-side producer of wbc_gait_batch's `contact` input, where the ground
// plant's word is simulator ground truth.  r estimates the generalized force beyond the planned Jc^T f_prev; the joint rows of a leg see only that
// leg's own foot, so per foot k, with jx the leg's joint indices (jidx_of_leg: reordered models work) and J_leg the own-leg 3x3 block of Jc that
// ground_law and integrate_body read:
//   A      = J_leg,k^T                      (3x3)
//   det    = det A
//   ok     = |det| > det_min
//   df     = ok ? adj(A) r_joint / det : 0  (adjugate form: no pivoting, no division when !ok)
//   f_est  = f_prev,k + df
//   fn     = n_k . f_est
//   bit_k  = !ok ? previous bit : (previous bit ? fn > f_off : fn > f_on)
// Only bits 0-3 of `contact` are read or written (the others are stored back as they were loaded).
// Same lane mapping as the gait and ground kernels (lane = 16*leg + state, one wavefront per workgroup): a lane loads its nine Jc words (the words
// ground_law loads), three r words, three f_prev words and three normals, solves in registers and stores its rows of f_est and fn_est; the four lanes
// of a state combine their bits with one wave64 ballot each (gait_gather) and the leg-0 lane stores contact and singular.  Lanes beyond the batch
// recompute its last state and store nothing.
// gait_estimated_kernel: the law, then the gait scheduler's body (gait_body.inc.hpp, the text gait_kernel is made of) with the word in registers --
// the word is stored for the caller, never read back.
// `contact` advances in place: every lane has loaded the previous word before the ballot that the stored word depends on, and a state's four lanes
// share a wavefront, so no lane can meet the new word.
// Out of scope: the base rows of r, a contact observer of its own, the rollout kernels and wbc_rollout_*, wbc_multi_*, the payload plant, late
// touchdown in the gait rule, terrain-normal footholds.
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "dyn_sweep.hip.hpp"
#include "gait.hip.hpp"

namespace wbc {

WBC_DEV double contact_abs(double x) { return fabs(x); }
WBC_DEV float contact_abs(float x) { return fabsf(x); }

// one lane's foot: returns f_est, leaves n . f_est in `fn`, the new bit in `bit`, !ok in `sing` and the word as loaded in `prev`.
// s32 = the state the lane computes, N32 = the batch size.
template <class T>
WBC_DEV V3<T> contact_law(const ContactIO<T>& c, unsigned long long jpack, int leg, unsigned s32, unsigned N32, T& fn, bool& bit, bool& sing, int& prev) {
  const LaneRows A(leg, s32, N32);   // (indices, not words: the loads stay on the __restrict__ pointers)
  int jx[3];
  jidx_of_leg((const DevModel<T>*)nullptr, jpack, leg, jx);
  prev = c.contact[s32];
  // columns of A = J_leg^T are the rows of the own-leg block: a_i[k] = Jc[3 leg + i][6 + jx[k]]
  T a[3][3], rj[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int col = 6 + jx[k];
    a[0][k] = c.Jc[A.leg_idx(0 + col, 54)]; a[1][k] = c.Jc[A.leg_idx(18 + col, 54)]; a[2][k] = c.Jc[A.leg_idx(36 + col, 54)];
    rj[k] = c.r[A.idx(col)];
  }
  const V3<T> fp = mk<T>(c.f_prev[A.leg_idx(0, 3)], c.f_prev[A.leg_idx(1, 3)], c.f_prev[A.leg_idx(2, 3)]);
  const V3<T> n = mk<T>(c.normals[A.leg_idx(0, 3)], c.normals[A.leg_idx(1, 3)], c.normals[A.leg_idx(2, 3)]);
  const V3<T> a0 = mk<T>(a[0][0], a[0][1], a[0][2]), a1 = mk<T>(a[1][0], a[1][1], a[1][2]), a2 = mk<T>(a[2][0], a[2][1], a[2][2]);
  const V3<T> rv = mk<T>(rj[0], rj[1], rj[2]);
  // adj(A) r = (r . a1 x a2, r . a2 x a0, r . a0 x a1), det A = a0 . a1 x a2
  const V3<T> c12 = cross(a1, a2), c20 = cross(a2, a0), c01 = cross(a0, a1);
  const T det = dot(a0, c12);
  sing = !(contact_abs(det) > c.P.det_min);
  V3<T> df = mk<T>((T)0, (T)0, (T)0);
  if (!sing) df = mk<T>(dot(rv, c12) / det, dot(rv, c20) / det, dot(rv, c01) / det);
  const V3<T> f = fp + df;
  fn = dot(n, f);
  const bool was = ((prev >> leg) & 1) != 0;
  bit = sing ? was : (fn > (was ? c.P.f_off : c.P.f_on));
  return f;
}

// the lane's stores: three rows of f_est, its fn_est, and (leg-0 lane) the state's words.  Returns the new four-bit word to every lane of the state.
template <class T>
WBC_DEV int contact_store(const ContactIO<T>& c, int leg, unsigned st, unsigned s32, unsigned N32, bool live, V3<T> f, T fn, bool bit, bool sing,
                          int prev) {
  const size_t N = N32;
  const unsigned long long bc = __ballot(bit), bs = __ballot(sing);
  const int word = gait_gather(bc, st);
  if (live) {
    if (c.f_est) {
      T* const fo = c.f_est + (size_t)(3 * leg) * N + s32;
      fo[0] = f.x; fo[N] = f.y; fo[2 * N] = f.z;
    }
    if (c.fn_est) c.fn_est[(size_t)leg * N + s32] = fn;
    if (leg == 0) {
      c.contact[s32] = (prev & ~15) | word;
      if (c.singular) c.singular[s32] = gait_gather(bs, st);
    }
  }
  return word;
}

template <class T>
__global__ __launch_bounds__(64) void contact_estimate_kernel(ContactArgs<T> a) {
  WBC_LAUNDERED_TID(tx);
  const LegLane l = leg_lane<16>(tx, a.N);
  T fn; bool bit, sing; int prev;
  const V3<T> f = contact_law<T>(a.c, a.jpack, l.leg, l.s32, (unsigned)a.N, fn, bit, sing, prev);
  (void)contact_store<T>(a.c, l.leg, l.st, l.s32, (unsigned)a.N, l.live, f, fn, bit, sing, prev);
}

template <class T>
__global__ __launch_bounds__(64) void gait_estimated_kernel(const DevModel<T>* __restrict__ model, GaitEstimatedArgs<T> ea) {
  int word;
  {
    WBC_LAUNDERED_TID(tx);
    const LegLane l = leg_lane<16>(tx, ea.g.N);
    T fn; bool bit, sing; int prev;
    const V3<T> f = contact_law<T>(ea.c, ea.g.jpack, l.leg, l.s32, (unsigned)ea.g.N, fn, bit, sing, prev);
    word = contact_store<T>(ea.c, l.leg, l.st, l.s32, (unsigned)ea.g.N, l.live, f, fn, bit, sing, prev);
  }
  // the gait scheduler's body on the same lane mapping (it forms the same leg_lane from the same work-item id), the word in registers
  const GaitArgs<T>& a = ea.g;
#define GAIT_SENSED_WORD word
#include "gait_body.inc.hpp"
#undef GAIT_SENSED_WORD
}

}  // namespace wbc
