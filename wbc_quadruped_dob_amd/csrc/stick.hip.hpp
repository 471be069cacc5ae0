// Stiction on the ground plant (include/wbc_hip.h at wbc_ground_stick_force_batch): the contact law of ground.hip.hpp with a per-foot anchor spring,
// so that a loaded foot holds its place instead of creeping at F / c_t.  The new state is the caller's and advances IN PLACE: anchor [12][N] (rows
// 3k .. 3k+2 = the world point foot k is stuck to) and stick [N] (in: bit k = foot k has an anchor; out: bit k = loaded, bit 4+k = slid this tick).
// p_f, v_f, phi, v_n, v_t, f_n, the contact bit and the gap are formed exactly as ground_law forms them.  The lines are restated here and not shared:
// behind a common helper (two shapes tried, docs/DESIGN_HISTORY.md) k_ground assembles as before and this unit keeps its instruction counts, but its
// loads are scheduled differently and stick_force_kernel measured 5 - 10 % slower.  Only the addresses (LaneRows) and the lane mapping (foot_lane, LegLane) are
// ground.hip.hpp's.  Then, per foot:
//   f_n == 0:  f_t = 0, both out bits clear, the anchor words untouched
//   f_n  > 0:  a = in bit ? anchor : p_f          (first loaded tick: the anchor is dropped where the foot is)
//              e = (p_f - a) - n (n . (p_f - a))  g = -k_t e - c_t v_t        cone = mu f_n
//              |g| >  cone:  s = cone / |g|, f_t = s g, anchor := p_f - s e, slid    (the stretch shrinks by the factor the force does)
//              |g| <= cone:  f_t = g, the anchor stays (a new one = p_f)
//   f_gr = f_n n + f_t
// k_t = 0 gives the stateless law's force as numbers: g = -0 e - c_t v_t.
// Same lane mapping as the ground kernels (lane = 16*leg + state, one wavefront per workgroup): a lane evaluates its foot, reads and writes only its own
// three anchor words, and stores them only where the law moves them.  The state's four lanes read the stick word; the leg-0 lane stores the new one
// after two wave64 ballots (loaded, slid) through gait_gather.  Lanes beyond the batch recompute its last state and store nothing.  No LDS.
// The stick word advances in place for the reason q, v do in ground.hip.hpp: a lane's slide decision is formed from its stretch e, which is formed
// from the anchor the in bit selects, so the ballot that makes the new word waits for the stick load of every lane of the wavefront -- and a state's
// four lanes share a wavefront.  The anchor words likewise: a lane stores only what it has formed from its own load of them.
// stick_integrate_kernel: the law, then integrate_body<.., GROUND> with the lane's force in registers, as ground_integrate_kernel hands it over.  The
// law's values, the anchor included, are dead before integrate_body starts, apart from the three force words.
// Out of scope: the payload plant, the rollout kernels and wbc_rollout_*, wbc_multi_*, late touchdown in the gait rule, terrain-normal footholds.
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "ground.hip.hpp"

namespace wbc {

WBC_DEV double stick_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
WBC_DEV float stick_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// what one lane's foot leaves beside f_gr
template <class T> struct StickOut {
  T phi;
  V3<T> anchor;   // the new anchor, stored where `move` is set
  bool touch, loaded, slid, move;
};

// one lane's foot: returns f_gr.  s32 = the state the lane computes, N32 = the batch size.
template <class T>
WBC_DEV V3<T> stick_law(const T* __restrict__ q, const T* __restrict__ v, const T* __restrict__ Jc, const GroundIO<T>& g, const StickIO<T>& sk,
                        unsigned long long jpack, int leg, unsigned s32, unsigned N32, StickOut<T>& o) {
  const LaneRows A(leg, s32, N32);
  int jx[3];
  jidx_of_leg((const DevModel<T>*)nullptr, jpack, leg, jx);
  // (ground_law's loads and arithmetic, word for word, down to f_n: a change there is a change here, contraction included)
  const V3<T> dl = mk<T>(Jc[A.leg_idx(18 * 1 + 5, 54)], Jc[A.leg_idx(18 * 2 + 3, 54)], Jc[A.leg_idx(18 * 0 + 4, 54)]);
  T jcl[3][3], qd[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int col = 6 + jx[k];
    jcl[0][k] = Jc[A.leg_idx(0 + col, 54)]; jcl[1][k] = Jc[A.leg_idx(18 + col, 54)]; jcl[2][k] = Jc[A.leg_idx(36 + col, 54)];
    qd[k] = v[A.idx(col)];
  }
  const V3<T> pb = mk<T>(q[A.idx(0)], q[A.idx(1)], q[A.idx(2)]);
  const V3<T> vb = mk<T>(v[A.idx(0)], v[A.idx(1)], v[A.idx(2)]), om = mk<T>(v[A.idx(3)], v[A.idx(4)], v[A.idx(5)]);
  const V3<T> n = mk<T>(g.normals[A.leg_idx(0, 3)], g.normals[A.leg_idx(1, 3)], g.normals[A.leg_idx(2, 3)]);
  const T d = g.height[A.leg_idx(0, 1)], mu = g.mu[A.leg_idx(0, 1)];
  const V3<T> a_in = mk<T>(sk.anchor[A.leg_idx(0, 3)], sk.anchor[A.leg_idx(1, 3)], sk.anchor[A.leg_idx(2, 3)]);
  const bool had = ((sk.stick[s32] >> leg) & 1) != 0;
  const V3<T> pf = pb + dl;
  const V3<T> vf = vb + cross(om, dl) + mk<T>(jcl[0][0] * qd[0] + jcl[0][1] * qd[1] + jcl[0][2] * qd[2],
                                              jcl[1][0] * qd[0] + jcl[1][1] * qd[1] + jcl[1][2] * qd[2],
                                              jcl[2][0] * qd[0] + jcl[2][1] * qd[1] + jcl[2][2] * qd[2]);
  o.phi = dot(n, pf) - d;
  const T vn = dot(n, vf);
  const V3<T> vt = vf - n * vn;
  const T raw = -g.P.k_n * o.phi - g.P.c_n * vn;
  const T fn = (o.phi < (T)0 && raw > (T)0) ? raw : (T)0;
  o.loaded = fn > (T)0;
  // the anchor spring: an unloaded foot or one without an anchor has e = 0 exactly (its anchor words are not looked at)
  const bool use = had && o.loaded;
  const V3<T> a = mk<T>(use ? a_in.x : pf.x, use ? a_in.y : pf.y, use ? a_in.z : pf.z);
  // (explicit multiply-adds from here to g: left to the compiler, the two kernels contracted these lines differently, and the fp32 force of the
  // one-launch plant differed from the stand-alone law's in the last bit on anchored feet.  g = fma(e, -k_t, -c_t v_t): with k_t = 0 the stateless g)
  const V3<T> da = pf - a;
  const T nda = stick_fma(n.z, da.z, stick_fma(n.y, da.y, n.x * da.x));
  const V3<T> e = mk<T>(stick_fma(-n.x, nda, da.x), stick_fma(-n.y, nda, da.y), stick_fma(-n.z, nda, da.z));
  const V3<T> gv = vt * (-g.P.c_t);
  const V3<T> gt = mk<T>(stick_fma(e.x, -sk.k_t, gv.x), stick_fma(e.y, -sk.k_t, gv.y), stick_fma(e.z, -sk.k_t, gv.z));
  const T gn = ground_sqrt(dot(gt, gt));
  const T cone = mu * fn;
  const bool over = gn > cone;
  const T s = over ? cone / gn : (T)1;   // (gn > cone >= 0 implies gn > 0: no 0/0; gn = 0 gives s = 1 and f_t = g = 0)
  o.touch = fn > g.P.f_touch;
  o.slid = o.loaded && over;
  o.move = o.loaded && (over || !had);   // a sticking foot's anchor stays bit for bit: not stored
  o.anchor = o.slid ? mk<T>(stick_fma(-e.x, s, pf.x), stick_fma(-e.y, s, pf.y), stick_fma(-e.z, s, pf.z)) : pf;
  return n * fn + gt * s;
}

// the lane's stores: ground_store's, its anchor words where the law moved them, and (leg-0 lane) the state's new stick word
template <class T>
WBC_DEV void stick_store(const GroundIO<T>& g, const StickIO<T>& sk, int leg, unsigned st, unsigned s32, unsigned N32, bool live, V3<T> f,
                         const StickOut<T>& o) {
  const size_t N = N32;
  const unsigned long long bc = __ballot(o.touch);
  const unsigned long long bl = __ballot(o.loaded);
  const unsigned long long bs = __ballot(o.slid);
  if (live) {
    T* const fo = g.f_gr + (size_t)(3 * leg) * N + s32;
    fo[0] = f.x; fo[N] = f.y; fo[2 * N] = f.z;
    if (g.gap) g.gap[(size_t)leg * N + s32] = o.phi;
    if (o.move) {
      T* const ao = sk.anchor + (size_t)(3 * leg) * N + s32;
      ao[0] = o.anchor.x; ao[N] = o.anchor.y; ao[2 * N] = o.anchor.z;
    }
    if (leg == 0) {
      if (g.contact) g.contact[s32] = gait_gather(bc, st);
      sk.stick[s32] = gait_gather(bl, st) | (gait_gather(bs, st) << 4);
    }
  }
}

template <class T>
__global__ __launch_bounds__(64) void stick_force_kernel(StickArgs<T> a) {
  const LegLane l = foot_lane(a.N);
  StickOut<T> o;
  const V3<T> f = stick_law<T>(a.q, a.v, a.Jc, a.g, a.s, a.jpack, l.leg, l.s32, (unsigned)a.N, o);
  stick_store<T>(a.g, a.s, l.leg, l.st, l.s32, (unsigned)a.N, l.live, f, o);
}

template <class T>
__global__ __launch_bounds__(64) void stick_integrate_kernel(const DevModel<T>* __restrict__ model, StickIntegrateArgs<T> a) {
  const LegLane l = foot_lane(a.N);
  StickOut<T> o;
  const V3<T> f = stick_law<T>(a.q, a.v, a.Jc, a.g, a.s, a.jpack, l.leg, l.s32, (unsigned)a.N, o);
  stick_store<T>(a.g, a.s, l.leg, l.st, l.s32, (unsigned)a.N, l.live, f, o);
  integrate_body<T, 16, IntegrateNoWait, 0, false, false, false, IntegrateNoWait, false, false, false, true>(
      model, a, IntegrateNoWait(), nullptr, nullptr, nullptr, IntegrateNoWait(), nullptr, nullptr, f);
}

}  // namespace wbc
