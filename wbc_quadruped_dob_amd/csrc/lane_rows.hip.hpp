// The leg-lane kernels' common opening, stated once: which (state, leg) a lane works on, and where that state's words lie in the [rows][N] arrays.
// Every kernel that runs "one lane per (state, leg)" -- the sweeps, the split dynamics, the observer, the integrator, the references, the gait and
// the contact plant -- maps lane = 16 * leg + (state slot within the wavefront) and reaches component row `comp` of its state at ptr[comp * N + state].
// (qp_lane.hip.hpp maps one lane per state and the QP bodies stage their own operands: neither is a user of this file.)
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"

namespace wbc {

// The work-item id passes through an empty asm at the top of every body: inside the persistent rollout kernel the bodies
// sit in the horizon loop, and without this every lane-derived predicate, LDS address and table index (hundreds of
// registers' worth) is hoisted out of that loop as "invariant" and spilled.  One no-op per call elsewhere.
#define WBC_LAUNDERED_TID(name) unsigned name = threadIdx.x; asm volatile("" : "+v"(name))

// ---------------------------------------------------------------------------------------------------------------- the lane mapping
// tx: the (laundered) work-item id the mapping was formed from; leg = row of 16 lanes within the wavefront; st = state slot within the wavefront;
// s32: the state the lane COMPUTES; live: that state is the lane's own and lies inside the batch (a lane that is not live stores nothing, or
// stores bit-identical duplicates: the body's choice, see the guards at its stores).
struct LegLane {
  unsigned tx;
  int leg;
  unsigned st, s32;
  bool live;
};
// The shapes differ in the state a lane would take, s_raw; they share the rest: a lane beyond the batch takes the batch's last state(s), N - W; a
// lane beyond the workgroup's SPW slots (roles of workgroups that own fewer than 16 states) repeats the workgroup's first state.
//   (a) WBC_SRAW_A: one wavefront per workgroup, or a role (one wavefront of a larger workgroup): the workgroup owns SPW <= 16 consecutive states
//   (b), (c) WBC_SRAW_W: BLOCK / 64 wavefronts of 16 lanes per leg, W consecutive states per lane (W = 2: N is even, so both states of a lane are in
//       range together); blk = the workgroup's index (a kernel may run several bodies side by side and number them itself: tile_tick.hip.hpp)
// Stated as macros over a body's `tx` and `N` that leave N32, leg, s_raw, slot_ok, live, s32 and legN as locals, in the order the bodies always
// stated them: leg_lane() below wraps them for the kernels that take the mapping as a LegLane (gait, the contact plant), and the bodies whose device
// code moves when the values come back through a struct (the roles of the one-launch tick and of the rollouts, the tile tick's bodies, swing_ref: a
// changed order of two scalar instructions is enough) expand WBC_LEG_LANE themselves -- docs/DESIGN_HISTORY.md.
// (s32 is left assignable: the RS_LANE2 role re-aims a lane.)
#define WBC_SRAW_A(SPW_) ((size_t)blockIdx.x * SPW_ + (tx & 15))
#define WBC_SRAW_W(BLOCK_, W_, blk) ((((size_t)(blk) * (BLOCK_ / 64) + (tx >> 6)) * 16 + (tx & 15)) * W_)
#define WBC_LEG_LANE_HEAD_                                                                                        \
  const unsigned N32 = (unsigned)N;                                                                               \
  (void)N32;                                                                                                      \
  const int leg = (int)((tx & 63) >> 4);
#define WBC_LEG_LANE_STATE_(SPW_, W_, s_raw_expr)                                                                 \
  const size_t s_raw = (s_raw_expr);                                                                              \
  const bool slot_ok = SPW_ == 16 || (int)(tx & 15) < SPW_;   /* (a constant for SPW = 16: folded where it is used) */ \
  const bool live = slot_ok && s_raw < N;                                                                         \
  unsigned s32 = (unsigned)(live ? s_raw : (slot_ok ? N - W_ : (size_t)blockIdx.x * SPW_));                       \
  const unsigned legN = (unsigned)leg * N32;                                                                      \
  (void)legN;
#define WBC_LEG_LANE(SPW_, W_, s_raw_expr) WBC_LEG_LANE_HEAD_ WBC_LEG_LANE_STATE_(SPW_, W_, s_raw_expr)
// shape (a) as a value; tx = the caller's laundered work-item id
template <int SPW = 16>
WBC_DEV LegLane leg_lane(unsigned tx, size_t N) {
  WBC_LEG_LANE_HEAD_
  const unsigned st = tx & 15;
  WBC_LEG_LANE_STATE_(SPW, 1, WBC_SRAW_A(SPW))
  return LegLane{tx, leg, st, s32, live};
}

// ---------------------------------------------------------------------------------------------------------------- the address forms
// Where the lane's words lie.  Every array is < 4 GiB (max_batch is capped at create), so a word is reached as (uniform 64-bit base in SGPRs) +
// (32-bit per-lane byte offset): no 64-bit vector address arithmetic.  Two forms, on purpose:
//   LDU / ROWU  component index wave-uniform: the row goes into the 64-bit base, the lane adds its 32-bit scaled state offset
//   LDV / ROWV  component index differs per lane: one 32-bit offset
//   LDL / ROWL  leg-strided: row c0 + stride * leg;  LDX, LDLX / ROWLX: + an element offset xN = x * N of the lane's own behind row c0
// Macros over the names a body defines -- N, N32, s32, legN (the mapping above) and RowV, what a lane loads and stores: the scalar T, or a packed
// pair of T where a lane carries two states.  sizeof(T) scales the state either way.  LD*: inputs.  ROW*: lvalues for the stores, so that the guard
// (`live`, `UNGUARD || live`, none) and the store policy stand at the call site.
// (Typed members over a LaneRows-like object were tried for these forms: the index forms below keep the contact kernels' device code, the byte
// forms moved the one-launch tick's, the rollouts' and the payload integrator's -- docs/DESIGN_HISTORY.md.)
#define ROW_AT(V_, ptr, bytes) (*(V_*)((char*)(ptr) + (bytes)))
#define ROW_BU_ (size_t)(s32 * (unsigned)sizeof(T))
#define ROW_BV_(comp, s) (size_t)(((unsigned)(comp) * N32 + (s)) * (unsigned)sizeof(T))
#define ROW_BX_(xN) (size_t)(((xN) + s32) * (unsigned)sizeof(T))
#define ROW_BL_(stride) (size_t)(((unsigned)(stride) * legN + s32) * (unsigned)sizeof(T))
#define ROW_BLX_(stride, xN) (size_t)(((unsigned)(stride) * legN + (xN) + s32) * (unsigned)sizeof(T))
#define LDU(ptr, comp) ROW_AT(const RowV, (ptr) + (size_t)(comp) * N, ROW_BU_)
#define LDV(ptr, comp) ROW_AT(const RowV, ptr, ROW_BV_(comp, s32))
#define LDX(ptr, c0, xN) ROW_AT(const RowV, (ptr) + (size_t)(c0) * N, ROW_BX_(xN))
#define LDL(ptr, c0, stride) ROW_AT(const RowV, (ptr) + (size_t)(c0) * N, ROW_BL_(stride))
#define LDLX(ptr, c0, stride, xN) ROW_AT(const RowV, (ptr) + (size_t)(c0) * N, ROW_BLX_(stride, xN))
#define ROWU(ptr, comp) ROW_AT(RowV, (ptr) + (size_t)(comp) * N, ROW_BU_)
#define ROWV(ptr, comp) ROW_AT(RowV, ptr, ROW_BV_(comp, s32))
#define ROWL(ptr, c0, stride) ROW_AT(RowV, (ptr) + (size_t)(c0) * N, ROW_BL_(stride))
#define ROWLX(ptr, c0, stride, xN) ROW_AT(RowV, (ptr) + (size_t)(c0) * N, ROW_BLX_(stride, xN))
// a pair store: the lanes (l, l + 1) of a row pair up and each writes one word of type T2_ for the states of both, s2 = the pair's first state
#define ROWV2(T2_, ptr, comp, s2) ROW_AT(T2_, ptr, ROW_BV_(comp, s2))
// four base-replicated words, one per lane of the quad: lane `leg` takes row c<leg> (the caller deals the values the same way, sel4<RowV>(leg, ...))
#define ROWV4(ptr, leg, c0, c1, c2, c3) ROWV(ptr, sel4<int>(leg, c0, c1, c2, c3))

// The index forms (elements of the caller's array; the load stays on the caller's __restrict__ pointer): row comp of the state, and row
// c0 + stride * leg of it (the leg's block of `stride` rows).  Typed for the contact kernels ...
struct LaneRows {
  size_t N;
  unsigned legN, s32;
  WBC_DEV LaneRows(int leg, unsigned s32_, unsigned N32) : N(N32), legN((unsigned)leg * N32), s32(s32_) {}
  WBC_DEV size_t idx(int comp) const { return (size_t)comp * N + s32; }
  WBC_DEV size_t leg_idx(int c0, int stride) const { return (size_t)c0 * N + (size_t)((unsigned)stride * legN + s32); }
};
// ... and as a macro over the body's own N and s32 for gait and swing_ref, whose row multiples came out as other instructions under idx()
#define ROWI(ptr, comp) ((ptr)[(size_t)(comp) * N + s32])

// the per-leg constant table (LDS, [word][leg]): word i of the lane's leg, for a body that names the table `cst` and its leg `leg`
#define CS(i) cst[(i) * 4 + leg]

}  // namespace wbc
