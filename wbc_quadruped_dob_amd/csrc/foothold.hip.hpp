// Foothold selection (include/wbc_hip.h at "Foothold selection"): a cost per node of the terrain map, and per lifted foot a search of the nodes around
// the gait rule's foothold for the cheapest one, latched as a POINT until the foot is down again.
//   terrain_cost_kernel                   cost[c] = w_step step(c) + w_slope slope2(c) per node: a 2-D stencil over an LDS tile of COST_TX x COST_TY nodes
//                                         with a halo of COST_HALO nodes whose indices are clipped to the grid on the way in, so that the stencil
//                                         itself has no border case but the slope's factor
//   foothold_select_kernel                the selection law alone on the mask and swing a gait call left (leg-lane mapping: lane = 16*leg + state,
//                                         one wavefront per workgroup; lanes beyond the batch recompute its last state and store nothing)
//   gait_terrain_select_kernel            gait_kernel's body (gait_body.inc.hpp, as text), the law, then terrain_feet_tail_at: gait_terrain_kernel with
//                                         foothold_lane between its two halves
//   gait_estimated_terrain_select_kernel  the same behind the contact law (gait_estimated_terrain_kernel's text)
// foothold_lane is one lane's law.  It reads p1_x, p1_y (and T, t0) back from `swing`: in the fused kernels the lane's own earlier store is ordered
// before its load.  It hands p1_x, p1_y as it leaves them to terrain_feet_tail_at in registers -- the bits terrain_feet_tail would read back.
// The four lanes of a state combine their latch and "selected" bits with one wave64 ballot each and the owner lane (leg 0) stores the word; every
// lane has loaded the word before that store and a workgroup is exactly one wavefront, so `latch` advances safely in place.
// The common path is one gather of `cost` per lifted foot.  The window (at most 9 x 9 gathers from a map that sits in L2) runs only in the lanes
// that start a selection and is divergent by design; it is not staged through LDS.  Contraction is off in the law and in the cost: J and cost are then
// the same roundings as the numpy restatement's (tests/foothold_ref.py), product by product.
// Out of scope: the rollout kernels and wbc_rollout_*, wbc_multi_*, late touchdown, terrain sensing, smoothed normals, kinematic reachability of the
// chosen node (the window is at most 4 cells wide each way).
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "terrain.hip.hpp"

namespace wbc {

constexpr int COST_TX = 32, COST_TY = 8, COST_HALO = 2;   // COST_HALO = the largest margin the host lets through (>= 1: the slope's own reach)

WBC_DEV double foothold_abs(double a) { return fabs(a); }
WBC_DEV float foothold_abs(float a) { return fabsf(a); }
WBC_DEV double foothold_floor(double a) { return floor(a); }
WBC_DEV float foothold_floor(float a) { return floorf(a); }

template <class T>
__global__ __launch_bounds__(COST_TX * COST_TY) void terrain_cost_kernel(TerrainCostArgs<T> a) {
#pragma clang fp contract(off)
  constexpr int LW = COST_TX + 2 * COST_HALO, LH = COST_TY + 2 * COST_HALO;
  __shared__ T tile[LH * LW];
  const int nx = a.g.nx, ny = a.g.ny;
  const unsigned b = blockIdx.x;
  const int bx = (int)(b % a.nbx), by = (int)((b / a.nbx) % a.nby);
  const unsigned base = (b / (a.nbx * a.nby)) * a.g.tile_nodes;
  const int ox = bx * COST_TX - COST_HALO, oy = by * COST_TY - COST_HALO;
  for (int i = threadIdx.x; i < LH * LW; i += COST_TX * COST_TY) {
    const int ly = i / LW, lx = i - ly * LW;
    const int gx = max(min(ox + lx, nx - 1), 0), gy = max(min(oy + ly, ny - 1), 0);
    tile[i] = a.g.z[base + (unsigned)gy * (unsigned)nx + (unsigned)gx];
  }
  __syncthreads();
  const int tx = threadIdx.x % COST_TX, ty = threadIdx.x / COST_TX;
  const int ix = bx * COST_TX + tx, iy = by * COST_TY + ty;
  if (ix >= nx || iy >= ny) return;
  const T* const c = tile + (ty + COST_HALO) * LW + (tx + COST_HALO);
  const T zc = c[0];
  T step = (T)0;
  for (int dy = -a.P.margin; dy <= a.P.margin; ++dy)
    for (int dx = -a.P.margin; dx <= a.P.margin; ++dx) step = terrain_max(step, foothold_abs(c[dy * LW + dx] - zc));
  // the halo's clipped indices make the difference one-sided at a border; there it spans one cell, elsewhere two
  const T sx = (c[1] - c[-1]) * a.g.inv_cell * ((ix == 0 || ix == nx - 1) ? (T)1 : (T)0.5);
  const T sy = (c[LW] - c[-LW]) * a.g.inv_cell * ((iy == 0 || iy == ny - 1) ? (T)1 : (T)0.5);
  const T slope2 = sx * sx + sy * sy;
  a.cost[base + (unsigned)iy * (unsigned)nx + (unsigned)ix] = a.P.w_step * step + a.P.w_slope * slope2;
}

// One lane's foot.  `bit`: the foot's new mask bit; latch_in: the state's latch word as loaded.  r: bit 0 = the foot is latched after this tick, bit 1 =
// it was selected this tick; x, y: the plan's p1_x, p1_y as the law leaves them in memory (what the terrain rule then samples p1_z at), meaningful
// for a lifted foot.  Stores (behind `live`): swing words 9 leg + 3, 9 leg + 4 and, at a selection, rows 2 leg, 2 leg + 1 of hold.
// Every load a branch may need is issued at the top, whatever the branch: the lane then waits for one round trip to memory, not for one per
// decision (the words exist for every foot; those of a branch not taken are not used).
template <class T> struct FootholdPick { int r; T x, y; };
template <class T>
WBC_DEV FootholdPick<T> foothold_lane(const DevTerrain<T>& g, const FootholdIO<T>& f, int leg, unsigned s32, size_t N, bool live, bool bit, int latch_in,
                                      T* swing) {
#pragma clang fp contract(off)
  T* const sw = swing + (size_t)(9 * leg) * N + s32;
  T* const hd = f.hold + (size_t)(2 * leg) * N + s32;
  const T x = sw[3 * N], y = sw[4 * N], Tsw = sw[7 * N], t0 = sw[8 * N];
  const T hx = hd[0], hy = hd[N];
  const T* const cost = f.cost + (g.tile ? (unsigned)g.tile[s32] : 0u) * g.tile_nodes;
  if (bit) return {0, x, y};
  if ((latch_in >> leg) & 1) {
    if (live) { sw[3 * N] = hx; sw[4 * N] = hy; }
    return {1, hx, hy};
  }
  const int R = f.P.radius;
  if (R == 0) return {0, x, y};
  const int nx = g.nx, ny = g.ny;
  // the nearest node; clamped as a T, so that a NaN's or a far point's node lies on the grid
  const int jx = (int)terrain_min(terrain_max(foothold_floor((x - g.x0) * g.inv_cell + (T)0.5), (T)0), (T)(nx - 1));
  const int jy = (int)terrain_min(terrain_max(foothold_floor((y - g.y0) * g.inv_cell + (T)0.5), (T)0), (T)(ny - 1));
  const T c0 = cost[(unsigned)jy * (unsigned)nx + (unsigned)jx];
  if (c0 <= f.P.cost_ok || t0 > f.P.u_max * Tsw) return {0, x, y};
  const int ix0 = max(jx - R, 0), ix1 = min(jx + R, nx - 1), iy0 = max(jy - R, 0), iy1 = min(jy + R, ny - 1);
  T best = (T)0, bxc = (T)0, byc = (T)0;
  bool have = false;
  for (int iy = iy0; iy <= iy1; ++iy) {
    const T yc = g.y0 + (T)iy * f.cell, dy = yc - y;
    for (int ix = ix0; ix <= ix1; ++ix) {
      const T xc = g.x0 + (T)ix * f.cell, dx = xc - x;
      const T J = cost[(unsigned)iy * (unsigned)nx + (unsigned)ix] + f.P.w_dist * (dx * dx + dy * dy);
      if (!have || J < best) { best = J; bxc = xc; byc = yc; have = true; }
    }
  }
  if (live) { hd[0] = bxc; hd[N] = byc; sw[3 * N] = bxc; sw[4 * N] = byc; }
  return {3, bxc, byc};
}

// the four lanes' bits -> the state's word, stored by the owner lane
WBC_DEV void foothold_store(int* latch, int r, int leg, unsigned st, unsigned s32, bool live) {
  const unsigned long long bl = __ballot((r & 1) != 0), bs = __ballot((r & 2) != 0);
  if (live && leg == 0) latch[s32] = gait_gather(bl, st) | (gait_gather(bs, st) << 4);
}

template <class T>
__global__ __launch_bounds__(64) void foothold_select_kernel(FootholdSelectArgs<T> a) {
  WBC_LAUNDERED_TID(tx);
  const LegLane l = leg_lane<16>(tx, a.N);
  const bool bit = ((a.mask[l.s32] >> l.leg) & 1) != 0;
  const FootholdPick<T> p = foothold_lane<T>(a.g, a.f, l.leg, l.s32, a.N, l.live, bit, a.f.latch[l.s32], a.swing);
  foothold_store(a.f.latch, p.r, l.leg, l.st, l.s32, l.live);
}

template <class T>
__global__ __launch_bounds__(64) void gait_terrain_select_kernel(const DevModel<T>* __restrict__ model, GaitTerrainSelectArgs<T> ta) {
  const GaitArgs<T>& a = ta.g;
#define GAIT_SENSED_WORD (a.contact ? a.contact[s32] : 0)
#include "gait_body.inc.hpp"
#undef GAIT_SENSED_WORD
  const FootholdPick<T> p = foothold_lane<T>(ta.t.g, ta.f, leg, s32, N, live, bit, ta.f.latch[s32], a.swing);
  foothold_store(ta.f.latch, p.r, leg, st, s32, live);
  terrain_feet_tail_at<T>(ta.t, pf, leg, s32, N, live, !bit, a.swing, p.x, p.y);
}

template <class T>
__global__ __launch_bounds__(64) void gait_estimated_terrain_select_kernel(const DevModel<T>* __restrict__ model, GaitEstimatedTerrainSelectArgs<T> ta) {
  int word;
  {
    WBC_LAUNDERED_TID(tx);
    const LegLane l = leg_lane<16>(tx, ta.e.g.N);
    T fn; bool bit, sing; int prev;
    const V3<T> f = contact_law<T>(ta.e.c, ta.e.g.jpack, l.leg, l.s32, (unsigned)ta.e.g.N, fn, bit, sing, prev);   // reads the previous tick's normals
    word = contact_store<T>(ta.e.c, l.leg, l.st, l.s32, (unsigned)ta.e.g.N, l.live, f, fn, bit, sing, prev);
  }
  const GaitArgs<T>& a = ta.e.g;
#define GAIT_SENSED_WORD word
#include "gait_body.inc.hpp"
#undef GAIT_SENSED_WORD
  const FootholdPick<T> p = foothold_lane<T>(ta.t.g, ta.f, leg, s32, N, live, bit, ta.f.latch[s32], a.swing);
  foothold_store(ta.f.latch, p.r, leg, st, s32, live);
  terrain_feet_tail_at<T>(ta.t, pf, leg, s32, N, live, !bit, a.swing, p.x, p.y);   // overwrites the lane's own three normals words: terrain.hip.hpp
}

}  // namespace wbc
