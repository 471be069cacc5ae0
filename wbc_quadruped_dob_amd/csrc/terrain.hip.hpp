// Terrain heightfield (include/wbc_hip.h at "Terrain heightfield"): the ground as a regular grid of heights per tile, sampled bilinearly on the device, so
// that a foot that moves meets other ground without host work between launches.  One law, terrain_law: clamp the point to the grid, pick the cell,
// interpolate the height zs, differentiate the cell's bilinear patch for the unit normal n, and form the offset d of the tangent plane n . x = d at
// the (clamped) point -- the plane the step, the contact estimate and the ground plant read as normals / height.  zs is continuous; n is piecewise and
// jumps at cell edges.
//   terrain_sample_kernel          the law at caller-given points, one lane per point
//   terrain_feet_kernel            the law under the four feet p_f(q) of every state (leg-lane mapping: lane = 16*leg + state, one wavefront per
//                                  workgroup; lanes beyond the batch recompute its last state and store nothing); with a mask, p1_z of every lifted
//                                  foot := zs at that plan's own (p1_x, p1_y)
//   gait_terrain_kernel            gait_kernel's body (gait_body.inc.hpp, as text), then the same tail on the body's own pf, leg, s32, live, bit
//   gait_estimated_terrain_kernel  contact law + that body + the tail.  `normals` is IN/OUT there: a lane's contact law loads its own foot's three
//                                  words of the previous tick's plane, and the tail, later in the same lane's program order, overwrites those three
//                                  words and no others -- no lane reads another lane's words, so the in-place write is safe.
// terrain_feet_tail holds the law's use and every store; all three leg-lane kernels call it.  It reads p1_x, p1_y back from `swing`: in the fused
// kernels the lane's own earlier store is ordered before its load, and words the body left untouched are read as they stand.
// The four node loads of a sample are a per-lane gather from z + (tile * ny * nx + iy * nx + ix): a 32-bit element offset (the host refuses grids of 2^28
// nodes or more).  Not staged through LDS: a lane touches four words of a grid that sits in L2.
// Out of scope: the rollout kernels and wbc_rollout_*, wbc_multi_*, the payload plant, late touchdown in the gait rule, choosing footholds by terrain
// quality, smoothed (C1) normals, terrain sensing or estimation (the map is given).
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "dyn_sweep.hip.hpp"
#include "gait.hip.hpp"
#include "contact_est.hip.hpp"

namespace wbc {

WBC_DEV double terrain_min(double a, double b) { return fmin(a, b); }
WBC_DEV float terrain_min(float a, float b) { return fminf(a, b); }
WBC_DEV double terrain_max(double a, double b) { return fmax(a, b); }
WBC_DEV float terrain_max(float a, float b) { return fmaxf(a, b); }

template <class T> struct TerrainPlane { T zs; V3<T> n; T d; };

// where the point's cell lies and where the point lies in it: node (ix, iy) as an element offset behind the tile's first node, u, w in [0, 1], and the
// clamped point.  (The lower bound on ix, iy changes nothing for a finite point -- gx >= 0 there -- and keeps a NaN's cell inside the grid.)
template <class T>
WBC_DEV unsigned terrain_cell(const DevTerrain<T>& g, T x, T y, T& xc, T& yc, T& u, T& w) {
  xc = terrain_min(terrain_max(x, g.x0), g.x_max);
  yc = terrain_min(terrain_max(y, g.y0), g.y_max);
  const T gx = (xc - g.x0) * g.inv_cell, gy = (yc - g.y0) * g.inv_cell;
  const int ix = max(min((int)gx, g.nx - 2), 0), iy = max(min((int)gy, g.ny - 2), 0);
  u = gx - (T)ix;
  w = gy - (T)iy;
  return (unsigned)iy * (unsigned)g.nx + (unsigned)ix;
}

// the height alone (the foothold's p1_z); `base` = the tile's first node, tile * ny * nx
template <class T>
WBC_DEV T terrain_height(const DevTerrain<T>& g, unsigned base, T x, T y) {
  T xc, yc, u, w;
  const unsigned o = base + terrain_cell(g, x, y, xc, yc, u, w);
  const T z00 = g.z[o], z10 = g.z[o + 1], z01 = g.z[o + (unsigned)g.nx], z11 = g.z[o + (unsigned)g.nx + 1];
  const T a = z00 + u * (z10 - z00), b = z01 + u * (z11 - z01);
  return a + w * (b - a);
}

// the whole law
template <class T>
WBC_DEV TerrainPlane<T> terrain_law(const DevTerrain<T>& g, unsigned base, T x, T y) {
  T xc, yc, u, w;
  const unsigned o = base + terrain_cell(g, x, y, xc, yc, u, w);
  const T z00 = g.z[o], z10 = g.z[o + 1], z01 = g.z[o + (unsigned)g.nx], z11 = g.z[o + (unsigned)g.nx + 1];
  const T a = z00 + u * (z10 - z00), b = z01 + u * (z11 - z01);
  TerrainPlane<T> p;
  p.zs = a + w * (b - a);
  const T zx = ((z10 - z00) + w * ((z11 - z01) - (z10 - z00))) * g.inv_cell, zy = (b - a) * g.inv_cell;
  const T r = rsqrt_t(zx * zx + zy * zy + (T)1);
  p.n = mk<T>(-zx * r, -zy * r, r);
  p.d = p.n.x * xc + p.n.y * yc + p.n.z * p.zs;
  return p;
}

template <class T>
__global__ __launch_bounds__(64) void terrain_sample_kernel(TerrainSampleArgs<T> a) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= a.M) return;
  const unsigned base = (a.g.tile ? (unsigned)a.g.tile[i] : 0u) * a.g.tile_nodes;
  const TerrainPlane<T> p = terrain_law<T>(a.g, base, a.xy[i], a.xy[a.M + i]);
  if (a.z) a.z[i] = p.zs;
  if (a.n) { a.n[i] = p.n.x; a.n[a.M + i] = p.n.y; a.n[2 * a.M + i] = p.n.z; }
  if (a.d) a.d[i] = p.d;
}

// One lane's foot: the plane under pf into rows 3 leg .. 3 leg + 2 of normals, height[leg] and surf[leg]; when the foot is lifted (`lifted`: a mask
// was given and its bit is clear), word 9 leg + 5 of swing (p1_z) := zs at that plan's own words 9 leg + 3, 9 leg + 4.
template <class T>
WBC_DEV void terrain_feet_tail(const TerrainOut<T>& t, V3<T> pf, int leg, unsigned s32, size_t N, bool live, bool lifted, T* swing) {
  const unsigned base = (t.g.tile ? (unsigned)t.g.tile[s32] : 0u) * t.g.tile_nodes;
  const TerrainPlane<T> p = terrain_law<T>(t.g, base, pf.x, pf.y);
  if (live) {
    T* const no = t.normals + (size_t)(3 * leg) * N + s32;
    no[0] = p.n.x; no[N] = p.n.y; no[2 * N] = p.n.z;
    t.height[(size_t)leg * N + s32] = p.d;
    if (t.surf) t.surf[(size_t)leg * N + s32] = p.zs;
    if (lifted) {
      T* const sw = swing + (size_t)(9 * leg) * N + s32;
      sw[5 * N] = terrain_height<T>(t.g, base, sw[3 * N], sw[4 * N]);
    }
  }
}

// terrain_feet_tail for a caller that holds the plan's (p1_x, p1_y) = swing words 9 leg + 3, 9 leg + 4 in registers (foothold.hip.hpp): the same
// stores from the same bits, without the round trip through memory
template <class T>
WBC_DEV void terrain_feet_tail_at(const TerrainOut<T>& t, V3<T> pf, int leg, unsigned s32, size_t N, bool live, bool lifted, T* swing, T p1x, T p1y) {
  const unsigned base = (t.g.tile ? (unsigned)t.g.tile[s32] : 0u) * t.g.tile_nodes;
  const TerrainPlane<T> p = terrain_law<T>(t.g, base, pf.x, pf.y);
  const T p1z = terrain_height<T>(t.g, base, p1x, p1y);
  if (live) {
    T* const no = t.normals + (size_t)(3 * leg) * N + s32;
    no[0] = p.n.x; no[N] = p.n.y; no[2 * N] = p.n.z;
    t.height[(size_t)leg * N + s32] = p.d;
    if (t.surf) t.surf[(size_t)leg * N + s32] = p.zs;
    if (lifted) swing[(size_t)(9 * leg + 5) * N + s32] = p1z;
  }
}

// p_f(q) of the lane's leg: the text of gait_body.inc.hpp's position chain (its lines 32-76), over the same names
template <class T>
WBC_DEV V3<T> terrain_foot_point(const DevModel<T>* __restrict__ model, const T* cst, const T* q, unsigned long long jpack, int leg, unsigned s32, size_t N) {
  T qb[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) qb[c] = ROWI(q, c);
  int jx[3];
  jidx_of_leg(model, jpack, leg, jx);
  T ql[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) ql[k] = ROWI(q, 7 + jx[k]);
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
  return mk<T>(qb[0], qb[1], qb[2]) + mul(R, d);
}

template <class T>
__global__ __launch_bounds__(64) void terrain_feet_kernel(const DevModel<T>* __restrict__ model, TerrainFeetArgs<T> a) {
  __shared__ T cst[CST_WORDS];
  for (int i = threadIdx.x; i < CST_WORDS; i += blockDim.x) cst[i] = model->cst[i];
  __syncthreads();
  WBC_LAUNDERED_TID(tx);
  const LegLane l = leg_lane<16>(tx, a.N);   // lanes beyond the batch recompute its last state and store nothing
  const V3<T> pf = terrain_foot_point<T>(model, cst, a.q, a.jpack, l.leg, l.s32, a.N);
  const bool lifted = a.mask && ((a.mask[l.s32] >> l.leg) & 1) == 0;
  terrain_feet_tail<T>(a.t, pf, l.leg, l.s32, a.N, l.live, lifted, a.swing);
}

template <class T>
__global__ __launch_bounds__(64) void gait_terrain_kernel(const DevModel<T>* __restrict__ model, GaitTerrainArgs<T> ta) {
  const GaitArgs<T>& a = ta.g;
#define GAIT_SENSED_WORD (a.contact ? a.contact[s32] : 0)
#include "gait_body.inc.hpp"
#undef GAIT_SENSED_WORD
  terrain_feet_tail<T>(ta.t, pf, leg, s32, N, live, !bit, a.swing);
}

template <class T>
__global__ __launch_bounds__(64) void gait_estimated_terrain_kernel(const DevModel<T>* __restrict__ model, GaitEstimatedTerrainArgs<T> ta) {
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
  terrain_feet_tail<T>(ta.t, pf, leg, s32, N, live, !bit, a.swing);   // overwrites the lane's own three normals words: see the top of this file
}

}  // namespace wbc
