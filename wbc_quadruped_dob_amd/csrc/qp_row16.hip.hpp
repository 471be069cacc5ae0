// What the GRF-QP families share, stated once: the helpers of the "one QP per 16-lane DPP row" mapping, the hand-over structs between a QP body and the
// kernel around it, and the forms every family writes the same way -- where a state's words lie, the 6 x 6 matrix G = alpha I + B B^T with its factor and
// the two substitutions through it, the contact basis with the pyramid and box rows, the words of Jc the QP reads, the row prologue and the diagnostic stamps.
// Users: qp_struct16.hip.hpp (the structured body), qp_group16.hip.hpp (the dense fp32 tile body), qp_kernels.hip.hpp (the tile predictors), qp_lane.hip.hpp,
// qp_general.hip.hpp and, through it, limit.hip.hpp.
// The forms are TEXT (macros over the names a body defines), not functions: a function template with reference outputs moved the fp64 device code
// (operands of v_mul_f64 exchanged, docs/DESIGN_HISTORY.md), and these kernels are kept instruction for instruction.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "device_types.hpp"

namespace wbc {

template <class T> struct Lim;
template <> struct Lim<double> { static constexpr double eps = 2.220446049250313e-16; static constexpr double inf = __builtin_huge_val(); };
template <> struct Lim<float> { static constexpr float eps = 1.1920929e-07f; static constexpr float inf = __builtin_huge_valf(); };
WBC_DEV double fabs_t(double x) { return fabs(x); }
WBC_DEV float fabs_t(float x) { return fabsf(x); }

template <int I, int N, class F> WBC_DEV void sfor(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); sfor<I + 1, N>(f); }
}
template <int I, int N, class F> WBC_DEV void sfor_down(F&& f) {  // I = N-1 ... 0
  if constexpr (N > 0) { f(std::integral_constant<int, N - 1>{}); sfor_down<I, N - 1>(f); }
}

// ---------------------------------------------------------------------------------------------------------------- the 16-lane row
// A CDNA DPP "row" is 16 lanes, and row_newbcast / row_mirror / row_half_mirror / quad_perm move data inside a row at VALU speed without touching LDS.
// One QP per row, four per wavefront: lane 4f+a (a<3) of a row owns variable (foot f, axis a); lane 4f+3 is a spare that carries constraints.
template <int CTRL> WBC_DEV float dppx(float x) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), CTRL, 0xF, 0xF, true));
}
template <int CTRL> WBC_DEV double dppx(double x) {
  // 64-bit form: row_newbcast becomes ONE v_mov_b64_dpp (the only DPP64 control on gfx90a+); the other
  // controls are split by the compiler into two 32-bit DPP movs
  const long long xi = __double_as_longlong(x);
  return __longlong_as_double(__builtin_amdgcn_update_dpp(xi, xi, CTRL, 0xF, 0xF, true));
}
template <int CTRL> WBC_DEV int dppx(int x) { return __builtin_amdgcn_mov_dpp(x, CTRL, 0xF, 0xF, true); }

constexpr int LJ(int j) { return j + j / 3; }  // lane (within the row) of variable j
// broadcast the value held by variable j's lane to the whole row
template <int J, class T> WBC_DEV T gbc(T x) { return dppx<0x150 + LJ(J)>(x); }
// all-reduce over the 16 lanes of a row: xor-1, xor-2 inside quads, then half-row and row mirrors
template <class T> WBC_DEV T gsum(T x) {
  x += dppx<0xB1>(x); x += dppx<0x4E>(x); x += dppx<0x141>(x); x += dppx<0x140>(x);
  return x;
}
// Row-wide argmin without a compare/select chain: the 5-bit id is written into the low mantissa bits of the
// value, which makes all keys distinct, so four DPP steps of v_min are an all-reduce that every lane agrees on.
// The value moves by < 2^-47 relative (f64) / 2^-18 (f32) -- selection only; callers that need the exact value
// of the winner fetch it from the winning lane.  BIG (finite) stands for "no candidate": inf | id would be a NaN.
template <class T> struct KeyT;
template <> struct KeyT<double> {
  static constexpr double BIG = 1e300;
  static WBC_DEV double pack(double v, int id) { return __longlong_as_double((__double_as_longlong(v) & ~63ll) | (long long)id); }
  static WBC_DEV int id(double k) { return (int)(__double_as_longlong(k) & 63ll); }
  static WBC_DEV double val(double k) { return __longlong_as_double(__double_as_longlong(k) & ~63ll); }
  // (v_min_f64 itself: fmin() makes the compiler canonicalise both operands first -- two v_max_f64 per step of the reduction,
  // eight dependent instructions per row argmin -- because it cannot know that the DPP-moved bit patterns are ordinary numbers)
  static WBC_DEV double mn(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
};
template <> struct KeyT<float> {
  static constexpr float BIG = 1e30f;
  static WBC_DEV float pack(float v, int id) { return __int_as_float((__float_as_int(v) & ~63) | id); }
  static WBC_DEV int id(float k) { return __float_as_int(k) & 63; }
  static WBC_DEV float val(float k) { return __int_as_float(__float_as_int(k) & ~63); }
  static WBC_DEV float mn(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
};
// in: v (BIG = none), id in [0,64).  out: row-uniform winner id in `id`, its value (low 6 mantissa bits cleared:
// relative error < 2^-46 in f64, 2^-17 in f32) in `v`; returns whether any lane had a candidate
template <class T> WBC_DEV bool gargmin(T& v, int& id) {
  using K = KeyT<T>;
  T k = K::pack(v, id);
  k = K::mn(k, dppx<0xB1>(k)); k = K::mn(k, dppx<0x4E>(k)); k = K::mn(k, dppx<0x141>(k)); k = K::mn(k, dppx<0x140>(k));
  id = K::id(k);
  v = K::val(k);
  return k < (T)(K::BIG * (T)0.5);
}
// read from a run-time lane of my own row
template <class T> WBC_DEV T gread(T x, int lane16, int rowbase) { return __shfl(x, rowbase | lane16); }

// Newton steps after v_rsq_f64 / v_rcp_f64 (2^-23 relative): 2 -> full double
WBC_DEV double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  double e = fma(-x * y, y, 1.0); y = fma(0.5 * y, e, y);
  e = fma(-x * y, y, 1.0); y = fma(0.5 * y, e, y);
  return y;
}
WBC_DEV float rsqrt_nr(float x) {
  float y = __builtin_amdgcn_rsqf(x);
  float e = fmaf(-x * y, y, 1.0f); y = fmaf(0.5f * y, e, y);
  return y;
}
WBC_DEV double rcp_nr(double x) {
  double y = __builtin_amdgcn_rcp(x);
  double e = fma(-x, y, 1.0); y = fma(y, e, y);
  e = fma(-x, y, 1.0); y = fma(y, e, y);
  return y;
}
// one Newton step: 2^-46 relative (where the result only scales a step or a projector row)
WBC_DEV double rcp_nr1(double x) {
  double y = __builtin_amdgcn_rcp(x);
  const double e = fma(-x, y, 1.0);
  return fma(y, e, y);
}
WBC_DEV float rcp_nr(float x) {
  float y = __builtin_amdgcn_rcpf(x);
  float e = fmaf(-x, y, 1.0f); y = fmaf(y, e, y);
  return y;
}

// The opening of a row-form body: the work-item id (laundered: lane-derived predicates stay inside this call, see WBC_LAUNDERED_TID in
// lane_rows.hip.hpp), the lane's row (rowbase = its first lane, grp = which of the wavefront's four), foot f and axis c3 within the row, and the
// variable v the lane owns (spare lanes, c3 == 3: unused).
#define WBC_QP_ROW_PROLOGUE                                                                                                       \
  unsigned tx = threadIdx.x;                                                                                                      \
  asm volatile("" : "+v"(tx));                                                                                                    \
  const int lane = tx & 63;                                                                                                       \
  const int l16 = lane & 15;                                                                                                      \
  const int rowbase = lane & 48;                                                                                                  \
  const int grp = lane >> 4;                                                                                                      \
  const int f = l16 >> 2, c3 = l16 & 3;                                                                                           \
  const bool isvar = c3 < 3;                                                                                                      \
  const int v = 3 * f + (isvar ? c3 : 0);

// ---------------------------------------------------------------------------------------------------------------- body <-> kernel
// What the one-launch tick and the rollouts (fused_tick.hip.hpp, rollout_body.inc.hpp) hand the structured body they run beside their producer roles:
// WSLDS: the step workspace of the workgroup's 16 states is read from LDS (wsl[word][16], written by the sweep phase of the same workgroup) instead
// of from HBM.
// RHAT (with WSLDS, observer-on fused tick): the observer role left rhat in the LDS image; b and tau_partial are
// completed by the body (b -= rhat_base, tau_partial -= rhat_joint).
// QpSync (WSLDS only): the producer roles of the fused tick publish the workspace in three steps, each behind an LDS
// counter -- lever arms, then w_des, early; rhat when the observer role is done, tau_partial and the own-leg Jacobian
// blocks when the force recursions are -- and the QP waits for each only where it first needs it: H and its factor
// come from the lever arms alone, the target wrench enters with g, tau_partial only in the torque map.
struct QpSync {
  int* geom; int* rhat; int* fin;
  int need_geom, need_b, need_rhat, need_fin;   // `geom` counts twice per tick: lever arms out, then w_des out
#ifdef WBC_FUSED_STAMP   // diagnostic build (tools/fused_stamp.py): 100 MHz timestamps of the roles, one column per workgroup
  double* stamp; unsigned stampN;
#endif
  // (round 5) the speculative start reads the observer state r_prev that the observer role of the SAME launch rewrites in place: every QP wavefront
  // counts here once its read has returned, and the observer role stores r only behind that count (fused_tick.hip.hpp) -- the read is ordered in
  // front of the write, so that iters and the last bits of tau do not depend on timing
  int* rp_ack = nullptr;
  // (round 5, persistent rollout) LDS image [42][16] of the solver's scalar type that ALSO receives this tick's results: tau (rows 0 .. 11, caller's joint
  // order), f (12 .. 23), and -- from the rnea role -- h (24 .. 41).  The integrator takes them from there behind an LDS-only barrier, instead of waiting
  // for the global stores to be acknowledged and reading them back through L2
  void* res = nullptr;
  // (round 5, persistent rollout with the image) true: tau, f, status, iters of THIS tick go to the image only -- nobody reads them from memory before the
  // launch's last tick (the next tick's observer takes tau_prev, f_prev from the image, the integrator tau and f)
  bool skip_out = false;
  // (four-wavefront rollout workgroups) the mass_jac role's LDS image [46][64] (dyn_split.hip.hpp, MJ_HAND_WORDS): the torque map takes the own-leg Jacobian
  // blocks from its words 24 .. 32 (row m of foot f, joint k at (24 + 3 m + k) * 64 + 16 f + slot) once `hand_flag` has reached `need_hand`, and the rnea
  // role does not compute them (RS_NOJC)
  const void* hand = nullptr; int* hand_flag = nullptr; int need_hand = 0;
  // (scored persistent rollout, score.hip.hpp) an LDS word per state of the workgroup that receives this tick's status beside the result image
  int* stat = nullptr;
};
#ifdef WBC_FUSED_STAMP
// (one column per workgroup: column = first state of the workgroup, i.e. blockIdx.x * states-per-workgroup)
#define WBC_FSTAMP_S(ptr, N_, slot, spw) do { if ((threadIdx.x & 63) == 0) (ptr)[(size_t)(slot) * (N_) + (size_t)blockIdx.x * (spw)] = (double)wall_clock64(); } while (0)
#define WBC_FSTAMP(ptr, N_, slot) WBC_FSTAMP_S(ptr, N_, slot, 16)
// -DWBC_RO_STAMP_ALT (tools/rollout_stamp.py): slots 1, 2, 3 belong to the mass_jac / integrator / rnea roles of the rollout kernel instead of to QP wavefront 0
#ifdef WBC_RO_STAMP_ALT
#define WBC_QSTAMP_OK(slot) ((slot) != 1 && (slot) != 2 && (slot) != 3)
#else
#define WBC_QSTAMP_OK(slot) true
#endif
#define WBC_QSTAMP(slot) do { if (WBC_QSTAMP_OK(slot) && sync && sync->stamp && (tx >> 6) == 0) WBC_FSTAMP_S(sync->stamp, sync->stampN, slot, SPW); } while (0)
#define WBC_QSTAMP3(slot) do { if (!RHAT && sync && sync->stamp && (tx >> 6) == 3) WBC_FSTAMP_S(sync->stamp, sync->stampN, slot, SPW); } while (0)
#else
#define WBC_QSTAMP(slot) do {} while (0)
#define WBC_QSTAMP3(slot) do {} while (0)
#endif
WBC_DEV void qp_wait(int* flag, int need) {
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < need) __builtin_amdgcn_s_sleep(1);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// TILED (qp_tile_kernel, qp_kernels.hip.hpp): the four rows of the wavefront solve the states `who` names (dealt by predicted work)
// instead of four consecutive ones; the workgroup is four such wavefronts.
struct QpWho {
  size_t state; bool live;
  const double* pre = nullptr;   // the tile predictor's record of this state (qp_kernels.hip.hpp), LDS
  // STG (staged tiles, qp_kernels.hip.hpp): the tile's inputs wait in an LDS image [ST_WORDS][stride] of the solver's scalar type, the state is column
  // `slot`; f, tau go back into the image and status / iters / active set into iimg ([4][tile]: mask, status, iters, set) -- the body touches no memory
  void* img = nullptr; int* iimg = nullptr; int slot = 0, stride = 0, tile = 0;
  void* tab = nullptr;   // this wavefront's solver tables (S16Lds<double>)
};
// rows of the staged image: normals 12, mu 4, lever arms 12, b = w_des - rhat_base 6, tau_partial - rhat_joint 12 (leg-major), own-leg Jacobian blocks 36
// (9 f + 3 m + k), then the results f 12, tau 12 (caller's joint order)
constexpr int ST_N = 0, ST_MU = 12, ST_D = 16, ST_B = 28, ST_TAUP = 34, ST_JCL = 46, ST_F = 82, ST_TAU = 94, ST_WORDS = 106;
struct QpNoIdle { WBC_DEV void operator()() const {} };

// -DWBC_QP_STAMP (diagnostic build only): per-wave cycle stamps go out in place of the iteration counts.  SEG(i) adds the cycles since the last
// SEG to segment i of the body's `seg` / `st_last`; GST_ITERS packs two 16-bit fields of cycles/16 per row of the wavefront into iters[s32]
// (set-up st_t1 - st_t0 and the segments), and is the plain store of `iter_` in every other build.
#ifdef WBC_QP_STAMP
#define SEG(i) do { const long long now_ = __builtin_readcyclecounter(); seg[i] += now_ - st_last; st_last = now_; } while (0)
#define GST_ITERS(iter_) do { \
    const long long vals[8] = {st_t1 - st_t0, seg[0], seg[1], seg[2], seg[3], seg[4], seg[5], seg[6]}; \
    long long lo = vals[0], hi = vals[1]; \
    if (grp == 1) { lo = vals[2]; hi = vals[3]; } else if (grp == 2) { lo = vals[4]; hi = vals[5]; } else if (grp == 3) { lo = vals[6]; hi = vals[7]; } \
    lo >>= 4; hi >>= 4; \
    if (lo > 0xFFFF) lo = 0xFFFF; \
    if (hi > 0x7FFF) hi = 0x7FFF; \
    if (a.iters) a.iters[s32] = (int)(lo | (hi << 16)); \
  } while (0)
#else
#define SEG(i) do {} while (0)
#define GST_ITERS(iter_) do { if (a.iters) a.iters[s32] = (iter_); } while (0)
#endif

// ---------------------------------------------------------------------------------------------------------------- where a state's words lie
// Component row `comp` of the body's state in a [rows][N] array: byte offset ((comp) * N32 + s32) * sizeof(storage type) behind the array's base, in 32-bit
// arithmetic (every array is < 4 GiB, lane_rows.hip.hpp).  Over the names a body defines: N32, s32, RowS = the type the array holds, RowA = the type the
// body computes in (the structured body and a predictor that feeds it: double over fp32 arrays).  lane_rows.hip.hpp's LDV / ROWV have no arithmetic
// type and scale by sizeof(T), which is the ARITHMETIC type in these bodies: the QP families keep this pair.  GLD_AT / GST_AT: another state than s32
// (the staged tiles copy whole rows).
#define QP_ROW_BYTES_(comp, s_) (size_t)(((unsigned)(comp) * N32 + (s_)) * (unsigned)sizeof(RowS))
#define GLD_AT(ptr, comp, s_) ((RowA)(*(const RowS*)((const char*)(ptr) + QP_ROW_BYTES_(comp, s_))))
#define GST_AT(ptr, comp, s_, val) (*(RowS*)((char*)(ptr) + QP_ROW_BYTES_(comp, s_)) = (RowS)(val))
#define GLD(ptr, comp) GLD_AT(ptr, comp, s32)
#define GST(ptr, comp, val) GST_AT(ptr, comp, s32, val)

// ---------------------------------------------------------------------------------------------------------------- the words of Jc the QP reads
// Jc is [12][18] per state, row 3 f + m = component m of foot f's velocity.  The lever arm d_f of foot f sits in the -[d]x block of its base-angular
// columns: d_x = Jc[3f+1][5], d_y = Jc[3f+2][3], d_z = Jc[3f][4]; the own-leg block is Jc[3f+m][6 + jm], jm = the caller's index of the joint.
// (text, not constexpr functions: as functions the index arithmetic reached the address forms in another shape, docs/DESIGN_HISTORY.md)
// I_: a cast applied to the row 3 f + m before it is scaled (empty for the QP families, which index in int or unsigned; limit.hip.hpp: (size_t))
#define JC_LEVER_WORD_(I_, f_, c_) ((c_) == 0 ? I_(3 * (f_) + 1) * 18 + 5 : ((c_) == 1 ? I_(3 * (f_) + 2) * 18 + 3 : I_(3 * (f_)) * 18 + 4))
#define JC_LEG_WORD_(I_, f_, m_, jm_) (I_(3 * (f_) + (m_)) * 18 + 6 + (jm_))
#define JC_LEVER_WORD(f_, c_) JC_LEVER_WORD_(, f_, c_)
#define JC_LEG_WORD(f_, m_, jm_) JC_LEG_WORD_(, f_, m_, jm_)

// ---------------------------------------------------------------------------------------------------------------- G = alpha I + B B^T and its factor
// B = S^(1/2) A (6 x 12), A = [I ; [d_f]x] per stance foot:  B B^T = S^(1/2) [nc I, -[sd]x ; [sd]x, sum(|d|^2 I - d d^T)] S^(1/2).
// In (locals of the site): nc = number of stance feet, (sx, sy, sz) = the sum of their lever arms, Pxx .. Pzz = the sums of the products of the lever
// arms' components, s0 .. s5 = the square roots of the weights; alpha_ = the regularisation, A_ = the arithmetic type, RS_ = the reciprocal square
// root (rsqrt_nr; the predictors that only select: the hardware seed).
// Out (new locals): G's entries -- g00 g11 g22 the force diagonal, gm.. the moment-force block s_(3+i) s_j [sd]x_ij, m.. the moment-moment block
// alpha I + s_(3+i) s_(3+j) (|d|^2 I - d d^T)_ij -- and its lower factor L: rows 0..2 diagonal (l0 l1 l2); row 3: [0 a01 a02 | l3];
// row 4: [a10 0 a12 | b10 l4]; row 5: [a20 a21 0 | b20 b21 l5]; il[k] = 1 / L_kk; c00, t11, t22 = the squares of l3, l4, l5.
#define WBC_QP_G_FACTOR(A_, RS_, alpha_)                                                                                                              \
  const A_ g00 = (alpha_) + s0 * s0 * nc, g11 = (alpha_) + s1 * s1 * nc, g22 = (alpha_) + s2 * s2 * nc;                                               \
  const A_ gm01 = -(s3 * s1) * sz, gm02 = (s3 * s2) * sy, gm10 = (s4 * s0) * sz, gm12 = -(s4 * s2) * sx, gm20 = -(s5 * s0) * sy, gm21 = (s5 * s1) * sx; \
  const A_ m00 = (alpha_) + (s3 * s3) * (Pyy + Pzz), m11 = (alpha_) + (s4 * s4) * (Pxx + Pzz), m22 = (alpha_) + (s5 * s5) * (Pxx + Pyy);               \
  const A_ m10 = -(s4 * s3) * Pxy, m20 = -(s5 * s3) * Pxz, m21 = -(s5 * s4) * Pyz;                                                                    \
  A_ il[6];                                                                                                                                           \
  il[0] = RS_(g00); il[1] = RS_(g11); il[2] = RS_(g22);                                                                                               \
  const A_ a01 = gm01 * il[1], a02 = gm02 * il[2], a10 = gm10 * il[0], a12 = gm12 * il[2], a20 = gm20 * il[0], a21 = gm21 * il[1];                     \
  const A_ c00 = m00 - a01 * a01 - a02 * a02, c11 = m11 - a10 * a10 - a12 * a12, c22 = m22 - a20 * a20 - a21 * a21;                                   \
  const A_ c10 = m10 - a12 * a02, c20 = m20 - a21 * a01, c21 = m21 - a20 * a10;                                                                       \
  il[3] = RS_(c00);                                                                                                                                   \
  const A_ b10 = c10 * il[3], b20 = c20 * il[3];                                                                                                      \
  const A_ t11 = c11 - b10 * b10;                                                                                                                     \
  il[4] = RS_(t11);                                                                                                                                   \
  const A_ b21 = (c21 - b20 * b10) * il[4];                                                                                                           \
  const A_ t22 = c22 - b20 * b20 - b21 * b21;                                                                                                         \
  il[5] = RS_(t22);
// w = (L [+ sqrt(alpha) I])^-1 r  and  y = (L [+ sqrt(alpha) I])^-T w through that factor (a01 .. b21 of the site), the diagonal given through its
// reciprocals inv[0 .. 5]: il, or 1 / (L_kk + sqrt(alpha)) in the dense body
#define WBC_QP_FWD(inv, r0, r1, r2, r3, r4, r5, w) do {                                  \
    w[0] = (r0) * inv[0]; w[1] = (r1) * inv[1]; w[2] = (r2) * inv[2];                    \
    w[3] = ((r3) - a01 * w[1] - a02 * w[2]) * inv[3];                                    \
    w[4] = ((r4) - a10 * w[0] - a12 * w[2] - b10 * w[3]) * inv[4];                       \
    w[5] = ((r5) - a20 * w[0] - a21 * w[1] - b20 * w[3] - b21 * w[4]) * inv[5];          \
  } while (0)
#define WBC_QP_BWD(inv, w, y) do {                                                       \
    y[5] = w[5] * inv[5];                                                                \
    y[4] = (w[4] - b21 * y[5]) * inv[4];                                                 \
    y[3] = (w[3] - b10 * y[4] - b20 * y[5]) * inv[3];                                    \
    y[2] = (w[2] - a02 * y[3] - a12 * y[4]) * inv[2];                                    \
    y[1] = (w[1] - a01 * y[3] - a21 * y[5]) * inv[1];                                    \
    y[0] = (w[0] - a10 * y[4] - a20 * y[5]) * inv[0];                                    \
  } while (0)
// the unit solve G x = e_c through the factor (zeros of a compile-time e_c are skipped by the compiler)
#define WBC_QP_UNIT_SOLVE(A_, c_, w, x) do {                                                                                                      \
    const A_ e0 = (c_) == 0 ? (A_)1 : (A_)0, e1 = (c_) == 1 ? (A_)1 : (A_)0, e2 = (c_) == 2 ? (A_)1 : (A_)0, e3 = (c_) == 3 ? (A_)1 : (A_)0,      \
             e4 = (c_) == 4 ? (A_)1 : (A_)0, e5 = (c_) == 5 ? (A_)1 : (A_)0;                                                                      \
    WBC_QP_FWD(il, e0, e1, e2, e3, e4, e5, w);                                                                                                    \
    WBC_QP_BWD(il, w, x);                                                                                                                         \
  } while (0)

// ---------------------------------------------------------------------------------------------------------------- contact basis, pyramid and box rows
// The oracle's contact frame: t1 = e_x (e_y for a normal along x: |n_x| >= 0.9) made orthogonal to the unit normal, t2 = n x t1.
// TANGENT_AXIS: from the x and y components of a UNIT normal, leaves the reference axis (rx, ry, 0) and rd = its component along the normal; the
// tangent before normalisation is (rx, ry, 0) - rd n  (qp_lane.hip.hpp forms it over its arrays and scales it in the same expression).
#define WBC_QP_TANGENT_AXIS(A_, n0, n1)                                      \
  const bool usex = fabs_t(n0) < (A_)0.9;                                    \
  const A_ rx = usex ? (A_)1 : (A_)0, ry = usex ? (A_)0 : (A_)1;             \
  const A_ rd = rx * (n0) + ry * (n1);
// BASIS: normalises the site's nx, ny, nz in place and leaves t1x .. t2z
#define WBC_QP_CONTACT_BASIS(A_, RS_)                                                                            \
  const A_ iln = RS_(nx * nx + ny * ny + nz * nz);                                                               \
  nx *= iln; ny *= iln; nz *= iln;                                                                               \
  WBC_QP_TANGENT_AXIS(A_, nx, ny)                                                                                \
  A_ t1x = rx - nx * rd, t1y = ry - ny * rd, t1z = -nz * rd;                                                     \
  const A_ it = RS_(t1x * t1x + t1y * t1y + t1z * t1z);                                                          \
  t1x *= it; t1y *= it; t1z *= it;                                                                               \
  const A_ t2x = ny * t1z - nz * t1y, t2y = nz * t1x - nx * t1z, t2z = nx * t1y - ny * t1x;
// The rows of a row-form body's lane (foot f, c3): constraint A (and B where hasB = c3 < 2) with coefficients cA., cB. and right-hand side rA:
//   c3 = 0: mu~ n -+ t1,   c3 = 1: mu~ n -+ t2,   c3 = 2: n . f >= fn_min,   c3 = 3: -n . f >= -fn_max.
// Over the body's T, n_ld (the lane's component of its foot's normal), mu_f, prm, c3, hasB and the row variables.
#define WBC_QP_FORM_ROWS do { \
    T nx = dppx<0x00>(n_ld), ny = dppx<0x55>(n_ld), nz = dppx<0xAA>(n_ld); \
    WBC_QP_CONTACT_BASIS(T, rsqrt_nr) \
    const T mt = mu_f * prm.mu_scale; \
    const T ttx = (c3 == 0) ? t1x : t2x, tty = (c3 == 0) ? t1y : t2y, ttz = (c3 == 0) ? t1z : t2z; \
    if (hasB) { \
      cAx = mt * nx - ttx; cAy = mt * ny - tty; cAz = mt * nz - ttz; rA = 0; \
      cBx = mt * nx + ttx; cBy = mt * ny + tty; cBz = mt * nz + ttz; \
    } else if (c3 == 2) { cAx = nx; cAy = ny; cAz = nz; rA = prm.fn_min; } \
    else { cAx = -nx; cAy = -ny; cAz = -nz; rA = -prm.fn_max; } \
  } while (0)

}  // namespace wbc
