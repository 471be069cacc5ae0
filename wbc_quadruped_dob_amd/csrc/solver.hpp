// Shared by the host units that call the HIP runtime (api_*.cpp): the solver handle, the per-call device and error scopes, the instrumented launch,
// and the builders of the kernels' argument structs that more than one unit uses.  Pure host code -- the kernels live in the k_*.hip translation
// units behind launch.hpp.  No CPU compute fallback exists: without a usable gfx950 device every solver entry point fails with WBC_E_NODEVICE/WBC_E_HIP.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "device_types.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "tick_plan.hpp"

#define HIP_TRY(expr)                                                                                     \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) return fail(WBC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
  } while (0)

constexpr size_t TIMING_MAX_SPANS = 4096;   // bounded ring: samples beyond it are dropped until the next collect
constexpr int ONE_SCRATCH = 200;        // first scalar of the helpers' scratch region of the single-robot image (88 scalars)
constexpr int ONE_SCALARS = 288;        // scalars in front of the image's ints (the tick uses the first 161)
// the fp64 helpers wbc_compute_swing_reference / _gait / _contact_estimate stage through ONE device block (api_one.cpp, stage_one): doubles, then ints.
// The largest user is the contact estimate: Jc r f_prev normals | f_est fn_est = 216 + 18 + 12 + 12 + 12 + 4 doubles; the gait call has the most ints
constexpr int STAGE_ONE_DOUBLES = 274, STAGE_ONE_INTS = 3;

struct wbc_solver {
  int dtype = WBC_F64;
  int device = 0;
  size_t max_batch = 0;
  wbc_params params;
  wbc_solver_options opt;
  int leg_body[4][3];
  void* d_model = nullptr;  // DevModel<T>
  void* d_ws = nullptr;     // WS_LDS_WORDS * max_batch * sizeof(T): the 66 step words + 18 words of rhat (separate observer kernel)
  int in_rollout = 0;       // inside the per-tick loop of wbc_rollout_batch, past its first tick
  int* d_todo = nullptr;    // 4 + max_batch ints: states the per-lane QP kernel hands to the dense active-set kernel (count, workgroups done, count of the last tick, pad; indices)
  int* d_aset = nullptr;    // max_batch ints: the active sets that wbc_rollout_batch's per-tick launches carry from tick to tick (rollout_warm)
  wbc::QpJidx jmap;
  unsigned long long jpack = 0;   // jmap as nibbles (pack_jidx): the dynamics bodies' joint indices, a kernel argument
  wbc::Resolved rz{};       // resolved thresholds (resolve_options)
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  void* d_ref = nullptr;     // DevRefParams<T>, set by wbc_solver_set_ref_params
  wbc_score_params score;    // the weights of the scored rollouts (wbc_solver_set_score_params; kernel arguments by value), defaults at creation
  wbc_swing_params swing;    // the gains of the swing-foot references (wbc_solver_set_swing_params; kernel arguments by value), defaults at creation
  wbc_ground_params ground;  // the contact law of the ground plant (wbc_solver_set_ground_params; kernel arguments by value), the defaults at creation
  wbc_stiction_params stiction;  // the anchor spring of the ground plant's stiction calls (wbc_solver_set_stiction_params; a kernel argument by value)
  wbc_gait_params gait;      // the schedule of the gait scheduler (wbc_solver_set_gait_params; kernel arguments by value), the model's defaults at creation
  wbc_contact_params contact_est;   // the thresholds of the contact estimate (wbc_solver_set_contact_params; a kernel argument by value), the defaults at creation
  wbc_foothold_params foothold;     // the weights of the foothold selection (wbc_solver_set_foothold_params; a kernel argument by value), the defaults at creation
  wbc_odom_params odom;             // the gains of the base estimate (wbc_solver_set_odom_params; kernel arguments by value), the defaults at creation
  wbc_trunk_params trunk;           // the trunk reference from the command (wbc_solver_set_trunk_params; kernel arguments by value), the defaults at creation
  void* d_stage_one = nullptr;      // the fp64 single-robot helpers' staging: STAGE_ONE_DOUBLES doubles + STAGE_ONE_INTS ints
  // torque-limit post-pass (wbc_limit_torques_batch): the limits travel as a kernel argument like the score weights
  double tau_max[WBC_MAXV];  // caller's joint order, HUGE_VAL = none; the model's effort limits at creation
  double model_effort[WBC_MAXV];
  int* d_limit = nullptr;    // LIMIT_LIST_HEAD + max_batch ints: [0] = how many states the scan listed, then their indices
  int limit_grid = 0;        // workgroups of limit_qp_kernel: one resident round on this device (limit_qp_grid)
  bool limit_skipped = true; // the last post-pass launched nothing (every limit +inf)
  // N=1 convenience buffers
  void* d_one = nullptr;
  void* h_one = nullptr;       // pinned host image of d_one: the single-robot calls move it with ONE copy each way
  void* h_one_dev = nullptr;   // device address of h_one (mapped): one_zerocopy lets the N = 1 kernels read / write it directly
  size_t one_bytes = 0;
  // wbc_solver_options.keep_structural: the M / Jc buffers (and N) of the last call that wrote their structural constants
  const void* kept_M = nullptr; const void* kept_Jc = nullptr; size_t kept_N = 0;
  unsigned one_seq = 0;        // completion tickets of the flag-polled single-robot ticks (one_zerocopy >= 2)
  bool one_flag_ok = true;     // cleared when the stream write-value / flag kernel is refused: back to hipStreamSynchronize
  // timing: a ring of event pairs allocated by wbc_solver_enable_timing (never inside a tick)
  bool timing = false;
  int timing_period = 1;   // instrument every timing_period-th tick
  unsigned long long calls = 0;
  bool sample_now = false;
  std::vector<hipEvent_t> ev_pool;   // 2 * TIMING_MAX_SPANS once timing has been enabled
  struct Span { int kind; hipEvent_t a, b; };
  std::vector<Span> spans;
  size_t dropped = 0;
};

namespace wbc {

// Every entry point runs on the solver's device and leaves the caller's current device as it found it.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); switched = (err == hipSuccess); }
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define ON_DEVICE(s_)                                                                                     \
  DeviceGuard guard_((s_)->device);                                                                       \
  if (guard_.err != hipSuccess) return fail(WBC_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

// ---- timing: spans borrow event pairs from a ring that wbc_solver_enable_timing allocated; nothing is created inside a tick
struct SpanScope {   // one instrumented kernel launch
  wbc_solver* s;
  LaunchCtx L;
  bool active = false;
  hipError_t err = hipSuccess;
  SpanScope(wbc_solver* s_, int kind, hipStream_t st) : s(s_) {
    L.st = st;
    L.f32_pack2 = s->opt.f32_pack2;
    if (!s->timing || !s->sample_now) return;
    if (s->spans.size() >= TIMING_MAX_SPANS) { ++s->dropped; return; }
    const size_t i = 2 * s->spans.size();
    wbc_solver::Span sp{kind, s->ev_pool[i], s->ev_pool[i + 1]};
    if (s->opt.timing_mode == WBC_TIMING_DISPATCH) { L.ev_start = sp.a; L.ev_stop = sp.b; }   // the dispatch's own timestamps
    else err = hipEventRecord(sp.a, st);
    s->spans.push_back(sp);
    active = true;
  }
  hipError_t end() {   // after the launch
    if (active && s->opt.timing_mode != WBC_TIMING_DISPATCH) return hipEventRecord(s->spans.back().b, L.st);
    return hipSuccess;
  }
  void cancel() { if (active) { s->spans.pop_back(); active = false; } }   // the launch failed
};
inline void timing_tick(wbc_solver* s) {  // once per API call: is this tick instrumented?
  s->sample_now = s->timing && (s->calls++ % (unsigned long long)s->timing_period) == 0;
}

// one instrumented launch on the solver `s` in scope: kind = index into the timing arrays (0 dyn_sweep, 1 QP (dense active set), 2 rnea_step / observer,
// 3 fused tick, 4 QP one state per lane, 5 persistent rollout)
#define TIMED_LAUNCH(kind_, stream_, what_, call_)                                                          \
  do {                                                                                                      \
    SpanScope sc_(s, kind_, stream_);                                                                       \
    if (sc_.err != hipSuccess) return fail(WBC_E_HIP, std::string("hipEventRecord: ") + hipGetErrorString(sc_.err)); \
    const LaunchCtx& L = sc_.L;                                                                             \
    hipError_t le_ = (call_);                                                                               \
    if (le_ != hipSuccess) { sc_.cancel(); return fail(WBC_E_HIP, std::string(what_) + " launch: " + hipGetErrorString(le_)); } \
    le_ = sc_.end();                                                                                        \
    if (le_ != hipSuccess) return fail(WBC_E_HIP, std::string("hipEventRecord: ") + hipGetErrorString(le_)); \
  } while (0)

template <class T> const DevModel<T>* dev_model(const wbc_solver* s) { return (const DevModel<T>*)s->d_model; }

template <class T> DevParams<T> to_dev_params(const wbc_params& p) {
  DevParams<T> d;
  for (int i = 0; i < 6; ++i) { d.S[i] = (T)p.S[i]; d.sS[i] = (T)std::sqrt(p.S[i]); }
  d.sqrt_alpha = (T)std::sqrt(p.alpha); d.rsqrt_alpha = (T)(1.0 / std::sqrt(p.alpha));
  d.alpha = (T)p.alpha; d.fn_min = (T)p.fn_min; d.fn_max = (T)p.fn_max; d.mu_scale = (T)p.mu_scale;
  d.dt = (T)p.dt; d.qp_tol = (T)p.qp_tol;
  d.observer_order = p.observer_order; d.max_iter = p.max_iter;
  for (int i = 0; i < 18; ++i) { d.K1[i] = (T)p.K1[i]; d.K2[i] = (T)p.K2[i]; }
  return d;
}

// The launch path of the one-launch batch entry points, behind their own argument checks: capacity, the solver's device, the caller's stream, the
// scalar type, the launch error.  launch(T(), L) fills the kernel's argument struct for the scalar type T and returns the launcher's hipError_t.
template <class F>
int launch_batch(wbc_solver* s, size_t N, void* stream, const char* what, F&& launch) {
  if (N > s->max_batch) return fail(WBC_E_CAPACITY, "N exceeds the solver's max_batch");
  ON_DEVICE(s);
  LaunchCtx L; L.st = (hipStream_t)stream;
  const hipError_t e = s->dtype == WBC_F64 ? launch(double(), L) : launch(float(), L);
  if (e != hipSuccess) return fail(WBC_E_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
  return WBC_OK;
}

// keep_structural: `skip` = this call may leave the structural zeros / ones of M and Jc alone (same buffers and N as the call that
// last WROTE them).  The buffers are recorded only once the launch that writes them has been enqueued (written()); a call that
// fails before that forgets them, so the next call writes every word again.
struct KeepScope {
  wbc_solver* s; const void* M; const void* Jc; size_t N; int skip = 0; bool done = false;
  KeepScope(wbc_solver* s_, const void* M_, const void* Jc_, size_t N_) : s(s_), M(M_), Jc(Jc_), N(N_) {
    // (in_rollout: ticks 1 .. horizon-1 of ONE wbc_rollout_batch call write the buffers tick 0 of the same call wrote)
    if (M) skip = ((s->opt.keep_structural || s->in_rollout) && M == s->kept_M && Jc == s->kept_Jc && N == s->kept_N) ? 1 : 0;
  }
  void written() { if (M) { s->kept_M = M; s->kept_Jc = Jc; s->kept_N = N; } done = true; }
  ~KeepScope() { if (M && !done) s->kept_M = nullptr; }
};

// ---- the kernels' argument structs from the C-ABI's: ONE builder each, filled in place; a caller then sets only the fields in which it differs
template <class T>
void sweep_args(SweepArgs<T>& a, const wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs) {
  std::memset(&a, 0, sizeof(a));
  a.jpack = s->jpack;
  a.N = N; a.q = (const T*)in->q; a.v = (const T*)in->v;
  a.M = (T*)out->M; a.h = (T*)out->h; a.Jc = (T*)out->Jc; a.pf = (T*)out->pf;
  a.w_des = (const T*)in->w_des; a.vdot_des = (const T*)in->vdot_des;
  a.tau_prev = (const T*)in->tau_prev; a.f_prev = (const T*)in->f_prev;
  a.obs_integ = obs ? (T*)obs->integ : nullptr; a.obs_r = obs ? (T*)obs->r : nullptr;
  a.ws = (T*)s->d_ws;
}
// (Jc, wdes, aset_in, aset_out: null; rprev: the observer state where the observer runs)
template <class T>
void qp_args(QpArgs<T>& qa, const wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs) {
  std::memset(&qa, 0, sizeof(qa));
  qa.jpack = s->jpack;
  qa.N = N; qa.ws = (const T*)s->d_ws; qa.normals = (const T*)in->normals; qa.mu = (const T*)in->mu; qa.mask = in->mask;
  qa.tau = (T*)out->tau; qa.f = (T*)out->f; qa.status = out->status; qa.iters = out->iters;
  qa.rprev = (s->params.observer_order > 0 && obs) ? (const T*)obs->r : nullptr;
}
// (the integrator's public entry points take bare pointers, so this one does too)
template <class T>
void integrate_args(IntegrateArgs<T>& a, const wbc_solver* s, size_t N, void* q, void* v, const void* M, const void* h, const void* Jc,
                    const void* tau, const void* f, const void* tau_ext, void* tau_traj) {
  std::memset(&a, 0, sizeof(a));
  a.N = N; a.q = (T*)q; a.v = (T*)v; a.M = (const T*)M; a.h = (const T*)h; a.Jc = (const T*)Jc;
  a.tau = (const T*)tau; a.f = (const T*)f; a.tau_ext = (const T*)tau_ext; a.tau_traj = (T*)tau_traj;
  a.dt = (T)s->params.dt;
  a.jpack = s->jpack;
}
// (simg, refimg, planimg, skip_out: set by the rollout kernel only)
template <class T>
void ref_args(RefArgs<T>& a, const wbc_solver* s, size_t N, const void* q, const void* v, const void* plan, double t, void* w_des,
              void* vdot_des, void* com) {
  std::memset(&a, 0, sizeof(a));
  a.N = N; a.q = (const T*)q; a.v = (const T*)v; a.plan = (const T*)plan; a.t = (T)t;
  a.w_des = (T*)w_des; a.vdot_des = (T*)vdot_des; a.com = (T*)com;
  a.jpack = s->jpack;
}

// the integrator's launch, with or without a payload on the plant: the public calls' (api_tick.cpp) and the per-tick loop's of rollout() (api_rollout.cpp)
template <class T>
hipError_t integrate_impl(const LaunchCtx& L, const wbc_solver* s, size_t N, void* q, void* v, const void* M, const void* h, const void* Jc,
                          const void* tau, const void* f, const void* tau_ext, void* tau_traj, const void* payload) {
  IntegrateArgs<T> a;
  integrate_args(a, s, N, q, v, M, h, Jc, tau, f, tau_ext, tau_traj);
  return payload ? k_integrate_plant<T>(L, dev_model<T>(s), a, (const T*)payload) : k_integrate<T>(L, dev_model<T>(s), a);
}
// (ABI 10) the plant's extras of wbc_*_plant_batch: NULL plant = the calls without it; a struct of an older, smaller build is refused (api_tick.cpp)
int plant_args(const wbc_plant* plant, const void** tau_ext, const void** payload);

}  // namespace wbc
