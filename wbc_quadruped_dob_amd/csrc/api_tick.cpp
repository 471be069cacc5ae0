// C-ABI (include/wbc_hip.h): one control tick of a batch -- the dynamics alone, the tick (cold and warm), the torque-limit post-pass behind it, the integrators.
#include "solver.hpp"

using namespace wbc;

template <class T>
static int dynamics_impl(wbc_solver* s, size_t N, const void* q, const void* v, void* M, void* h, void* Jc, void* pf,
                         void* p, void* beta, hipStream_t st) {
  SweepArgs<T> a;
  std::memset(&a, 0, sizeof(a));
  a.jpack = s->jpack;
  a.N = N; a.q = (const T*)q; a.v = (const T*)v;
  a.M = (T*)M; a.h = (T*)h; a.Jc = (T*)Jc; a.pf = (T*)pf; a.p = (T*)p; a.beta = (T*)beta;
  const int mode = (M ? SW_MATS : 0) | ((p || beta) ? SW_OBS : 0);
  KeepScope keep(s, M, Jc, N);
  a.skip_consts = keep.skip;
  timing_tick(s);
  TIMED_LAUNCH(0, st, "dyn_sweep", k_dyn_sweep<T>(L, mode, dev_model<T>(s), to_dev_params<T>(s->params), a));
  keep.written();
  return WBC_OK;
}

extern "C" int wbc_dynamics_batch(wbc_solver* s, size_t N, const void* q, const void* v, void* M, void* h, void* Jc,
                                  void* pf, void* p, void* beta, void* stream) {
  if (!s || !q || !v) return fail(WBC_E_INVALID, "null argument");
  if (N == 0) return WBC_OK;
  if (N > s->max_batch) return fail(WBC_E_CAPACITY, "N exceeds the solver's max_batch");   // (also keeps the 32-bit lane offsets in range)
  if ((M || h || Jc) && !(M && h && Jc)) return fail(WBC_E_INVALID, "M, h, Jc must be given together");
  if (!M && !pf && !p && !beta) return fail(WBC_E_INVALID, "no output requested");
  ON_DEVICE(s);
  hipStream_t st = (hipStream_t)stream;
  return s->dtype == WBC_F64 ? dynamics_impl<double>(s, N, q, v, M, h, Jc, pf, p, beta, st)
                             : dynamics_impl<float>(s, N, q, v, M, h, Jc, pf, p, beta, st);
}

// Large observer-on batch: the observer update runs as its own light kernel in front of (option obs_split_serial = 0: beside, on the second stream) an
// observer-free front half `front(L)` -- rhat travels through 18 extra workspace words and the QP kernel completes b and tau_partial with it
template <class T, class F>
static int observer_then(wbc_solver* s, hipStream_t st, const DevParams<T>& dp, const SweepArgs<T>& a, const char* what, F&& front) {
  if (s->opt.obs_split_serial) {   // same stream, one after the other
    TIMED_LAUNCH(2, st, "observer", k_observer<T>(L, dev_model<T>(s), dp, a));
    TIMED_LAUNCH(0, st, what, front(L));
    return WBC_OK;
  }
  HIP_TRY(hipEventRecord(s->ev_fork, st));
  HIP_TRY(hipStreamWaitEvent(s->aux, s->ev_fork, 0));
  TIMED_LAUNCH(2, s->aux, "observer", k_observer<T>(L, dev_model<T>(s), dp, a));
  HIP_TRY(hipEventRecord(s->ev_join, s->aux));
  TIMED_LAUNCH(0, st, what, front(L));
  HIP_TRY(hipStreamWaitEvent(st, s->ev_join, 0));   // the QP needs rhat
  return WBC_OK;
}

template <class T>
static int step_impl(wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out,
                     const wbc_observer_state* obs, hipStream_t st, bool warm_api, const int* aset_in, int* aset_out) {
  SweepArgs<T> a;
  sweep_args(a, s, N, in, out, obs);
  const bool mats = out->M != nullptr, ob = s->params.observer_order > 0;
  KeepScope keep(s, out->M, out->Jc, N);
  a.skip_consts = keep.skip;
  timing_tick(s);
  QpArgs<T> qa;
  qp_args(qa, s, N, in, out, obs);
  qa.aset_in = aset_in; qa.aset_out = aset_out;
  // two-kernel tick with M/h/Jc outputs: the QP takes its geometry from Jc and the sweep skips those workspace words
  qa.Jc = mats ? (const T*)out->Jc : nullptr;
  a.ws_geom = mats ? 0 : 1;
  const DevParams<T> dp = to_dev_params<T>(s->params);
  // (what runs, and why: plan_tick.  A warm call WITHOUT a set to start from -- tick 0 of a per-tick-launch rollout, the first tick of a closed loop --
  //  is planned as the cold tick it is: between the warm and the cold per-lane thresholds the cold tiles are the faster kernels; they still report the set)
  //  -- unless the cold plan's QP kernel is the fp32 12 x 12 body, which reports no set: then the warm plan's kernels run, started from the empty set.)
  TickPlan pl = plan_tick(s->dtype, s->params.observer_order, s->opt, s->rz, N, mats, out->pf != nullptr, warm_api);
  if (warm_api && aset_in == nullptr) {
    const TickPlan pc = plan_tick(s->dtype, s->params.observer_order, s->opt, s->rz, N, mats, out->pf != nullptr, false);
    if (pc.qp_body == QP_BODY_STRUCTURED) pl = pc;
  }
  const bool warm = warm_api && aset_in != nullptr && pl.qp_warm;
  switch (pl.fused) {
    case FUSED_TICK:
      TIMED_LAUNCH(3, st, "fused tick", k_fused_tick<T>(L, ob, mats, dev_model<T>(s), dp, a, qa, s->jmap, warm));
      keep.written();
      return WBC_OK;
    case FUSED_PAIR:
      TIMED_LAUNCH(3, st, "fused pair tick", k_fused_pair<T>(L, dev_model<T>(s), dp, a, qa, s->jmap));
      keep.written();
      return WBC_OK;
    case FUSED_TILE_TICK:   // (the roles leave w_des to the QP stage: SW_NOB)
      qa.wdes = (const T*)in->w_des;
      TIMED_LAUNCH(3, st, "tile tick", k_tile_tick<T>(L, ob, pl.tile, dev_model<T>(s), dp, a, qa, s->jmap));
      keep.written();
      return WBC_OK;
    case FUSED_NONE: break;
  }
  // front halves that do not change the target wrench leave it to the QP kernels to read the caller's w_des (QpArgs::wdes)
  const bool front_writes_b = ob && !pl.obs_split;   // the all-in-one observer forms: b = w_des - rhat_base
  qa.wdes = front_writes_b ? nullptr : (const T*)in->w_des;   // (those front halves run their SW_NOB / RS_NOB variants)
  a.qp_todo = pl.lane ? s->d_todo : nullptr;   // the front-half kernel empties the hand-over list (one thread; a kernel of its own took 4.7 us per tick)
  switch (pl.front) {
    case FRONT_OBS_THEN_RNEA: {   // no M, h, Jc wanted, large observer-on batch: observer kernel, observer-free rnea_step
      const int mode = RS_STEP | RS_NOB | (out->pf ? RS_PF : 0);
      if (const int rc = observer_then<T>(s, st, dp, a, "rnea_step", [&](const LaunchCtx& L) { return k_rnea_step<T>(L, mode, dev_model<T>(s), dp, a); })) return rc;
      break;
    }
    case FRONT_RNEA: {   // no M, h, Jc wanted: the CRBA-free rnea_step kernel is the whole front half
      const int mode = RS_STEP | (ob ? RS_OBS : RS_NOB) | (out->pf ? RS_PF : 0);
      TIMED_LAUNCH(2, st, "rnea_step", k_rnea_step<T>(L, mode, dev_model<T>(s), dp, a));
      break;
    }
    case FRONT_SWEEP_OBS_ROLES:   // mid-size observer-on batch: the observer update and the observer-free sweep as the two roles of one launch
      TIMED_LAUNCH(0, st, "sweep_obs", k_sweep_obs<T>(L, dev_model<T>(s), dp, a));
      break;
    case FRONT_OBS_THEN_SWEEP:
      // large observer-on batch: observer kernel, then a dyn_sweep WITHOUT the observer passes (252 instead of 370 VGPRs: two waves per SIMD, shared
      // tables), which writes M, h, Jc
      if (const int rc = observer_then<T>(s, st, dp, a, "dyn_sweep", [&](const LaunchCtx& L) { return k_dyn_sweep<T>(L, SW_MATS | SW_STEP | SW_NOB, dev_model<T>(s), dp, a); })) return rc;
      break;
    case FRONT_SWEEP:
      TIMED_LAUNCH(0, st, "dyn_sweep", k_dyn_sweep<T>(L, SW_MATS | SW_STEP | (ob ? SW_OBS : SW_NOB), dev_model<T>(s), dp, a));
      break;
  }
  keep.written();
  if (pl.lane) {
    TIMED_LAUNCH(4, st, "qp_lane", k_qp_lane<T>(L, pl.obs_split, dp, qa, s->jmap, s->d_todo, warm));
    TIMED_LAUNCH(1, st, "qp", k_qp<T>(L, pl.obs_split, 0, dp, qa, s->jmap, s->d_todo, warm));
    return WBC_OK;
  }
  TIMED_LAUNCH(1, st, "qp", k_qp<T>(L, pl.obs_split, pl.tile, dp, qa, s->jmap, nullptr, warm, (int)pl.qp_body));
  return WBC_OK;
}

// argument checks of one tick (no HIP call): shared with wbc_multi_*, which validates every shard before it enqueues any
int wbc::check_step_args(const wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out,
                         const wbc_observer_state* obs, bool rollout) {
  if (!s || !in || !out) return fail(WBC_E_INVALID, "null argument");
  if (N == 0) return WBC_OK;
  if (N > s->max_batch) return fail(WBC_E_CAPACITY, "N exceeds the solver's max_batch");
  if (!in->q || !in->v || !in->w_des || !in->vdot_des || !in->normals || !in->mu || !in->mask)
    return fail(WBC_E_INVALID, "null input buffer");
  if (!out->tau || !out->f || !out->status) return fail(WBC_E_INVALID, "null output buffer");
  if ((out->M || out->h || out->Jc) && !(out->M && out->h && out->Jc))
    return fail(WBC_E_INVALID, "M, h, Jc must be given together");
  if (rollout && !out->M) return fail(WBC_E_INVALID, "rollouts need the M, h, Jc buffers (forward dynamics reads them)");
  if (s->params.observer_order > 0) {
    if (!obs || !obs->integ || !obs->r) return fail(WBC_E_INVALID, "observer on: observer state buffers required");
    if (!rollout && (!in->tau_prev || !in->f_prev)) return fail(WBC_E_INVALID, "observer on: tau_prev and f_prev required");
  }
  return WBC_OK;
}

// behind both tick entry points: the checks, the solver's device, the scalar type
static int step_entry(wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs, void* stream, bool warm,
                      const int* active_in, int* active_out) {
  const int rc0 = check_step_args(s, N, in, out, obs, false);
  if (rc0) return rc0;
  if (N == 0) return WBC_OK;
  ON_DEVICE(s);
  hipStream_t st = (hipStream_t)stream;
  return s->dtype == WBC_F64 ? step_impl<double>(s, N, in, out, obs, st, warm, active_in, active_out)
                             : step_impl<float>(s, N, in, out, obs, st, warm, active_in, active_out);
}

extern "C" int wbc_step_batch(wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out,
                              const wbc_observer_state* obs, void* stream) {
  return step_entry(s, N, in, out, obs, stream, false, nullptr, nullptr);
}

// One tick of a DEPENDENT sequence (a closed loop, a rollout driven by the caller): the GRF QP of every state starts from active_in
extern "C" int wbc_step_batch_warm(wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out,
                                   const wbc_observer_state* obs, const int* active_in, int* active_out, void* stream) {
  return step_entry(s, N, in, out, obs, stream, true, active_in, active_out);
}

// ---- joint torque limits behind a tick (limit.hip.hpp)
extern "C" int wbc_solver_set_torque_limits(wbc_solver* s, const wbc_torque_limits* l) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (!l) { std::memcpy(s->tau_max, s->model_effort, sizeof(s->tau_max)); return WBC_OK; }
  if (l->struct_size < sizeof(wbc_torque_limits)) return fail(WBC_E_INVALID, "wbc_torque_limits: struct_size too small");
  for (int j = 0; j < 12; ++j)
    if (!(l->tau_max[j] > 0)) return fail(WBC_E_INVALID, "wbc_torque_limits: tau_max must be > 0 (HUGE_VAL = no limit)");
  for (int j = 0; j < WBC_MAXV; ++j) s->tau_max[j] = j < 12 ? l->tau_max[j] : HUGE_VAL;
  return WBC_OK;
}

// the post-pass's own argument checks (no HIP call)
static int check_limit_args(const wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs) {
  if (!s || !in || !out) return fail(WBC_E_INVALID, "null argument");
  if (N == 0) return WBC_OK;   // (as check_step_args: an empty batch needs no buffers)
  if (N > s->max_batch) return fail(WBC_E_CAPACITY, "N exceeds the solver's max_batch");
  if (!in->w_des || !in->normals || !in->mu || !in->mask) return fail(WBC_E_INVALID, "null input buffer");
  if (!out->tau || !out->f || !out->status) return fail(WBC_E_INVALID, "null output buffer");
  if (!out->M || !out->h || !out->Jc) return fail(WBC_E_INVALID, "torque limits: out->M, h, Jc are required (the post-pass reads Jc)");
  if (s->params.observer_order > 0 && (!obs || !obs->r)) return fail(WBC_E_INVALID, "observer on: observer state buffers required");
  return WBC_OK;
}

template <class T>
static int limit_impl(wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs, int* limited, hipStream_t st) {
  bool any = false;
  for (int j = 0; j < 12; ++j) any = any || s->tau_max[j] < HUGE_VAL;
  s->limit_skipped = !any;
  if (!any) {   // nothing can saturate: no launch, every state is outcome 0
    if (limited) HIP_TRY(hipMemsetAsync(limited, 0, N * sizeof(int), st));
    return WBC_OK;
  }
  LimitArgs<T> a;
  std::memset(&a, 0, sizeof(a));
  a.N = N; a.Jc = (const T*)out->Jc; a.wdes = (const T*)in->w_des;
  a.rhat = s->params.observer_order > 0 ? (const T*)obs->r : nullptr;
  a.normals = (const T*)in->normals; a.mu = (const T*)in->mu; a.mask = in->mask;
  a.tau = (T*)out->tau; a.f = (T*)out->f; a.status = out->status; a.iters = out->iters; a.limited = limited;
  a.list = s->d_limit; a.jpack = s->jpack;
  for (int i = 0; i < 12; ++i) a.lim[i] = s->tau_max[s->jmap.j[i]];
  const wbc_params& p = s->params;
  for (int i = 0; i < 6; ++i) a.S[i] = p.S[i];
  a.alpha = p.alpha; a.fn_min = p.fn_min; a.fn_max = p.fn_max; a.mu_scale = p.mu_scale; a.tol = p.qp_tol; a.max_iter = p.max_iter;
  HIP_TRY(hipMemsetAsync(s->d_limit, 0, sizeof(int), st));
  LaunchCtx L; L.st = st;
  hipError_t e = k_limit_scan<T>(L, a);
  if (e == hipSuccess) e = k_limit_qp<T>(L, a, s->limit_grid);
  if (e != hipSuccess) return fail(WBC_E_HIP, std::string("torque-limit launch: ") + hipGetErrorString(e));
  return WBC_OK;
}

extern "C" int wbc_limit_torques_batch(wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs,
                                       int* limited, void* stream) {
  const int rc0 = check_limit_args(s, N, in, out, obs);
  if (rc0) return rc0;
  if (N == 0) return WBC_OK;
  ON_DEVICE(s);
  hipStream_t st = (hipStream_t)stream;
  return s->dtype == WBC_F64 ? limit_impl<double>(s, N, in, out, obs, limited, st) : limit_impl<float>(s, N, in, out, obs, limited, st);
}

extern "C" int wbc_step_limited_batch(wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs,
                                      int* limited, void* stream) {
  int rc = check_step_args(s, N, in, out, obs, false);   // every check of both halves before anything is enqueued
  if (rc) return rc;
  rc = check_limit_args(s, N, in, out, obs);
  if (rc) return rc;
  rc = wbc_step_batch(s, N, in, out, obs, stream);
  if (rc) return rc;
  return wbc_limit_torques_batch(s, N, in, out, obs, limited, stream);
}

// diagnostics: how many states the LAST post-pass listed for a re-solve (synchronises)
extern "C" int wbc_solver_limited_count(wbc_solver* s, int* resolved) {
  if (!s || !resolved) return fail(WBC_E_INVALID, "null argument");
  if (s->limit_skipped) { *resolved = 0; return WBC_OK; }
  ON_DEVICE(s);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(resolved, s->d_limit, sizeof(int), hipMemcpyDeviceToHost));
  return WBC_OK;
}

// ---- the integrators (integrate_impl: solver.hpp)
static int integrate_batch(wbc_solver* s, size_t N, void* q, void* v, const void* M, const void* h, const void* Jc, const void* tau, const void* f,
                           const void* tau_ext, const void* payload, void* stream) {
  if (!s || !q || !v || !M || !h || !Jc || !tau || !f) return fail(WBC_E_INVALID, "null argument");
  if (N == 0) return WBC_OK;
  return launch_batch(s, N, stream, "integrate", [&](auto scalar, const LaunchCtx& L) {
    return integrate_impl<decltype(scalar)>(L, s, N, q, v, M, h, Jc, tau, f, tau_ext, nullptr, payload);
  });
}

extern "C" int wbc_integrate_batch(wbc_solver* s, size_t N, void* q, void* v, const void* M, const void* h,
                                   const void* Jc, const void* tau, const void* f, const void* tau_ext, void* stream) {
  return integrate_batch(s, N, q, v, M, h, Jc, tau, f, tau_ext, nullptr, stream);
}

int wbc::plant_args(const wbc_plant* plant, const void** tau_ext, const void** payload) {
  *tau_ext = nullptr; *payload = nullptr;
  if (!plant) return WBC_OK;
  if (plant->struct_size < sizeof(wbc_plant)) return fail(WBC_E_INVALID, "wbc_plant: struct_size too small");
  *tau_ext = plant->tau_ext; *payload = plant->payload;
  return WBC_OK;
}

extern "C" int wbc_integrate_plant_batch(wbc_solver* s, size_t N, void* q, void* v, const void* M, const void* h, const void* Jc,
                                         const void* tau, const void* f, const wbc_plant* plant, void* stream) {
  const void *tau_ext, *payload;
  const int rc = plant_args(plant, &tau_ext, &payload);
  if (rc) return rc;
  return integrate_batch(s, N, q, v, M, h, Jc, tau, f, tau_ext, payload, stream);
}
