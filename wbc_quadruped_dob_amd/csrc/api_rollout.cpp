// C-ABI (include/wbc_hip.h): the rollout family (one launch or per-tick launches), its scoring and per-group selection, and the CoM reference generator.
#include "solver.hpp"

using namespace wbc;

// ---- scored rollouts (score.hip.hpp): the solver's weights and the call's buffers as ONE kernel argument
template <class T> static ScoreArgs<T> score_args(const wbc_solver* s, size_t N, const wbc_rollout_score* score, bool accumulate) {
  ScoreArgs<T> a;
  std::memset(&a, 0, sizeof(a));
  const wbc_score_params& p = s->score;
  a.N = N; a.goal = (const T*)score->goal; a.cost = (T*)score->cost; a.fail = score->fail_ticks; a.accumulate = accumulate ? 1 : 0;
  a.w.w_tau = (T)p.w_tau; a.w.w_f = (T)p.w_f; a.w.w_fail = (T)p.w_fail; a.w.w_q = (T)p.w_q; a.w.w_qd = (T)p.w_qd; a.w.terminal = (T)p.terminal;
  for (int i = 0; i < 3; ++i) { a.w.w_pos[i] = (T)p.w_pos[i]; a.w.w_rot[i] = (T)p.w_rot[i]; a.w.w_vel[i] = (T)p.w_vel[i]; a.w.w_omega[i] = (T)p.w_omega[i]; }
  for (int i = 0; i < 12; ++i) a.w.q_nom[i] = (T)p.q_nom[i];
  return a;
}
// score == NULL or score->cost == NULL: the unscored call (*use = NULL); otherwise struct_size first (as wbc_plant), then goal and cost together
static int score_arg_check(const wbc_rollout_score* score, const wbc_rollout_score** use) {
  *use = nullptr;
  if (!score) return WBC_OK;
  if (score->struct_size < sizeof(wbc_rollout_score)) return fail(WBC_E_INVALID, "wbc_rollout_score: struct_size too small");
  if (!score->cost) {
    if (score->goal || score->fail_ticks) return fail(WBC_E_INVALID, "wbc_rollout_score: goal / fail_ticks without cost");
    return WBC_OK;
  }
  if (!score->goal) return fail(WBC_E_INVALID, "wbc_rollout_score: cost without goal");
  *use = score;
  return WBC_OK;
}
// the per-tick path: one tick's l_k behind the tick's integrate launch (score_tick_kernel)
static int score_tick(wbc_solver* s, size_t N, const void* q, const void* v, const void* tau, const void* f, const int* status,
                      const wbc_rollout_score* score, bool accumulate, int is_last, hipStream_t st) {
  LaunchCtx L; L.st = st;
  hipError_t e;
  if (s->dtype == WBC_F64) e = k_score_tick<double>(L, score_args<double>(s, N, score, accumulate), (const double*)q, (const double*)v, (const double*)tau, (const double*)f, status, is_last);
  else e = k_score_tick<float>(L, score_args<float>(s, N, score, accumulate), (const float*)q, (const float*)v, (const float*)tau, (const float*)f, status, is_last);
  if (e != hipSuccess) return fail(WBC_E_HIP, std::string("score launch: ") + hipGetErrorString(e));
  return WBC_OK;
}

// ---- the rollout family: what a call carries beyond the tick's batch structs, all of it optional; the entry points fill it
struct RolloutExtras {
  const void* tau_ext = nullptr;             // [nv][N] external torques on the plant
  const void* payload = nullptr;             // the plant's trunk carries it, in the persistent kernel and in the per-tick integrate launches alike
  const void* plan = nullptr;                // non-null: the planner in the loop, w_des / vdot_des are regenerated every tick
  void* tau_traj = nullptr;                  // [horizon][nj][N]
  void* com_traj = nullptr;                  // [horizon][6][N] (the planner records it)
  const wbc_rollout_score* score = nullptr;  // non-null (and through score_arg_check): the running cost is accumulated
};

// small batches: the whole horizon in ONE launch (rollout_kernel / rollout_scored_kernel, fused_tick.hip.hpp); in->tau_prev / f_prev are out's tau / f
template <class T>
static int rollout_persistent(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in, const wbc_batch_out* out,
                              const wbc_observer_state* obs, const RolloutExtras& x, hipStream_t st) {
  RolloutLaunch<T> r;
  sweep_args(r.a, s, N, in, out, obs);
  r.a.skip_consts = 0;   // (tick 0 writes M / Jc in full; the later ticks of the launch leave their structural zeros / ones alone: rollout_kernel)
  r.a.ws_geom = 1;
  s->kept_M = nullptr;
  qp_args(r.qa, s, N, in, out, obs);   // (aset_in null: every tick of the launch but the first starts from the previous tick's set, kept in registers)
  // (cold rollouts with the planner in the loop keep the QP waiting for rhat: the speculative start lost there, 26.8 -> 29.0 us per tick)
  if (x.plan) r.qa.rprev = nullptr;
  integrate_args(r.ia, s, N, (void*)in->q, (void*)in->v, out->M, out->h, out->Jc, out->tau, out->f, x.tau_ext, x.tau_traj);
  ref_args(r.ra, s, N, in->q, in->v, x.plan, 0.0, (void*)in->w_des, (void*)in->vdot_des, x.com_traj);
  r.observer = s->params.observer_order > 0;
  // states per workgroup: 4 while that still fits one workgroup per CU (a tick then waits for the slowest of 4 QPs, not 16)
  r.spw = (s->opt.rollout_spw == 4 || (s->opt.rollout_spw == 0 && N <= 1024)) ? 4 : 16;
  r.model = dev_model<T>(s); r.prm = to_dev_params<T>(s->params); r.jmap = s->jmap; r.horizon = horizon;
  r.G = (const DevRefParams<T>*)s->d_ref;
  r.warm = x.score || s->opt.rollout_warm != 0;   // (the scored kernels are always warm)
  r.payload = (const T*)x.payload;
  ScoreArgs<T> sc;
  if (x.score) sc = score_args<T>(s, N, x.score, x.score->accumulate != 0);
  r.score = x.score ? &sc : nullptr;
  timing_tick(s);
  TIMED_LAUNCH(5, st, x.score ? "scored rollout" : "rollout", k_rollout<T>(L, r));
  return WBC_OK;
}

static bool rollout_as_one_launch(const wbc_solver* s, size_t N) { return N <= s->rz.fused_max && s->opt.rollout_persistent; }

// every wbc_rollout_*_batch: one launch, or per tick [reference] -> step (warm or cold) -> integrate -> [score]
static int rollout(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs,
                   const RolloutExtras& x, void* stream) {
  if (!s || !in || !out) return fail(WBC_E_INVALID, "null argument");
  if (horizon < 1) return fail(WBC_E_INVALID, "horizon must be >= 1");
  if (x.score && !out->status) return fail(WBC_E_INVALID, "scored rollouts need the status buffer");
  if (!out->M || !out->h || !out->Jc) return fail(WBC_E_INVALID, "rollouts need the M, h, Jc buffers (forward dynamics reads them)");
  if (x.plan) {
    if (!in->q || !in->v || !in->w_des || !in->vdot_des) return fail(WBC_E_INVALID, "null input buffer");
    if (!s->d_ref) return fail(WBC_E_INVALID, "call wbc_solver_set_ref_params first");
  }
  if (N == 0) return WBC_OK;   // empty shard
  wbc_batch_in tick = *in;
  tick.tau_prev = out->tau;  // the previous tick's outputs are this tick's tau_prev / f_prev: the sweep reads them
  tick.f_prev = out->f;      // before the QP kernel of the same tick overwrites them
  const bool f64 = s->dtype == WBC_F64;
  hipStream_t st = (hipStream_t)stream;
  if (rollout_as_one_launch(s, N)) {
    if (N > s->max_batch) return fail(WBC_E_CAPACITY, "N exceeds the solver's max_batch");
    if (!in->q || !in->v || !in->w_des || !in->vdot_des || !in->normals || !in->mu || !in->mask)
      return fail(WBC_E_INVALID, "null input buffer");
    if (!out->tau || !out->f || !out->status) return fail(WBC_E_INVALID, "null output buffer");
    if (s->params.observer_order > 0 && (!obs || !obs->integ || !obs->r))
      return fail(WBC_E_INVALID, "observer on: observer state buffers required");
    ON_DEVICE(s);
    return f64 ? rollout_persistent<double>(s, N, horizon, &tick, out, obs, x, st) : rollout_persistent<float>(s, N, horizon, &tick, out, obs, x, st);
  }
  // (per-tick launches: wbc_step_batch checks the buffers)
  const size_t ts = f64 ? 8 : 4;
  const size_t nj = 12;
  ON_DEVICE(s);
  // rollout_warm with per-tick launches: where the planner's warm tick really starts from the sets (fused launch, warm one-wavefront kernel,
  // warm per-lane pair); in between the cold tiles are the faster kernels (plan_tick)
  const bool warm_ticks = s->opt.rollout_warm && plan_tick(s->dtype, s->params.observer_order, s->opt, s->rz, N, true, out->pf != nullptr, true).qp_warm;
  for (int t = 0; t < horizon; ++t) {
    int rc;
    if (x.plan) {
      void* com = x.com_traj ? (void*)((char*)x.com_traj + (size_t)t * 6 * N * ts) : nullptr;
      rc = wbc_reference_batch(s, N, in->q, in->v, x.plan, (double)t * s->params.dt, (void*)in->w_des, (void*)in->vdot_des, com, stream);
      if (rc) return rc;
    }
    if (t == 0) s->kept_M = nullptr;   // tick 0 writes M, Jc in full whatever an earlier call left there
    s->in_rollout = t > 0;
    // tick t > 0 starts its QPs from the active sets tick t - 1 left in d_aset
    rc = warm_ticks ? wbc_step_batch_warm(s, N, &tick, out, obs, t > 0 ? s->d_aset : nullptr, s->d_aset, stream)
                    : wbc_step_batch(s, N, &tick, out, obs, stream);
    s->in_rollout = 0;
    if (rc) return rc;
    void* traj = x.tau_traj ? (void*)((char*)x.tau_traj + (size_t)t * nj * N * ts) : nullptr;
    LaunchCtx L; L.st = st;
    const hipError_t e = f64 ? integrate_impl<double>(L, s, N, (void*)in->q, (void*)in->v, out->M, out->h, out->Jc, out->tau, out->f, x.tau_ext, traj, x.payload)
                             : integrate_impl<float>(L, s, N, (void*)in->q, (void*)in->v, out->M, out->h, out->Jc, out->tau, out->f, x.tau_ext, traj, x.payload);
    if (e != hipSuccess) return fail(WBC_E_HIP, std::string("integrate launch: ") + hipGetErrorString(e));
    if (x.score) {
      rc = score_tick(s, N, in->q, in->v, out->tau, out->f, out->status, x.score, t > 0 || x.score->accumulate != 0, t == horizon - 1, st);
      if (rc) return rc;
    }
  }
  return WBC_OK;
}

extern "C" int wbc_rollout_batch(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in, const wbc_batch_out* out,
                                 const wbc_observer_state* obs, const void* tau_ext, void* tau_traj, void* stream) {
  RolloutExtras x;
  x.tau_ext = tau_ext; x.tau_traj = tau_traj;
  return rollout(s, N, horizon, in, out, obs, x, stream);
}

extern "C" int wbc_rollout_plant_batch(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in, const wbc_batch_out* out,
                                       const wbc_observer_state* obs, const wbc_plant* plant, void* tau_traj, void* stream) {
  RolloutExtras x;
  const int rc = plant_args(plant, &x.tau_ext, &x.payload);
  if (rc) return rc;
  x.tau_traj = tau_traj;
  return rollout(s, N, horizon, in, out, obs, x, stream);
}

// (the planner's entry points refuse a call without a plan: to rollout() a null plan is the call without the planner)
extern "C" int wbc_rollout_tracking_batch(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in,
                                          const wbc_batch_out* out, const wbc_observer_state* obs, const void* tau_ext,
                                          const void* plan, void* tau_traj, void* com_traj, void* stream) {
  if (!plan) return fail(WBC_E_INVALID, "null argument");
  RolloutExtras x;
  x.tau_ext = tau_ext; x.plan = plan; x.tau_traj = tau_traj; x.com_traj = com_traj;
  return rollout(s, N, horizon, in, out, obs, x, stream);
}

extern "C" int wbc_rollout_tracking_plant_batch(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in, const wbc_batch_out* out,
                                                const wbc_observer_state* obs, const wbc_plant* plant, const void* plan, void* tau_traj,
                                                void* com_traj, void* stream) {
  RolloutExtras x;
  const int rc = plant_args(plant, &x.tau_ext, &x.payload);
  if (rc) return rc;
  if (!plan) return fail(WBC_E_INVALID, "null argument");
  x.plan = plan; x.tau_traj = tau_traj; x.com_traj = com_traj;
  return rollout(s, N, horizon, in, out, obs, x, stream);
}

// ---- scored rollouts: the weights, the superset rollout, one tick's cost, the per-group selection
extern "C" void wbc_score_params_default(wbc_score_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->w_fail = 1e6;
  p->terminal = 1;
}

extern "C" int wbc_solver_set_score_params(wbc_solver* s, const wbc_score_params* p) {
  if (!p) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = check_struct_size(p, "wbc_score_params: struct_size too small (call wbc_score_params_default first)")) return rc;
  const double w[] = {p->w_tau, p->w_f, p->w_fail, p->w_pos[0], p->w_pos[1], p->w_pos[2], p->w_rot[0], p->w_rot[1], p->w_rot[2], p->w_vel[0], p->w_vel[1], p->w_vel[2],
                      p->w_omega[0], p->w_omega[1], p->w_omega[2], p->w_q, p->w_qd, p->terminal};
  for (double x : w)   // (this set alone accepts +inf: not check_finite_nonneg)
    if (!(x >= 0)) return fail(WBC_E_INVALID, "wbc_score_params: weights and terminal must be non-negative");
  if (!s) return fail(WBC_E_INVALID, "null solver");
  s->score = *p;
  return WBC_OK;
}

extern "C" int wbc_rollout_scored_batch(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in, const wbc_batch_out* out,
                                        const wbc_observer_state* obs, const wbc_plant* plant, const void* plan, void* tau_traj, void* com_traj,
                                        const wbc_rollout_score* score, void* stream) {
  RolloutExtras x;
  int rc = score_arg_check(score, &x.score);
  if (rc) return rc;
  rc = plant_args(plant, &x.tau_ext, &x.payload);
  if (rc) return rc;
  if (!plan && com_traj) return fail(WBC_E_INVALID, "com_traj needs a plan (the planner records it)");
  x.plan = plan; x.tau_traj = tau_traj; x.com_traj = com_traj;
  return rollout(s, N, horizon, in, out, obs, x, stream);
}

extern "C" int wbc_score_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* tau, const void* f, const int* status,
                               const wbc_rollout_score* score, int is_last, void* stream) {
  if (!s || !score) return fail(WBC_E_INVALID, "null argument");
  if (score->struct_size < sizeof(wbc_rollout_score)) return fail(WBC_E_INVALID, "wbc_rollout_score: struct_size too small");
  if (!score->goal || !score->cost) return fail(WBC_E_INVALID, "wbc_rollout_score: goal and cost are required");
  if (!q || !v || !tau || !f || !status) return fail(WBC_E_INVALID, "null argument");
  if (N == 0) return WBC_OK;
  ON_DEVICE(s);
  return score_tick(s, N, q, v, tau, f, status, score, score->accumulate != 0, is_last != 0, (hipStream_t)stream);
}

extern "C" int wbc_rollout_select(int dtype, size_t n_groups, size_t group, const void* cost, double lambda, int* best, void* best_cost,
                                  void* weights, void* stream) {
  if (dtype != WBC_F64 && dtype != WBC_F32) return fail(WBC_E_INVALID, "dtype must be WBC_F64 or WBC_F32");
  if (group < 1 || group > 4096) return fail(WBC_E_INVALID, "group must be in 1 .. 4096");
  if (n_groups > (size_t)0x7fffffff) return fail(WBC_E_INVALID, "n_groups is out of range (one workgroup per group)");   // (so n_groups * group cannot overflow)
  if (!cost || !best) return fail(WBC_E_INVALID, "null argument");
  if (n_groups == 0) return WBC_OK;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = dtype == WBC_F64
      ? k_rollout_select<double>(st, n_groups, group, (const double*)cost, lambda, best, (double*)best_cost, (double*)weights)
      : k_rollout_select<float>(st, n_groups, group, (const float*)cost, (float)lambda, best, (float*)best_cost, (float*)weights);
  if (e != hipSuccess) return fail(WBC_E_HIP, std::string("select launch: ") + hipGetErrorString(e));
  return WBC_OK;
}

// ---- CoM reference generator
extern "C" void wbc_ref_params_default(wbc_ref_params* g) {
  if (!g) return;
  std::memset(g, 0, sizeof(*g));
  const double kp[3] = {100, 100, 150}, kd[3] = {20, 20, 25}, kr[3] = {200, 200, 100}, dr[3] = {25, 25, 15};
  const double in[3] = {0.8, 1.85, 2.05};  // composite inertia of the synthetic quadruped in its nominal stance
  for (int i = 0; i < 3; ++i) { g->kp_com[i] = kp[i]; g->kd_com[i] = kd[i]; g->kp_rot[i] = kr[i]; g->kd_rot[i] = dr[i]; g->inertia_nom[i] = in[i]; }
  g->kp_joint = 200; g->kd_joint = 28;
}

template <class T> static int upload_ref(wbc_solver* s, const wbc_ref_params* g) {
  DevRefParams<T> d;
  for (int i = 0; i < 3; ++i) {
    d.kp_com[i] = (T)g->kp_com[i]; d.kd_com[i] = (T)g->kd_com[i]; d.kp_rot[i] = (T)g->kp_rot[i]; d.kd_rot[i] = (T)g->kd_rot[i];
    d.inertia_nom[i] = (T)g->inertia_nom[i];
  }
  d.kp_joint = (T)g->kp_joint; d.kd_joint = (T)g->kd_joint;
  for (int i = 0; i < 12; ++i) d.q_nom[i] = (T)g->q_nom[i];
  if (!s->d_ref) HIP_TRY(hipMalloc(&s->d_ref, sizeof(DevRefParams<double>)));
  HIP_TRY(hipMemcpy(s->d_ref, &d, sizeof(d), hipMemcpyHostToDevice));
  return WBC_OK;
}

extern "C" int wbc_solver_set_ref_params(wbc_solver* s, const wbc_ref_params* g) {
  if (!s || !g) return fail(WBC_E_INVALID, "null argument");
  for (int i = 0; i < 3; ++i)
    if (!(g->inertia_nom[i] >= 0)) return fail(WBC_E_INVALID, "inertia_nom must be non-negative");
  ON_DEVICE(s);
  return s->dtype == WBC_F64 ? upload_ref<double>(s, g) : upload_ref<float>(s, g);
}

extern "C" int wbc_reference_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* plan, double t,
                                   void* w_des, void* vdot_des, void* com, void* stream) {
  if (!s || !q || !v || !plan || !w_des || !vdot_des) return fail(WBC_E_INVALID, "null argument");
  if (!s->d_ref) return fail(WBC_E_INVALID, "call wbc_solver_set_ref_params first");
  if (N == 0) return WBC_OK;
  return launch_batch(s, N, stream, "reference", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    RefArgs<T> a;
    ref_args(a, s, N, q, v, plan, t, w_des, vdot_des, com);
    return k_reference<T>(L, dev_model<T>(s), (const DevRefParams<T>*)s->d_ref, a);
  });
}
