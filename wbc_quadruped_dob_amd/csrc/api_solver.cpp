// C-ABI (include/wbc_hip.h): the solver's lifetime (the device model, the buffers every call shares), its parameters and diagnostics, and the timing ring.
#include <new>

#include "solver.hpp"

using namespace wbc;

template <class T> static void build_dev_model(const FlatModel& f, const int leg_body[4][3], DevModel<T>& d) {
  std::memset(&d, 0, sizeof(d));
  auto put = [&](int leg, int idx, double v) { d.cst[idx * 4 + leg] = (T)v; };
  // body b's inertia about its joint origin (parallel axes), xx xy xz yy yz zz, through store(e, value)
  auto inertia_at_origin = [&](int b, auto store) {
    const double m = f.mass[b], *c = &f.com[3 * b], *I = &f.Ic[6 * b];
    const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    const double Io[6] = {I[0] + m * (cc - c[0] * c[0]), I[1] - m * c[0] * c[1], I[2] - m * c[0] * c[2],
                          I[3] + m * (cc - c[1] * c[1]), I[4] - m * c[1] * c[2], I[5] + m * (cc - c[2] * c[2])};
    for (int e = 0; e < 6; ++e) store(e, Io[e]);
  };
  for (int l = 0; l < 4; ++l) {
    for (int k = 0; k < 3; ++k) {
      const int b = leg_body[l][k], o = JOINT_WORDS * k;
      const double* Rt = &f.Rt[9 * b];
      const double* ax = &f.axis[3 * b];
      double A0[9], A2[9];
      // A0 = Rt a a^T ; A2 = Rt [a]x
      double Ra[3];
      for (int i = 0; i < 3; ++i) Ra[i] = Rt[3 * i] * ax[0] + Rt[3 * i + 1] * ax[1] + Rt[3 * i + 2] * ax[2];
      const double K[9] = {0, -ax[2], ax[1], ax[2], 0, -ax[0], -ax[1], ax[0], 0};
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          A0[3 * i + j] = Ra[i] * ax[j];
          double s = 0;
          for (int q = 0; q < 3; ++q) s += Rt[3 * i + q] * K[3 * q + j];
          A2[3 * i + j] = s;
        }
      for (int e = 0; e < 9; ++e) { put(l, o + e, A0[e]); put(l, o + 9 + e, Rt[e] - A0[e]); put(l, o + 18 + e, A2[e]); }
      for (int e = 0; e < 3; ++e) { put(l, o + 27 + e, f.rt[3 * b + e]); put(l, o + 30 + e, ax[e]); }
      const double m = f.mass[b], *c = &f.com[3 * b];
      put(l, o + 33, m);
      for (int e = 0; e < 3; ++e) put(l, o + 34 + e, m * c[e]);
      inertia_at_origin(b, [&](int e, double v) { put(l, o + 37 + e, v); });
      d.jidx[l][k] = b - 1;
    }
    for (int e = 0; e < 3; ++e) put(l, 129 + e, f.foot_off[3 * l + e]);
  }
  d.base_m = (T)f.mass[0];
  for (int e = 0; e < 3; ++e) d.base_h[e] = (T)(f.mass[0] * f.com[e]);
  inertia_at_origin(0, [&](int e, double v) { d.base_Io[e] = (T)v; });
  for (int e = 0; e < 3; ++e) d.grav[e] = (T)f.gravity[e];
  // structural zeros of the packed mass matrix
  int nz = 0;
  auto mi = [](int i, int j) { if (i > j) { int t = i; i = j; j = t; } return i * 18 - i * (i - 1) / 2 + (j - i); };
  for (int l1 = 0; l1 < 4; ++l1)
    for (int l2 = l1 + 1; l2 < 4; ++l2)
      for (int ka = 0; ka < 3; ++ka)
        for (int kb = 0; kb < 3; ++kb) d.zidx[nz++] = mi(6 + d.jidx[l1][ka], 6 + d.jidx[l2][kb]);
  const int bz[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 4}, {2, 5}};
  for (auto& e : bz) d.zidx[nz++] = mi(e[0], e[1]);
  for (; nz < 64; ++nz) d.zidx[nz] = -1;
}

template <class T> static hipError_t upload_model(wbc_solver* s, const FlatModel& f) {
  DevModel<T> dm;
  build_dev_model(f, s->leg_body, dm);
  const hipError_t e = hipMalloc(&s->d_model, sizeof(dm));
  return e != hipSuccess ? e : hipMemcpy(s->d_model, &dm, sizeof(dm), hipMemcpyHostToDevice);
}

extern "C" int wbc_solver_create_ex(const wbc_model* m, const wbc_params* p, int dtype, int device, size_t max_batch,
                                    const wbc_solver_options* opt, wbc_solver** out) {
  if (!m || !out || max_batch == 0 || (dtype != WBC_F64 && dtype != WBC_F32)) return fail(WBC_E_INVALID, "bad argument");
  *out = nullptr;
  if (max_batch > ((size_t)1 << 21))  // keeps every component-major array below 4 GiB (32-bit lane offsets)
    return fail(WBC_E_CAPACITY, "max_batch above 2^21 states per solver: shard the batch over more solvers");
  int rc = check_params_public(p);
  if (rc) return rc;
  wbc_solver_options o;
  rc = options_from_caller(opt, o);
  if (rc) return rc;
  if (o.rollout_spw != 0 && o.rollout_spw != 4 && o.rollout_spw != 16) return fail(WBC_E_INVALID, "rollout_spw must be 0 (auto), 4 or 16");
  {   // the tile sizes the kernels of this scalar type exist for (k_qp.hip)
    const int ok64[] = {0, -1, 32, 36, 40, 44, 48, 52, 56, 60, 64, 128, 256, 512};
    const int ok32[] = {0, -1, 32, 36, 40, 44, 48, 52, 56, 60, 64, 72, 80, 88, 96, 104, 112, 120, 128, 256, 512};
    bool found = false;
    if (dtype == WBC_F64) { for (int v : ok64) found = found || o.qp_tile == v; }
    else { for (int v : ok32) found = found || o.qp_tile == v; found = found || (o.qp_tile > 0 && o.qp_tile <= wbc::STILE_MAX_TILE && o.qp_tile % 4 == 0); }
    if (!found) return fail(WBC_E_INVALID, "qp_tile: 0 (auto), -1 (off), 32, 64, 128, 256, 512; fp64 also 36 ... 60 in steps of 4, fp32 also every multiple of 4 up to 192");
  }
  if (o.timing_mode != WBC_TIMING_DISPATCH && o.timing_mode != WBC_TIMING_EVENT_PAIR) return fail(WBC_E_INVALID, "bad timing_mode");
  if (o.f32_pack2 < -1 || o.f32_pack2 > 1) return fail(WBC_E_INVALID, "f32_pack2 must be -1, 0 or 1");
  if (o.keep_structural != 0 && o.keep_structural != 1) return fail(WBC_E_INVALID, "keep_structural must be 0 or 1");
  if (o.one_zerocopy < 0 || o.one_zerocopy > 3) return fail(WBC_E_INVALID, "one_zerocopy must be 0 ... 3");
  if (o.rollout_warm != 0 && o.rollout_warm != 1) return fail(WBC_E_INVALID, "rollout_warm must be 0 or 1");
  if (o.obs_colaunch < -1 || o.obs_colaunch > 1) return fail(WBC_E_INVALID, "obs_colaunch must be -1, 0 or 1");
  if (o.tile_tick < -1 || o.tile_tick > 1) return fail(WBC_E_INVALID, "tile_tick must be -1, 0 or 1");
  int leg_body[4][3];
  std::string err;
  rc = quadruped_topology(m->fm, leg_body, err);
  if (rc) return fail(rc, err);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(WBC_E_NODEVICE, "no HIP device: the WBC hot path has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(WBC_E_INVALID, "device index out of range");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(WBC_E_NODEVICE, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);
  wbc_solver* s = new (std::nothrow) wbc_solver;
  if (!s) return fail(WBC_E_INVALID, "out of memory");
  s->dtype = dtype; s->device = device; s->max_batch = max_batch; s->params = *p; s->opt = o;
  wbc_score_params_default(&s->score);
  wbc_swing_params_default(&s->swing);
  wbc_gait_params_default(m, &s->gait);
  wbc_ground_params_default(&s->ground);
  wbc_stiction_params_default(&s->stiction);
  wbc_contact_params_default(&s->contact_est);
  wbc_foothold_params_default(&s->foothold);
  wbc_odom_params_default(&s->odom);
  wbc_trunk_params_default(&s->trunk);
  for (int j = 0; j < WBC_MAXV; ++j) s->model_effort[j] = (j < m->fm.nj() && j < (int)m->fm.effort_limit.size()) ? m->fm.effort_limit[j] : HUGE_VAL;
  std::memcpy(s->tau_max, s->model_effort, sizeof(s->tau_max));
  s->limit_grid = limit_qp_grid(prop.multiProcessorCount);
  s->rz = resolve_options(dtype, o);
  std::memcpy(s->leg_body, leg_body, sizeof(leg_body));
  for (int l = 0; l < 4; ++l) for (int k = 0; k < 3; ++k) s->jmap.j[3 * l + k] = leg_body[l][k] - 1;
  s->jpack = pack_jidx(s->jmap.j);
  const size_t ts = dtype == WBC_F64 ? 8 : 4;
  DeviceGuard guard(device);
  hipError_t e = guard.err;
  if (e == hipSuccess) e = dtype == WBC_F64 ? upload_model<double>(s, m->fm) : upload_model<float>(s, m->fm);
  if (e == hipSuccess) e = hipMalloc(&s->d_ws, (size_t)WS_LDS_WORDS * max_batch * ts);
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_todo, (max_batch + 4) * sizeof(int));
  if (e == hipSuccess) e = hipMemset(s->d_todo, 0, 4 * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_aset, max_batch * sizeof(int));
  if (e == hipSuccess) e = hipMemset(s->d_aset, 0, max_batch * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_limit, (max_batch + LIMIT_LIST_HEAD) * sizeof(int));
  if (e == hipSuccess) e = hipMemset(s->d_limit, 0, LIMIT_LIST_HEAD * sizeof(int));
  // N = 1 image: q19 v18 w6 a18 n12 mu4 tp12 fp12 integ18 r18 tau12 f12 (scalars; 161 of ONE_TICK_SCALARS), a scratch region for
  // the start-up / planner helpers (wbc_observer_init, wbc_compute_reference: they must not touch what a caller keeps in the
  // image between ticks, wbc_one_map), then the ints mask | status | iters | completion ticket
  s->one_bytes = ONE_SCALARS * sizeof(double) + 4 * sizeof(int);
  if (e == hipSuccess) e = hipMalloc(&s->d_one, s->one_bytes);
  if (e == hipSuccess) e = hipHostMalloc(&s->h_one, s->one_bytes, hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer(&s->h_one_dev, s->h_one, 0);
  // (the completion ticket lives in this image: a recycled pinned block must not look like ticket 1 of a solver whose first tick is still running)
  if (e == hipSuccess) { std::memset(s->h_one, 0, s->one_bytes); e = hipMemset(s->d_one, 0, s->one_bytes); }
  if (e == hipSuccess) e = hipMalloc(&s->d_stage_one, STAGE_ONE_DOUBLES * sizeof(double) + STAGE_ONE_INTS * sizeof(int));
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->aux, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming);
  // kernels with more than 64 kB of dynamic LDS (staged QP tiles, tile tick): the limit is raised here, not inside a tick (which may be under stream capture)
  if (e == hipSuccess) e = dtype == WBC_F64 ? k_qp_prepare<double>() : k_qp_prepare<float>();
  if (e == hipSuccess) e = dtype == WBC_F64 ? k_tile_prepare<double>() : k_tile_prepare<float>();
  if (e != hipSuccess) {
    std::string msg = std::string("device allocation failed: ") + hipGetErrorString(e);
    wbc_solver_destroy(s);
    return fail(WBC_E_HIP, msg);
  }
  *out = s;
  return WBC_OK;
}

extern "C" int wbc_solver_create(const wbc_model* m, const wbc_params* p, int dtype, int device, size_t max_batch,
                                 wbc_solver** out) {
  return wbc_solver_create_ex(m, p, dtype, device, max_batch, nullptr, out);
}

extern "C" void wbc_solver_destroy(wbc_solver* s) {
  if (!s) return;
  DeviceGuard guard(s->device);
  if (s->d_model) (void)hipFree(s->d_model);
  if (s->d_ws) (void)hipFree(s->d_ws);
  if (s->d_todo) (void)hipFree(s->d_todo);
  if (s->d_aset) (void)hipFree(s->d_aset);
  if (s->d_limit) (void)hipFree(s->d_limit);
  if (s->d_one) (void)hipFree(s->d_one);
  if (s->h_one) (void)hipHostFree(s->h_one);
  if (s->d_ref) (void)hipFree(s->d_ref);
  if (s->d_stage_one) (void)hipFree(s->d_stage_one);
  if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
  if (s->ev_join) (void)hipEventDestroy(s->ev_join);
  if (s->aux) (void)hipStreamDestroy(s->aux);
  for (hipEvent_t ev : s->ev_pool) (void)hipEventDestroy(ev);
  delete s;
}

extern "C" int wbc_solver_set_params(wbc_solver* s, const wbc_params* p) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  int rc = check_params_public(p);
  if (rc) return rc;
  s->params = *p;
  return WBC_OK;
}

extern "C" int wbc_solver_device(const wbc_solver* s) { return s ? s->device : -1; }

extern "C" int wbc_solver_plan_tick(const wbc_solver* s, size_t N, int with_mats, int with_pf, int warm, wbc_tick_plan* plan) {
  if (!s || !plan) return fail(WBC_E_INVALID, "null argument");
  plan_to_public(plan_tick(s->dtype, s->params.observer_order, s->opt, s->rz, N, with_mats != 0, with_pf != 0, warm != 0), plan);
  return WBC_OK;
}

// keep_structural: forget which M / Jc buffers hold their structural constants (the caller freed, reallocated or overwrote them)
extern "C" int wbc_solver_invalidate_structural(wbc_solver* s) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  s->kept_M = nullptr; s->kept_Jc = nullptr; s->kept_N = 0;
  return WBC_OK;
}

// diagnostics: how many states of the LAST two-kernel tick the per-lane QP kernel handed to the dense kernel (synchronises)
extern "C" int wbc_solver_qp_handover(wbc_solver* s, int* count) {
  if (!s || !count) return fail(WBC_E_INVALID, "null argument");
  ON_DEVICE(s);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(count, s->d_todo + 2, sizeof(int), hipMemcpyDeviceToHost));   // [2]: what qp_list_kernel saw before it emptied the list
  return WBC_OK;
}

// ---- timing (SpanScope, solver.hpp): the ring of event pairs and its read-out
extern "C" int wbc_solver_enable_timing(wbc_solver* s, int on) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (on && s->ev_pool.size() != 2 * TIMING_MAX_SPANS) {
    ON_DEVICE(s);
    // built in a local vector and swapped in only when complete: a pool left short by a failed hipEventCreate would be
    // indexed past its end by the next SpanScope
    std::vector<hipEvent_t> pool;
    pool.reserve(2 * TIMING_MAX_SPANS);
    for (size_t i = 0; i < 2 * TIMING_MAX_SPANS; ++i) {
      hipEvent_t ev;
      const hipError_t e = hipEventCreate(&ev);
      if (e != hipSuccess) {
        for (hipEvent_t x : pool) (void)hipEventDestroy(x);
        return fail(WBC_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
      }
      pool.push_back(ev);
    }
    for (hipEvent_t x : s->ev_pool) (void)hipEventDestroy(x);
    s->ev_pool.swap(pool);
    s->spans.reserve(TIMING_MAX_SPANS);
  }
  s->timing = on != 0;
  s->timing_period = on > 1 ? on : 1;  // on = k > 1: sample every k-th tick (keeps the event cost out of the rest)
  s->calls = 0;
  s->sample_now = false;
  s->spans.clear();
  s->dropped = 0;
  return WBC_OK;
}

// cap = entries of the caller's arrays: kinds beyond it are dropped, never written (the unsized call wrote as many entries as THIS
// build knows, whatever the caller was built against)
extern "C" int wbc_solver_collect_timing_n(wbc_solver* s, double* ms, int* launches, int cap) {
  if (!s || !ms || !launches || cap < 0) return fail(WBC_E_INVALID, "bad argument");
  const int n = cap < WBC_TIMING_KINDS ? cap : WBC_TIMING_KINDS;
  for (int k = 0; k < n; ++k) { ms[k] = 0; launches[k] = 0; }
  ON_DEVICE(s);
  for (auto& sp : s->spans) {
    HIP_TRY(hipEventSynchronize(sp.b));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, sp.a, sp.b));
    if (sp.kind < n) { ms[sp.kind] += t; launches[sp.kind]++; }
  }
  s->spans.clear();
  s->dropped = 0;
  return WBC_OK;
}
// the unsized call of ABI <= 6 writes the FIVE entries every version of it has had (kind 5, the persistent rollout kernel, needs the sized call)
extern "C" int wbc_solver_collect_timing(wbc_solver* s, double* ms, int* launches) { return wbc_solver_collect_timing_n(s, ms, launches, 5); }
