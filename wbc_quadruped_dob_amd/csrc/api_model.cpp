// C-ABI (include/wbc_hip.h): the robot model and the controller parameters.  Plain C++: no HIP header, no device.
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "host_internal.hpp"

using namespace wbc;

extern "C" int wbc_model_load_urdf(const char* path, const char* const* foot_links, int n_foot_links, wbc_model** out) {
  if (!path || !out || n_foot_links < 0 || (n_foot_links > 0 && !foot_links)) return fail(WBC_E_INVALID, "null argument");
  *out = nullptr;
  std::vector<std::string> feet;
  for (int i = 0; i < n_foot_links; ++i) {
    if (!foot_links[i]) return fail(WBC_E_INVALID, "null foot link name");
    feet.emplace_back(foot_links[i]);
  }
  wbc_model* m = new (std::nothrow) wbc_model;
  if (!m) return fail(WBC_E_INVALID, "out of memory");
  std::string err;
  int rc;
  try {
    rc = load_urdf(path, feet, m->fm, err);
  } catch (const std::exception& e) {
    rc = WBC_E_PARSE; err = e.what();
  }
  if (rc != WBC_OK) { delete m; return fail(rc, err); }
  *out = m;
  return WBC_OK;
}

extern "C" int wbc_model_from_flat(int nb, const int* parent, const double* Rt, const double* rt, const double* axis,
                                   const double* mass, const double* com, const double* Ic, int nf,
                                   const int* foot_body, const double* foot_off, const double* gravity,
                                   wbc_model** out) {
  if (!out || nb < 1 || nb > 64 || nf < 0 || nf > 16 || !parent || !Rt || !rt || !axis || !mass || !com || !Ic ||
      (nf > 0 && (!foot_body || !foot_off)))
    return fail(WBC_E_INVALID, "bad argument");
  *out = nullptr;
  for (int i = 0; i < nb; ++i)
    if ((i == 0 && parent[i] != -1) || (i > 0 && (parent[i] < 0 || parent[i] >= i)))
      return fail(WBC_E_INVALID, "parent[] must satisfy parent[0] = -1, 0 <= parent[i] < i");
  for (int k = 0; k < nf; ++k)
    if (foot_body[k] < 0 || foot_body[k] >= nb) return fail(WBC_E_INVALID, "foot_body out of range");
  wbc_model* m = new (std::nothrow) wbc_model;
  if (!m) return fail(WBC_E_INVALID, "out of memory");
  FlatModel& f = m->fm;
  f.nb = nb;
  f.parent.assign(parent, parent + nb);
  f.Rt.assign(Rt, Rt + 9 * nb);
  f.rt.assign(rt, rt + 3 * nb);
  f.axis.assign(axis, axis + 3 * nb);
  f.mass.assign(mass, mass + nb);
  f.com.assign(com, com + 3 * nb);
  f.Ic.assign(Ic, Ic + 6 * nb);
  f.foot_body.assign(foot_body, foot_body + nf);
  f.foot_off.assign(foot_off, foot_off + 3 * nf);
  if (gravity) for (int k = 0; k < 3; ++k) f.gravity[k] = gravity[k];
  f.joint_names.assign(nb - 1, "");
  f.foot_links.assign(nf, "");
  f.body_names.assign(nb, "");
  *out = m;
  return WBC_OK;
}

extern "C" void wbc_model_free(wbc_model* m) { delete m; }

extern "C" int wbc_model_dims(const wbc_model* m, int* nb, int* nq, int* nv, int* nj, int* nf) {
  if (!m) return fail(WBC_E_INVALID, "null model");
  if (nb) *nb = m->fm.nb;
  if (nq) *nq = m->fm.nq();
  if (nv) *nv = m->fm.nv();
  if (nj) *nj = m->fm.nj();
  if (nf) *nf = m->fm.nf();
  return WBC_OK;
}

extern "C" int wbc_model_get_flat(const wbc_model* m, int* parent, double* Rt, double* rt, double* axis, double* mass,
                                  double* com, double* Ic, int* foot_body, double* foot_off, double* gravity) {
  if (!m) return fail(WBC_E_INVALID, "null model");
  const FlatModel& f = m->fm;
  auto cp = [](auto* dst, const auto& v) { if (dst) std::memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
  cp(parent, f.parent); cp(Rt, f.Rt); cp(rt, f.rt); cp(axis, f.axis); cp(mass, f.mass); cp(com, f.com); cp(Ic, f.Ic);
  cp(foot_body, f.foot_body); cp(foot_off, f.foot_off);
  if (gravity) for (int k = 0; k < 3; ++k) gravity[k] = f.gravity[k];
  return WBC_OK;
}

extern "C" const char* wbc_model_joint_name(const wbc_model* m, int j) {
  if (!m || j < 0 || j >= (int)m->fm.joint_names.size()) return nullptr;
  return m->fm.joint_names[j].c_str();
}
extern "C" const char* wbc_model_foot_link(const wbc_model* m, int k) {
  if (!m || k < 0 || k >= (int)m->fm.foot_links.size()) return nullptr;
  return m->fm.foot_links[k].c_str();
}
extern "C" double wbc_model_total_mass(const wbc_model* m) {
  if (!m) return 0.0;
  double s = 0;
  for (double x : m->fm.mass) s += x;
  return s;
}

extern "C" int wbc_model_effort_limits(const wbc_model* m, double* lim) {
  if (!m || !lim) return fail(WBC_E_INVALID, "null argument");
  const int nj = m->fm.nj();
  for (int j = 0; j < nj; ++j) lim[j] = j < (int)m->fm.effort_limit.size() ? m->fm.effort_limit[j] : HUGE_VAL;
  return WBC_OK;
}

extern "C" void wbc_params_default(wbc_params* p, int dtype) {
  if (!p) return;
  for (int i = 0; i < 6; ++i) p->S[i] = 1.0;
  p->alpha = 1e-3; p->fn_min = 0.0; p->fn_max = 400.0; p->mu_scale = 1.0; p->dt = 1e-3;
  p->observer_order = 0; p->max_iter = 100;
  p->qp_tol = (dtype == WBC_F32) ? 1e-3 : 1e-9;
  for (int i = 0; i < WBC_MAXV; ++i) { p->K1[i] = 50.0; p->K2[i] = 200.0; }
}

int wbc::check_params_public(const wbc_params* p) {
  if (!p) return fail(WBC_E_INVALID, "null params");
  if (!(p->alpha > 0)) return fail(WBC_E_INVALID, "alpha must be > 0 (strict convexity of the GRF QP)");
  if (!(p->fn_max >= p->fn_min)) return fail(WBC_E_INVALID, "fn_max < fn_min");
  if (p->observer_order < 0 || p->observer_order > 2) return fail(WBC_E_INVALID, "observer_order must be 0, 1 or 2");
  if (p->max_iter < 1) return fail(WBC_E_INVALID, "max_iter must be >= 1");
  for (int i = 0; i < 6; ++i) if (!(p->S[i] >= 0)) return fail(WBC_E_INVALID, "S must be >= 0");
  return WBC_OK;
}

// the gait scheduler's default schedule is the model's: a trot over the hips of this robot
extern "C" void wbc_gait_params_default(const wbc_model* m, wbc_gait_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->period = 0.4;
  const double off[4] = {0.0, 0.5, 0.5, 0.0};   // feet {0, 3} and {1, 2}: the diagonal pairs
  for (int k = 0; k < 4; ++k) { p->duty[k] = 0.6; p->offset[k] = off[k]; }
  p->clearance = 0.05; p->k_v = 0.03; p->late = 0.5; p->retarget = 1;
  int leg_body[4][3];
  std::string err;
  if (m && quadruped_topology(m->fm, leg_body, err) == WBC_OK)
    for (int k = 0; k < 4; ++k) { p->base_xy[k][0] = m->fm.rt[3 * leg_body[k][0]]; p->base_xy[k][1] = m->fm.rt[3 * leg_body[k][0] + 1]; }
}

extern "C" int wbc_abi_version(void) { return 10; }  // 10: wbc_plant, wbc_integrate_plant_batch / wbc_rollout_plant_batch / wbc_rollout_tracking_plant_batch (plant payload); 9: wbc_solver_options.fused_pair, wbc_tick_plan.fused = 3 (fused_pair_kernel); 8: wbc_solver_options.tile_tick, wbc_tick_plan.fused = 2 / qp_body = 2 (staged QP tiles); 7: wbc_solver_collect_timing_n (the unsized call writes 5 entries again), wbc_solver_options.multi_threads / multi_spin_us, wbc_multi_tick_gather / wbc_multi_issue_threads / wbc_multi_host_stats; 6: wbc_plan_tick / wbc_solver_plan_tick / wbc_dispatch_thresholds, wbc_solver_invalidate_structural, warm start (wbc_step_batch_warm, wbc_multi_step_batch_warm, wbc_solver_options.rollout_warm, wbc_tick_plan.qp_warm, WBC_PLAN_* flags), wbc_multi_allgather_tau_async / wbc_multi_gather_wait; 5: wbc_qp_dense_batch; 4: wbc_one_map / wbc_one_tick, wbc_solver_options.f32_pack2 and one_zerocopy 2 / 3 (options struct grows at its end: struct_size keeps version-3 callers valid); 3: wbc_solver_options / wbc_solver_create_ex, wbc_observer_init, wbc_multi_* (2: integrate takes Jc, timing arrays have 4 entries, reference / tracking entry points)
