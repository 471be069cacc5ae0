// C-ABI (include/wbc_hip.h): the walking tick's families -- swing-foot references, the gait scheduler, the ground-contact plant and its stiction, contact
// sensing from the observer's residual, the terrain heightfield, foothold selection, the base state from leg odometry.  Each: its parameters, the builder of its kernel argument, its one-launch batch calls.
#include "solver.hpp"

using namespace wbc;

// ---- swing-foot references: the gains, the stand-alone call, the CoM reference generator with the swing law fused in
extern "C" void wbc_swing_params_default(wbc_swing_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  for (int i = 0; i < 3; ++i) { p->kp[i] = 400; p->kd[i] = 40; }   // critically damped
  p->damping = 1e-4;
}

extern "C" int wbc_solver_set_swing_params(wbc_solver* s, const wbc_swing_params* p) {
  if (!s || !p) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = check_struct_size(p, "wbc_swing_params: struct_size too small (call wbc_swing_params_default first)")) return rc;
  if (const int rc = check_finite_nonneg({p->kp[0], p->kp[1], p->kp[2], p->kd[0], p->kd[1], p->kd[2], p->damping},
                                         "wbc_swing_params: gains and damping must be finite and non-negative")) return rc;
  s->swing = *p;
  return WBC_OK;
}

template <class T>
static void swing_args(SwingArgs<T>& a, const wbc_solver* s, const int* mask, const void* swing, void* foot) {
  std::memset(&a, 0, sizeof(a));
  a.mask = mask; a.swing = (const T*)swing; a.foot = (T*)foot;
  for (int i = 0; i < 3; ++i) { a.P.kp[i] = (T)s->swing.kp[i]; a.P.kd[i] = (T)s->swing.kd[i]; }
  a.P.damping = (T)s->swing.damping;
}

extern "C" int wbc_swing_reference_batch(wbc_solver* s, size_t N, const void* q, const void* v, const int* mask, const void* swing, double t,
                                         void* vdot_des, void* foot, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !mask || !swing || !vdot_des) return fail(WBC_E_INVALID, "null argument");
  return launch_batch(s, N, stream, "swing reference", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    SwingRefArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.N = N; a.q = (const T*)q; a.v = (const T*)v; a.t = (T)t; a.vdot_des = (T*)vdot_des; a.jpack = s->jpack;
    swing_args(a.s, s, mask, swing, foot);
    return k_swing_reference<T>(L, dev_model<T>(s), a);
  });
}

extern "C" int wbc_reference_swing_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* plan, const int* mask, const void* swing,
                                         double t, void* w_des, void* vdot_des, void* com, void* foot, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !plan || !mask || !swing || !w_des || !vdot_des) return fail(WBC_E_INVALID, "null argument");
  if (!s->d_ref) return fail(WBC_E_INVALID, "call wbc_solver_set_ref_params first");
  return launch_batch(s, N, stream, "reference + swing", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    RefArgs<T> a;
    ref_args(a, s, N, q, v, plan, t, w_des, vdot_des, com);
    SwingArgs<T> sa;
    swing_args(sa, s, mask, swing, foot);
    return k_reference_swing<T>(L, dev_model<T>(s), (const DevRefParams<T>*)s->d_ref, a, sa);
  });
}

// ---- gait scheduler: the schedule (its defaults are the model's: api_model.cpp), the batch call (phase, mask and the lifted feet's plan words advance in place)
extern "C" int wbc_solver_set_gait_params(wbc_solver* s, const wbc_gait_params* p) {
  if (!s || !p) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = check_struct_size(p, "wbc_gait_params: struct_size too small (call wbc_gait_params_default first)")) return rc;
  if (!(p->period > 0) || !std::isfinite(p->period)) return fail(WBC_E_INVALID, "wbc_gait_params: period must be finite and > 0");
  for (int k = 0; k < 4; ++k) {
    if (!(p->duty[k] > 0 && p->duty[k] <= 1)) return fail(WBC_E_INVALID, "wbc_gait_params: 0 < duty <= 1");
    if (!(p->offset[k] >= 0 && p->offset[k] < 1)) return fail(WBC_E_INVALID, "wbc_gait_params: 0 <= offset < 1");
    if (!std::isfinite(p->base_xy[k][0]) || !std::isfinite(p->base_xy[k][1])) return fail(WBC_E_INVALID, "wbc_gait_params: base_xy must be finite");
  }
  if (const int rc = check_finite_nonneg({p->clearance}, "wbc_gait_params: clearance must be finite and >= 0")) return rc;
  if (!std::isfinite(p->k_v)) return fail(WBC_E_INVALID, "wbc_gait_params: k_v must be finite");
  if (!(p->late > 0 && p->late <= 1)) return fail(WBC_E_INVALID, "wbc_gait_params: 0 < late <= 1");
  if (p->retarget != 0 && p->retarget != 1) return fail(WBC_E_INVALID, "wbc_gait_params: retarget must be 0 or 1");
  s->gait = *p;
  return WBC_OK;
}

// (the caller has zeroed `a`; shared with wbc_gait_estimated_batch, which forms the contact word in the same launch and passes contact = null)
template <class T>
static void gait_args(GaitArgs<T>& a, const wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const int* contact, void* phase,
                      int* mask, void* swing, int* events) {
  a.N = N; a.q = (const T*)q; a.v = (const T*)v; a.cmd = (const T*)cmd; a.contact = contact;
  a.phase = (T*)phase; a.mask = mask; a.swing = (T*)swing; a.events = events; a.jpack = s->jpack;
  const wbc_gait_params& g = s->gait;
  a.P.dphi = (T)(s->params.dt / g.period); a.P.period = (T)g.period; a.P.clearance = (T)g.clearance; a.P.k_v = (T)g.k_v; a.P.late = (T)g.late;
  for (int k = 0; k < 4; ++k) {
    a.P.duty[k] = (T)g.duty[k]; a.P.offset[k] = (T)g.offset[k];
    a.P.inv_sw[k] = g.duty[k] == 1.0 ? (T)0 : (T)(1.0 / (1.0 - g.duty[k]));
    a.P.T_sw[k] = (T)((1.0 - g.duty[k]) * g.period);
    a.P.bx[k] = (T)g.base_xy[k][0]; a.P.by[k] = (T)g.base_xy[k][1];
  }
  a.P.retarget = g.retarget;
}

extern "C" int wbc_gait_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const int* contact, void* phase, int* mask,
                              void* swing, int* events, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !cmd || !phase || !mask || !swing) return fail(WBC_E_INVALID, "null argument");
  return launch_batch(s, N, stream, "gait", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    GaitArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    gait_args(a, s, N, q, v, cmd, contact, phase, mask, swing, events);
    return k_gait<T>(L, dev_model<T>(s), a);
  });
}

// ---- ground-contact plant: the contact law's constants, the law alone, the law + forward dynamics as one launch
extern "C" void wbc_ground_params_default(wbc_ground_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->k_n = 2e4; p->c_n = 150.0; p->c_t = 200.0; p->f_touch = 5.0;   // how they were fixed: include/wbc_hip.h
}

extern "C" int wbc_solver_set_ground_params(wbc_solver* s, const wbc_ground_params* p) {
  if (!s || !p) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = check_struct_size(p, "wbc_ground_params: struct_size too small (call wbc_ground_params_default first)")) return rc;
  if (const int rc = check_finite_nonneg({p->k_n, p->c_n, p->c_t, p->f_touch}, "wbc_ground_params: k_n, c_n, c_t, f_touch must be finite and >= 0")) return rc;
  s->ground = *p;
  return WBC_OK;
}

template <class T>
static void ground_io(GroundIO<T>& g, const wbc_solver* s, const void* normals, const void* height, const void* mu, void* f_gr, int* contact, void* gap) {
  g.normals = (const T*)normals; g.height = (const T*)height; g.mu = (const T*)mu;
  g.f_gr = (T*)f_gr; g.contact = contact; g.gap = (T*)gap;
  g.P.k_n = (T)s->ground.k_n; g.P.c_n = (T)s->ground.c_n; g.P.c_t = (T)s->ground.c_t; g.P.f_touch = (T)s->ground.f_touch;
}

extern "C" int wbc_ground_force_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* Jc, const void* normals, const void* height,
                                      const void* mu, void* f_gr, int* contact, void* gap, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !Jc || !normals || !height || !mu || !f_gr) return fail(WBC_E_INVALID, "null argument");
  return launch_batch(s, N, stream, "ground force", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    GroundArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.N = N; a.q = (const T*)q; a.v = (const T*)v; a.Jc = (const T*)Jc; a.jpack = s->jpack;
    ground_io(a.g, s, normals, height, mu, f_gr, contact, gap);
    return k_ground_force<T>(L, dev_model<T>(s), a);
  });
}

extern "C" int wbc_integrate_ground_batch(wbc_solver* s, size_t N, void* q, void* v, const void* M, const void* h, const void* Jc, const void* tau,
                                          const void* normals, const void* height, const void* mu, const void* tau_ext, void* f_gr, int* contact,
                                          void* gap, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !M || !h || !Jc || !tau || !normals || !height || !mu || !f_gr) return fail(WBC_E_INVALID, "null argument");
  return launch_batch(s, N, stream, "integrate ground", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    GroundIntegrateArgs<T> a;
    integrate_args<T>(a, s, N, q, v, M, h, Jc, tau, nullptr, tau_ext, nullptr);   // (zeroes the IntegrateArgs part; f is not read)
    ground_io(a.g, s, normals, height, mu, f_gr, contact, gap);
    return k_ground_integrate<T>(L, dev_model<T>(s), a);
  });
}

// ---- stiction on the ground plant: the anchor spring's stiffness, the law alone, the law + forward dynamics as one launch
extern "C" void wbc_stiction_params_default(wbc_stiction_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->k_t = 2e4;   // how it was fixed: include/wbc_hip.h
}

extern "C" int wbc_solver_set_stiction_params(wbc_solver* s, const wbc_stiction_params* p) {
  if (!s || !p) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = check_struct_size(p, "wbc_stiction_params: struct_size too small (call wbc_stiction_params_default first)")) return rc;
  if (const int rc = check_finite_nonneg({p->k_t}, "wbc_stiction_params: k_t must be finite and >= 0")) return rc;
  s->stiction = *p;
  return WBC_OK;
}

template <class T>
static void stick_io(StickIO<T>& k, const wbc_solver* s, void* anchor, int* stick) {
  k.anchor = (T*)anchor; k.stick = stick; k.k_t = (T)s->stiction.k_t;
}

extern "C" int wbc_ground_stick_force_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* Jc, const void* normals,
                                            const void* height, const void* mu, void* anchor, int* stick, void* f_gr, int* contact, void* gap,
                                            void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !Jc || !normals || !height || !mu || !anchor || !stick || !f_gr) return fail(WBC_E_INVALID, "null argument");
  return launch_batch(s, N, stream, "ground stick force", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    StickArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.N = N; a.q = (const T*)q; a.v = (const T*)v; a.Jc = (const T*)Jc; a.jpack = s->jpack;
    ground_io(a.g, s, normals, height, mu, f_gr, contact, gap);
    stick_io(a.s, s, anchor, stick);
    return k_stick_force<T>(L, dev_model<T>(s), a);
  });
}

extern "C" int wbc_integrate_ground_stick_batch(wbc_solver* s, size_t N, void* q, void* v, const void* M, const void* h, const void* Jc,
                                                const void* tau, const void* normals, const void* height, const void* mu, const void* tau_ext,
                                                void* anchor, int* stick, void* f_gr, int* contact, void* gap, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !M || !h || !Jc || !tau || !normals || !height || !mu || !anchor || !stick || !f_gr) return fail(WBC_E_INVALID, "null argument");
  return launch_batch(s, N, stream, "integrate ground stick", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    StickIntegrateArgs<T> a;
    integrate_args<T>(a, s, N, q, v, M, h, Jc, tau, nullptr, tau_ext, nullptr);   // (zeroes the IntegrateArgs part; f is not read)
    ground_io(a.g, s, normals, height, mu, f_gr, contact, gap);
    stick_io(a.s, s, anchor, stick);
    return k_stick_integrate<T>(L, dev_model<T>(s), a);
  });
}

// ---- contact sensing from the observer's residual: the thresholds, the law alone, the law + the gait scheduler as one launch
extern "C" void wbc_contact_params_default(wbc_contact_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->f_on = 15.0; p->f_off = 5.0; p->det_min = 1.5e-3;   // how they were fixed: include/wbc_hip.h
}

extern "C" int wbc_solver_set_contact_params(wbc_solver* s, const wbc_contact_params* p) {
  if (!s || !p) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = check_struct_size(p, "wbc_contact_params: struct_size too small (call wbc_contact_params_default first)")) return rc;
  if (const int rc = check_finite_nonneg({p->f_on, p->f_off, p->det_min}, "wbc_contact_params: f_on, f_off, det_min must be finite and >= 0")) return rc;
  if (p->f_off > p->f_on) return fail(WBC_E_INVALID, "wbc_contact_params: f_off must not exceed f_on");
  s->contact_est = *p;
  return WBC_OK;
}

template <class T>
static void contact_io(ContactIO<T>& c, const wbc_solver* s, const void* Jc, const void* r, const void* f_prev, const void* normals, int* contact,
                       void* f_est, void* fn_est, int* singular) {
  c.Jc = (const T*)Jc; c.r = (const T*)r; c.f_prev = (const T*)f_prev; c.normals = (const T*)normals;
  c.contact = contact; c.f_est = (T*)f_est; c.fn_est = (T*)fn_est; c.singular = singular;
  c.P.f_on = (T)s->contact_est.f_on; c.P.f_off = (T)s->contact_est.f_off; c.P.det_min = (T)s->contact_est.det_min;
}

extern "C" int wbc_contact_estimate_batch(wbc_solver* s, size_t N, const void* Jc, const void* r, const void* f_prev, const void* normals, int* contact,
                                          void* f_est, void* fn_est, int* singular, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!Jc || !r || !f_prev || !normals || !contact) return fail(WBC_E_INVALID, "null argument");
  return launch_batch(s, N, stream, "contact estimate", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    ContactArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.N = N; a.jpack = s->jpack;
    contact_io(a.c, s, Jc, r, f_prev, normals, contact, f_est, fn_est, singular);
    return k_contact_estimate<T>(L, dev_model<T>(s), a);
  });
}

extern "C" int wbc_gait_estimated_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* Jc, const void* r,
                                        const void* f_prev, const void* normals, int* contact, void* phase, int* mask, void* swing, int* events,
                                        void* f_est, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !cmd || !Jc || !r || !f_prev || !normals || !contact || !phase || !mask || !swing) return fail(WBC_E_INVALID, "null argument");
  return launch_batch(s, N, stream, "gait estimated", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    GaitEstimatedArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    gait_args(a.g, s, N, q, v, cmd, nullptr, phase, mask, swing, events);
    contact_io(a.c, s, Jc, r, f_prev, normals, contact, f_est, nullptr, nullptr);
    return k_gait_estimated<T>(L, dev_model<T>(s), a);
  });
}

// ---- terrain heightfield: the struct's checks, the law at points, under the feet, and behind the two gait calls as one launch each
static int terrain_check(const wbc_terrain* t) {
  if (t->struct_size != sizeof(wbc_terrain)) return fail(WBC_E_INVALID, "wbc_terrain: wrong struct_size");
  if (t->nx < 2 || t->ny < 2) return fail(WBC_E_INVALID, "wbc_terrain: nx and ny must be >= 2");
  if (t->n_tiles < 1) return fail(WBC_E_INVALID, "wbc_terrain: n_tiles must be >= 1");
  if (!std::isfinite(t->x0) || !std::isfinite(t->y0)) return fail(WBC_E_INVALID, "wbc_terrain: x0 and y0 must be finite");
  if (!(t->cell > 0) || !std::isfinite(t->cell)) return fail(WBC_E_INVALID, "wbc_terrain: cell must be finite and > 0");
  if (!t->z) return fail(WBC_E_INVALID, "wbc_terrain: z is null");
  if ((unsigned long long)t->n_tiles * (unsigned long long)t->ny * (unsigned long long)t->nx >= (1ull << 28))
    return fail(WBC_E_INVALID, "wbc_terrain: n_tiles * ny * nx must stay below 2^28 nodes");
  return WBC_OK;
}

// (behind terrain_check)
template <class T>
static void terrain_dev(DevTerrain<T>& g, const wbc_terrain* t) {
  g.z = (const T*)t->z; g.tile = t->tile; g.nx = t->nx; g.ny = t->ny; g.tile_nodes = (unsigned)t->ny * (unsigned)t->nx;
  g.x0 = (T)t->x0; g.y0 = (T)t->y0; g.inv_cell = (T)(1.0 / t->cell);
  g.x_max = (T)(t->x0 + (t->nx - 1) * t->cell); g.y_max = (T)(t->y0 + (t->ny - 1) * t->cell);
}
template <class T>
static void terrain_out(TerrainOut<T>& o, const wbc_terrain* t, void* normals, void* height, void* surf) {
  o.normals = (T*)normals; o.height = (T*)height; o.surf = (T*)surf;
  terrain_dev(o.g, t);
}

extern "C" int wbc_terrain_sample_batch(wbc_solver* s, const wbc_terrain* terrain, size_t M, const void* xy, void* z, void* n, void* d, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (M == 0) return WBC_OK;
  if (!terrain || !xy) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = terrain_check(terrain)) return rc;
  return launch_batch(s, M, stream, "terrain sample", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    TerrainSampleArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.M = M; a.xy = (const T*)xy; a.z = (T*)z; a.n = (T*)n; a.d = (T*)d;
    terrain_dev(a.g, terrain);
    return k_terrain_sample<T>(L, a);
  });
}

extern "C" int wbc_terrain_feet_batch(wbc_solver* s, const wbc_terrain* terrain, size_t N, const void* q, const int* mask, void* swing, void* normals,
                                      void* height, void* surf, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!terrain || !q || !normals || !height) return fail(WBC_E_INVALID, "null argument");
  if ((mask == nullptr) != (swing == nullptr)) return fail(WBC_E_INVALID, "mask and swing are given both or neither");
  if (const int rc = terrain_check(terrain)) return rc;
  return launch_batch(s, N, stream, "terrain feet", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    TerrainFeetArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.N = N; a.q = (const T*)q; a.mask = mask; a.swing = (T*)swing; a.jpack = s->jpack;
    terrain_out(a.t, terrain, normals, height, surf);
    return k_terrain_feet<T>(L, dev_model<T>(s), a);
  });
}

extern "C" int wbc_gait_terrain_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const int* contact, void* phase, int* mask,
                                      void* swing, int* events, const wbc_terrain* terrain, void* normals, void* height, void* surf, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !cmd || !phase || !mask || !swing || !terrain || !normals || !height) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = terrain_check(terrain)) return rc;
  return launch_batch(s, N, stream, "gait terrain", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    GaitTerrainArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    gait_args(a.g, s, N, q, v, cmd, contact, phase, mask, swing, events);
    terrain_out(a.t, terrain, normals, height, surf);
    return k_gait_terrain<T>(L, dev_model<T>(s), a);
  });
}

extern "C" int wbc_gait_estimated_terrain_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* Jc, const void* r,
                                                const void* f_prev, void* normals, int* contact, void* phase, int* mask, void* swing, int* events,
                                                void* f_est, const wbc_terrain* terrain, void* height, void* surf, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !cmd || !Jc || !r || !f_prev || !normals || !contact || !phase || !mask || !swing || !terrain || !height)
    return fail(WBC_E_INVALID, "null argument");
  if (const int rc = terrain_check(terrain)) return rc;
  return launch_batch(s, N, stream, "gait estimated terrain", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    GaitEstimatedTerrainArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    gait_args(a.e.g, s, N, q, v, cmd, nullptr, phase, mask, swing, events);
    contact_io(a.e.c, s, Jc, r, f_prev, normals, contact, f_est, nullptr, nullptr);
    terrain_out(a.t, terrain, normals, height, surf);
    return k_gait_estimated_terrain<T>(L, dev_model<T>(s), a);
  });
}

// ---- foothold selection: the weights, the cost map of a terrain, the law alone, and behind the two fused terrain calls as one launch each
extern "C" void wbc_foothold_params_default(wbc_foothold_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->radius = 3; p->margin = 1;
  p->w_step = 1.0; p->w_slope = 0.0078125; p->w_dist = 4.0; p->cost_ok = 0.00875; p->u_max = 0.75;   // how they were fixed: include/wbc_hip.h
}

extern "C" int wbc_solver_set_foothold_params(wbc_solver* s, const wbc_foothold_params* p) {
  if (!s || !p) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = check_struct_size(p, "wbc_foothold_params: struct_size too small (call wbc_foothold_params_default first)")) return rc;
  if (p->radius < 0 || p->radius > 4) return fail(WBC_E_INVALID, "wbc_foothold_params: 0 <= radius <= 4");
  if (p->margin < 0 || p->margin > 2) return fail(WBC_E_INVALID, "wbc_foothold_params: 0 <= margin <= 2");
  if (const int rc = check_finite_nonneg({p->w_step, p->w_slope, p->w_dist, p->cost_ok, p->u_max},
                                         "wbc_foothold_params: w_step, w_slope, w_dist, cost_ok, u_max must be finite and >= 0")) return rc;
  if (p->u_max > 1) return fail(WBC_E_INVALID, "wbc_foothold_params: 0 <= u_max <= 1");
  s->foothold = *p;
  return WBC_OK;
}

template <class T>
static void foothold_params(DevFootholdParams<T>& P, const wbc_solver* s) {
  const wbc_foothold_params& f = s->foothold;
  P.w_step = (T)f.w_step; P.w_slope = (T)f.w_slope; P.w_dist = (T)f.w_dist; P.cost_ok = (T)f.cost_ok; P.u_max = (T)f.u_max;
  P.radius = f.radius; P.margin = f.margin;
}
// (behind terrain_check)
template <class T>
static void foothold_io(FootholdIO<T>& f, const wbc_solver* s, const wbc_terrain* t, const void* cost, void* hold, int* latch) {
  f.cost = (const T*)cost; f.hold = (T*)hold; f.latch = latch; f.cell = (T)t->cell;
  foothold_params(f.P, s);
}

extern "C" int wbc_terrain_cost_batch(wbc_solver* s, const wbc_terrain* terrain, void* cost, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (!terrain || !cost) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = terrain_check(terrain)) return rc;
  return launch_batch(s, 0, stream, "terrain cost", [&](auto scalar, const LaunchCtx& L) {   // (no batch: nothing to hold against max_batch)
    using T = decltype(scalar);
    TerrainCostArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    terrain_dev(a.g, terrain);
    a.cost = (T*)cost;
    a.nbx = ((unsigned)terrain->nx + 31u) / 32u; a.nby = ((unsigned)terrain->ny + 7u) / 8u;   // COST_TX, COST_TY of foothold.hip.hpp
    foothold_params(a.P, s);
    return k_terrain_cost<T>(L, a, (unsigned)terrain->n_tiles);
  });
}

extern "C" int wbc_foothold_select_batch(wbc_solver* s, const wbc_terrain* terrain, const void* cost, size_t N, const int* mask, void* swing, void* hold,
                                         int* latch, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!terrain || !cost || !mask || !swing || !hold || !latch) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = terrain_check(terrain)) return rc;
  return launch_batch(s, N, stream, "foothold select", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    FootholdSelectArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.N = N; a.mask = mask; a.swing = (T*)swing;
    terrain_dev(a.g, terrain);
    foothold_io(a.f, s, terrain, cost, hold, latch);
    return k_foothold_select<T>(L, a);
  });
}

extern "C" int wbc_gait_terrain_select_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const int* contact, void* phase,
                                             int* mask, void* swing, int* events, const wbc_terrain* terrain, void* normals, void* height, void* surf,
                                             const void* cost, void* hold, int* latch, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !cmd || !phase || !mask || !swing || !terrain || !normals || !height || !cost || !hold || !latch)
    return fail(WBC_E_INVALID, "null argument");
  if (const int rc = terrain_check(terrain)) return rc;
  return launch_batch(s, N, stream, "gait terrain select", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    GaitTerrainSelectArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    gait_args(a.g, s, N, q, v, cmd, contact, phase, mask, swing, events);
    terrain_out(a.t, terrain, normals, height, surf);
    foothold_io(a.f, s, terrain, cost, hold, latch);
    return k_gait_terrain_select<T>(L, dev_model<T>(s), a);
  });
}

extern "C" int wbc_gait_estimated_terrain_select_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* Jc,
                                                       const void* r, const void* f_prev, void* normals, int* contact, void* phase, int* mask,
                                                       void* swing, int* events, void* f_est, const wbc_terrain* terrain, void* height, void* surf,
                                                       const void* cost, void* hold, int* latch, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !cmd || !Jc || !r || !f_prev || !normals || !contact || !phase || !mask || !swing || !terrain || !height || !cost || !hold || !latch)
    return fail(WBC_E_INVALID, "null argument");
  if (const int rc = terrain_check(terrain)) return rc;
  return launch_batch(s, N, stream, "gait estimated terrain select", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    GaitEstimatedTerrainSelectArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    gait_args(a.e.g, s, N, q, v, cmd, nullptr, phase, mask, swing, events);
    contact_io(a.e.c, s, Jc, r, f_prev, normals, contact, f_est, nullptr, nullptr);
    terrain_out(a.t, terrain, normals, height, surf);
    foothold_io(a.f, s, terrain, cost, hold, latch);
    return k_gait_estimated_terrain_select<T>(L, dev_model<T>(s), a);
  });
}

// ---- base state from leg odometry: the gains, the law alone, the law + the contact estimate + the gait scheduler as one launch
extern "C" void wbc_odom_params_default(wbc_odom_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->a_v = 0.125; p->a_p = 0.25;   // how they were fixed: include/wbc_hip.h
}

extern "C" int wbc_solver_set_odom_params(wbc_solver* s, const wbc_odom_params* p) {
  if (!s || !p) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = check_struct_size(p, "wbc_odom_params: struct_size too small (call wbc_odom_params_default first)")) return rc;
  if (!(p->a_v > 0 && p->a_v <= 1)) return fail(WBC_E_INVALID, "wbc_odom_params: 0 < a_v <= 1");
  if (!(p->a_p >= 0 && p->a_p <= 1)) return fail(WBC_E_INVALID, "wbc_odom_params: 0 <= a_p <= 1");
  s->odom = *p;
  return WBC_OK;
}

template <class T>
static void odom_io(OdomIO<T>& o, const wbc_solver* s, const int* contact, const int* mask, const void* normals, const void* height, void* base,
                    void* anchor, int* odo, void* q_est, void* v_est) {
  o.contact = contact; o.mask = mask; o.normals = (const T*)normals; o.height = (const T*)height;
  o.base = (T*)base; o.anchor = (T*)anchor; o.odo = odo; o.q_est = (T*)q_est; o.v_est = (T*)v_est;
  o.a_v = (T)s->odom.a_v; o.a_p = (T)s->odom.a_p; o.dt = (T)s->params.dt;
}

extern "C" int wbc_base_estimate_batch(wbc_solver* s, size_t N, const void* q, const void* v, const int* contact, const int* mask, const void* normals,
                                       const void* height, void* base, void* anchor, int* odo, void* q_est, void* v_est, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !contact || !mask || !base || !anchor || !odo || !q_est || !v_est) return fail(WBC_E_INVALID, "null argument");
  if ((normals == nullptr) != (height == nullptr)) return fail(WBC_E_INVALID, "normals and height are given together or both NULL");
  return launch_batch(s, N, stream, "base estimate", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    OdomArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.N = N; a.q = (const T*)q; a.v = (const T*)v; a.jpack = s->jpack;
    odom_io(a.o, s, contact, mask, normals, height, base, anchor, odo, q_est, v_est);
    return k_base_estimate<T>(L, dev_model<T>(s), a);
  });
}

extern "C" int wbc_gait_estimated_odom_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* Jc, const void* r,
                                             const void* f_prev, const void* normals, int* contact, void* phase, int* mask, void* swing, int* events,
                                             void* f_est, const void* height, void* base, void* anchor, int* odo, void* q_est, void* v_est,
                                             void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !cmd || !Jc || !r || !f_prev || !normals || !contact || !phase || !mask || !swing || !base || !anchor || !odo || !q_est || !v_est)
    return fail(WBC_E_INVALID, "null argument");
  return launch_batch(s, N, stream, "gait estimated odom", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    GaitEstimatedOdomArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    gait_args(a.e.g, s, N, q, v, cmd, nullptr, phase, mask, swing, events);
    contact_io(a.e.c, s, Jc, r, f_prev, normals, contact, f_est, nullptr, nullptr);
    odom_io(a.o, s, contact, mask, normals, height, base, anchor, odo, q_est, v_est);
    return k_gait_estimated_odom<T>(L, dev_model<T>(s), a);
  });
}

// ---- trunk reference from the velocity command: the parameters, the argument builder, the reference call and the call with the swing law fused in
extern "C" void wbc_trunk_params_default(wbc_trunk_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->height = 0.4; p->leash = 0.05; p->yaw_leash = 0.5; p->a_s = 0.03125; p->tilt = 1.0; p->nz_min = 0.5; p->det_min = 1e-6;   // how they were fixed: include/wbc_hip.h
}

extern "C" int wbc_solver_set_trunk_params(wbc_solver* s, const wbc_trunk_params* p) {
  if (!s || !p) return fail(WBC_E_INVALID, "null argument");
  if (const int rc = check_struct_size(p, "wbc_trunk_params: struct_size too small (call wbc_trunk_params_default first)")) return rc;
  if (!std::isfinite(p->height)) return fail(WBC_E_INVALID, "wbc_trunk_params: height must be finite");
  if (!(p->leash > 0)) return fail(WBC_E_INVALID, "wbc_trunk_params: leash must be > 0 (+inf allowed)");
  if (!(p->yaw_leash > 0 && p->yaw_leash <= 3.14159265358979323846)) return fail(WBC_E_INVALID, "wbc_trunk_params: 0 < yaw_leash <= pi");
  if (!(p->a_s >= 0 && p->a_s <= 1)) return fail(WBC_E_INVALID, "wbc_trunk_params: 0 <= a_s <= 1");
  if (!(p->tilt >= 0 && p->tilt <= 1)) return fail(WBC_E_INVALID, "wbc_trunk_params: 0 <= tilt <= 1");
  if (!(p->nz_min > 0 && p->nz_min <= 1)) return fail(WBC_E_INVALID, "wbc_trunk_params: 0 < nz_min <= 1");
  if (!(p->det_min > 0) || !std::isfinite(p->det_min)) return fail(WBC_E_INVALID, "wbc_trunk_params: det_min must be finite and > 0");
  // the kernels hold the values in the solver's scalar type: the bounds must survive the rounding (an fp32 solver: nz_min = 1e-300 would become 0, a
  // plane with n_z = 0 would pass, and its division would put NaN into trunk).  Behind the range checks: those never read the solver
  if (s->dtype == WBC_F32) {
    if (!((float)p->leash > 0)) return fail(WBC_E_INVALID, "wbc_trunk_params: leash rounds to 0 in the solver's scalar type");
    if (!((float)p->nz_min > 0)) return fail(WBC_E_INVALID, "wbc_trunk_params: nz_min rounds to 0 in the solver's scalar type");
    if (!((float)p->det_min > 0) || !std::isfinite((float)p->det_min))
      return fail(WBC_E_INVALID, "wbc_trunk_params: det_min rounds to 0 or overflows in the solver's scalar type");
    if (!std::isfinite((float)p->height)) return fail(WBC_E_INVALID, "wbc_trunk_params: height overflows in the solver's scalar type");
  }
  s->trunk = *p;
  return WBC_OK;
}

template <class T>
static void cmd_ref_args(CmdRefArgs<T>& a, const wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* normals,
                         const void* height, const int* reset, void* trunk, void* w_des, void* vdot_des, void* com, void* ref) {
  std::memset(&a, 0, sizeof(a));
  a.N = N; a.q = (const T*)q; a.v = (const T*)v; a.cmd = (const T*)cmd; a.normals = (const T*)normals; a.height = (const T*)height;
  a.reset = reset; a.trunk = (T*)trunk; a.w_des = (T*)w_des; a.vdot_des = (T*)vdot_des; a.com = (T*)com; a.ref = (T*)ref;
  a.jpack = s->jpack;
  const wbc_trunk_params& t = s->trunk;
  const double pi = 3.14159265358979323846;
  a.P.height = (T)t.height; a.P.leash = (T)t.leash; a.P.a_s = (T)t.a_s; a.P.tilt = (T)t.tilt; a.P.nz_min = (T)t.nz_min; a.P.det_min = (T)t.det_min;
  a.P.dt = (T)s->params.dt; a.P.pi = (T)pi; a.P.two_pi = (T)(2.0 * pi); a.P.cos_yl = (T)std::cos(t.yaw_leash);
}

extern "C" int wbc_reference_cmd_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* normals, const void* height,
                                       const int* reset, void* trunk, void* w_des, void* vdot_des, void* com, void* ref, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !cmd || !normals || !height || !trunk || !w_des || !vdot_des) return fail(WBC_E_INVALID, "null argument");
  if (N > s->max_batch) return fail(WBC_E_CAPACITY, "N exceeds the solver's max_batch");
  if (!s->d_ref) return fail(WBC_E_INVALID, "call wbc_solver_set_ref_params first");
  return launch_batch(s, N, stream, "reference cmd", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    CmdRefArgs<T> a;
    cmd_ref_args(a, s, N, q, v, cmd, normals, height, reset, trunk, w_des, vdot_des, com, ref);
    return k_reference_cmd<T>(L, dev_model<T>(s), (const DevRefParams<T>*)s->d_ref, a);
  });
}

extern "C" int wbc_reference_cmd_swing_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* normals,
                                             const void* height, const int* reset, void* trunk, const int* mask, const void* swing, void* w_des,
                                             void* vdot_des, void* com, void* ref, void* foot, void* stream) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (N == 0) return WBC_OK;
  if (!q || !v || !cmd || !normals || !height || !trunk || !mask || !swing || !w_des || !vdot_des) return fail(WBC_E_INVALID, "null argument");
  if (N > s->max_batch) return fail(WBC_E_CAPACITY, "N exceeds the solver's max_batch");
  if (!s->d_ref) return fail(WBC_E_INVALID, "call wbc_solver_set_ref_params first");
  return launch_batch(s, N, stream, "reference cmd + swing", [&](auto scalar, const LaunchCtx& L) {
    using T = decltype(scalar);
    CmdRefArgs<T> a;
    cmd_ref_args(a, s, N, q, v, cmd, normals, height, reset, trunk, w_des, vdot_des, com, ref);
    SwingArgs<T> sa;
    swing_args(sa, s, mask, swing, foot);
    return k_reference_cmd_swing<T>(L, dev_model<T>(s), (const DevRefParams<T>*)s->d_ref, a, sa);
  });
}
