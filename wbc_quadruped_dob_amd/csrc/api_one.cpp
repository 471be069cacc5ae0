// C-ABI (include/wbc_hip.h): the single-robot calls.  The tick and its start-up / planner helpers run on the solver's pinned image (their latency is
// measured: wbc_solver_options.one_zerocopy); the fp64 helpers of the walking tick go through one device staging block with pageable copies.
#include <chrono>

#include "solver.hpp"

using namespace wbc;

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield");
#endif
}

// ---- single-robot tick on the solver's pinned image.  Layout (scalars of the solver's dtype, then ints):
static const int ONE_OFF[] = {0, 19, 37, 43, 61, 73, 77, 89, 101, 119, 137, 149, 161};  // q v w a n mu tp fp ig r tau f end
// ints behind the 200 scalars: [0] mask, [1] status, [2] iters, [3] completion ticket (one_zerocopy >= 2)

// n scalars of the image from / to the caller's doubles, in the solver's scalar type (src null: zeros; dst null: skipped)
static void image_put(wbc_solver* s, int o, const double* src, int n) {
  for (int i = 0; i < n; ++i) {
    if (s->dtype == WBC_F64) ((double*)s->h_one)[o + i] = src ? src[i] : 0.0;
    else ((float*)s->h_one)[o + i] = src ? (float)src[i] : 0.0f;
  }
}
static void image_get(const wbc_solver* s, int o, double* dst, int n) {
  if (!dst) return;
  for (int i = 0; i < n; ++i) dst[i] = s->dtype == WBC_F64 ? ((const double*)s->h_one)[o + i] : (double)((const float*)s->h_one)[o + i];
}

// Runs wbc_step_batch(N = 1) on the image and returns when tau, f, status (and the observer state) are in the HOST image.
//   one_zerocopy = 0: copy the image to the device scratch, tick, copy back, hipStreamSynchronize
//   one_zerocopy = 1: the kernels read / write the pinned image directly (mapped host memory), hipStreamSynchronize
//   one_zerocopy = 2: as 1, but completion is a 32-bit ticket that the STREAM writes into the image behind the tick
//                     (hipStreamWriteValue32) and the host polls in memory -- no runtime call on the wait path
//   one_zerocopy = 3: as 2 with a one-thread kernel writing the ticket (for stacks that refuse the stream write)
static int one_tick_on_image(wbc_solver* s) {
  const size_t ts = s->dtype == WBC_F64 ? 8 : 4;
  const int* off = ONE_OFF;
  unsigned char* hb = (unsigned char*)s->h_one;
  const int zcm = s->opt.one_zerocopy;
  const bool zc = zcm != 0;
  unsigned char* d = (unsigned char*)(zc ? s->h_one_dev : s->d_one);
  int* dints = (int*)(d + ONE_SCALARS * sizeof(double));
  int* hints = (int*)(hb + ONE_SCALARS * sizeof(double));
  if (!zc) HIP_TRY(hipMemcpyAsync(d, hb, s->one_bytes, hipMemcpyHostToDevice, nullptr));
  wbc_batch_in in;
  in.q = d + off[0] * ts; in.v = d + off[1] * ts; in.w_des = d + off[2] * ts; in.vdot_des = d + off[3] * ts;
  in.normals = d + off[4] * ts; in.mu = d + off[5] * ts; in.mask = dints;
  in.tau_prev = d + off[6] * ts; in.f_prev = d + off[7] * ts;
  wbc_batch_out out;
  std::memset(&out, 0, sizeof(out));
  out.tau = d + off[10] * ts; out.f = d + off[11] * ts; out.status = dints + 1; out.iters = dints + 2;
  wbc_observer_state os{d + off[8] * ts, d + off[9] * ts};
  int rc = wbc_step_batch(s, 1, &in, &out, &os, nullptr);
  if (rc) return rc;
  if (!zc) HIP_TRY(hipMemcpyAsync(hb, d, s->one_bytes, hipMemcpyDeviceToHost, nullptr));
  if (zcm >= 2 && s->one_flag_ok) {
    unsigned ticket = ++s->one_seq;
    if (ticket == 0) ticket = ++s->one_seq;                       // (0 is the "not yet" value below)
    __atomic_store_n((unsigned*)(hints + 3), 0u, __ATOMIC_RELEASE);   // before the launch: a match can only come from THIS tick's write
    hipError_t e = zcm == 2 ? hipStreamWriteValue32(nullptr, dints + 3, ticket, 0) : k_flag(nullptr, (unsigned*)(dints + 3), ticket);
    if (e == hipSuccess) {
      // stream order puts the ticket behind the tick's kernels, whose writes to the (fine-grained) image are released at
      // their end: ticket visible => outputs visible.  Bounded spin, then the runtime's wait (a stalled device must not hang us).
      const unsigned* flag = (const unsigned*)(hints + 3);
      const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(5);   // a healthy tick takes ~15 us
      for (;;) {
        for (int spin = 0; spin < 256; ++spin) {
          if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == ticket) return WBC_OK;
          cpu_relax();
        }
        if (std::chrono::steady_clock::now() > t_end) break;
      }
    } else {
      (void)hipGetLastError();
      s->one_flag_ok = false;   // refused on this stack: the plain wait from now on
    }
  }
  HIP_TRY(hipStreamSynchronize(nullptr));
  return WBC_OK;
}

extern "C" int wbc_compute_torques(wbc_solver* s, const double* q, const double* v, const double* w_des,
                                   const double* vdot_des, const double* normals, const double* mu, int mask,
                                   const double* tau_prev, const double* f_prev, double* obs_integ, double* obs_r,
                                   double* tau, double* f, int* status) {
  if (!s || !q || !v || !w_des || !vdot_des || !normals || !mu || !tau || !f || !status)
    return fail(WBC_E_INVALID, "null argument");
  const bool ob = s->params.observer_order > 0;
  if (ob && (!tau_prev || !f_prev || !obs_integ || !obs_r)) return fail(WBC_E_INVALID, "observer on: state required");
  ON_DEVICE(s);
  // host staging in the solver's dtype: a pinned image of the device scratch (doubles/floats, then mask | status | iters),
  // one asynchronous copy each way around the launch and one synchronisation (was four blocking copies from pageable memory)
  const int* off = ONE_OFF;
  int* hints = (int*)((unsigned char*)s->h_one + ONE_SCALARS * sizeof(double));
  image_put(s, off[0], q, 19); image_put(s, off[1], v, 18); image_put(s, off[2], w_des, 6); image_put(s, off[3], vdot_des, 18); image_put(s, off[4], normals, 12);
  image_put(s, off[5], mu, 4); image_put(s, off[6], tau_prev, 12); image_put(s, off[7], f_prev, 12); image_put(s, off[8], obs_integ, 18); image_put(s, off[9], obs_r, 18);
  image_put(s, off[10], nullptr, 12); image_put(s, off[11], nullptr, 12);
  hints[0] = mask; hints[1] = 0; hints[2] = 0;
  int rc = one_tick_on_image(s);
  if (rc) return rc;
  image_get(s, off[10], tau, 12); image_get(s, off[11], f, 12);
  if (ob) { image_get(s, off[8], obs_integ, 18); image_get(s, off[9], obs_r, 18); }
  *status = hints[1];
  return WBC_OK;
}

// The single-robot loop WITHOUT staging copies: the caller keeps its state in the solver's pinned image and rewrites only
// what changed between ticks (fp64 solvers: the image's scalars are doubles).
extern "C" int wbc_one_map(wbc_solver* s, wbc_one_image* img) {
  if (!s || !img) return fail(WBC_E_INVALID, "null argument");
  if (s->dtype != WBC_F64) return fail(WBC_E_INVALID, "wbc_one_map: fp64 solvers only (the image holds the solver's scalar type)");
  double* hb = (double*)s->h_one;
  int* hints = (int*)((unsigned char*)s->h_one + ONE_SCALARS * sizeof(double));
  const int* off = ONE_OFF;
  img->q = hb + off[0]; img->v = hb + off[1]; img->w_des = hb + off[2]; img->vdot_des = hb + off[3]; img->normals = hb + off[4];
  img->mu = hb + off[5]; img->tau_prev = hb + off[6]; img->f_prev = hb + off[7]; img->obs_integ = hb + off[8]; img->obs_r = hb + off[9];
  img->tau = hb + off[10]; img->f = hb + off[11];
  img->mask = hints; img->status = hints + 1; img->iters = hints + 2;
  return WBC_OK;
}

extern "C" int wbc_one_tick(wbc_solver* s) {
  if (!s) return fail(WBC_E_INVALID, "null solver");
  if (s->dtype != WBC_F64) return fail(WBC_E_INVALID, "wbc_one_tick: fp64 solvers only");
  ON_DEVICE(s);
  return one_tick_on_image(s);
}

// Observer start-up for the single-robot host-pointer loop: integ(0) = p(0) = M(q) v, r(0) = 0 (see wbc_observer_state).
extern "C" int wbc_observer_init(wbc_solver* s, const double* q, const double* v, double* obs_integ, double* obs_r) {
  if (!s || !q || !v || !obs_integ || !obs_r) return fail(WBC_E_INVALID, "null argument");
  ON_DEVICE(s);
  const size_t ts = s->dtype == WBC_F64 ? 8 : 4;
  const int o = ONE_SCRATCH;   // scratch region of the pinned image (q at +0, v at +19, p = M v at +37): the tick's part stays as the caller left it
  unsigned char* hb = (unsigned char*)s->h_one;
  image_put(s, o, q, 19); image_put(s, o + 19, v, 18);
  unsigned char* d = (unsigned char*)s->d_one;
  HIP_TRY(hipMemcpyAsync(d + o * ts, hb + o * ts, 37 * ts, hipMemcpyHostToDevice, nullptr));
  const unsigned long long calls0 = s->calls;   // start-up helper, not a tick: the every-k-th-tick sampling phase stays as it is
  const bool timing0 = s->timing;
  s->timing = false;
  int rc = wbc_dynamics_batch(s, 1, d + o * ts, d + (o + 19) * ts, nullptr, nullptr, nullptr, nullptr, d + (o + 37) * ts, nullptr, nullptr);
  s->timing = timing0; s->calls = calls0;
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(hb + (o + 37) * ts, d + (o + 37) * ts, 18 * ts, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  image_get(s, o + 37, obs_integ, 18);
  for (int i = 0; i < 18; ++i) obs_r[i] = 0.0;
  return WBC_OK;
}

extern "C" int wbc_compute_reference(wbc_solver* s, const double* q, const double* v, const double* plan, double t,
                                     double* w_des, double* vdot_des, double* com) {
  if (!s || !q || !v || !plan || !w_des || !vdot_des) return fail(WBC_E_INVALID, "null argument");
  if (!s->d_ref) return fail(WBC_E_INVALID, "call wbc_solver_set_ref_params first");
  ON_DEVICE(s);
  const size_t ts = s->dtype == WBC_F64 ? 8 : 4;
  const int o0 = ONE_SCRATCH;   // scratch region of the pinned image: the tick's part stays as the caller left it
  const int off[] = {o0 + 0, o0 + 19, o0 + 37, o0 + 49, o0 + 55, o0 + 73, o0 + 79};  // q v plan | w_des vdot_des com end
  unsigned char* hb = (unsigned char*)s->h_one;   // pinned staging, one copy each way
  image_put(s, off[0], q, 19); image_put(s, off[1], v, 18); image_put(s, off[2], plan, PLAN_WORDS);
  unsigned char* d = (unsigned char*)s->d_one;
  HIP_TRY(hipMemcpyAsync(d + o0 * ts, hb + o0 * ts, 49 * ts, hipMemcpyHostToDevice, nullptr));
  int rc = wbc_reference_batch(s, 1, d + off[0] * ts, d + off[1] * ts, d + off[2] * ts, t, d + off[3] * ts, d + off[4] * ts,
                               d + off[5] * ts, nullptr);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(hb + (o0 + 49) * ts, d + (o0 + 49) * ts, 30 * ts, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  image_get(s, off[3], w_des, 6); image_get(s, off[4], vdot_des, 18); image_get(s, off[5], com, 6);
  return WBC_OK;
}

// ---- the fp64 single-robot forms of the walking tick's batch calls: staged through the solver's own device block (the pinned image's scratch region is
// too small for the 36 plan words), pageable copies on the null stream.  One call: the first n_up doubles of h and the n_int ints of hi go up,
// call(d, di) runs the batch call with N = 1 on the block's doubles d and ints di, the doubles [back0, back0 + n_back) and the first n_int_back ints come back.
template <class F>
static int stage_one(wbc_solver* s, double* h, int n_up, int* hi, int n_int, int back0, int n_back, int n_int_back, F&& call) {
  double* d = (double*)s->d_stage_one;
  int* di = (int*)(d + STAGE_ONE_DOUBLES);
  HIP_TRY(hipMemcpy(d, h, n_up * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(di, hi, n_int * sizeof(int), hipMemcpyHostToDevice));
  if (const int rc = call(d, di)) return rc;
  HIP_TRY(hipMemcpy(h + back0, d + back0, n_back * sizeof(double), hipMemcpyDeviceToHost));
  if (n_int_back) HIP_TRY(hipMemcpy(hi, di, n_int_back * sizeof(int), hipMemcpyDeviceToHost));
  return WBC_OK;
}

extern "C" int wbc_compute_swing_reference(wbc_solver* s, const double* q, const double* v, int mask, const double* swing, double t, double* vdot_des,
                                           double* foot) {
  if (!s || !q || !v || !swing || !vdot_des) return fail(WBC_E_INVALID, "null argument");
  if (s->dtype != WBC_F64) return fail(WBC_E_INVALID, "wbc_compute_swing_reference: fp64 solvers only");
  ON_DEVICE(s);
  const int oq = 0, ov = 19, os = 37, oa = 73, of = 91;   // q v swing | vdot_des | foot, and one int: the mask
  double h[of + FOOT_WORDS];
  std::memcpy(h + oq, q, 19 * sizeof(double)); std::memcpy(h + ov, v, 18 * sizeof(double));
  std::memcpy(h + os, swing, SWING_WORDS * sizeof(double)); std::memcpy(h + oa, vdot_des, 18 * sizeof(double));
  const int rc = stage_one(s, h, of, &mask, 1, oa, 18 + FOOT_WORDS, 0, [&](double* d, int* di) {
    return wbc_swing_reference_batch(s, 1, d + oq, d + ov, di, d + os, t, d + oa, d + of, nullptr);
  });
  if (rc) return rc;
  std::memcpy(vdot_des, h + oa, 18 * sizeof(double));
  if (foot) std::memcpy(foot, h + of, FOOT_WORDS * sizeof(double));
  return WBC_OK;
}

extern "C" int wbc_compute_gait(wbc_solver* s, const double* q, const double* v, const double* cmd, int contact, double* phase, int* mask, double* swing,
                                int* events) {
  if (!s || !q || !v || !cmd || !phase || !mask || !swing) return fail(WBC_E_INVALID, "null argument");
  if (s->dtype != WBC_F64) return fail(WBC_E_INVALID, "wbc_compute_gait: fp64 solvers only");
  ON_DEVICE(s);
  const int oq = 0, ov = 19, oc = 37, op = 41, os = 42;   // q v cmd | phase swing, and three ints: contact, mask, events
  double h[os + SWING_WORDS];
  std::memcpy(h + oq, q, 19 * sizeof(double)); std::memcpy(h + ov, v, 18 * sizeof(double)); std::memcpy(h + oc, cmd, 4 * sizeof(double));
  h[op] = *phase; std::memcpy(h + os, swing, SWING_WORDS * sizeof(double));
  int hi[3] = {contact, *mask, 0};
  const int rc = stage_one(s, h, os + SWING_WORDS, hi, 3, op, 1 + SWING_WORDS, 3, [&](double* d, int* di) {
    return wbc_gait_batch(s, 1, d + oq, d + ov, d + oc, di, d + op, di + 1, d + os, di + 2, nullptr);
  });
  if (rc) return rc;
  *phase = h[op]; std::memcpy(swing, h + os, SWING_WORDS * sizeof(double));
  *mask = hi[1];
  if (events) *events = hi[2];
  return WBC_OK;
}

extern "C" int wbc_compute_contact_estimate(wbc_solver* s, const double* Jc, const double* r, const double* f_prev, const double* normals, int* contact,
                                            double* f_est, double* fn_est, int* singular) {
  if (!s || !Jc || !r || !f_prev || !normals || !contact) return fail(WBC_E_INVALID, "null argument");
  if (s->dtype != WBC_F64) return fail(WBC_E_INVALID, "wbc_compute_contact_estimate: fp64 solvers only");
  ON_DEVICE(s);
  const int oj = 0, orr = 216, ofp = 234, on = 246, ofe = 258, ofn = 270;   // Jc r f_prev normals | f_est fn_est, and two ints: contact, singular
  double h[STAGE_ONE_DOUBLES];
  static_assert(ofn + 4 == STAGE_ONE_DOUBLES, "the staging block is sized for this call");
  std::memcpy(h + oj, Jc, 216 * sizeof(double)); std::memcpy(h + orr, r, 18 * sizeof(double));
  std::memcpy(h + ofp, f_prev, 12 * sizeof(double)); std::memcpy(h + on, normals, 12 * sizeof(double));
  int hi[2] = {*contact, 0};
  const int rc = stage_one(s, h, ofe, hi, 2, ofe, 16, 2, [&](double* d, int* di) {
    return wbc_contact_estimate_batch(s, 1, d + oj, d + orr, d + ofp, d + on, di, d + ofe, d + ofn, di + 1, nullptr);
  });
  if (rc) return rc;
  *contact = hi[0];
  if (f_est) std::memcpy(f_est, h + ofe, 12 * sizeof(double));
  if (fn_est) std::memcpy(fn_est, h + ofn, 4 * sizeof(double));
  if (singular) *singular = hi[1];
  return WBC_OK;
}

extern "C" int wbc_compute_base_estimate(wbc_solver* s, const double* q, const double* v, int contact, int mask, const double* normals,
                                         const double* height, double* base, double* anchor, int* odo, double* q_est, double* v_est) {
  if (!s || !q || !v || !base || !anchor || !odo || !q_est || !v_est) return fail(WBC_E_INVALID, "null argument");
  if ((normals == nullptr) != (height == nullptr)) return fail(WBC_E_INVALID, "normals and height are given together or both NULL");
  if (s->dtype != WBC_F64) return fail(WBC_E_INVALID, "wbc_compute_base_estimate: fp64 solvers only");
  ON_DEVICE(s);
  const int oq = 0, ov = 19, on = 37, oh = 49, ob = 53, oa = 59, oqe = 71, ove = 90;   // q v normals height | base anchor q_est v_est, and three ints: contact, mask, odo
  double h[ove + 18];
  static_assert(ove + 18 <= STAGE_ONE_DOUBLES, "the staging block holds this call");
  std::memset(h, 0, sizeof(h));
  std::memcpy(h + oq, q, 19 * sizeof(double)); std::memcpy(h + ov, v, 18 * sizeof(double));
  if (normals) { std::memcpy(h + on, normals, 12 * sizeof(double)); std::memcpy(h + oh, height, 4 * sizeof(double)); }
  std::memcpy(h + ob, base, 6 * sizeof(double)); std::memcpy(h + oa, anchor, 12 * sizeof(double));
  int hi[3] = {contact, mask, *odo};
  const int rc = stage_one(s, h, oqe, hi, 3, ob, ove + 18 - ob, 3, [&](double* d, int* di) {
    return wbc_base_estimate_batch(s, 1, d + oq, d + ov, di, di + 1, normals ? d + on : nullptr, normals ? d + oh : nullptr, d + ob, d + oa, di + 2,
                                   d + oqe, d + ove, nullptr);
  });
  if (rc) return rc;
  std::memcpy(base, h + ob, 6 * sizeof(double)); std::memcpy(anchor, h + oa, 12 * sizeof(double));
  std::memcpy(q_est, h + oqe, 19 * sizeof(double)); std::memcpy(v_est, h + ove, 18 * sizeof(double));
  *odo = hi[2];
  return WBC_OK;
}

extern "C" int wbc_compute_reference_cmd(wbc_solver* s, const double* q, const double* v, const double* cmd, const double* normals, const double* height,
                                         int reset, double* trunk, double* w_des, double* vdot_des, double* com, double* ref) {
  if (!s || !q || !v || !cmd || !normals || !height || !trunk || !w_des || !vdot_des) return fail(WBC_E_INVALID, "null argument");
  if (s->dtype != WBC_F64) return fail(WBC_E_INVALID, "wbc_compute_reference_cmd: fp64 solvers only");
  ON_DEVICE(s);
  const int oq = 0, ov = 19, oc = 37, on = 41, oh = 53, ot = 57, ow = 63, oa = 69, om = 87, orf = 93;   // q v cmd normals height | trunk w_des vdot_des com ref, one int: reset
  double h[orf + TRUNKREF_WORDS];
  static_assert(orf + TRUNKREF_WORDS <= STAGE_ONE_DOUBLES, "the staging block holds this call");
  std::memset(h, 0, sizeof(h));
  std::memcpy(h + oq, q, 19 * sizeof(double)); std::memcpy(h + ov, v, 18 * sizeof(double)); std::memcpy(h + oc, cmd, 4 * sizeof(double));
  std::memcpy(h + on, normals, 12 * sizeof(double)); std::memcpy(h + oh, height, 4 * sizeof(double)); std::memcpy(h + ot, trunk, 6 * sizeof(double));
  int hi[1] = {reset};
  const int rc = stage_one(s, h, ow, hi, 1, ot, orf + TRUNKREF_WORDS - ot, 0, [&](double* d, int* di) {
    return wbc_reference_cmd_batch(s, 1, d + oq, d + ov, d + oc, d + on, d + oh, di, d + ot, d + ow, d + oa, d + om, d + orf, nullptr);
  });
  if (rc) return rc;
  std::memcpy(trunk, h + ot, 6 * sizeof(double)); std::memcpy(w_des, h + ow, 6 * sizeof(double)); std::memcpy(vdot_des, h + oa, 18 * sizeof(double));
  if (com) std::memcpy(com, h + om, 6 * sizeof(double));
  if (ref) std::memcpy(ref, h + orf, TRUNKREF_WORDS * sizeof(double));
  return WBC_OK;
}
