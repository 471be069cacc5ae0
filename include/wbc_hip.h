/* wbc_hip.h -- C-ABI of the MI355X (gfx950) batched whole-body-control hot path.
 *
 * Drop-in boundary for the per-tick computation of `dogbot_controller`
 * (reference: /root/reference/.gitmodules:4-6; the controller is started as
 * `rosrun dogbot_controller dogbot <path>/dogbot.urdf`, /root/reference/README.md:60, and
 * contains "a momentum-based observer estimator, and an optimization problem based on the
 * modulation of ground reaction forces", /root/reference/README.md:11).
 *
 * PROVISIONAL: the controller's source is an un-vendored submodule that is absent from
 * /root/reference, so the names and signatures of its compute-torques entry point and its ROS
 * message types cannot be cited.  Each entry point below states which reference
 * interface it stands for; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Rules of the ABI: extern "C"; plain pointers and sizes; no exceptions cross it; every function
 * returns an int status (WBC_OK = 0); the caller owns every batch buffer; a solver is bound to one
 * HIP device, is not thread-safe, distinct solvers are; no allocation or synchronisation happens
 * inside wbc_step_batch / wbc_dynamics_batch (they are hipGraph-capturable -- except while per-kernel
 * timing is enabled: a dispatch that carries timing events cannot be captured).  Every entry point runs
 * on its solver's device and restores the caller's current HIP device before it returns.
 *
 * Batch layout in HBM: structure-of-arrays, component-major: x[c * N + s] is component c of state s
 * (N = batch size of the call).  Scalars are double (WBC_F64) or float (WBC_F32) per the solver.
 *   q        [nq = 7+nj][N]  base position (world), base quaternion (x,y,z,w), joint angles
 *   v        [nv = 6+nj][N]  base linear velocity (world), base angular velocity (world), joint rates
 *   w_des    [6][N]          desired contact wrench on the base rows (force; moment about base origin)
 *   vdot_des [nv][N]         desired generalized acceleration
 *   normals  [3*nf][N]       terrain normal under each foot (world)
 *   mu       [nf][N]         friction coefficient under each foot
 *   mask     [N] int32       bit k set = foot k in stance
 *   tau_prev [nj][N], f_prev [3*nf][N]   previous tick's outputs (observer only)
 *   obs_integ, obs_r [nv][N] observer state, in/out (observer only)
 *   tau [nj][N], f [3*nf][N], status [N] int32 (0 ok, 1 QP iteration limit, 2 QP infeasible), iters [N] int32
 *   M [nv(nv+1)/2][N]  packed upper triangle, idx(i,j) = i*nv - i(i-1)/2 + (j-i), i <= j
 *   h [nv][N], Jc [3*nf*nv][N] (row (3k+m)*nv + c), pf [3*nf][N]
 */
#ifndef WBC_HIP_H
#define WBC_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WBC_MAXV 32 /* capacity of the per-dof gain arrays */

enum wbc_status {
  WBC_OK = 0,
  WBC_E_INVALID = 1,  /* null pointer / bad argument */
  WBC_E_IO = 2,       /* URDF file cannot be read */
  WBC_E_PARSE = 3,    /* URDF malformed or uses an unsupported element */
  WBC_E_TOPOLOGY = 4, /* not a floating base with 4 legs x 3 revolute joints + 4 feet */
  WBC_E_NODEVICE = 5, /* no HIP device / kernels for gfx950 cannot run here */
  WBC_E_HIP = 6,      /* a HIP runtime call failed (see wbc_last_error) */
  WBC_E_CAPACITY = 7  /* N exceeds the solver's max_batch */
};

enum wbc_dtype { WBC_F64 = 0, WBC_F32 = 1 };

typedef struct wbc_model wbc_model;   /* host-side flattened robot model */
typedef struct wbc_solver wbc_solver; /* device-side context */

/* Controller parameters.  In the reference these are presumably compile-time constants of the
 * controller ([UNVERIFIED]); here all are run-time. */
typedef struct wbc_params {
  double S[6];        /* wrench-tracking weights: force xyz, moment xyz */
  double alpha;       /* GRF regularisation (> 0) */
  double fn_min;      /* normal-force bounds per stance foot */
  double fn_max;
  double mu_scale;    /* 1 = pyramid with mu, 1/sqrt(2) = inscribed pyramid */
  double dt;          /* control period, s */
  int observer_order; /* 0 = off, 1, 2 */
  int max_iter;       /* QP active-set iteration cap */
  double qp_tol;      /* constraint-violation tolerance, N */
  double K1[WBC_MAXV];
  double K2[WBC_MAXV];
} wbc_params;

/* ---- model: stands for the controller's URDF ingestion (argv[1], README.md:60) ---- */
/* foot_links may be NULL: then the last link hanging off each leg's distal body is the foot. */
int wbc_model_load_urdf(const char* path, const char* const* foot_links, int n_foot_links, wbc_model** out);
int wbc_model_from_flat(int nb, const int* parent, const double* Rt, const double* rt, const double* axis,
                        const double* mass, const double* com, const double* Ic, int nf, const int* foot_body,
                        const double* foot_off, const double* gravity, wbc_model** out);
void wbc_model_free(wbc_model* m);
int wbc_model_dims(const wbc_model* m, int* nb, int* nq, int* nv, int* nj, int* nf);
/* copies the flat arrays out (sizes per wbc_model_dims; any pointer may be NULL) */
int wbc_model_get_flat(const wbc_model* m, int* parent, double* Rt, double* rt, double* axis, double* mass,
                       double* com, double* Ic, int* foot_body, double* foot_off, double* gravity);
const char* wbc_model_joint_name(const wbc_model* m, int j); /* NULL if out of range / unnamed */
const char* wbc_model_foot_link(const wbc_model* m, int k);
double wbc_model_total_mass(const wbc_model* m);
/* <limit effort="..."> of each actuated joint: lim[nj], caller's joint order (wbc_model_joint_name); HUGE_VAL where the URDF gives none
 * and for wbc_model_from_flat models */
int wbc_model_effort_limits(const wbc_model* m, double* lim);

void wbc_params_default(wbc_params* p, int dtype);

/* ---- solver ---- */
int wbc_solver_create(const wbc_model* m, const wbc_params* p, int dtype, int device, size_t max_batch,
                      wbc_solver** out);

/* Kernel-selection options.  The defaults are the measured winners; nothing in the library reads the
 * environment, so a C++ host sees every switch here.  Call wbc_solver_options_default first, then change fields. */
enum wbc_timing_mode { WBC_TIMING_DISPATCH = 0, /* the dispatch's own start/stop timestamps (what rocprofv3 reports) */
                       WBC_TIMING_EVENT_PAIR = 1 /* an event pair recorded around the launch (+2-3 us per span) */ };
typedef struct wbc_solver_options {
  size_t struct_size;     /* sizeof(wbc_solver_options) of the caller's build (set by wbc_solver_options_default) */
  long long fused_max;    /* ticks of at most this many states run as ONE launch of wavefront roles; -1 = auto
                             (11264, observer on 12288; rollouts: 4096 -- wbc_plan_tick / wbc_dispatch_thresholds report it; at auto, fp64 observer-off ticks with matrix outputs
                             leave the one-launch tick at 8192 states already: tile_tick below), 0 = always the two-kernel tick */
  int rollout_persistent; /* 1 (default): rollouts of at most fused_max (auto: 4096) states = one launch per rollout; 0: per-tick launches */
  int rollout_spw;        /* states per workgroup of the rollout kernel: 0 = auto (4 up to 1024 states, else 16), 4, 16 */
  long long obs_split_min;/* observer-on two-kernel ticks of at least this many states run the observer update as its own
                             kernel instead of inside the sweep; -1 = auto (fp32: from 33792 states on, fp64: from 20480),
                             -2 = never */
  int one_zerocopy;       /* (default 3) single-robot host-pointer calls: 0 = staging copies + hipStreamSynchronize; 1 = the kernel reads / writes the
                             pinned image directly (mapped host memory); 2 = as 1, and completion is a ticket the stream writes into the
                             image behind the tick (hipStreamWriteValue32), polled by the host in memory: no runtime call on the wait
                             path; 3 = as 2 with a one-thread kernel writing the ticket.  2 / 3 fall back to 1 when the stack refuses */
  int timing_mode;        /* enum wbc_timing_mode, used by wbc_solver_enable_timing */
  int qp_tile;            /* GRF-QP kernel of the two-kernel tick: 0 = auto (tiles of states dealt to the wavefronts by predicted work,
                             sized so that the launch is ONE round of resident workgroups: fp64 from 14336 states on, 32 ... 64 states
                             per tile; fp32 from 16384 to 49152 states STAGED tiles -- one workgroup per CU holds ceil(N / 256) states
                             and their inputs in LDS -- then 72 ... 128 states per tile; one-wavefront workgroups below), -1 = never
                             tiles, otherwise always tiles of that many states: 32 | 64 | 128 | 256 | 512, fp64 also 36 ... 60 in
                             steps of 4, fp32 also every multiple of 4 up to 192 (staged) */
  int obs_split_serial;   /* that observer kernel runs 1 (default) = on the caller's stream before the sweep, 0 = beside it on a
                             second stream (measured slower: the two compete for the same SIMDs) */
  int qp_lane;            /* two-kernel ticks solve the QPs one state per LANE first (semismooth Newton on the residual wrench)
                             and send what that does not finish to the dense active-set kernel: 0 = auto (fp64 batches from
                             106496 states on, fp32 from 212992), 1 = always, -1 = never.  States solved per lane report status 0 and
                             iters = Newton iterations (<= 5); the others the dense kernel's status / iteration count.
                             wbc_params.qp_tol and max_iter govern the DENSE kernel only: the per-lane kernel accepts a state when
                             the residual of its optimality equation is below 1e-11 (fp32: 2e-5) x (1 + |target wrench|) or a full
                             Newton step leaves the active faces unchanged (then the point is the exact solution for those faces) */
  int f32_pack2;          /* fp32 dynamics sweep with TWO states per lane (packed v_pk_* arithmetic, whole 128-byte lines per 16-lane
                             row, half the wavefronts): 0 = auto (even batches from 32768 states on), 1 = every even batch, -1 = never */
  int keep_structural;    /* 54 of the 171 packed-M words and 108 of the 216 Jc words per state are structural zeros / ones (cross-leg
                             blocks, identity and skew-diagonal entries): 37 % of what the dynamics sweep stores.  1: a call that gets the
                             SAME M and Jc buffers and the same N as the previous call on this solver does not rewrite them -- the caller
                             promises not to touch M / Jc between ticks (any other pointer or N: written in full again).  0 (default):
                             every call writes every word.  The buffers are identified by ADDRESS: freeing and reallocating them (or a
                             caching allocator handing the same address out again) counts as touching them -- call
                             wbc_solver_invalidate_structural then */
  int rollout_warm;       /* (default 1) wbc_rollout_batch / wbc_rollout_tracking_batch: every tick after the first starts its GRF QPs from the
                             active set of the previous tick (see wbc_step_batch_warm).  The QP is strictly convex, so the results do not
                             depend on it -- the time per tick does.  0: every tick solves from the unconstrained minimum */
  int multi_threads;      /* (ABI 7; read by wbc_multi_create only) one persistent ISSUE THREAD per shard, bound to the shard's device: an entry point
                             validates every shard on the caller's thread, posts one ticket, the threads enqueue their shards in parallel and the call
                             returns when all have -- eight devices are no longer fed one launch after the other from one thread.  1 = on, -1 = never (the
                             serial issue of ABI <= 6), 0 = auto = serial (ABI 8: the threads are opt-in until they have been run on more than one device) */
  int multi_spin_us;      /* (default 200) an idle issue thread polls for its next ticket this long before it parks on a condition variable: a tick loop
                             never pays a wake-up, a 1 kHz control loop does not burn a core per shard */
  int obs_colaunch;       /* (ABI 7) observer-on two-kernel ticks with M/h/Jc outputs: the observer update and the observer-free sweep as the TWO ROLES OF
                             ONE LAUNCH (wbc_tick_plan.front = 4) while both roles' wavefronts are resident together -- fp32 batches of 12290 ... 32768
                             states (even; both roles with two states per lane), BASELINE's configs[3] shard; fp64 batches of 12289 ... 14336.
                             0 = auto, 1 = whenever the tick is a two-kernel tick with the observer on, -1 = never */
  int tile_tick;          /* (ABI 8) fp32 observer-on ticks with M/h/Jc outputs of an even batch: ONE launch of 128-state workgroups, one per CU -- the sweep and
                             observer roles of obs_colaunch side by side in a workgroup, then the staged QP tile of the same states behind one barrier
                             (wbc_tick_plan.fused = 2).  0 = auto (from 8194 states on -- up to 12288 in front of the one-launch tick while fused_max is at auto; 64 / 96 / 128 states per workgroup: one round of workgroups up to 32768 states,
                             BASELINE's configs[3] shard), 1 = every such tick beyond the fused_tick size, -1 = never.  Also fp64 observer-off ticks of 8193 ... 28672 states (48 ... 112-state workgroups, ahead of the one-launch tick while
                             fused_max is at auto; 1: every size beyond the fused_tick size) and fp64 observer-on ticks of 8193 ... 196608 states (32 / 48 / 64-state
                             workgroups of sweep + observer wavefronts, 64-state ones in rounds beyond 16384 states).  fp32 observer-off ticks: only with tile_tick = 1
                             (measured: +16 % at 32768 states, a loss at 49152 and below 16384 -- profiles/r06q_tile_tick_f32_noobs.log).  Auto applies only while qp_tile, qp_lane, obs_colaunch and obs_split_min are at auto themselves */
  int fused_pair;         /* (ABI 9) observer-off cold ticks with M/h/Jc outputs of N >= 64 states: the one-launch tick as twelve-wavefront workgroups of 32 states
                             (wbc_tick_plan.fused = 3: two of the 16-state workgroups in one, at 168 registers, so that BOTH halves are resident on a CU together -- 8192 states are
                             one round of workgroups instead of two; a batch that is not a multiple of 32 gets one more workgroup anchored at its end).  0 = auto (fp64 4225 ... 8192 states, fp32 4225 ... 16384, wbc_dispatch_thresholds reports them; only while
                             fused_max, tile_tick and the kernel selectors above are at auto), 1 = every such tick up to 65536 states, -1 = never */
} wbc_solver_options;
void wbc_solver_options_default(wbc_solver_options* o);
int wbc_solver_create_ex(const wbc_model* m, const wbc_params* p, int dtype, int device, size_t max_batch,
                         const wbc_solver_options* opt /* NULL = defaults */, wbc_solver** out);
int wbc_solver_device(const wbc_solver* s); /* HIP device index, -1 for NULL */
/* keep_structural: the next call writes M / Jc in full again whatever buffers it gets */
int wbc_solver_invalidate_structural(wbc_solver* s);

/* Which kernels a tick of N states runs with these options (no device needed): the measured switches of DESIGN.md section 5 as data, so
 * that a caller -- and the parity tests, which straddle every switch -- never restate them.  All fields are informational. */
typedef struct wbc_tick_plan {
  size_t struct_size; /* in: sizeof of the caller's build (0 = this build's); out: bytes written */
  int fused;          /* 1: the whole tick is ONE fused_tick launch (wavefront roles); everything below is 0 then.  3 (ABI 9): the same as 32-state workgroups
                         (fused_pair_kernel, wbc_solver_options.fused_pair).  2: ONE tile_tick launch (sweep | observer roles,
                         then the staged QP tile of the same states: front = 4, qp = 1, qp_body = 2, qp_tile = states per workgroup say what runs inside it) */
  int front;          /* two-kernel ticks, front half: 0 = dyn_sweep (observer inside when on), 1 = rnea_step (caller passes no M/h/Jc),
                         2 = observer kernel + observer-free dyn_sweep, 3 = observer kernel + observer-free rnea_step (no M/h/Jc),
                         4 = observer update and observer-free dyn_sweep as the two roles of ONE launch (sweep_obs_kernel) */
  int qp;             /* 0 = qp_group16 (one-wavefront workgroups), 1 = qp_tile (tiles dealt by predicted work), 2 = qp_lane + qp_list */
  int qp_tile;        /* states per tile when qp == 1 */
  int qp_body;        /* 0 = wrench-space dual active set in fp64 arithmetic, 1 = 12 x 12 orthogonal-factor body in fp32 (fp32 tiles beyond 65 536 states),
                         2 = as 0 on STAGED tiles: the tile's inputs go through LDS, results are stored row by row (fp32 solvers, tiles <= 192) */
  int sweep_pack2;    /* fp32 dyn_sweep with two states per lane */
  int sweep_block;    /* threads per workgroup of the dyn_sweep launch (64 / 256); 0 when no dyn_sweep runs */
  int qp_warm;        /* wbc_step_batch_warm: 1 = the QP kernels START from the carried active sets, 0 = they only report them (the sizes at which
                         the cold tiles are the faster kernels) */
} wbc_tick_plan;
/* warm != 0: the plan of wbc_step_batch_warm */
int wbc_plan_tick(int dtype, int observer_order, const wbc_solver_options* opt /* NULL = defaults */, size_t N, int with_mats, int with_pf,
                  int warm, wbc_tick_plan* plan);
int wbc_solver_plan_tick(const wbc_solver* s, size_t N, int with_mats, int with_pf, int warm, wbc_tick_plan* plan);
/* the batch sizes N at which the plan differs from that of N - 1 (fp32: N - 2; odd batches never pack), ascending; *n = how many
 * (at most 16), the first min(*n, cap) are written to out.  flags: WBC_PLAN_WITH_MATS (the caller passes M / h / Jc buffers) |
 * WBC_PLAN_WARM (the switches of wbc_step_batch_warm) */
#define WBC_PLAN_WITH_MATS 1
#define WBC_PLAN_WARM 2
int wbc_dispatch_thresholds(int dtype, int observer_order, const wbc_solver_options* opt, int flags, size_t* out, int cap, int* n);
/* diagnostics (synchronises the device): states of the last two-kernel tick that the per-lane QP kernel handed to the dense one */
int wbc_solver_qp_handover(wbc_solver* s, int* count);
void wbc_solver_destroy(wbc_solver* s);
/* Replaces the solver's parameters (checked as at creation; a rejected set changes nothing).  Every field is RUN-TIME data: the batch calls read the
 * parameters when they are ENQUEUED and pass them to their kernels as arguments, so every call made after this one -- ticks, rollouts, the gait
 * scheduler's control period -- runs under the new values, bit-identical to a solver created with them; work already enqueued keeps the old ones.
 * Nothing is captured by argument structs a caller prepared earlier (the Python binding's Solver.prepare_step closure follows the solver).  A
 * hipGraph CAPTURED before the call keeps the parameters it was captured with: re-capture after changing them.  observer_order may change; a tick
 * under an order > 0 needs the observer state buffers.  Not inside a stream capture; not concurrently with a call on the same solver. */
int wbc_solver_set_params(wbc_solver* s, const wbc_params* p);

typedef struct wbc_batch_in {
  const void* q;
  const void* v;
  const void* w_des;
  const void* vdot_des;
  const void* normals;
  const void* mu;
  const int* mask;
  const void* tau_prev; /* observer only, else may be NULL */
  const void* f_prev;   /* observer only, else may be NULL */
} wbc_batch_in;

typedef struct wbc_batch_out {
  void* tau;
  void* f;
  int* status;
  int* iters; /* may be NULL.  The solver's own count per state -- dual active-set trips (one-launch ticks with the observer on: of both phases of the
               * speculative start), Newton steps where the per-lane kernel solved the state; informational, never part of the parity contract */
  void* M;    /* optional dynamics outputs: all NULL or M, h, Jc all non-NULL */
  void* h;
  void* Jc;
  void* pf;   /* may be NULL */
} wbc_batch_out;

/* Momentum-observer state, in/out across ticks.  START-UP CONTRACT: the residual is r = K1 (M v - integ), so before the
 * first observer-on tick integ must hold the generalized momentum p(0) = M(q0) v0 of the state the loop starts from and
 * r must be zero -- zeros in integ are only right for a robot at rest (otherwise the first ticks carry a spurious
 * estimate of about K1 p(0) that decays with time constant 1/K1).  Batch callers get p from
 * wbc_dynamics_batch(..., p = integ, ...); the single-robot loop calls wbc_observer_init. */
typedef struct wbc_observer_state {
  void* integ;
  void* r;
} wbc_observer_state;

/* Dynamics sweep only: M(q), h(q,v), Jc(q) (+ optional pf, p = M v, beta = C^T v - g).
 * Stands for the rigid-body-dynamics calls the controller makes each tick (north_star:
 * "CRBA mass matrix, RNEA bias forces, contact Jacobians from the DogBot URDF").
 * All pointers are device pointers on the solver's device; `stream` is a hipStream_t (NULL = default). */
int wbc_dynamics_batch(wbc_solver* s, size_t N, const void* q, const void* v, void* M, void* h, void* Jc,
                       void* pf, void* p, void* beta, void* stream);

/* One control tick for N independent states: dynamics -> observer -> GRF QP -> torque map.
 * Stands for the controller's per-tick compute-torques entry point (name [UNVERIFIED]). */
int wbc_step_batch(wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out,
                   const wbc_observer_state* obs, void* stream);

/* One tick of a DEPENDENT sequence -- the reference controller runs in a loop on one robot (/root/reference/README.md:58-62), and
 * consecutive ticks share most of the active set of their GRF QP.  active_in [N] int32 (may be NULL = start cold) is the active set
 * each state's dual active-set iteration starts from: normally what the previous tick wrote to active_out [N] (may be NULL; in
 * place allowed).  Encoding, per state: for foot k with unit normal n, tangents t1, t2 and mu~ = mu * mu_scale
 *     bit 4k + j,      j = 0 .. 3:  the rows  (mu~ n - t1) . f >= 0,  (mu~ n - t2) . f >= 0,  n . f >= fn_min,  -n . f >= -fn_max
 *     bit 16 + 4k + j, j = 0 .. 1:  the rows  (mu~ n + t1) . f >= 0,  (mu~ n + t2) . f >= 0
 * Bits of swing feet are ignored.  The set is a HINT: the solver builds the minimiser on it in one block step and continues the
 * iteration from there when it is an S-pair of the dual method (independent rows, non-negative multipliers), otherwise it starts
 * cold -- the QP is strictly convex, so tau, f and status never depend on the hint, only `iters` (= iterations after the block step)
 * and the time do.  Same buffers, checks and stream semantics as wbc_step_batch.  Which kernels run: wbc_plan_tick with warm = 1 -- a call with
 * active_in = NULL runs (and is planned as) the cold tick, which still reports the sets. */
int wbc_step_batch_warm(wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs,
                        const int* active_in, int* active_out, void* stream);

/* SURVEY.md 8(f)-1 -- the step Gazebo performs in the reference loop (/root/reference/README.md:58), as the simplest
 * model that closes the loop for rollouts: forward dynamics with the planned GRFs applied,
 *   vdot = M^-1 (S^T tau + Jc^T f + tau_ext - h),  then semi-implicit Euler on (q, v) IN PLACE with the solver's dt.
 * M, h, Jc, tau, f are the outputs of the wbc_step_batch of the same tick (foot lever arms and the own-leg Jacobian
 * blocks are read from Jc).  tau_ext [nv][N] may be NULL. */
int wbc_integrate_batch(wbc_solver* s, size_t N, void* q, void* v, const void* M, const void* h, const void* Jc,
                        const void* tau, const void* f, const void* tau_ext, void* stream);

/* `horizon` dependent ticks of {wbc_step_batch, wbc_integrate_batch} with constant references (BASELINE.json
 * configs[4]: MPC-style WBC-in-the-loop rollouts).  in->q / in->v are ADVANCED IN PLACE (const is cast away);
 * out->tau / out->f must hold the previous tick's outputs (or zeros) on entry and serve as tau_prev / f_prev;
 * out->M, out->h, out->Jc are required.  tau_traj (optional) receives tau of every tick: [horizon][nj][N].
 * On return the out-> buffers (tau, f, status, iters, M, h, Jc, pf), the observer state and (tracking) w_des / vdot_des hold the LAST
 * tick's values, as after per-tick calls; while the call runs their contents are unspecified (rollouts of up to 1024 states are one launch that
 * keeps state, torques and observer inputs on chip from tick to tick and writes them out once). */
int wbc_rollout_batch(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in, const wbc_batch_out* out,
                      const wbc_observer_state* obs, const void* tau_ext, void* tau_traj, void* stream);

/* (ABI 10) Plant model mismatch: rollouts and forward dynamics whose PLANT carries a rigid payload on its trunk (body 0) while the controller
 * keeps the nominal model -- the case the disturbance observer exists for.  Plant dynamics:
 *   (M + dM(q)) vdot = S^T tau + Jc^T f + tau_ext - (h + dh(q, v)),   then the semi-implicit Euler step of wbc_integrate_batch.
 * A body fixed to the trunk changes only the 6x6 base block of M and the 6 base rows of h, so the correction is exact.
 * M, h, Jc in `out` stay the controller's nominal-model outputs.  plant == NULL or plant->payload == NULL runs exactly the calls without
 * `plant` (same kernels, same bits).  Stream rules as for those calls: no allocation, no synchronisation, capturable in a hipGraph. */
#define WBC_PAYLOAD_WORDS 10
/* payload [10][N], solver scalar type, component-major like every batch array:
 *   0: m (kg, >= 0)   1..3: c, payload CoM in the BASE frame (m)   4..9: I about c, base axes: xx yy zz xy xz yz (kg m^2)
 * A row of zeros = no payload for that state.  Values are not checked on the device: m >= 0 and a physical (PSD) inertia are
 * the caller's promise, as for q / v today. */
typedef struct wbc_plant {
  size_t struct_size;    /* sizeof(wbc_plant) of the caller's build */
  const void* tau_ext;   /* [nv][N] or NULL: as in wbc_integrate_batch / wbc_rollout_batch */
  const void* payload;   /* [WBC_PAYLOAD_WORDS][N] or NULL */
} wbc_plant;
int wbc_integrate_plant_batch(wbc_solver* s, size_t N, void* q, void* v, const void* M, const void* h, const void* Jc,
                              const void* tau, const void* f, const wbc_plant* plant, void* stream);
int wbc_rollout_plant_batch(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in, const wbc_batch_out* out,
                            const wbc_observer_state* obs, const wbc_plant* plant, void* tau_traj, void* stream);

/* SURVEY.md 8(f)-3 -- the caller on the input side of the tick: "a motion planner for the trajectory of the robot's
 * center of mass" (/root/reference/README.md:11) produces the references the whole-body controller tracks.  The
 * planner's source is absent from the reference ([UNVERIFIED] interface); this entry point is the build's definition:
 *   plan [12][N]: c0 (3) start CoM, c1 (3) goal CoM (world), T duration [s], t0 time already elapsed [s],
 *                 quat_des (x,y,z,w) desired trunk attitude
 *   rest-to-rest quintic c_ref(u), u = clamp((t0 + t) / T, 0, 1)   (T <= 0: the goal itself)
 *   a_cmd = cdd_ref + kp_com (c_ref - c) + kd_com (cd_ref - cd)      c, cd = CoM position / velocity of (q, v)
 *   alpha_cmd = kp_rot e_R - kd_rot omega,  e_R = 2 vec(quat_des (x) quat^-1) with non-negative scalar part
 *   vdot_des = [a_cmd; alpha_cmd; kp_joint (q_nom - q_j) - kd_joint qd_j]
 *   w_des = [F; (c - p_b) x F + R diag(inertia_nom) R^T alpha_cmd],  F = m_total (a_cmd - gravity)
 * Writes w_des [6][N] and vdot_des [nv][N] (the wbc_batch_in fields of the same names); com (optional) [6][N] = c, cd. */
typedef struct wbc_ref_params {
  double kp_com[3], kd_com[3];
  double kp_rot[3], kd_rot[3];
  double kp_joint, kd_joint;
  double inertia_nom[3];    /* nominal trunk inertia, body axes */
  double q_nom[WBC_MAXV];   /* nominal joint posture, caller's joint order */
} wbc_ref_params;
#define WBC_PLAN_WORDS 12
void wbc_ref_params_default(wbc_ref_params* g);
int wbc_solver_set_ref_params(wbc_solver* s, const wbc_ref_params* g);
int wbc_reference_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* plan, double t,
                        void* w_des, void* vdot_des, void* com, void* stream);

/* wbc_rollout_batch with the planner in the loop: every tick k first regenerates in->w_des / in->vdot_des from `plan`
 * at t = k * dt (those two buffers are OVERWRITTEN; const is cast away), then steps and integrates.
 * com_traj (optional) receives the CoM state the planner saw at every tick: [horizon][6][N]. */
int wbc_rollout_tracking_batch(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in, const wbc_batch_out* out,
                               const wbc_observer_state* obs, const void* tau_ext, const void* plan, void* tau_traj,
                               void* com_traj, void* stream);
/* wbc_rollout_tracking_batch with the plant of wbc_rollout_plant_batch (ABI 10) */
int wbc_rollout_tracking_plant_batch(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in, const wbc_batch_out* out,
                                     const wbc_observer_state* obs, const wbc_plant* plant, const void* plan, void* tau_traj,
                                     void* com_traj, void* stream);

/* Scored rollouts: a running quadratic cost of a rollout's state path, accumulated on chip, and the choice of the best of K candidates per group --
 * what a sampling MPC runs rollouts for (rollout -> cost -> argmin / MPPI weights, all on the stream, capturable in one hipGraph).
 * ADDITIVE to ABI 10: wbc_abi_version() stays 10 and no existing struct changes; a caller detects the feature by these symbols (dlsym).
 * Per state, for tick k = 0 .. H-1, on the state (q, v) the tick ENDS in (after its integrator step) and on the tau, f, status it produced:
 *   l_k = w_tau sum_j tau_j^2 + w_f sum_i f_i^2 + w_fail [status_k != 0]
 *       + s_k ( sum_c w_pos[c] (p_c - g_p[c])^2      p  = base position q[0..2]
 *             + sum_c w_rot[c] e_c^2                 e  = the attitude error e_R of wbc_reference_batch with quat_des := g_quat, base quaternion q[3..6]
 *             + sum_c w_vel[c] (v_c - g_v[c])^2      v  = base linear velocity v[0..2]
 *             + sum_c w_omega[c] om_c^2              om = base angular velocity v[3..5]
 *             + w_q sum_j (qj_j - q_nom_j)^2 + w_qd sum_j qdj_j^2 )      joints in the caller's order
 *   s_k = 1 for k < H-1, s_(H-1) = terminal
 *   cost = (accumulate ? cost_in : 0) + sum_k l_k        fail_ticks = (accumulate ? in : 0) + #{k : status_k != 0}
 * goal [WBC_GOAL_WORDS][N], solver scalar type, component-major: g_p (3), g_quat (x, y, z, w), g_v (3).  Arithmetic and the sum in the solver's scalar type. */
#define WBC_GOAL_WORDS 10
typedef struct wbc_score_params {
  size_t struct_size;    /* sizeof(wbc_score_params) of the caller's build */
  double w_tau, w_f, w_fail;
  double w_pos[3], w_rot[3], w_vel[3], w_omega[3];
  double w_q, w_qd;
  double terminal;       /* s_k of the last tick, >= 0 */
  double q_nom[WBC_MAXV];
} wbc_score_params;
/* every weight 0 except w_fail = 1e6; terminal = 1; q_nom = 0 */
void wbc_score_params_default(wbc_score_params* p);
/* all weights and terminal >= 0 (WBC_E_INVALID otherwise).  The weights travel as a kernel argument: nothing is uploaded, later scored calls use them.
 * Not inside a stream capture (a captured graph keeps the weights it was captured with). */
int wbc_solver_set_score_params(wbc_solver* s, const wbc_score_params* p);
typedef struct wbc_rollout_score {
  size_t struct_size;    /* sizeof(wbc_rollout_score) of the caller's build */
  const void* goal;      /* [WBC_GOAL_WORDS][N] */
  void* cost;            /* [N], solver scalar type */
  int* fail_ticks;       /* [N] int32 or NULL */
  int accumulate;        /* 0: the sums start at zero; else at what cost / fail_ticks hold (a horizon continued over several calls) */
} wbc_rollout_score;
/* The superset rollout.  plant == NULL: the nominal plant; plan == NULL: constant references (com_traj must then be NULL).
 * score == NULL or score->cost == NULL: exactly the existing entry point of that (plant, plan) combination -- same kernels, same bits.
 * Scored launches of the one-launch path always start every tick after the first from the previous tick's active set (rollout_warm = 1:
 * results do not depend on it).  Stream rules as for the other rollouts: no allocation, no synchronisation, hipGraph-capturable. */
int wbc_rollout_scored_batch(wbc_solver* s, size_t N, int horizon, const wbc_batch_in* in, const wbc_batch_out* out,
                             const wbc_observer_state* obs, const wbc_plant* plant, const void* plan, void* tau_traj, void* com_traj,
                             const wbc_rollout_score* score, void* stream);
/* One tick's l_k, for callers that drive their own loop: q, v = the state the tick ended in, tau, f, status = what it produced;
 * is_last selects s_k = terminal.  score->accumulate = 0: cost = l_k (the first tick of a sum); else l_k is added to score->cost. */
int wbc_score_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* tau, const void* f, const int* status,
                    const wbc_rollout_score* score, int is_last, void* stream);
/* N = n_groups * group candidates; group g = states [g * group, (g + 1) * group), 1 <= group <= 4096.  Per group:
 *   best [n_groups] int32 = index WITHIN the group of the smallest cost (ties: the lowest index; NaN counts as +inf; all +inf / NaN: -1)
 *   best_cost [n_groups] (optional)
 *   weights [N] (optional) = exp(-(c_i - c_min) / lambda) / their sum over the group (MPPI); lambda <= 0: one-hot on best;
 *                            a group with best = -1 gets all-zero weights
 * No solver: dtype (WBC_F64 / WBC_F32) names the scalar type; runs on the current device.  Bit-identical from run to run. */
int wbc_rollout_select(int dtype, size_t n_groups, size_t group, const void* cost, double lambda, int* best, void* best_cost,
                       void* weights, void* stream);

/* Joint torque limits behind a tick.  ADDITIVE to ABI 10 (wbc_abi_version() stays 10, no existing struct changes; detect it by these symbols).
 * wbc_step_batch itself never applies limits.  The post-pass works per state on the tick's own outputs: a state whose torques are all within
 * |tau_j| <= tau_max[j] (compared exactly, no tolerance) is left untouched bit for bit; a state with a STANCE-leg joint beyond its limit gets its GRF QP
 * solved again on chip with the rows |tau0_j - a_j^T f| <= tau_max[j] added (tau0 = tau + (Jc^T f)_joint rows, the force-free torque; a_j = column 6 + j of
 * Jc; same objective, friction pyramid and normal-force box as the tick, wbc_params.qp_tol and max_iter, fp64 arithmetic for both scalar types), and f, tau,
 * status, iters are rewritten from it.  limited [N] int32 says what happened:
 *   0  within the limits: tau, f, status, iters untouched
 *   1  re-solved: status = 0, iters = the limited QP's iterations, every stance-leg |tau_j| <= tau_max[j] + qp_tol
 *   2  clamped: a SWING-leg joint was beyond its limit (no contact force can change it: tau_j = +-tau_max[j]; f and the stance legs follow 0 or 1), or
 *      the limited QP ended in status 1 / 2 (the tick's f and status stay, every tau_j is clipped).  A clamped state's tau no longer realises vdot_des.
 * Stream rules as for wbc_step_batch: two launches and a 4-byte memset on the caller's stream, no allocation, no synchronisation, hipGraph-capturable.
 * The limits travel as a kernel argument: nothing is uploaded, and a captured graph keeps the limits it was captured with.  When every limit is
 * HUGE_VAL nothing is launched.  N == 0 returns WBC_OK without looking at the buffers, as wbc_step_batch does.  The list of saturated states and its
 * counter belong to the solver: post-passes of ONE solver must be ordered on one stream (or by events); two of them running at once on different
 * streams race on that list.  A clipped torque is tau_max[j] rounded to the solver's scalar type.  Not part of the one-launch rollout kernels or of the wbc_multi_* entry points (a shard's caller runs the post-pass on the
 * shard's solver and stream); velocity and position limits are not modelled. */
typedef struct wbc_torque_limits {
  size_t struct_size;        /* sizeof(wbc_torque_limits) of the caller's build */
  double tau_max[WBC_MAXV];  /* > 0, caller's joint order; HUGE_VAL = none */
} wbc_torque_limits;
/* l == NULL: back to the model's effort limits (what a new solver starts with).  Not inside a stream capture. */
int wbc_solver_set_torque_limits(wbc_solver* s, const wbc_torque_limits* l);
/* the post-pass alone, behind ANY tick of the same N on the same stream (wbc_step_batch, wbc_step_batch_warm, a shard's tick): in / out / obs are that
 * tick's; out->M, h, Jc are required (Jc is read); limited may be NULL */
int wbc_limit_torques_batch(wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs,
                            int* limited, void* stream);
/* wbc_step_batch followed by wbc_limit_torques_batch; every argument check of both runs before anything is enqueued */
int wbc_step_limited_batch(wbc_solver* s, size_t N, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs,
                           int* limited, void* stream);
/* diagnostics (synchronises the device): how many states the last post-pass re-solved */
int wbc_solver_limited_count(wbc_solver* s, int* resolved);

/* Swing-foot references: Cartesian foot tracking for swing legs.  ADDITIVE to ABI 10 (wbc_abi_version() stays 10, no existing struct changes; detect it
 * by these symbols).  wbc_reference_batch asks a lifted leg only for the joint posture law; these calls replace that leg's rows of vdot_des by the joint
 * accelerations that make its foot follow a planned trajectory, which the tick then turns into the leg's inverse-dynamics torque.
 *   swing [WBC_SWING_WORDS = 36][N], solver scalar type, component-major; foot k owns rows 9k .. 9k+8:
 *     9k .. 9k+2  p0   lift-off position (world)          9k+6  hgt  apex clearance, m
 *     9k+3 .. +5  p1   touchdown position (world)         9k+7  T    swing duration, s        9k+8  t0  time already elapsed, s
 *   u = clamp((t0 + t) / T, 0, 1)   (T <= 0: u = 1),  d = p1 - p0,  z = (0, 0, 1)
 *   s0, s1, s2: the rest-to-rest quintic of wbc_reference_batch and its first two time derivatives (factors 1/T, 1/T^2; 0 when T <= 0)
 *   b = 64 u^3 (1-u)^3,   b' = 192 u^2 (1-u)^2 (1-2u),   b'' = 384 u (1-u) (1 - 5u + 5u^2)
 *   p_ref = p0 + s0 d + hgt b z,   pd_ref = s1 d + hgt b'/T z,   pdd_ref = s2 d + hgt b''/T^2 z      (every derivative term is 0 at u = 0 and u = 1)
 * For every foot k whose bit in `mask` is CLEAR, with J_k = foot k's three rows of Jc = [J_kb (3x6) | J_kl (3x3, the leg's own joint columns)]:
 *   a_cmd = pdd_ref + kp o (p_ref - p_f) + kd o (pd_ref - J_k v)
 *   rhs   = a_cmd - Jdot_k v - J_kb vdot_des[0..5]
 *   (J_kl J_kl^T + damping 1) y = rhs,      vdot_des[6 + j] = (J_kl^T y)_j   for the three joints j of leg k, caller's joint order
 * Jdot_k v is the foot point's world acceleration at vdot = 0 (velocity-product recursion down the leg); it equals d/de [J_k(q (+) e v)] v at e = 0 with
 * (+) the configuration update of wbc_integrate_batch.  vdot_des[0..5] are read as they stand on entry (typically wbc_reference_batch has just written
 * them).  Rows of stance legs, the base rows and w_des are not touched, bit for bit; a caller who wants the posture law for a lifted leg sets that leg's
 * bit in the mask passed to THIS call.  Damped least squares is used for every state, not only next to a singularity: the result is continuous in q.
 * foot (optional) [WBC_FOOT_WORDS = 24][N]: rows 6k .. 6k+2 = p_f, 6k+3 .. 6k+5 = J_k v, for ALL four feet.
 * Stream rules as for wbc_reference_batch (the two batch calls): no allocation, no synchronisation, hipGraph-capturable; N == 0 returns WBC_OK without
 * looking at the buffers; a NULL required pointer: WBC_E_INVALID; N > max_batch: WBC_E_CAPACITY.
 * Out of scope: the one-launch rollout kernels and wbc_rollout_*, wbc_multi_*, contact schedules and touchdown detection, an apex direction aligned
 * with the terrain normal. */
#define WBC_SWING_WORDS 36
#define WBC_FOOT_WORDS 24
typedef struct wbc_swing_params {
  size_t struct_size;    /* sizeof(wbc_swing_params) of the caller's build */
  double kp[3], kd[3];   /* world axes, >= 0 */
  double damping;        /* lambda^2, m^2, >= 0 */
} wbc_swing_params;
/* kp = 400, kd = 40 (critically damped), damping = 1e-4: this build's definition, as wbc_ref_params_default is */
void wbc_swing_params_default(wbc_swing_params* p);
/* a negative or non-finite entry: WBC_E_INVALID.  The values travel as a kernel argument: nothing is uploaded, later swing calls use them.
 * Not inside a stream capture (a captured graph keeps the values it was captured with). */
int wbc_solver_set_swing_params(wbc_solver* s, const wbc_swing_params* p);
int wbc_swing_reference_batch(wbc_solver* s, size_t N, const void* q, const void* v, const int* mask, const void* swing, double t,
                              void* vdot_des /* in/out */, void* foot, void* stream);
/* wbc_reference_batch followed by wbc_swing_reference_batch, as ONE launch.  w_des, com, the base rows and the stance legs' rows of vdot_des are
 * bit-identical to wbc_reference_batch's; the swing legs' rows equal the two-call sequence's to rounding (not bit for bit: DESIGN.md 4.10). */
int wbc_reference_swing_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* plan, const int* mask, const void* swing,
                              double t, void* w_des, void* vdot_des, void* com, void* foot, void* stream);
/* Single-robot, host-pointer, fp64 form of wbc_swing_reference_batch (q[19], v[18], swing[36] in; vdot_des[18] in/out; the optional foot[24] out):
 * the companion of wbc_compute_reference.  Synchronises. */
int wbc_compute_swing_reference(wbc_solver* s, const double* q, const double* v, int mask, const double* swing, double t,
                                double* vdot_des /* in/out */, double* foot);

/* Gait scheduler: contact masks, footholds and swing plans on the device.  ADDITIVE to ABI 10 (wbc_abi_version() stays 10, no existing struct changes;
 * detect it by these symbols).  The swing calls above take `mask` and the 36 `swing` words from the caller; this call writes them, so that a walking
 * tick is four launches on one stream with no host work between them:  gait -> reference_swing -> step -> integrate.
 *   cmd [WBC_GAIT_CMD_WORDS = 4][N], solver scalar type, component-major: rows 0, 1 the commanded trunk velocity vx, vy in the HEADING frame, row 2 the
 *         commanded yaw rate wz, row 3 the ground height z_g (world z of the foothold)
 *   phase [N]  in/out: the gait phase phi in [0, 1)
 *   mask [N]   in: the previous tick's mask (before the first tick the caller stores 0b1111);  out: this tick's mask
 *   swing [WBC_SWING_WORDS][N]  in/out: the plan words of wbc_swing_reference_batch.  This call writes t0 itself, so the swing call behind it is given t = 0
 *   contact [N] or NULL: bit k set = foot k senses ground (NULL: no bit set)
 *   events [N] or NULL: bit k set = foot k lifted off this tick, bit 4 + k set = it touched down this tick
 * With dt the solver's control period the host forms, in double, rounded to the solver's scalar type and passed as kernel arguments:
 *   dphi = dt / period,   inv_sw[k] = 1 / (1 - duty[k])  (0 when duty[k] == 1),   T_sw[k] = (1 - duty[k]) period
 * Per state:
 *   1. phi' = phi + dphi;  if phi' >= 1: phi' -= 1.  phi' is stored.
 *   2. per foot k:  phi_k = phi' + offset[k];  if phi_k >= 1: phi_k -= 1;   sched_k = phi_k < duty[k];   u_k = (phi_k - duty[k]) inv_sw[k]  (used only
 *      when !sched_k)
 *   3. the new bit from the previous bit b_k and the sensed bit c_k:
 *        sched_k              -> 1
 *        !sched_k, b_k == 1   -> 1 if u_k >= late (a stance foot that finds itself late in its swing window stays down: it missed its lift-off or landed
 *                                  early), else 0: a LIFT-OFF
 *        !sched_k, b_k == 0   -> 1 if c_k and u_k >= late (an early touchdown), else 0
 *   4. the nine swing words of foot k:
 *        new bit 1            all nine untouched, bit for bit
 *        lift-off             p0 = the foot's current world position p_f(q),  hgt = clearance,  T = T_sw[k],  t0 = u_k T_sw[k],  p1 = the foothold
 *        continuing swing     t0 = u_k T_sw[k];  p1 = the foothold when retarget;  p0, hgt, T untouched, bit for bit
 *   5. the foothold (Raibert: where the nominal foothold will be at touchdown + half a stance of commanded travel + velocity feedback).  With
 *      h = (R00, R10) of the base rotation, normalised (the heading; undefined when the trunk's x axis is vertical), Rz the 2x2 rotation it defines:
 *        b = Rz base_xy[k],   v_c = Rz (vx, vy),   v = v[0..1],   T_rem = (1 - u_k) T_sw[k],   T_st = duty[k] period
 *        p1_xy = p_b,xy + b + v T_rem + 1/2 T_st v_c + k_v (v - v_c) + 1/2 T_st wz (-b_y, b_x),      p1_z = z_g
 * Only additions, subtractions and comparisons -- and the single rounded product u_k, which no compiler can contract -- decide the mask: mask, events and
 * every word this call leaves untouched are EXACT (the same bits as the same arithmetic on a CPU in the same scalar type).  p0, p1 and t0 are exact only to
 * rounding, because the compiler may contract their products.
 * Stream rules as for wbc_swing_reference_batch: no allocation, no synchronisation, hipGraph-capturable; phase, mask and swing advance IN PLACE; N == 0
 * returns WBC_OK without looking at the buffers; a NULL required pointer: WBC_E_INVALID; N > max_batch: WBC_E_CAPACITY.
 * Out of scope: the rollout kernels and wbc_rollout_*; wbc_multi_*; late touchdown (the schedule says stance and no contact is sensed); fusing this
 * call into the fused reference + swing kernel, whose fp64 instantiation already uses 256 VGPRs and would spill.  (Footholds and foot
 * planes on a mapped terrain: wbc_gait_terrain_batch, "Terrain heightfield" below.) */
#define WBC_GAIT_CMD_WORDS 4
typedef struct wbc_gait_params {
  size_t struct_size;   /* sizeof(wbc_gait_params) of the caller's build */
  double period;        /* gait cycle, s, > 0 */
  double duty[4];       /* stance fraction per foot, 0 < duty <= 1 (1 = never lifts) */
  double offset[4];     /* phase offset per foot, 0 <= offset < 1 */
  double clearance;     /* hgt written into the swing plan, m, >= 0 */
  double k_v;           /* velocity-feedback gain of the foothold, s, finite */
  double late;          /* 0 < late <= 1: a stance foot lifts only while u < late; sensed contact ends a swing only when u >= late */
  int    retarget;      /* 1: p1 recomputed every tick of the swing; 0: latched at lift-off */
  double base_xy[4][2]; /* nominal foothold of foot k relative to the base origin, heading frame, m */
} wbc_gait_params;
/* period 0.4, duty 0.6, offset {0, .5, .5, 0} (feet {0, 3} and {1, 2} are the diagonal pairs), clearance 0.05, k_v 0.03, late 0.5, retarget 1;
 * base_xy[k] = x, y of the origin of the first joint of foot k's leg in the base frame, caller's foot order (zeros when m is NULL or not a quadruped) */
void wbc_gait_params_default(const wbc_model* m /* may be NULL */, wbc_gait_params* p);
/* a value outside the ranges above or a non-finite value: WBC_E_INVALID.  The values travel as a kernel argument: nothing is uploaded, later gait calls
 * use them.  Not inside a stream capture (a captured graph keeps the values it was captured with). */
int wbc_solver_set_gait_params(wbc_solver* s, const wbc_gait_params* p);
int wbc_gait_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const int* contact /* may be NULL */,
                   void* phase /* in/out [N] */, int* mask /* in/out [N] */, void* swing /* in/out [36][N] */, int* events /* may be NULL, [N] */,
                   void* stream);
/* Single-robot, host-pointer, fp64 form of wbc_gait_batch (q[19], v[18], cmd[4] in; phase[1], mask[1], swing[36] in/out; the optional events[1] out).
 * Synchronises. */
int wbc_compute_gait(wbc_solver* s, const double* q, const double* v, const double* cmd, int contact, double* phase, int* mask, double* swing,
                     int* events);

/* Ground-contact plant: terrain reaction forces and sensed foot contact.  ADDITIVE to ABI 10 (wbc_abi_version() stays 10, no existing struct changes;
 * detect it by these symbols).  wbc_integrate_batch applies the PLANNED ground reaction forces; these calls put a ground under the plant instead, which
 * pushes back on every foot whatever the controller planned, and they produce the `contact` word wbc_gait_batch reads.  The walking tick becomes
 *   gait(contact = the previous tick's) -> reference_swing -> step -> integrate_ground          (still four launches, no host work between them).
 * The law is stateless and handles each foot on its own.  The terrain under foot k is the plane n_k . x = d_k:
 *   normals [12][N]  the buffer the tick already takes (rows 3k .. 3k+2 = n_k, unit length)
 *   height  [4][N]   d_k, solver scalar type: one plane offset PER FOOT, so a bump or a hole under a single foot is a different d_k
 *   mu      [4][N]   the tick's friction coefficients, used UNSCALED (mu_scale belongs to the QP's pyramid and is not applied here)
 * With lever_k = p_f,k - p_b read from the base-angular columns of this tick's Jc and J_leg,k its own-leg 3x3 block (the words wbc_integrate_batch reads):
 *   p_f = p_b + lever_k          v_f = pdot_b + omega x lever_k + J_leg,k qdot_leg,k
 *   phi = n . p_f - d_k          (the gap; negative = penetration)
 *   v_n = n . v_f                v_t = v_f - v_n n
 *   f_n = phi < 0 ? max(0, -k_n phi - c_n v_n) : 0
 *   g   = -c_t v_t
 *   s   = |g| > mu_k f_n ? mu_k f_n / |g| : 1          (|g| = 0: f_t = 0, no 0/0)
 *   f_t = s g
 *   f_gr,k = f_n n + f_t         contact bit k = f_n > f_touch
 * Outputs: f_gr [12][N] (rows 3k .. 3k+2 = foot k, the rows wbc_integrate_batch reads as f), contact [N] or NULL (bit k = foot k, the encoding of
 * wbc_gait_batch), gap [4][N] or NULL (phi_k).
 * wbc_ground_force_batch evaluates the law alone.  wbc_integrate_ground_batch evaluates it and then advances q, v IN PLACE exactly as
 * wbc_integrate_batch with f = f_gr does, in ONE launch; the force is applied to EVERY foot, the commanded f is no input of the plant at all.
 * The plant is explicit (the damping term uses the old v), so it is stable only while the damping and the stiffness are small against the foot's
 * effective mass m_eff = 1 / (n Jc M^-1 Jc^T n) -- well under a kilogram for the synthetic model -- at the solver's dt.  The four feet are coupled
 * through the trunk: what must stay below 2 is the largest eigenvalue of dt (Jc M^-1 Jc^T) diag(c_t, c_t, c_n) over all twelve foot rows, which is
 * two to three and a half times the per-foot ratio c_n dt / m_eff (0.97 against 0.45 with the defaults, 2.03 against 0.60 with c_n 200, c_t 500).  The defaults
 *   k_n = 2e4 N/m,  c_n = 150 N s/m,  c_t = 200 N s/m,  f_touch = 5 N
 * were fixed on the CPU with the numpy restatement of this law (tests/ground_ref.py) at the solver's default dt = 1e-3: a standing robot released with
 * its feet 5 mm above flat ground settles to sum_k n . f_gr,k = m_total |g| and a mean penetration of m_total |g| / (4 k_n), and no contact bit
 * toggles afterwards.  (k_n 2e4, c_n 200, c_t 500 did not pass: that eigenvalue was 2.03 and the foot forces alternated from tick to tick for good;
 * with the defaults it is 0.97.  tests/test_ground_oracle.py holds the measured settling time, residuals and stability ratios.)  A caller with another
 * dt or a lighter leg scales c_n, c_t with m_eff / dt.
 * Viscous friction has no stiction -- a foot under a tangential load F creeps at F / c_t under THESE calls; wbc_ground_stick_force_batch /
 * wbc_integrate_ground_stick_batch ("Stiction" below) add a per-foot anchor spring that holds it.
 * Stream rules as for wbc_gait_batch: no allocation, no synchronisation, hipGraph-capturable; N == 0 returns WBC_OK without looking at the buffers; a NULL
 * required pointer: WBC_E_INVALID; N > max_batch: WBC_E_CAPACITY.
 * Out of scope: the payload plant (wbc_integrate_plant_batch); the rollout kernels and wbc_rollout_*; wbc_multi_*; late touchdown in the gait rule.
 * (Stiction: the calls of the next section.  normals and height from a map: "Terrain heightfield" below.) */
typedef struct wbc_ground_params {
  size_t struct_size;     /* sizeof(wbc_ground_params) of the caller's build */
  double k_n, c_n, c_t;   /* N/m, N s/m, N s/m; all >= 0 and finite */
  double f_touch;         /* N, >= 0 */
} wbc_ground_params;
void wbc_ground_params_default(wbc_ground_params* p);
/* a negative or non-finite value: WBC_E_INVALID.  The values travel as a kernel argument: nothing is uploaded, later ground calls use them.  Not inside a
 * stream capture (a captured graph keeps the values it was captured with). */
int wbc_solver_set_ground_params(wbc_solver* s, const wbc_ground_params* p);
int wbc_ground_force_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* Jc, const void* normals, const void* height,
                           const void* mu, void* f_gr, int* contact /* may be NULL */, void* gap /* may be NULL */, void* stream);
int wbc_integrate_ground_batch(wbc_solver* s, size_t N, void* q, void* v, const void* M, const void* h, const void* Jc, const void* tau,
                               const void* normals, const void* height, const void* mu, const void* tau_ext /* may be NULL */, void* f_gr,
                               int* contact /* may be NULL */, void* gap /* may be NULL */, void* stream);

/* Stiction on the ground plant: a per-foot anchor spring.  ADDITIVE to ABI 10 (wbc_abi_version() stays 10, no existing struct, call or default changes;
 * detect it by these symbols).  The ground plant's friction is viscous, so a loaded foot creeps at F / c_t: it cannot hold a robot on a slope, and
 * every stance foot of the walking loop drifts.  These two calls are the ground calls with one more term in the tangential force, a spring between the
 * foot and the world point it is stuck to.  The walking tick becomes
 *   gait(contact = the previous tick's) -> reference_swing -> step -> integrate_ground_stick     (still four launches, no host work between them).
 * The new state belongs to the caller and advances IN PLACE:
 *   anchor [12][N]  solver scalar type; rows 3k .. 3k+2 = the world point foot k is stuck to
 *   stick  [N]      int.  in: bit k = foot k has an anchor.  out: bit k = foot k is loaded (f_n > 0) and so has an anchor for the next tick; bit 4+k =
 *                   foot k slid this tick.  Only bits 0-3 are read.  The caller stores 0 before the first tick; anchor needs no initial value.
 * p_f, v_f, phi, v_n, v_t, f_n, the contact bit and gap are formed exactly as the ground calls form them, from the same words of q, v, Jc, normals,
 * height, mu and the same wbc_ground_params.  Then, per foot:
 *   f_n == 0:  f_t = 0;  out bit k = 0, out bit 4+k = 0;  the three anchor words are not touched
 *   f_n  > 0:  a    = in bit k ? anchor_k : p_f          (first loaded tick: the anchor is dropped where the foot is, e = 0)
 *              e    = (p_f - a) - n (n . (p_f - a))      (the tangential stretch)
 *              g    = -k_t e - c_t v_t
 *              cone = mu_k f_n
 *              |g| >  cone:  s = cone / |g|;  f_t = s g;  anchor_k := p_f - s e;  out bit 4+k = 1     (slide: the stretch shrinks by the same factor)
 *              |g| <= cone:  f_t = g;  anchor_k stays (one that was there is not written; a new one = p_f);  out bit 4+k = 0
 *              out bit k = 1
 *   f_gr,k = f_n n + f_t
 * |g| = 0 gives f_t = 0 with no 0/0.  With k_t = 0 the force is the ground calls', as numbers.  The force and the anchor are continuous across the cone
 * (s = 1 there) and across f_n -> 0 (the cone closes, s -> 0, the anchor follows the foot).
 * wbc_ground_stick_force_batch evaluates the law alone.  wbc_integrate_ground_stick_batch evaluates it and then advances q, v IN PLACE exactly as
 * wbc_integrate_batch with f = f_gr does, in ONE launch.
 * The spring is explicit like the rest of the plant.  With a = the largest eigenvalue of dt (Jc M^-1 Jc^T) diag(c_t, c_t, c_n) over the twelve foot rows
 * (0.97 with the defaults) and b = that of dt^2 (Jc M^-1 Jc^T) diag(k_t, k_t, k_n), one mode of the semi-implicit step is stable while b < 4 - 2 a.
 * The default
 *   k_t = 2e4 N/m   (= k_n)
 * was fixed on the CPU with the numpy restatement of this law (tests/stick_ref.py) at dt = 1e-3 and 2^-10: a standing robot on planes tilted by
 * 0.2 rad, which slides 6 cm/s for ever under the viscous law, stops; the walking loop's stance feet slip less than half as far.
 * tests/test_stick_oracle.py holds the measured figures, a and b among them.  A caller with another dt or a lighter leg scales k_t with m_eff / dt^2.
 * Stream rules as for the ground calls: no allocation, no synchronisation, hipGraph-capturable; N == 0 returns WBC_OK without looking at the buffers; a
 * NULL required pointer (anchor and stick included): WBC_E_INVALID; N > max_batch: WBC_E_CAPACITY.
 * Out of scope: the payload plant (wbc_integrate_plant_batch); the rollout kernels and wbc_rollout_*; wbc_multi_*; late touchdown in the gait rule.
 * (normals and height from a map: "Terrain heightfield" below.) */
typedef struct wbc_stiction_params {
  size_t struct_size;     /* sizeof(wbc_stiction_params) of the caller's build */
  double k_t;             /* N/m, >= 0 and finite */
} wbc_stiction_params;
void wbc_stiction_params_default(wbc_stiction_params* p);
/* a negative or non-finite value: WBC_E_INVALID.  The value travels as a kernel argument: nothing is uploaded, later stiction calls use it.  Not inside a
 * stream capture (a captured graph keeps the value it was captured with). */
int wbc_solver_set_stiction_params(wbc_solver* s, const wbc_stiction_params* p);
int wbc_ground_stick_force_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* Jc, const void* normals, const void* height,
                                 const void* mu, void* anchor, int* stick, void* f_gr, int* contact /* may be NULL */, void* gap /* may be NULL */,
                                 void* stream);
int wbc_integrate_ground_stick_batch(wbc_solver* s, size_t N, void* q, void* v, const void* M, const void* h, const void* Jc, const void* tau,
                                     const void* normals, const void* height, const void* mu, const void* tau_ext /* may be NULL */, void* anchor,
                                     int* stick, void* f_gr, int* contact /* may be NULL */, void* gap /* may be NULL */, void* stream);

/* Contact sensing from the disturbance observer: estimated foot forces and a contact word with hysteresis.  ADDITIVE to ABI 10 (wbc_abi_version()
 * stays 10, no existing struct, call or default changes; detect it by these symbols).  The `contact` word the ground calls produce is the plant's own
 * normal force: simulator ground truth.  A controller on a robot has the momentum observer's residual r instead.  The observer's update is
 *   integ += dt (S^T tau_prev + Jc^T f_prev + beta + r),   r = K1 (M v - integ),
 * so r estimates the generalized force that acts beyond the planned Jc^T f_prev: on the ground, Jc^T (f_gr - f_prev), low-passed with the time
 * constant 1 / K1.  The joint rows of a leg see only that leg's own foot, so the estimate needs no base rows and no 12 x 12 solve.  Inputs, device
 * pointers, component-major, solver scalar type:
 *   Jc      [3 nf nv][N]  the last wbc_step_batch's out->Jc
 *   r       [nv][N]       the observer residual AFTER that step (wbc_obs_state.r)
 *   f_prev  [12][N]       the buffer that step was given as in->f_prev
 *   normals [12][N]       the tick's contact normals
 *   contact [N] int       IN/OUT.  in: bits 0-3 = the previous estimate (the caller stores 0 before the first call).  Only bits 0-3 are read or
 *                         written; the other bits are kept.
 * Per foot k, with J_leg,k the own-leg 3x3 block of Jc (the words wbc_integrate_batch and the ground calls read; the leg's joint columns come from
 * the model, so joint orders that are not leg-major work) and r_joint its three joint rows of r:
 *   A      = J_leg,k^T
 *   det    = det A
 *   ok     = |det| > det_min
 *   df     = ok ? adj(A) r_joint / det : 0      (the adjugate form: no pivoting, and no division when !ok)
 *   f_est  = f_prev,k + df
 *   fn     = n_k . f_est
 *   bit k  = !ok ? the previous bit : (the previous bit ? fn > f_off : fn > f_on)
 * Outputs: contact [N] (bits 0-3); f_est [12][N] or NULL; fn_est [4][N] or NULL; singular [N] int or NULL (bit k = !ok).
 * wbc_contact_estimate_batch evaluates the law alone.  wbc_gait_estimated_batch evaluates it and then runs wbc_gait_batch's rule on the word it has
 * just formed, in ONE launch; every output is bit for bit what wbc_contact_estimate_batch followed by wbc_gait_batch(contact = that word) gives.
 * The walking tick stays at four launches:
 *   gait_estimated -> reference_swing -> step (observer on) -> integrate_ground[_stick]
 * Both calls work under either observer_order.  With observer_order = 0 the step does not write r: the caller simply has no meaningful residual (a
 * zero r gives f_est = f_prev).  The estimate lags the true force by about 1 / K1 (20 ms = 20 ticks of 2^-10 s with the default K1 = 50); an early
 * touchdown on a 15 mm bump came 3 ticks after the plant's own bit, since the force there rises far past f_on and only the start of the lag shows.
 * The defaults
 *   f_on = 15 N,  f_off = 5 N,  det_min = 1.5e-3 m^3
 * were fixed on the CPU with the numpy restatement of this law (tests/contact_ref.py) in the walking loop of the ground plant with the observer on
 * (observer_order = 1, K1 = 50, dt = 2^-10, a 15 mm bump under one foot).  Tried, f_on / f_off: 5 / 5 (the plant's f_touch, no hysteresis) finds every
 * early touchdown the plant's own bits give, but one bit chattered 0 -> 1 -> 0 on consecutive ticks in the 16-robot loop: it did NOT pass.  10 / 5
 * does not chatter, but its smallest threshold margin is 1.9e-6 of the largest force, next to the 1e-6 the tests ask for.  15 / 5 does not chatter, finds
 * every bumped foot 3 ticks behind the plant's bit and keeps a margin of 2.2e-5.  30 / 5 finds 4 of 18 early touchdowns and the bumped feet 7 and 8 ticks late.
 * Every one of these loops stayed upright with every QP status 0.  det_min: inside the synthetic model's joint limits |det J_leg| reaches 0 (it changes
 * its sign where the leg passes through its straight posture), so the limits bound nothing; within 0.5 rad of the walking loops' standing posture on every joint it stays above
 * 1.88e-2 m^3, and 1.5e-3 leaves a factor of twelve below that.  A leg nearer to a singular posture keeps its previous bit.
 * tests/test_contact_oracle.py holds the measured figures.
 * Stream rules as for the ground calls: no allocation, no synchronisation, hipGraph-capturable; N == 0 returns WBC_OK without looking at the buffers; a
 * NULL required pointer (contact included): WBC_E_INVALID; N > max_batch: WBC_E_CAPACITY.
 * Out of scope: the base rows of r; a contact observer of its own; the rollout kernels and wbc_rollout_*; wbc_multi_*; the payload plant; late
 * touchdown in the gait rule.  (The same call on a mapped terrain: wbc_gait_estimated_terrain_batch, "Terrain heightfield" below.) */
typedef struct wbc_contact_params {
  size_t struct_size;     /* sizeof(wbc_contact_params) of the caller's build */
  double f_on, f_off;     /* N; >= 0 and finite, f_off <= f_on */
  double det_min;         /* m^3; >= 0 and finite */
} wbc_contact_params;
void wbc_contact_params_default(wbc_contact_params* p);
/* a negative or non-finite value, or f_off > f_on: WBC_E_INVALID.  The values travel as a kernel argument: nothing is uploaded, later calls use them.
 * Not inside a stream capture (a captured graph keeps the values it was captured with). */
int wbc_solver_set_contact_params(wbc_solver* s, const wbc_contact_params* p);
int wbc_contact_estimate_batch(wbc_solver* s, size_t N, const void* Jc, const void* r, const void* f_prev, const void* normals,
                               int* contact /* in/out [N] */, void* f_est /* may be NULL */, void* fn_est /* may be NULL */,
                               int* singular /* may be NULL */, void* stream);
int wbc_gait_estimated_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* Jc, const void* r, const void* f_prev,
                             const void* normals, int* contact /* in/out [N] */, void* phase /* in/out [N] */, int* mask /* in/out [N] */,
                             void* swing /* in/out [36][N] */, int* events /* may be NULL, [N] */, void* f_est /* may be NULL */, void* stream);
/* Single-robot, host-pointer, fp64 form of wbc_contact_estimate_batch (Jc[216] row-major 12 x 18, r[18], f_prev[12], normals[12] in; contact[1] in/out;
 * the optional f_est[12], fn_est[4], singular[1] out).  Synchronises. */
int wbc_compute_contact_estimate(wbc_solver* s, const double* Jc, const double* r, const double* f_prev, const double* normals, int* contact,
                                 double* f_est, double* fn_est, int* singular);

/* Terrain heightfield: per-foot planes and foothold heights on the device.  ADDITIVE to ABI 10 (wbc_abi_version() stays 10, no existing struct, call or
 * default changes; detect it by these symbols).  The step, the contact estimate and the ground calls take one plane per foot (normals [12][N],
 * height [4][N]) as caller buffers, and wbc_gait_batch puts every foothold at the single height cmd row 3.  These calls write those planes and the
 * footholds' heights from a map, so that a foot that moves meets other ground with no host work between launches.  The map: n_tiles regular grids of
 * node heights, one tile per state.  All buffers are caller-owned DEVICE memory like every batch array; the struct is read on the host at call time and
 * its scalars travel as kernel arguments: nothing is uploaded, allocated or synchronised, and every call is hipGraph-capturable (a captured graph keeps
 * the values it was captured with).
 * The host forms, in double, rounded to the solver's scalar type T and passed in:  x0, y0,  inv_cell = 1 / cell,  x_max = x0 + (nx - 1) cell,
 * y_max = y0 + (ny - 1) cell.  The law for a point (x, y) on tile t, in T, in this operation order:
 *   xc = min(max(x, x0), x_max)            yc likewise        (a point off the grid sees the tangent plane at the nearest edge point)
 *   gx = (xc - x0) inv_cell                ix = min((int)gx, nx - 2)     u = gx - ix        (gy, iy, w likewise)
 *   z00, z10, z01, z11 = nodes (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) of tile t
 *   a = z00 + u (z10 - z00)    b = z01 + u (z11 - z01)
 *   zs = a + w (b - a)
 *   zx = ((z10 - z00) + w ((z11 - z01) - (z10 - z00))) inv_cell         zy = (b - a) inv_cell
 *   n  = (-zx, -zy, 1) rsqrt(zx^2 + zy^2 + 1)                            (1 / sqrt, as the kernels normalise today)
 *   d  = n.x xc + n.y yc + n.z zs
 * zs is continuous.  n (and with it d) is piecewise: it is the normal of the cell's bilinear patch and JUMPS at cell edges.  Non-finite x, y are the
 * caller's promise, as for q; so are tile values outside [0, n_tiles).  The compiler may contract the products, so the outputs are exact only to
 * rounding -- except where u and w are exactly 0 or 1 (a point on a node of a dyadic grid): there every product in zs is exact, zs is that of the
 * same arithmetic on a CPU bit for bit, and with u = w = 0 (every node but the last row's and column's) zs is the node's own bits.
 *   wbc_terrain_sample_batch   the law at M <= max_batch caller-given points xy [2][M] (row 0 x, row 1 y; terrain->tile is then [M] or NULL):
 *                              z [M], n [3][M], d [M], each may be NULL -- for planners and tests.
 *   wbc_terrain_feet_batch     per state and foot k, p_f(q) from the leg's position chain (the arithmetic wbc_gait_batch latches p0 with; joint orders
 *                              that are not leg-major work), then the law at p_f,xy:  rows 3k .. 3k+2 of normals = n,  height[k] = d,  surf[k] = zs
 *                              (surf [4][N] may be NULL).  These are the planes wbc_step_batch, the contact estimate and the ground calls read.
 *                              mask and swing are given both or neither.  Given: for every foot whose bit of mask is CLEAR, swing word 9k+5 (p1_z) :=
 *                              zs at that plan's own (p1_x, p1_y) = words 9k+3, 9k+4.  No other swing word is touched, and feet with a set bit are
 *                              untouched bit for bit.  The rule is idempotent, so it is the same for retarget 0 and 1.
 *   wbc_gait_terrain_batch     wbc_gait_batch's arguments + terrain, normals, height, surf: ONE launch whose outputs are those of wbc_gait_batch followed
 *                              by wbc_terrain_feet_batch(mask, swing = what the gait call left).  cmd row 3 is then dead for lifted feet.
 *                              phase, mask, events and every swing word but p0 are the two launches' bit for bit (p1_z too: it is sampled at p1_x,
 *                              p1_y as read back from memory).  normals, height, surf and the p0 of a foot that lifts off in this call descend from
 *                              p_f(q), and the compiler contracts the leg chain differently in the three kernels: they agree to rounding, not to
 *                              the bit (on a walking loop's states p0 has so far come out equal; on states with joints over several turns and
 *                              attitudes over the sphere about one lifting foot in ten differs in its last bits -- tests/test_gpu_walk_edges.py).
 *   wbc_gait_estimated_terrain_batch   the same behind wbc_gait_estimated_batch.  normals is IN/OUT: the contact law reads the previous tick's
 *                              planes, then they are overwritten with this tick's (before the first tick the caller stores any unit normals).
 * The walking tick stays at four launches with no host work between them:
 *   gait[_estimated]_terrain -> reference_swing -> step -> integrate_ground[_stick]
 * with ONE normals and ONE height buffer through all four.
 * Why: on the CPU restatement of the loop (tests/terrain_ref.py; 4 robots, 512 ticks of 2^-10 s, the stiction plant, 4 tiles of 64 x 48 nodes, cell
 * 2^-6, a 0.05 ramp with a 6 mm ripple) the gap p_f,z - zs(p_f,xy) of a foot at the tick of its touchdown event stays within 0.80 mm of the
 * surface when p1_z and the normals come from the map, as on flat ground (0.61 mm), and reaches 14.9 mm when p1_z = z_g and the
 * controller's normals are e_z -- the foot is declared down while still in the air.  Every QP status is 0 in all three loops.  tests/test_terrain_oracle.py holds the measured figures.  With
 * footholds read from the map, late touchdown in the gait rule is not needed for mapped terrain.
 * A bad struct gives WBC_E_INVALID: nx or ny < 2, n_tiles < 1, a non-finite x0, y0 or cell, cell <= 0, a NULL z, a wrong struct_size, or
 * n_tiles ny nx >= 2^28 nodes (every node is reached by a 32-bit byte offset).
 * Stream rules as for the gait calls: N == 0 (M == 0) returns WBC_OK without looking at anything; a NULL required pointer (terrain included; mask
 * without swing or swing without mask): WBC_E_INVALID; then the struct's own checks; N > max_batch: WBC_E_CAPACITY -- all before the device is touched.
 * There is no single-robot host-pointer form: the grid would have to be uploaded inside the call.
 * Out of scope: the rollout kernels and wbc_rollout_*; wbc_multi_*; the payload plant; late touchdown in the gait rule; choosing footholds by terrain
 * quality (avoiding edges and slopes); smoothed (C1) normals; terrain sensing or estimation: the map is given. */
typedef struct wbc_terrain {
  size_t struct_size; /* sizeof(wbc_terrain) of the caller's build */
  int nx, ny;         /* nodes per row, rows; each >= 2 */
  int n_tiles;        /* >= 1 */
  double x0, y0;      /* world x, y of node (0, 0); finite */
  double cell;        /* node spacing, m; > 0, finite */
  const void* z;      /* DEVICE, solver scalar type, [n_tiles][ny][nx]: z[(t ny + iy) nx + ix] = height at (x0 + ix cell, y0 + iy cell) */
  const int* tile;    /* DEVICE [N] (or [M]) or NULL = tile 0 for every state; values in [0, n_tiles) are the caller's promise */
} wbc_terrain;
int wbc_terrain_sample_batch(wbc_solver* s, const wbc_terrain* terrain, size_t M, const void* xy, void* z /* may be NULL */, void* n /* may be NULL */,
                             void* d /* may be NULL */, void* stream);
int wbc_terrain_feet_batch(wbc_solver* s, const wbc_terrain* terrain, size_t N, const void* q, const int* mask /* may be NULL */,
                           void* swing /* in/out [36][N]; NULL with mask */, void* normals /* out [12][N] */, void* height /* out [4][N] */,
                           void* surf /* may be NULL, [4][N] */, void* stream);
int wbc_gait_terrain_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const int* contact /* may be NULL */,
                           void* phase /* in/out [N] */, int* mask /* in/out [N] */, void* swing /* in/out [36][N] */, int* events /* may be NULL, [N] */,
                           const wbc_terrain* terrain, void* normals /* out [12][N] */, void* height /* out [4][N] */, void* surf /* may be NULL */,
                           void* stream);
int wbc_gait_estimated_terrain_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* Jc, const void* r,
                                     const void* f_prev, void* normals /* in/out [12][N] */, int* contact /* in/out [N] */, void* phase /* in/out [N] */,
                                     int* mask /* in/out [N] */, void* swing /* in/out [36][N] */, int* events /* may be NULL, [N] */,
                                     void* f_est /* may be NULL */, const wbc_terrain* terrain, void* height /* out [4][N] */,
                                     void* surf /* may be NULL */, void* stream);

/* Foothold selection: a terrain cost map and a per-foot search on the device.  ADDITIVE to ABI 10 (wbc_abi_version() stays 10, no existing struct, call,
 * default or kernel output changes; detect it by these symbols).  The terrain calls above give a lifted foot the height of its foothold; the foothold
 * itself lands wherever the gait rule puts it, on an edge as readily as on a flat spot.  These calls move it to a nearby node of the map that is cheap.
 * Cost map, wbc_terrain_cost_batch: one launch per map at set-up time.  cost is caller-owned DEVICE memory [n_tiles][ny][nx] of the solver's scalar
 * type, laid out like terrain->z.  Per node c = (ix, iy) of a tile, in T, no product contracted:
 *   step   = max over |dx|, |dy| <= margin of |z(clip(ix+dx), clip(iy+dy)) - z(c)|        (indices clipped to the grid; subtraction, abs and max
 *                                                                                           only: exact)
 *   sx     = (z(ix+1, iy) - z(ix-1, iy)) inv_cell / 2;  at ix = 0 and ix = nx-1 the difference is one-sided and multiplied by inv_cell alone
 *   sy     likewise;   slope2 = sx^2 + sy^2
 *   cost   = w_step step + w_slope slope2
 * Selection law, per state and foot k, behind the gait rule of the same tick.  Caller-owned state, advanced in place:
 *   hold  [8][N]   rows 2k, 2k+1 = the latched x, y of foot k.  Needs no initial value.
 *   latch [N] int  in: bit k = foot k has a latched foothold (only bits 0-3 are read; the caller stores 0 before the first tick).
 *                  out: bits 0-3 = the new latches, bit 4+k = foot k was selected THIS tick.
 * With `bit` the foot's bit of mask and sw its nine plan words (x = sw[3], y = sw[4] as the gait rule left them):
 *   bit set (stance)         latch bit k := 0; nothing else is touched
 *   lifted and latched       sw[3], sw[4] := hold; no search.  A POINT is latched, not an offset: with retarget = 1 the nominal foothold drifts by more
 *                            than half a cell during a swing, and a latched offset put 25 % / 59 % of the touchdowns of the loops below on costly nodes
 *   lifted, not latched      jx = clamp((int)floor((x - x0) inv_cell + 0.5), 0, nx-1), jy likewise: the nearest node;  c0 = cost[jx, jy]
 *                            c0 <= cost_ok, or sw[8] > u_max sw[7] (too late in the swing to move the target), or radius = 0: the foot is KEPT -- no
 *                            word is written, it is not latched, and it is examined again next tick
 *                            otherwise scan iy = jy-R .. jy+R (outer, ascending), ix = jx-R .. jx+R (inner, ascending), each range clipped to the grid:
 *                              xc = x0 + ix cell,  yc = y0 + iy cell,  J = cost[ix, iy] + w_dist ((xc - x)^2 + (yc - y)^2)
 *                            and take the first candidate with strictly smaller J (if no node of the window is below cost_ok the minimum is still
 *                            taken).  hold := (xc, yc); sw[3], sw[4] := hold; latch bit k := 1; bit 4+k := 1
 * p1_z (word 5) is written afterwards by the terrain rule of wbc_terrain_feet_batch at the plan's own (p1_x, p1_y); a selected foothold is a node, so on
 * a dyadic grid p1_z is that node's own bits.  x0, y0 and cell arrive rounded to T; on a dyadic grid xc, yc are exact.
 *   wbc_foothold_select_batch               the law alone, on mask and swing as a gait call left them
 *   wbc_gait_terrain_select_batch           wbc_gait_terrain_batch's arguments + cost, hold, latch: ONE launch whose outputs are those of wbc_gait_batch,
 *                                           then wbc_foothold_select_batch, then wbc_terrain_feet_batch(mask, swing) -- bit for bit, but for normals,
 *                                           height and surf, which are wbc_gait_terrain_batch's own bits (they agree with wbc_terrain_feet_batch's
 *                                           to rounding, as that call's do), and for the p0 of a foot that lifts off in this call, which descends
 *                                           from p_f(q) as they do and agrees with wbc_gait_batch's to rounding.  With radius = 0 and no latch bit set its other outputs are
 *                                           wbc_gait_terrain_batch's bit for bit.
 *   wbc_gait_estimated_terrain_select_batch the same behind wbc_gait_estimated_batch
 * The walking tick stays at four launches with no host work between them:
 *   gait[_estimated]_terrain_select -> reference_swing -> step -> integrate_ground[_stick]
 * Per tick the common path costs one gather of cost per lifted foot; the window (at most 81 gathers) runs only in the lanes that start a selection.
 * The defaults
 *   radius = 3, margin = 1, w_step = 1, w_slope = 2^-7, w_dist = 4 (1/m), cost_ok = 8.75e-3, u_max = 0.75
 * were fixed on the CPU with the numpy restatement of this law (tests/foothold_ref.py) in the walking loop of tests/terrain_ref.py (4 robots, 512 ticks
 * of 2^-10 s, the stiction plant, 4 tiles of 64 x 48 nodes, cell 2^-6).  radius, margin, w_step, w_dist and u_max are the prototype's.  The rule for the
 * other two: on that file's "flat" ground and "tiles" (the rippled ramps) no node a foot is ever aimed at may exceed cost_ok, so that those loops
 * reproduce the loops without selection bit for bit; cost_ok is the largest cost aimed at there times 1.5, and it must lie below half the cost of a
 * ridge-adjacent node of the test terrain (flat ground + 2 cm ridges along y every 8 or every 4 cells: 0.02, so below 0.01).  Tried, w_slope -> the
 * largest cost aimed at on the tiles -> times 1.5:  0 -> 5.024e-3 -> 7.54e-3;  2^-7 -> 5.832e-3 -> 8.75e-3;  2^-6 -> 6.639e-3 -> 9.96e-3 (0.4 % below the
 * bound);  2^-5 -> 8.255e-3 -> 1.24e-2 (fails).  2^-7 is the largest that keeps a margin (12.5 %).  On flat ground every cost is 0.
 * With these, in the loops on the ridges (32 touchdowns each, every QP status 0): touchdowns on a node whose 3 x 3 neighbourhood holds a height step
 * fall from 41 % to 0 (ridges every 8 cells) and from 84 % to 0 (every 4 cells; without selection one robot there walks 1.7 cm forward and 2.8 cm
 * sideways and another 8.2 cm forward with its base down to 0.386 m; with it all four walk 4.5 .. 4.9 cm, within 2.2 mm sideways, base 0.398 .. 0.407 m).
 * The latest selection starts at u = 0.48, the largest move of a foothold is 2.97 cm, and the smallest relative gap between the best and the second-best
 * candidate is 1.7e-4 / 4.0e-3.
 * tests/test_foothold_oracle.py holds the measured figures.
 * wbc_foothold_params: a negative or non-finite value, u_max > 1, radius outside 0..4 or margin outside 0..2 gives WBC_E_INVALID.  The values travel as
 * kernel arguments: nothing is uploaded, later calls use them; a cost map is as good as the w_step, w_slope and margin it was made with.  Not inside a
 * stream capture (a captured graph keeps the values it was captured with).
 * Stream rules as for the terrain calls: no allocation, no synchronisation, hipGraph-capturable; N == 0 returns WBC_OK without looking at anything
 * (wbc_terrain_cost_batch has no N); a NULL required pointer (terrain, cost, hold, latch included): WBC_E_INVALID; then the terrain struct's own checks;
 * N > max_batch: WBC_E_CAPACITY -- all before the device is touched.  There is no single-robot host-pointer form, for the terrain calls' reason.
 * Out of scope: the rollout kernels and wbc_rollout_*; wbc_multi_*; late touchdown; terrain sensing; smoothed normals; kinematic reachability of the
 * chosen node (it lies at most radius cells, 4 at the most, from the gait rule's foothold in x and in y: the caller sizes radius * cell to the leg). */
typedef struct wbc_foothold_params {
  size_t struct_size;   /* sizeof(wbc_foothold_params) of the caller's build */
  int radius;           /* R, cells: 0 .. 4; 0 = never select */
  int margin;           /* the step term's neighbourhood, cells: 0 .. 2 */
  double w_step, w_slope, w_dist;   /* >= 0 and finite; per m, per 1, per m (w_dist multiplies a squared distance) */
  double cost_ok;       /* >= 0 and finite: a nearest node at most this costly is kept */
  double u_max;         /* 0 .. 1: no selection starts later than this share of the swing */
} wbc_foothold_params;
void wbc_foothold_params_default(wbc_foothold_params* p);
int wbc_solver_set_foothold_params(wbc_solver* s, const wbc_foothold_params* p);
int wbc_terrain_cost_batch(wbc_solver* s, const wbc_terrain* terrain, void* cost /* out [n_tiles][ny][nx] */, void* stream);
int wbc_foothold_select_batch(wbc_solver* s, const wbc_terrain* terrain, const void* cost, size_t N, const int* mask, void* swing /* in/out [36][N] */,
                              void* hold /* in/out [8][N] */, int* latch /* in/out [N] */, void* stream);
int wbc_gait_terrain_select_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const int* contact /* may be NULL */,
                                  void* phase /* in/out [N] */, int* mask /* in/out [N] */, void* swing /* in/out [36][N] */,
                                  int* events /* may be NULL, [N] */, const wbc_terrain* terrain, void* normals /* out [12][N] */,
                                  void* height /* out [4][N] */, void* surf /* may be NULL */, const void* cost, void* hold /* in/out [8][N] */,
                                  int* latch /* in/out [N] */, void* stream);
int wbc_gait_estimated_terrain_select_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* Jc, const void* r,
                                            const void* f_prev, void* normals /* in/out [12][N] */, int* contact /* in/out [N] */,
                                            void* phase /* in/out [N] */, int* mask /* in/out [N] */, void* swing /* in/out [36][N] */,
                                            int* events /* may be NULL, [N] */, void* f_est /* may be NULL */, const wbc_terrain* terrain,
                                            void* height /* out [4][N] */, void* surf /* may be NULL */, const void* cost, void* hold /* in/out [8][N] */,
                                            int* latch /* in/out [N] */, void* stream);

/* Base state from leg odometry: estimated rows 0-2 of q and v for the walking tick.  ADDITIVE to ABI 10 (wbc_abi_version() stays 10, no existing struct,
 * call, default or kernel output changes; detect it by these symbols).  Every launch of the tick reads the base position q[0..2] and the base linear
 * velocity v[0..2]: on a simulator the plant's own, on a robot nobody's.  A controller has joint encoders, an attitude and a gyro (the quaternion rows
 * of q, the angular rows of v) and the contact word it forms itself.  A loaded stance foot does not move, so it measures the trunk's velocity through
 * its leg's Jacobian and the trunk's position through its leg's forward kinematics.  All arithmetic in the solver's scalar type T, per state.
 * Inputs, device pointers, component-major:
 *   q       [nq][N]   the sensor state: rows 3-6 the attitude (any non-zero quaternion: the law normalises it before it forms R), rows 7.. the joint
 *                     angles.  Rows 0-2 are NEVER read.
 *   v       [nv][N]   rows 3-5 the world angular velocity, rows 6.. the joint rates.  Rows 0-2 are NEVER read.
 *   contact [N] int   bits 0-3: foot k senses ground (the estimated word of wbc_contact_estimate_batch, or the plant's)
 *   mask    [N] int   bits 0-3: the previous tick's stance mask
 *   normals [12][N], height [4][N]   the planes the step, the contact estimate and the ground calls read; given together, or both NULL
 * Caller-owned state, advanced in place:
 *   base    [6][N]    rows 0-2 p^, rows 3-5 v^.  The caller stores the start state.
 *   anchor  [12][N]   rows 3k .. 3k+2 = the world point foot k stands on.  Needs no initial value.
 *   odo     [N] int   in: bit k = foot k has an anchor (only bits 0-3 are read; the caller stores 0 before the first tick).
 *                     out: bits 0-3 = the new anchors, bit 4+k = foot k was anchored THIS tick.
 * Outputs: q_est [nq][N], v_est [nv][N]: rows 0-2 are p^ and v^, every other row is the input's bits.  They may be q and v themselves: the rows from
 * 3 on are then not written.
 * Per foot k, from the leg chain and velocity recursion of wbc_swing_reference_batch (d_k the foot point and vf_k its velocity in base coordinates
 * with the base origin at rest, the base turning with R^T omega; the leg's joint columns come from the model, so joint orders that are not leg-major
 * work):
 *   lever_k = R d_k       u_k = R vf_k  (the foot's velocity relative to the base origin's)
 *   S_k = contact bit k && mask bit k      cnt = |S|      inv[c] = T(1) / T(c)
 * Velocity:  cnt > 0:  vm = -((u_0 + u_1) + (u_2 + u_3)) inv[cnt], the terms of feet outside S selected to exact 0 (not multiplied);
 *                      v^ := v^ + a_v (vm - v^).       cnt = 0:  v^ is kept.
 * Position:  p_pred = p^ + dt v^  (the new v^; dt is the solver's).  A = S && the in-bits of odo.
 *            A != {}:  pm = ((x_0 + x_1) + (x_2 + x_3)) inv[|A|] with x_k = anchor_k - lever_k (exact 0 outside A);  p^ := p_pred + a_p (pm - p_pred).
 *            A == {}:  p^ := p_pred.
 * Anchors:   k in S without an anchor:  x = p^ + lever_k (the new p^);  with planes, x := x - n_k (n_k . x - height_k);  anchor_k := x, bit k := 1,
 *                                       bit 4+k := 1
 *            k in S and A:              its three anchor words are untouched, bit for bit; bit k stays 1
 *            k not in S:                bit k := 0, its anchor words untouched (and never read: they may hold anything)
 * odo, the copied rows and every untouched word are EXACT.  p^, v^ and new anchors are exact only to rounding: the compiler may contract products.
 *   wbc_base_estimate_batch        the law alone
 *   wbc_gait_estimated_odom_batch  wbc_gait_estimated_batch's arguments + height (may be NULL: no planes), base, anchor, odo, q_est, v_est: ONE launch
 *                                  that evaluates (1) this law on contact and mask AS LOADED -- the previous tick's words, read before anything
 *                                  overwrites them -- (2) the contact law, (3) the gait rule on the ESTIMATED base rows, held in registers.  Its
 *                                  outputs are those of wbc_base_estimate_batch followed by wbc_gait_estimated_batch(q_est, v_est).
 *   wbc_compute_base_estimate      the single-robot, host-pointer, fp64 form (q[19], v[18], the two words, normals[12] and height[4] or both NULL in;
 *                                  base[6], anchor[12], odo[1] in/out; q_est[19], v_est[18] out).  Synchronises.
 * The walking tick becomes
 *   gait_estimated_odom -> reference_swing(q_est, v_est) -> step(q_est, v_est; observer on) -> integrate_ground[_stick](the true q, v)
 * still four launches with no host work between them, and none of the first three reads a base row of the plant's state.
 * The defaults
 *   a_v = 2^-3,  a_p = 2^-2
 * were fixed on the CPU with the numpy restatement of this law (tests/odom_ref.py) in the walking loop of the stiction plant (tests/stick_ref.py's
 * walk_case: 4 robots, 512 ticks of 2^-10 s, a 15 mm bump under one foot, command 0.1 m/s), the controller links given q_est, v_est and the plant the
 * truth.  The ground is a penalty spring: a loaded foot sinks m g / (2 k_n), about 5 mm, and moves while it does, so raw odometry (a_v = a_p = 1) is
 * noisy and an anchor taken where the foot touched leaves z one penetration depth low at every step; the blend and the drop of a new anchor onto
 * the foot's known plane remove both.  What remains is a bounded bias of about one penetration depth: the estimate reads high, so the trunk rides a
 * few mm low.  The vertical velocity stays rough (this law has no accelerometer).
 * Measured there (every QP status 0 in every loop but where said; the loop on the true state walks 4.95 .. 5.12 cm and ends at base z 0.4024 .. 0.4033 m):
 *   a_v / a_p       forward travel       base z at the end      worst |p^ - p| x / y / z     rms v error x / y / z
 *   2^-3 / 2^-2     3.47 .. 5.41 cm      0.3937 .. 0.4103 m     31.3 / 5.7 / 8.9 mm          0.063 / 0.033 / 0.063 m/s     (the defaults)
 *   2^-4 / 2^-2     3.16 .. 4.22 cm      0.3953 .. 0.4102 m     28.7 / 5.5 / 9.3 mm          0.059 / 0.033 / 0.069
 *   2^-2 / 2^-2     3.69 .. 5.37 cm      0.3944 .. 0.4101 m     34.9 / 6.6 / 8.4 mm          0.069 / 0.034 / 0.073; worst v error 0.72 m/s (defaults: 0.38)
 *   2^-3 / 2^-1     3.51 .. 5.57 cm      0.3935 .. 0.4108 m     33.1 / 6.5 / 8.9 mm          0.063 / 0.032 / 0.063
 *   2^-3 / 2^-3     3.65 .. 5.32 cm      0.3940 .. 0.4096 m     29.4 / 5.4 / 8.8 mm          0.062 / 0.032 / 0.063
 *   1 / 1 (raw)     17.9 .. 25.4 cm      0.495 .. 0.527 m       114 / 123 / 608 mm           3.1 / 3.3 / 4.3; did NOT pass: the estimate runs away (v error up to 105 m/s)
 *   2^-3 / 2^-2 without planes:  0.74 .. 4.27 cm, z^ reads 15 .. 19 mm high at the end and keeps the penetration of every step: did NOT pass
 * No dyadic neighbour of the start values is better in travel and in error at once, so they stay.  The x error is larger than the y and z errors because
 * it is taken at touchdowns: the foot that meets the 15 mm bump lands early, carries 40 N and slides at 0.5 .. 0.2 m/s for thirty ticks while both
 * words call it down, and the estimated word of a foot the schedule has just put down carries its planned force, so its bit is set a tick or two
 * before the foot is.  With the plant's own word in place of the estimated one the figures are 3.02 .. 5.57 cm, 38.0 / 5.7 / 7.7 mm.
 * Both gains are dyadic, so the blends' products are exact.  tests/test_odom_oracle.py holds the measured figures.
 * wbc_odom_params: a_v outside (0, 1], a_p outside [0, 1] or a non-finite value gives WBC_E_INVALID.  The values travel as kernel arguments: nothing is
 * uploaded, later calls use them.  Not inside a stream capture (a captured graph keeps the values it was captured with).
 * Stream rules as for the contact calls: no allocation, no synchronisation, hipGraph-capturable; N == 0 returns WBC_OK without looking at the buffers; a
 * NULL required pointer, or normals without height (or the reverse): WBC_E_INVALID; N > max_batch: WBC_E_CAPACITY -- all before the device is touched.
 * Out of scope: an accelerometer or a Kalman covariance; attitude estimation; compensating the penetration bias from f_est; the terrain and
 * foothold-select fused variants (a caller there runs wbc_base_estimate_batch as a fifth launch); the rollout kernels and wbc_rollout_*; wbc_multi_*. */
typedef struct wbc_odom_params {
  size_t struct_size;   /* sizeof(wbc_odom_params) of the caller's build */
  double a_v;           /* the velocity blend: 0 < a_v <= 1 */
  double a_p;           /* the position blend: 0 <= a_p <= 1 (0 = dead reckoning on v^) */
} wbc_odom_params;
void wbc_odom_params_default(wbc_odom_params* p);
int wbc_solver_set_odom_params(wbc_solver* s, const wbc_odom_params* p);
int wbc_base_estimate_batch(wbc_solver* s, size_t N, const void* q, const void* v, const int* contact, const int* mask,
                            const void* normals /* may be NULL with height */, const void* height /* may be NULL with normals */,
                            void* base /* in/out [6][N] */, void* anchor /* in/out [12][N] */, int* odo /* in/out [N] */, void* q_est /* out [nq][N] */,
                            void* v_est /* out [nv][N] */, void* stream);
int wbc_gait_estimated_odom_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* Jc, const void* r,
                                  const void* f_prev, const void* normals, int* contact /* in/out [N] */, void* phase /* in/out [N] */,
                                  int* mask /* in/out [N] */, void* swing /* in/out [36][N] */, int* events /* may be NULL, [N] */,
                                  void* f_est /* may be NULL */, const void* height /* may be NULL */, void* base /* in/out [6][N] */,
                                  void* anchor /* in/out [12][N] */, int* odo /* in/out [N] */, void* q_est /* out [nq][N] */,
                                  void* v_est /* out [nv][N] */, void* stream);
int wbc_compute_base_estimate(wbc_solver* s, const double* q, const double* v, int contact, int mask, const double* normals /* may be NULL with height */,
                              const double* height, double* base, double* anchor, int* odo, double* q_est, double* v_est);

/* Trunk reference from the velocity command: turning, leash, terrain posture.  ADDITIVE to ABI 10 (wbc_abi_version() stays 10, no existing struct,
 * default or kernel changes; the feature is detected by these symbols).  wbc_reference[_swing]_batch track plan [12][N], a quintic between two points
 * with one fixed quat_des that the host writes.  These calls form the trunk's reference on the device from the cmd buffer the gait call reads
 * (rows 0-2: vx, vy in the heading frame, wz; row 3 is not read) and from the normals / height planes the terrain call writes (on flat ground:
 * (0, 0, 1) and the ground's height), and advance a small per-robot state in place.  The walking tick becomes
 *     gait[_estimated][_terrain[_select]] -> reference_cmd_swing -> step -> integrate_ground[_stick]
 * still four launches; with q_est, v_est of the odometry call it reads no base row of the plant.
 *   trunk [WBC_TRUNK_WORDS][N], solver scalar type, component-major, caller-owned, advanced IN PLACE:
 *     0,1 x, y of the reference CoM   2 psi, reference heading in (-pi, pi]   3 z_s, support height at (x, y)   4,5 s_x, s_y, support slopes dz/dx, dz/dy
 *   To start a robot pass reset [N] non-zero for it in its first call (trunk's words are then not read, except z_s where no foot plane qualifies), or
 *   store x, y = the CoM, psi = the heading, z_s = the ground's height under it and zero slopes.
 *   ref [WBC_TRUNKREF_WORDS][N], optional output: c_ref (3), cd_ref (3), quat_des (x, y, z, w).
 * The law, per state, in the solver's scalar type T, in this order.  dt is the solver's control period; dt, pi, 2 pi and cos(yaw_leash) are formed on
 * the host in double and rounded to T.  c, cd: the CoM position and velocity of (q, v) as wbc_reference_batch forms them.  p_f,k: foot k's world
 * position from the leg's position chain (origins down the leg in base coordinates, as the gait call latches p0).  h_r = (R00, R10) normalised: the
 * trunk's heading, as in the gait call.
 *   0 reset (where reset is given and non-zero): (x, y) := c_xy; psi := atan2(h_r,y, h_r,x); step 3 runs with a_s = 1 -- as assignments, z_s := z*,
 *     s_x := b, s_y := c, so that no word of trunk is read (it may hold anything, NaN included) -- and the slopes become 0 if there is no fit (also
 *     with no qualifying foot at all; z_s is then kept as given: the one word a reset can read).
 *   1 heading: psi+ = psi + wz dt; g(a) = h_r . (cos a, sin a); the heading advances iff g(psi+) >= cos(yaw_leash) or g(psi+) >= g(psi), and then
 *     w_des_z = wz; otherwise psi+ = psi and w_des_z = 0.  Then the wrap: psi+ > pi subtracts 2 pi, psi+ <= -pi adds 2 pi.
 *   2 position: v_w = Rz(psi+)(vx, vy); (x+, y+) = (x, y) + v_w dt; e = (x+, y+) - c_xy; |e|^2 > leash^2: (x+, y+) = c_xy + e leash rsqrt(|e|^2).
 *   3 support plane under the four feet (lifted ones too: the terrain call writes a plane under each): w_k = (n_k,z >= nz_min);
 *     zs_k = (d_k - n_k,x p_f,x - n_k,y p_f,y) / n_k,z, the surface height under the foot; m = sum w_k.
 *     m >= 1: means xb, yb, zb over those feet, centred sums Sxx, Sxy, Syy, Sxz, Syz, det = Sxx Syy - Sxy^2.
 *     m >= 3 and det > det_min: b = (Syy Sxz - Sxy Syz) / det, c = (Sxx Syz - Sxy Sxz) / det; s_x += a_s (b - s_x), s_y += a_s (c - s_y);
 *       z* = zb + b (x+ - xb) + c (y+ - yb).
 *     m >= 1 otherwise (two feet, collinear feet): the slopes are held; z* = zb + s_x (x+ - xb) + s_y (y+ - yb).
 *     m = 0: z_s, s_x, s_y are held.                                 In the first three cases z_s += a_s (z* - z_s).
 *   4 reference: c_ref = (x+, y+, z_s + height); cd_ref = (v_w, s_x v_w,x + s_y v_w,y); cdd_ref = 0.
 *   5 desired attitude: n = (-tilt s_x, -tilt s_y, 1) normalised; q_tilt = (-n_y, n_x, 0, 1 + n_z) normalised, the shortest rotation that takes e_z
 *     to n (no branch: n_z > 0); q_yaw = (0, 0, sin psi+/2, cos psi+/2); quat_des = q_tilt (x) q_yaw.  quat_des takes e_z to n exactly.  The trunk's
 *     x axis then has heading psi+ exactly where the slope lies along or across the heading, and within (1 - cos theta) / (2 cos theta) ~ theta^2 / 4
 *     rad of it otherwise (theta = the lean angle: 0.01 rad on a 0.2 slope).
 *   6 outputs: a_cmd = kp_com o (c_ref - c) + kd_com o (cd_ref - cd); alpha_cmd = kp_rot o e_R + kd_rot o ((0, 0, w_des_z) - omega), e_R and omega
 *     as wbc_reference_batch forms and reads them; the joint posture rows, F and w_des as there, with the solver's wbc_ref_params
 *     (wbc_solver_set_ref_params must have been called).  In the fused call the swing law follows as in wbc_reference_swing_batch, at t = 0 (the gait
 *     call wrote t0).
 *   7 trunk is stored, and ref if given.
 * Exact words: psi and w_des_z where the heading is held; z_s, s_x, s_y bit for bit where m = 0, and s_x, s_y bit for bit where there is no fit
 * (in a reset: exactly 0).  The device forms every product of steps 0-6 (p_f included) unfused, in both kernels; it differs
 * from another evaluation of the law only by its sin / cos / atan2 / rsqrt and by the fused products inside c and cd: every other word holds to
 * rounding.
 * wbc_reference_cmd_swing_batch is ONE launch in both scalar types.  Its trunk, ref, w_des, com, base rows and stance-leg rows are bit-identical to
 * wbc_reference_cmd_batch's; the swing rows equal wbc_reference_cmd_batch followed by wbc_swing_reference_batch (t = 0) to rounding.
 * How the defaults were fixed: on the CPU, in the two loops of tests/trunk_ref.py (gait -> terrain planes -> this law -> swing law -> tick -> the
 * stiction plant, dt 2^-10; tests/test_trunk_oracle.py holds the figures).  Loop A, 4 robots on flat ground, vx 0.1, wz 0.5, 1 024 ticks: the trunk
 * yaws 0.494 rad of 0.5 commanded (the plan-driven loop: 0.007, and its CoM stops after 0.049 m where this one walks 0.097 of 0.1); |c_ref - c| <= 5.9
 * mm; the CoM 1.8 .. 4.6 mm above `height` over the support.  Loop B, 2 robots, vx 0.15, 6 144 ticks, flat ground into a 0.2 ramp: the fitted slope
 * goes 0 -> 0.200, pitch settles at -0.172 rad, the CoM stays 0.5 .. 8.1 mm above `height` over the fitted support, |c_ref - c| <= 12.3 mm, the CoM
 * travels 0.888 m of 0.9 and climbs 0.115 m.  Every QP status 0 in both.  Tried: a_s 2^-3 and 2^-7 (loop B within 0.5 mm / 0.0004 rad of 2^-5:
 * kept); tilt 0 and 0.5 (pitch -0.007 / -0.090, every status 0: 1 kept, the trunk parallel to its support); leash 0.004 (acts: 2 mm less path in
 * loop A; 0.05 never acts in either loop and is a guard against a stuck robot, not a tracking term); yaw_leash 0.01 and 0.002 (hold the heading in
 * 784 and 2 584 of 4 096 robot-ticks, yaw 0.398 / 0.183 rad; 0.5 never holds).  The issue's starting values stood.
 * wbc_trunk_params: height non-finite; leash <= 0 or NaN (+inf is allowed: no leash); yaw_leash outside (0, pi]; a_s or tilt outside [0, 1]; nz_min
 * outside (0, 1]; det_min <= 0 or non-finite; a struct_size too small: WBC_E_INVALID.  The bounds hold in the solver's scalar type: on an fp32 solver a
 * leash, nz_min or det_min that rounds to 0, or a det_min or height that overflows, is refused as well.  The values travel as a kernel argument: nothing is uploaded,
 * later calls use them.  Not inside a stream capture (a captured graph keeps the values it was captured with).
 * Stream rules as for wbc_reference_swing_batch: no allocation, no synchronisation, hipGraph-capturable; N == 0 returns WBC_OK without looking at
 * anything; a NULL required pointer: WBC_E_INVALID; N > max_batch: WBC_E_CAPACITY -- all before the device is touched.
 * wbc_compute_reference_cmd: the single-robot host-pointer form (fp64 solvers; synchronises); trunk[6] in/out.
 * Out of scope: the rollout kernels and wbc_rollout_*; wbc_multi_*; a pitch/roll-rate feed-forward; a convex-MPC force plan; CoM references shaped by
 * the gait phase. */
#define WBC_TRUNK_WORDS 6
#define WBC_TRUNKREF_WORDS 10
typedef struct wbc_trunk_params {
  size_t struct_size;   /* sizeof(wbc_trunk_params) of the caller's build */
  double height;        /* CoM height above the support, m, finite */
  double leash;         /* m, > 0 (may be +inf): the reference CoM stays within this distance of the CoM */
  double yaw_leash;     /* rad, 0 < yaw_leash <= pi: the reference heading is not advanced further away from the trunk's than this */
  double a_s;           /* 0 <= a_s <= 1: per-tick blend of the support plane */
  double tilt;          /* 0 <= tilt <= 1: share of the support slope the trunk leans with */
  double nz_min;        /* 0 < nz_min <= 1: a foot plane flatter than this in n_z is left out of the support */
  double det_min;       /* m^4, > 0: smallest determinant of the fit */
} wbc_trunk_params;
void wbc_trunk_params_default(wbc_trunk_params* p);
int wbc_solver_set_trunk_params(wbc_solver* s, const wbc_trunk_params* p);
int wbc_reference_cmd_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* normals, const void* height,
                            const int* reset /* may be NULL, [N] */, void* trunk /* in/out [6][N] */, void* w_des, void* vdot_des,
                            void* com /* may be NULL */, void* ref /* may be NULL, [10][N] */, void* stream);
int wbc_reference_cmd_swing_batch(wbc_solver* s, size_t N, const void* q, const void* v, const void* cmd, const void* normals, const void* height,
                                  const int* reset /* may be NULL, [N] */, void* trunk /* in/out [6][N] */, const int* mask, const void* swing,
                                  void* w_des, void* vdot_des, void* com /* may be NULL */, void* ref /* may be NULL */, void* foot /* may be NULL */,
                                  void* stream);
int wbc_compute_reference_cmd(wbc_solver* s, const double* q, const double* v, const double* cmd, const double* normals, const double* height,
                              int reset, double* trunk, double* w_des, double* vdot_des, double* com /* may be NULL */, double* ref /* may be NULL */);

/* Single-robot, host-pointer, double-precision convenience call: the shape of the reference's
 * one-robot tick (BASELINE.json configs[0]).  Runs wbc_step_batch with N = 1 on the GPU and
 * synchronises.  obs_integ/obs_r (host, nv each) are in/out and may be NULL when the observer is off. */
int wbc_compute_torques(wbc_solver* s, const double* q, const double* v, const double* w_des,
                        const double* vdot_des, const double* normals, const double* mu, int mask,
                        const double* tau_prev, const double* f_prev, double* obs_integ, double* obs_r,
                        double* tau, double* f, int* status);

/* The single-robot loop without staging copies (fp64 solvers): wbc_one_map hands out HOST pointers into the solver's pinned
 * image -- the caller keeps q, v, references, terrain and the observer state there and rewrites only what changed -- and
 * wbc_one_tick runs one tick on the image in place and returns when tau, f, status, iters (and the updated observer state) are
 * in it.  The wait follows wbc_solver_options.one_zerocopy (2: polled ticket, no hipStreamSynchronize).  Stands for the same
 * per-tick entry point as wbc_compute_torques (name [UNVERIFIED]); one solver = one robot = one image. */
typedef struct wbc_one_image {
  double *q, *v, *w_des, *vdot_des, *normals, *mu, *tau_prev, *f_prev, *obs_integ, *obs_r;   /* inputs (observer state: in/out) */
  double *tau, *f;                                                                           /* outputs */
  int *mask, *status, *iters;
} wbc_one_image;
int wbc_one_map(wbc_solver* s, wbc_one_image* img);
int wbc_one_tick(wbc_solver* s);

/* Observer start-up for the single-robot host-pointer loop (see wbc_observer_state): writes integ = M(q) v and r = 0
 * (host arrays of nv doubles).  Synchronises. */
int wbc_observer_init(wbc_solver* s, const double* q, const double* v, double* obs_integ, double* obs_r);

/* Single-robot, host-pointer form of wbc_reference_batch (q[19], v[18], plan[12] in; w_des[6], vdot_des[18] and the
 * optional com[6] out): the planner call of a one-robot control loop.  Synchronises. */
int wbc_compute_reference(wbc_solver* s, const double* q, const double* v, const double* plan, double t,
                          double* w_des, double* vdot_des, double* com);

/* ---- measurement: per-kernel HIP-event timing on the stream the kernels are launched on (wbc_solver_options.timing_mode:
 * the dispatch's own start / stop events, or an event pair recorded around the launch).  Enabling allocates a ring of
 * 4096 event pairs once; samples beyond it are dropped until wbc_solver_collect_timing drains the ring, so a tick never
 * allocates.  While timing is on, the instrumented dispatches are not hipGraph-capturable. ---- */
int wbc_solver_enable_timing(wbc_solver* s, int on); /* 0 off; 1 every kernel launch; k > 1: every k-th tick */
#define WBC_TIMING_KINDS 6   /* kinds this build knows */
/* synchronises the recorded events; returns summed milliseconds and launch counts since the last reset, indexed
 * 0 = dyn_sweep kernel, 1 = QP kernel, 2 = rnea_step kernel (no-M/h/Jc ticks) / stand-alone observer kernel,
 * 3 = fused tick kernel (sweep + QP of small batches in one launch), 4 = per-lane QP kernel (then 1 = the dense kernel's
 * pass over the states the per-lane kernel handed over), 5 = persistent rollout kernel (one launch = a whole horizon); resets the accumulators. */
int wbc_solver_collect_timing_n(wbc_solver* s, double* ms, int* launches, int cap /* entries of ms / launches: at most cap are written */);
/* the unsized call of ABI <= 6: writes FIVE entries (kinds 0 .. 4), what every version of it has written; use the sized call */
int wbc_solver_collect_timing(wbc_solver* s, double* ms, int* launches);

/* ---- multi-device: ONE host process, one solver per GPU of the node.  The reference is a single C++
 * process (/root/reference/README.md:58-60); this is how that process shards a batch over the node without Python.
 * The batch splits into contiguous slices (wbc_shard_range), shard k runs on devices[k] on its own stream; there is NO
 * data-path collective.  Optional consumer-side collective: every device receives all torques -- RCCL ncclAllGather
 * over xGMI (communicators from ncclCommInitAll; librccl is loaded on demand) or peer copies. ---- */
typedef struct wbc_multi wbc_multi;
enum wbc_gather_backend { WBC_GATHER_NONE = 0, WBC_GATHER_RCCL = 1, WBC_GATHER_PEER_COPY = 2 };
/* contiguous balanced slices: the first (n_total % n_shards) shards hold one extra state */
int wbc_shard_range(size_t n_total, int n_shards, int shard, size_t* start, size_t* count);
/* devices[k] = HIP device of shard k (RCCL: all distinct; NONE / PEER_COPY: a device may host several shards).
 * max_batch_total bounds n_total of every later call; opt may be NULL. */
int wbc_multi_create(const wbc_model* m, const wbc_params* p, int dtype, const int* devices, int n_devices,
                     size_t max_batch_total, int gather_backend, const wbc_solver_options* opt, wbc_multi** out);
void wbc_multi_destroy(wbc_multi* mm);
int wbc_multi_size(const wbc_multi* mm);                    /* number of shards */
int wbc_multi_device(const wbc_multi* mm, int shard);       /* HIP device of a shard */
wbc_solver* wbc_multi_solver(wbc_multi* mm, int shard);     /* the shard's solver (dynamics, timing, reference ... on its device) */
/* hipStream_t the shard's work is enqueued on.  These are hipStreamNonBlocking streams: they do NOT synchronise with the
 * null stream or with any stream of the caller.  Buffers produced elsewhere (copies, fills, a previous consumer) must be
 * complete -- or ordered with hipStreamWaitEvent on this stream -- before wbc_multi_step_batch / wbc_multi_rollout_batch /
 * wbc_multi_allgather_tau are called, and results are visible to other streams only after wbc_multi_synchronize (or an
 * event recorded on this stream). */
void* wbc_multi_stream(wbc_multi* mm, int shard);
int wbc_multi_rccl_ranks(const wbc_multi* mm);              /* ranks of the RCCL communicator; 0 when RCCL is not in use */
int wbc_multi_set_params(wbc_multi* mm, const wbc_params* p);   /* wbc_solver_set_params on every shard: checked once, then applied to all */
/* One control tick of n_total states.  in[k] / out[k] / obs[k] (arrays of wbc_multi_size entries; obs may be NULL when
 * the observer is off) describe shard k's slice: device pointers on devices[k], component-major with N = the shard's
 * count.  Enqueues every shard on its stream and returns without synchronising. */
int wbc_multi_step_batch(wbc_multi* mm, size_t n_total, const wbc_batch_in* in, const wbc_batch_out* out,
                         const wbc_observer_state* obs);
/* wbc_step_batch_warm per shard (a sharded closed loop): active[k] = shard k's carried active sets, int32 [count_k] on devices[k],
 * read as the start of this tick's QPs and rewritten in place with the sets they end on (all zero = cold) */
int wbc_multi_step_batch_warm(wbc_multi* mm, size_t n_total, const wbc_batch_in* in, const wbc_batch_out* out,
                              const wbc_observer_state* obs, int* const* active);
/* wbc_rollout_batch per shard (BASELINE.json configs[4]: rank-local for all ticks); tau_ext[k] may be NULL (as may tau_ext) */
int wbc_multi_rollout_batch(wbc_multi* mm, size_t n_total, int horizon, const wbc_batch_in* in, const wbc_batch_out* out,
                            const wbc_observer_state* obs, const void* const* tau_ext);
/* All-gather of the torques behind a tick (on the shard streams): tau_local[k] = shard k's [nj][count_k] on devices[k];
 * tau_all[k] on devices[k] receives wbc_multi_size blocks of nj * count_0 scalars, block j = shard j's tau exactly as
 * shard j laid it out ([nj][count_j], packed; the tail of a shorter shard's block is padding). */
int wbc_multi_allgather_tau(wbc_multi* mm, size_t n_total, const void* const* tau_local, void* const* tau_all);
/* The same gather OFF the tick's critical path: it is enqueued on per-shard gather streams behind the tick that is on the shard streams
 * now and runs BESIDE the next tick.  The caller double-buffers tau (two tau buffers per shard, ticks alternate between them) and names
 * the slot (0 / 1) of the buffer being gathered; wbc_multi_gather_wait(slot) makes every shard stream wait -- on the device, the host
 * returns at once -- for that slot's last gather: call it before the tick that overwrites that slot's tau.  Per tick k, slot b = k & 1:
 *     wbc_multi_gather_wait(mm, b);  wbc_multi_step_batch(... out[b] ...);  wbc_multi_allgather_tau_async(mm, n, tau_b, tau_all_b, b);  */
int wbc_multi_allgather_tau_async(wbc_multi* mm, size_t n_total, const void* const* tau_local, void* const* tau_all, int slot);
int wbc_multi_gather_wait(wbc_multi* mm, int slot);
/* WBC_GATHER_PEER_COPY: where every device can map every other's memory, shard j's block reaches all devices through ONE kernel that stores into the
 * tau_all buffers directly (peer mappings).  That needs every tau_all[k] to be plain hipMalloc memory of devices[k]: the library checks each new set of
 * buffers once (hipPointerGetAttributes: device memory of the right device) and falls back to hipMemcpyPeerAsync per block otherwise -- but memory from a
 * virtual-memory pool (PyTorch expandable segments, hipMallocAsync) can pass that check without being mapped on the peers.  Callers with such buffers
 * switch the push kernel off: on = 1 -> always copies, 0 (default) -> push where allowed.  wbc_multi_gather_pushes: 1 when the next peer gather would push. */
int wbc_multi_set_peer_copies(wbc_multi* mm, int on);
int wbc_multi_gather_pushes(const wbc_multi* mm);
/* One call per tick of that double-buffered loop: wbc_multi_gather_wait(slot), the tick (wbc_multi_step_batch, or _warm when active is given)
 * writing out[k].tau -- the slot's buffer -- and wbc_multi_allgather_tau_async of out[k].tau into tau_all[k]: two tickets to the issue threads. */
int wbc_multi_tick_gather(wbc_multi* mm, size_t n_total, const wbc_batch_in* in, const wbc_batch_out* out, const wbc_observer_state* obs,
                          int* const* active /* may be NULL */, void* const* tau_all, int slot);
int wbc_multi_synchronize(wbc_multi* mm);                   /* waits for every shard stream (and gather stream) */
int wbc_multi_issue_threads(const wbc_multi* mm);           /* number of issue threads (0: the shards are issued on the caller's thread) */
/* host time the caller has spent INSIDE the tick / rollout / gather entry points since the last reset: what feeding the devices costs */
int wbc_multi_host_stats(wbc_multi* mm, unsigned long long* calls, double* seconds, int reset);
/* diagnostics: the time of `iters` EMPTY tickets through the issue threads (what a round trip costs apart from the HIP calls inside it) */
int wbc_multi_probe_issue(wbc_multi* mm, int iters, double* seconds);
/* self-test of the issue threads without a device (run by the CPU test-suite): every thread must run every ticket exactly once, in order, and a thread's
 * error must reach the caller; spin_us = 0 forces the parked (condition variable) path, pause_us > 0 lets the threads park between tickets */
int wbc_multi_selftest_issue(int threads, int tickets, int spin_us, int pause_us);
/* Host-resident batch (a C++ caller that holds host arrays, e.g. the ROS side): in / out / obs hold HOST pointers to
 * component-major arrays [ncomp][n_total] of the solver's scalar type; slices are scattered to the devices with pitched
 * copies, stepped, and tau, f, status, iters (and the observer state, when obs is given) gathered back.  out->M, h, Jc,
 * pf must be NULL.  Synchronises.  PCIe-bound by construction. */
int wbc_multi_step_host(wbc_multi* mm, size_t n_total, const wbc_batch_in* host_in, const wbc_batch_out* host_out,
                        const wbc_observer_state* host_obs);

/* ------------------------------------------------------------------------------------------------------------------------
 * Dense QPs of run-time size -- the general path beside the controller's own 12-variable GRF QP (which wbc_step_batch solves
 * with kernels written around its structure).  Replaces: whatever QP library the reference controller links for its
 * "optimization problem based on the modulation of ground reaction forces" (/root/reference/README.md:11; the source is an
 * absent submodule, .gitmodules:4-6, so its variable set is unknown -- a formulation that also carries accelerations, slacks or
 * joint-torque rows is assembled by the caller and solved here).
 *
 *     min 1/2 x^T H x + g^T x    s.t.   C_i x = d_i (i < meq),   C_i x >= d_i (meq <= i < m);    1 <= n <= 36, 0 <= m <= 64
 *
 * All pointers are DEVICE pointers on the current device, PROBLEM-major (one problem's data contiguous): H [N][n*n] row-major,
 * symmetric positive definite (both triangles given, the lower one is read); g [N][n]; C [N][m*n] row-major; d [N][m]; x [N][n];
 * lambda [N][m] or NULL (multipliers: >= 0 for inequality rows, any sign for equality rows; 0 for inactive rows); status [N]:
 * 0 optimal, 1 iteration limit, 2 infeasible, 3 H not positive definite; iters [N] or NULL.  One QP per wavefront, factors and
 * working set in LDS (Goldfarb-Idnani dual active set); enqueued on hipStream (NULL = the default stream), returns without
 * synchronising.  dtype: WBC_F64 / WBC_F32 = the scalar type of every array and of the arithmetic. */
int wbc_qp_dense_batch(int dtype, size_t N, int n, int m, int meq, const void* H, const void* g, const void* C, const void* d,
                       int max_iter, double tol, void* x, void* lambda, int* status, int* iters, void* hipStream);

const char* wbc_strerror(int status);
const char* wbc_last_error(void); /* thread-local detail string of the last failure */
int wbc_abi_version(void); /* 10 */

#ifdef __cplusplus
}
#endif
#endif /* WBC_HIP_H */
