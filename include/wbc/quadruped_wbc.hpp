// quadruped_wbc.hpp -- header-only C++ host class over the C-ABI (include/wbc_hip.h).
//
// Mirrors the shape of the reference controller's per-tick entry point as far as it is observable:
// a controller object built from the URDF path given on the command line
// (/root/reference/README.md:60) whose tick turns the robot state into joint torques
// (/root/reference/README.md:11).  The reference's class and method names live in an absent
// submodule (/root/reference/.gitmodules:4-6) and are [UNVERIFIED]; rename to taste when binding.
//
// The ROS message adaptors at the bottom are compiled only with -DWBC_WITH_ROS.  ROS is absent from this image: the
// section is compile-checked against field-layout stubs of the three message headers (tests/stubs/, labelled as
// stubs -- they pin nothing about the real controller's topics or types, which are [UNVERIFIED]).
#pragma once
#include <array>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "../wbc_hip.h"
#ifdef WBC_WITH_ROS
#include <gazebo_msgs/ModelStates.h>
#include <sensor_msgs/JointState.h>
#include <std_msgs/Float64MultiArray.h>
#endif

namespace wbc {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& where)
      : std::runtime_error(where + ": " + wbc_strerror(c) + " (" + wbc_last_error() + ")"), code(c) {}
};
inline void check(int rc, const char* where) { if (rc != WBC_OK) throw Error(rc, where); }

// Plain-data stand-ins with the field layout of the ROS messages a Gazebo quadruped loop uses.
struct BaseState {            // gazebo_msgs/ModelStates entry: pose + twist of the floating base, world frame
  double position[3];
  double orientation_xyzw[4];
  double linear[3];
  double angular[3];
};
struct JointState {           // sensor_msgs/JointState: name[], position[], velocity[]
  std::vector<std::string> name;
  std::vector<double> position, velocity;
};
struct ContactState {         // per-foot stance flag, terrain normal and friction (planner / contact sensors)
  bool stance[4];
  double normal[4][3];
  double mu[4];
};
struct ComPlan {              // input of the CoM planner (wbc_reference_batch's plan row)
  double start[3], goal[3];   // CoM start / goal, world
  double duration;            // s; <= 0 = hold the goal
  double quat_des_xyzw[4];    // desired trunk attitude
};
struct SwingPlan {            // one foot's row of wbc_swing_reference_batch's swing plan
  double liftoff[3], touchdown[3];   // world
  double clearance;           // apex height above the straight line, m
  double duration;            // s; <= 0 = hold the touchdown point
  double elapsed;             // s already spent in this swing at t = 0
};
struct GaitCommand {          // one robot's row of wbc_gait_batch's cmd
  double vx, vy;              // commanded trunk velocity, heading frame, m/s
  double wz;                  // commanded yaw rate, rad/s
  double ground_z;            // world z of the footholds
};
struct GaitState {            // what the gait scheduler carries from tick to tick
  double phase = 0.0;         // in [0, 1)
  bool stance[4] = {true, true, true, true};
  std::array<SwingPlan, 4> swing{};   // elapsed is rewritten every tick: pass t = 0 to swingReference / referenceSwing
  int events = 0;             // bit k: foot k lifted off on the last tick, bit 4 + k: it touched down
};
struct Command {              // what the planner hands to the tick
  double w_des[6];            // desired contact wrench on the base rows
  std::array<double, 18> vdot_des;
};

class QuadrupedWBC {
 public:
  // urdf_path: argv[1] of the reference's `dogbot` executable
  explicit QuadrupedWBC(const std::string& urdf_path, const wbc_params* params = nullptr, int device = 0,
                        const std::vector<std::string>& foot_links = {}) {
    std::vector<const char*> fl;
    for (auto& s : foot_links) fl.push_back(s.c_str());
    check(wbc_model_load_urdf(urdf_path.c_str(), fl.empty() ? nullptr : fl.data(), (int)fl.size(), &model_),
          "wbc_model_load_urdf");
    wbc_params p;
    if (params) p = *params; else wbc_params_default(&p, WBC_F64);
    params_ = p;
    int rc = wbc_solver_create(model_, &p, WBC_F64, device, 1, &solver_);
    if (rc != WBC_OK) { wbc_model_free(model_); model_ = nullptr; throw Error(rc, "wbc_solver_create"); }
    check(wbc_model_dims(model_, nullptr, &nq_, &nv_, &nj_, &nf_), "wbc_model_dims");
    for (int j = 0; j < nj_; ++j) joint_names_.push_back(wbc_model_joint_name(model_, j));
    obs_integ_.assign(nv_, 0.0); obs_r_.assign(nv_, 0.0);
    tau_prev_.assign(nj_, 0.0); f_prev_.assign(3 * nf_, 0.0);
  }
  ~QuadrupedWBC() { if (solver_) wbc_solver_destroy(solver_); if (model_) wbc_model_free(model_); }
  QuadrupedWBC(const QuadrupedWBC&) = delete;
  QuadrupedWBC& operator=(const QuadrupedWBC&) = delete;

  const std::vector<std::string>& jointNames() const { return joint_names_; }

  // One control tick for one robot: returns joint torques in jointNames() order; grf_out (12) optional.
  // Throws on ABI errors; returns the QP status (0 optimal, 1 iteration limit, 2 infeasible).
  int computeTorques(const BaseState& base, const JointState& js, const ContactState& contacts, const Command& cmd,
                     std::vector<double>& tau_out, double* grf_out = nullptr) {
    std::vector<double> q, v;
    packState(base, js, q, v);
    double normals[12], mu[4];
    int mask = 0;
    for (int f = 0; f < nf_; ++f) {
      if (contacts.stance[f]) mask |= 1 << f;
      for (int k = 0; k < 3; ++k) normals[3 * f + k] = contacts.normal[f][k];
      mu[f] = contacts.mu[f];
    }
    tau_out.assign(nj_, 0.0);
    std::vector<double> f(3 * nf_);
    int status = -1;
    const bool obs = params_.observer_order > 0;
    if (obs && !obs_started_) {  // start-up contract of the observer (wbc_observer_state): integ(0) = p(0) = M(q0) v0, r(0) = 0
      check(wbc_observer_init(solver_, q.data(), v.data(), obs_integ_.data(), obs_r_.data()), "wbc_observer_init");
      obs_started_ = true;
    }
    check(wbc_compute_torques(solver_, q.data(), v.data(), cmd.w_des, cmd.vdot_des.data(), normals, mu, mask,
                              obs ? tau_prev_.data() : nullptr, obs ? f_prev_.data() : nullptr,
                              obs ? obs_integ_.data() : nullptr, obs ? obs_r_.data() : nullptr, tau_out.data(), f.data(),
                              &status),
          "wbc_compute_torques");
    tau_prev_ = tau_out; f_prev_ = f;
    if (grf_out) for (int k = 0; k < 3 * nf_; ++k) grf_out[k] = f[k];
    return status;
  }

  // The planner side of the tick (/root/reference/README.md:11 "a motion planner for the trajectory of the robot's
  // center of mass"): turns a CoM plan evaluated `t` seconds after its start into the Command computeTorques tracks.
  // com_out (6, optional) receives the CoM position and velocity of the given state.
  void setReferenceGains(const wbc_ref_params& g) { check(wbc_solver_set_ref_params(solver_, &g), "wbc_solver_set_ref_params"); ref_set_ = true; }
  Command plan(const BaseState& base, const JointState& js, const ComPlan& cp, double t, double* com_out = nullptr) {
    if (!ref_set_) { wbc_ref_params g; wbc_ref_params_default(&g); setReferenceGains(g); }
    std::vector<double> q, v;
    packState(base, js, q, v);
    double row[WBC_PLAN_WORDS];
    for (int k = 0; k < 3; ++k) { row[k] = cp.start[k]; row[3 + k] = cp.goal[k]; }
    row[6] = cp.duration; row[7] = 0.0;
    for (int k = 0; k < 4; ++k) row[8 + k] = cp.quat_des_xyzw[k];
    Command c;
    check(wbc_compute_reference(solver_, q.data(), v.data(), row, t, c.w_des, c.vdot_des.data(), com_out), "wbc_compute_reference");
    return c;
  }

  // Swing-foot references (wbc_hip.h, "Swing-foot references"): Cartesian tracking for the feet that contacts.stance marks as lifted.
  // swingReference(): cmd.vdot_des comes from plan() (or the caller); the lifted legs' joint rows are replaced by the foot-tracking law.
  // referenceSwing(): plan() followed by swingReference().  foot_out (24, optional): p_f (3) and J_k v (3) of all four feet.
  void setSwingGains(const wbc_swing_params& p) { check(wbc_solver_set_swing_params(solver_, &p), "wbc_solver_set_swing_params"); }
  void swingReference(const BaseState& base, const JointState& js, const ContactState& contacts, const std::array<SwingPlan, 4>& sp, double t,
                      Command& cmd, double* foot_out = nullptr) {
    std::vector<double> q, v;
    packState(base, js, q, v);
    double row[WBC_SWING_WORDS];
    int mask = 0;
    for (int f = 0; f < 4; ++f) {
      if (contacts.stance[f]) mask |= 1 << f;
      for (int k = 0; k < 3; ++k) { row[9 * f + k] = sp[f].liftoff[k]; row[9 * f + 3 + k] = sp[f].touchdown[k]; }
      row[9 * f + 6] = sp[f].clearance; row[9 * f + 7] = sp[f].duration; row[9 * f + 8] = sp[f].elapsed;
    }
    check(wbc_compute_swing_reference(solver_, q.data(), v.data(), mask, row, t, cmd.vdot_des.data(), foot_out), "wbc_compute_swing_reference");
  }
  Command referenceSwing(const BaseState& base, const JointState& js, const ContactState& contacts, const ComPlan& cp,
                         const std::array<SwingPlan, 4>& sp, double t, double* com_out = nullptr, double* foot_out = nullptr) {
    Command c = plan(base, js, cp, t, com_out);
    swingReference(base, js, contacts, sp, t, c, foot_out);
    return c;
  }

  // Gait scheduler (wbc_hip.h, "Gait scheduler"): one control period of the phase clock.  gaitParamsDefault(): the default schedule with this model's
  // hip origins as nominal footholds.  gait(): advances st in place -- the phase, the stance flags, and the plans of the lifted feet (lift-off point
  // latched, Raibert foothold, elapsed time); sensed[k] = foot k senses ground (nullptr: none does).  The tick is then
  // gait(), referenceSwing(base, js, contacts with st.stance, cp, st.swing, 0.0), computeTorques().
  wbc_gait_params gaitParamsDefault() const { wbc_gait_params p; wbc_gait_params_default(model_, &p); return p; }
  void setGaitParams(const wbc_gait_params& p) { check(wbc_solver_set_gait_params(solver_, &p), "wbc_solver_set_gait_params"); }
  void gait(const BaseState& base, const JointState& js, const GaitCommand& gc, GaitState& st, const bool* sensed = nullptr) {
    std::vector<double> q, v;
    packState(base, js, q, v);
    const double cmd[WBC_GAIT_CMD_WORDS] = {gc.vx, gc.vy, gc.wz, gc.ground_z};
    double row[WBC_SWING_WORDS];
    int mask = 0, contact = 0;
    for (int f = 0; f < 4; ++f) {
      if (st.stance[f]) mask |= 1 << f;
      if (sensed && sensed[f]) contact |= 1 << f;
      for (int k = 0; k < 3; ++k) { row[9 * f + k] = st.swing[f].liftoff[k]; row[9 * f + 3 + k] = st.swing[f].touchdown[k]; }
      row[9 * f + 6] = st.swing[f].clearance; row[9 * f + 7] = st.swing[f].duration; row[9 * f + 8] = st.swing[f].elapsed;
    }
    check(wbc_compute_gait(solver_, q.data(), v.data(), cmd, contact, &st.phase, &mask, row, &st.events), "wbc_compute_gait");
    for (int f = 0; f < 4; ++f) {
      st.stance[f] = ((mask >> f) & 1) != 0;
      for (int k = 0; k < 3; ++k) { st.swing[f].liftoff[k] = row[9 * f + k]; st.swing[f].touchdown[k] = row[9 * f + 3 + k]; }
      st.swing[f].clearance = row[9 * f + 6]; st.swing[f].duration = row[9 * f + 7]; st.swing[f].elapsed = row[9 * f + 8];
    }
  }

  // Ground-contact plant (wbc_hip.h, "Ground-contact plant"): the contact law's constants, for callers that run the batch calls
  // wbc_ground_force_batch / wbc_integrate_ground_batch on solver()'s device buffers -- the plant is a simulation-side call and has no single-robot
  // host-pointer form.  groundParamsDefault(): k_n 2e4, c_n 150, c_t 200, f_touch 5.
  static wbc_ground_params groundParamsDefault() { wbc_ground_params p; wbc_ground_params_default(&p); return p; }
  void setGroundParams(const wbc_ground_params& p) { check(wbc_solver_set_ground_params(solver_, &p), "wbc_solver_set_ground_params"); }
  void groundForce(size_t N, const void* q, const void* v, const void* Jc, const void* normals, const void* height, const void* mu, void* f_gr,
                   int* contact = nullptr, void* gap = nullptr, void* stream = nullptr) {
    check(wbc_ground_force_batch(solver_, N, q, v, Jc, normals, height, mu, f_gr, contact, gap, stream), "wbc_ground_force_batch");
  }
  void integrateGround(size_t N, void* q, void* v, const void* M, const void* h, const void* Jc, const void* tau, const void* normals,
                       const void* height, const void* mu, const void* tau_ext /* may be nullptr */, void* f_gr, int* contact = nullptr,
                       void* gap = nullptr, void* stream = nullptr) {   // (the argument order of the C call)
    check(wbc_integrate_ground_batch(solver_, N, q, v, M, h, Jc, tau, normals, height, mu, tau_ext, f_gr, contact, gap, stream),
          "wbc_integrate_ground_batch");
  }

  // Stiction on the ground plant (wbc_hip.h, "Stiction on the ground plant"): the ground calls with a per-foot anchor spring.  anchor [12][N] and
  // stick [N] are the caller's device buffers and advance in place; the caller stores 0 into stick before the first tick.
  // stictionParamsDefault(): k_t 2e4.
  static wbc_stiction_params stictionParamsDefault() { wbc_stiction_params p; wbc_stiction_params_default(&p); return p; }
  void setStictionParams(const wbc_stiction_params& p) { check(wbc_solver_set_stiction_params(solver_, &p), "wbc_solver_set_stiction_params"); }
  void groundStickForce(size_t N, const void* q, const void* v, const void* Jc, const void* normals, const void* height, const void* mu,
                        void* anchor, int* stick, void* f_gr, int* contact = nullptr, void* gap = nullptr, void* stream = nullptr) {
    check(wbc_ground_stick_force_batch(solver_, N, q, v, Jc, normals, height, mu, anchor, stick, f_gr, contact, gap, stream),
          "wbc_ground_stick_force_batch");
  }
  void integrateGroundStick(size_t N, void* q, void* v, const void* M, const void* h, const void* Jc, const void* tau, const void* normals,
                            const void* height, const void* mu, const void* tau_ext, void* anchor, int* stick, void* f_gr, int* contact = nullptr,
                            void* gap = nullptr, void* stream = nullptr) {   // (the argument order of the C call)
    check(wbc_integrate_ground_stick_batch(solver_, N, q, v, M, h, Jc, tau, normals, height, mu, tau_ext, anchor, stick, f_gr, contact, gap, stream),
          "wbc_integrate_ground_stick_batch");
  }

  // Terrain heightfield (wbc_hip.h, "Terrain heightfield"): the planes under the feet and the footholds' heights from a map, for callers that run the
  // batch calls on solver()'s device buffers.  The wbc_terrain's z and tile are DEVICE pointers, so there is no single-robot host-pointer form.
  // gaitTerrain / gaitEstimatedTerrain are wbc_gait_batch / wbc_gait_estimated_batch followed by terrainFeet on the mask and swing they leave, one launch
  // each; the same normals and height buffers then go to the step and to integrateGround[Stick].  (The argument order of the C calls.)
  void terrainSample(const wbc_terrain& t, size_t M, const void* xy, void* z, void* n, void* d, void* stream = nullptr) {
    check(wbc_terrain_sample_batch(solver_, &t, M, xy, z, n, d, stream), "wbc_terrain_sample_batch");
  }
  void terrainFeet(const wbc_terrain& t, size_t N, const void* q, const int* mask /* with swing, or both nullptr */, void* swing, void* normals,
                   void* height, void* surf = nullptr, void* stream = nullptr) {
    check(wbc_terrain_feet_batch(solver_, &t, N, q, mask, swing, normals, height, surf, stream), "wbc_terrain_feet_batch");
  }
  void gaitTerrain(size_t N, const void* q, const void* v, const void* cmd, const int* contact /* may be nullptr */, void* phase, int* mask,
                   void* swing, int* events /* may be nullptr */, const wbc_terrain& t, void* normals, void* height, void* surf = nullptr,
                   void* stream = nullptr) {
    check(wbc_gait_terrain_batch(solver_, N, q, v, cmd, contact, phase, mask, swing, events, &t, normals, height, surf, stream),
          "wbc_gait_terrain_batch");
  }
  void gaitEstimatedTerrain(size_t N, const void* q, const void* v, const void* cmd, const void* Jc, const void* r, const void* f_prev,
                            void* normals /* in/out */, int* contact, void* phase, int* mask, void* swing, int* events /* may be nullptr */,
                            void* f_est /* may be nullptr */, const wbc_terrain& t, void* height, void* surf = nullptr, void* stream = nullptr) {
    check(wbc_gait_estimated_terrain_batch(solver_, N, q, v, cmd, Jc, r, f_prev, normals, contact, phase, mask, swing, events, f_est, &t, height, surf,
                                           stream),
          "wbc_gait_estimated_terrain_batch");
  }

  // Foothold selection (wbc_hip.h, "Foothold selection"): a cost per node of the map (terrainCost, once per map and parameter set) and, per lifted foot,
  // the cheapest node near the gait rule's foothold, latched until the foot is down.  cost [n_tiles][ny][nx], hold [8][N] and latch [N] (0 before the
  // first tick) are caller-owned DEVICE buffers.  gaitTerrainSelect / gaitEstimatedTerrainSelect are gaitTerrain / gaitEstimatedTerrain with the
  // selection between the gait rule and the terrain rule, one launch each.  (The argument order of the C calls.)
  void setFootholdParams(const wbc_foothold_params& p) { check(wbc_solver_set_foothold_params(solver_, &p), "wbc_solver_set_foothold_params"); }
  void terrainCost(const wbc_terrain& t, void* cost, void* stream = nullptr) { check(wbc_terrain_cost_batch(solver_, &t, cost, stream), "wbc_terrain_cost_batch"); }
  void footholdSelect(const wbc_terrain& t, const void* cost, size_t N, const int* mask, void* swing, void* hold, int* latch, void* stream = nullptr) {
    check(wbc_foothold_select_batch(solver_, &t, cost, N, mask, swing, hold, latch, stream), "wbc_foothold_select_batch");
  }
  void gaitTerrainSelect(size_t N, const void* q, const void* v, const void* cmd, const int* contact /* may be nullptr */, void* phase, int* mask,
                         void* swing, int* events /* may be nullptr */, const wbc_terrain& t, void* normals, void* height, void* surf /* may be nullptr */,
                         const void* cost, void* hold, int* latch, void* stream = nullptr) {
    check(wbc_gait_terrain_select_batch(solver_, N, q, v, cmd, contact, phase, mask, swing, events, &t, normals, height, surf, cost, hold, latch, stream),
          "wbc_gait_terrain_select_batch");
  }
  void gaitEstimatedTerrainSelect(size_t N, const void* q, const void* v, const void* cmd, const void* Jc, const void* r, const void* f_prev,
                                  void* normals /* in/out */, int* contact, void* phase, int* mask, void* swing, int* events /* may be nullptr */,
                                  void* f_est /* may be nullptr */, const wbc_terrain& t, void* height, void* surf /* may be nullptr */, const void* cost,
                                  void* hold, int* latch, void* stream = nullptr) {
    check(wbc_gait_estimated_terrain_select_batch(solver_, N, q, v, cmd, Jc, r, f_prev, normals, contact, phase, mask, swing, events, f_est, &t, height,
                                                  surf, cost, hold, latch, stream),
          "wbc_gait_estimated_terrain_select_batch");
  }

  // Base state from leg odometry (wbc_hip.h, "Base state from leg odometry"): rows 0-2 of q_est, v_est estimated from the joints, the attitude, the gyro
  // and the contact word; rows 0-2 of q and v are never read.  base [6][N] (the start state), anchor [12][N] and odo [N] (0 before the first tick) are
  // caller-owned DEVICE buffers, advanced in place; normals and height are given together or both nullptr.  gaitEstimatedOdom is baseEstimate on the
  // words as they arrive, then gaitEstimated on the estimated rows, one launch.  (The argument order of the C calls.)
  void setOdomParams(const wbc_odom_params& p) { check(wbc_solver_set_odom_params(solver_, &p), "wbc_solver_set_odom_params"); }
  void baseEstimate(size_t N, const void* q, const void* v, const int* contact, const int* mask, const void* normals, const void* height, void* base,
                    void* anchor, int* odo, void* q_est, void* v_est, void* stream = nullptr) {
    check(wbc_base_estimate_batch(solver_, N, q, v, contact, mask, normals, height, base, anchor, odo, q_est, v_est, stream), "wbc_base_estimate_batch");
  }
  void gaitEstimatedOdom(size_t N, const void* q, const void* v, const void* cmd, const void* Jc, const void* r, const void* f_prev, const void* normals,
                         int* contact, void* phase, int* mask, void* swing, int* events /* may be nullptr */, void* f_est /* may be nullptr */,
                         const void* height /* may be nullptr */, void* base, void* anchor, int* odo, void* q_est, void* v_est, void* stream = nullptr) {
    check(wbc_gait_estimated_odom_batch(solver_, N, q, v, cmd, Jc, r, f_prev, normals, contact, phase, mask, swing, events, f_est, height, base, anchor,
                                        odo, q_est, v_est, stream),
          "wbc_gait_estimated_odom_batch");
  }

  // Trunk reference from the velocity command (wbc_hip.h, "Trunk reference from the velocity command"): w_des and vdot_des from cmd and the foot
  // planes instead of a host-written plan.  trunk [6][N] is a caller-owned DEVICE buffer, advanced in place; reset [N] non-zero (first call) starts it
  // from the state.  referenceCmdSwing is referenceCmd, then the swing law at t = 0, one launch.  (The argument order of the C calls.)
  void setTrunkParams(const wbc_trunk_params& p) { check(wbc_solver_set_trunk_params(solver_, &p), "wbc_solver_set_trunk_params"); }
  void referenceCmd(size_t N, const void* q, const void* v, const void* cmd, const void* normals, const void* height, const int* reset /* may be nullptr */,
                    void* trunk, void* w_des, void* vdot_des, void* com = nullptr, void* ref = nullptr, void* stream = nullptr) {
    check(wbc_reference_cmd_batch(solver_, N, q, v, cmd, normals, height, reset, trunk, w_des, vdot_des, com, ref, stream), "wbc_reference_cmd_batch");
  }
  void referenceCmdSwing(size_t N, const void* q, const void* v, const void* cmd, const void* normals, const void* height,
                         const int* reset /* may be nullptr */, void* trunk, const int* mask, const void* swing, void* w_des, void* vdot_des,
                         void* com = nullptr, void* ref = nullptr, void* foot = nullptr, void* stream = nullptr) {
    check(wbc_reference_cmd_swing_batch(solver_, N, q, v, cmd, normals, height, reset, trunk, mask, swing, w_des, vdot_des, com, ref, foot, stream),
          "wbc_reference_cmd_swing_batch");
  }

  // Joint torque limits (wbc_hip.h, "Joint torque limits behind a tick").  effortLimits(): the URDF's <limit effort> per joint in jointNames() order,
  // HUGE_VAL where it gives none.  setTorqueLimits(): the limits the post-pass enforces (one value > 0 per joint; empty = back to the URDF's).
  std::vector<double> effortLimits() const {
    std::vector<double> lim(nj_);
    check(wbc_model_effort_limits(model_, lim.data()), "wbc_model_effort_limits");
    return lim;
  }
  void setTorqueLimits(const std::vector<double>& tau_max) {
    if (tau_max.empty()) { check(wbc_solver_set_torque_limits(solver_, nullptr), "wbc_solver_set_torque_limits"); return; }
    if ((int)tau_max.size() != nj_) throw std::invalid_argument("setTorqueLimits: one limit per joint");
    wbc_torque_limits l;
    l.struct_size = sizeof(l);
    for (int j = 0; j < WBC_MAXV; ++j) l.tau_max[j] = j < nj_ ? tau_max[j] : HUGE_VAL;
    check(wbc_solver_set_torque_limits(solver_, &l), "wbc_solver_set_torque_limits");
  }
  // wbc_step_limited_batch on this robot's solver (one state): in / out / obs hold DEVICE pointers as for wbc_step_batch, out.M, h, Jc included;
  // limited (device, one int32) may be null.  Enqueues on `stream` and returns without synchronising.
  void stepLimited(const wbc_batch_in& in, const wbc_batch_out& out, const wbc_observer_state* obs, int* limited, void* stream = nullptr) {
    check(wbc_step_limited_batch(solver_, 1, &in, &out, obs, limited, stream), "wbc_step_limited_batch");
  }

  // Observer state (the only per-robot state carried across ticks): snapshot / restore / initialise.
  void setObserverState(const std::vector<double>& integ, const std::vector<double>& r) { obs_integ_ = integ; obs_r_ = r; obs_started_ = true; }
  void resetObserver() { obs_started_ = false; }   // the next computeTorques re-seeds integ = M v, r = 0
  const std::vector<double>& disturbanceEstimate() const { return obs_r_; }

 private:
  void packState(const BaseState& base, const JointState& js, std::vector<double>& q, std::vector<double>& v) const {
    q.assign(nq_, 0.0); v.assign(nv_, 0.0);
    for (int k = 0; k < 3; ++k) { q[k] = base.position[k]; v[k] = base.linear[k]; v[3 + k] = base.angular[k]; }
    for (int k = 0; k < 4; ++k) q[3 + k] = base.orientation_xyzw[k];
    // JointState carries names: map by name, as ROS controllers do
    for (int j = 0; j < nj_; ++j) {
      bool found = false;
      for (size_t i = 0; i < js.name.size(); ++i)
        if (js.name[i] == joint_names_[j]) { q[7 + j] = js.position[i]; v[6 + j] = js.velocity[i]; found = true; break; }
      if (!found) throw std::invalid_argument("JointState lacks joint " + joint_names_[j]);
    }
  }
  bool ref_set_ = false;
  wbc_model* model_ = nullptr;
  wbc_solver* solver_ = nullptr;
  wbc_params params_;
  int nq_ = 0, nv_ = 0, nj_ = 0, nf_ = 0;
  bool obs_started_ = false;
  std::vector<std::string> joint_names_;
  std::vector<double> obs_integ_, obs_r_, tau_prev_, f_prev_;
};

#ifdef WBC_WITH_ROS
// Compile-checked against stubs only (ROS absent from the build image).  Adaptors from the standard message types of a
// Gazebo + ros_control loop (/root/reference/README.md:38 names ros-control / ros-controllers as dependencies):
//   BaseState  <- gazebo_msgs::ModelStates (pose[i], twist[i] of the robot model)
//   JointState <- sensor_msgs::JointState
//   torques    -> std_msgs::Float64MultiArray for a JointGroupEffortController (ros_controllers), jointNames() order
// index of the robot in a ModelStates message; -1 when absent
inline int findModel(const gazebo_msgs::ModelStates& ms, const std::string& model_name) {
  for (size_t i = 0; i < ms.name.size(); ++i) if (ms.name[i] == model_name) return (int)i;
  return -1;
}
inline BaseState fromRos(const gazebo_msgs::ModelStates& ms, size_t i) {
  BaseState b;
  b.position[0] = ms.pose[i].position.x; b.position[1] = ms.pose[i].position.y; b.position[2] = ms.pose[i].position.z;
  b.orientation_xyzw[0] = ms.pose[i].orientation.x; b.orientation_xyzw[1] = ms.pose[i].orientation.y;
  b.orientation_xyzw[2] = ms.pose[i].orientation.z; b.orientation_xyzw[3] = ms.pose[i].orientation.w;
  b.linear[0] = ms.twist[i].linear.x; b.linear[1] = ms.twist[i].linear.y; b.linear[2] = ms.twist[i].linear.z;
  b.angular[0] = ms.twist[i].angular.x; b.angular[1] = ms.twist[i].angular.y; b.angular[2] = ms.twist[i].angular.z;
  return b;
}
inline JointState fromRos(const sensor_msgs::JointState& m) { return JointState{m.name, m.position, m.velocity}; }
inline std_msgs::Float64MultiArray toRos(const std::vector<double>& tau) {
  std_msgs::Float64MultiArray cmd;
  cmd.data = tau;
  return cmd;
}
#endif

}  // namespace wbc
