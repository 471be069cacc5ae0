// Host-callable launchers of the gfx950 kernels.  Each kernel family is its own translation unit (k_*.hip), compiled
// once per scalar type (-DWBC_SCALAR=double|float), so the library builds in parallel and a change to one kernel
// recompiles only the units that contain it.  The host side (api_*.cpp, wbc_multi.cpp) sees nothing but these
// declarations and the plain-data argument structs of device_types.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "qp_general_args.hpp"
#include "limit_args.hpp"
#include "plan_consts.hpp"

namespace wbc {

// The batch sizes at which a launcher changes kernel variant live in plan_consts.hpp (no HIP header), shared with the host side's tick planner
// (wbc_plan_tick, tick_plan.cpp), which so reports exactly what the launchers do.

// stream of the launch + (optionally) the events that receive the dispatch's own start / stop timestamps
struct LaunchCtx {
  hipStream_t st = nullptr;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  int f32_pack2 = 0;   // wbc_solver_options.f32_pack2 (dyn_sweep launches only)
};

// dyn_sweep_kernel<T, MODE>: MODE = SW_MATS | SW_STEP | SW_OBS bits (device_types.hpp); workgroup size chosen from N
template <class T> hipError_t k_dyn_sweep(const LaunchCtx& L, int mode, const DevModel<T>* model, const DevParams<T>& prm, const SweepArgs<T>& a);
// rnea_step_kernel<T, MODE>: CRBA-free front half of ticks whose caller passes no M/h/Jc buffers; MODE = RS_STEP [| RS_OBS] [| RS_PF]
template <class T> hipError_t k_rnea_step(const LaunchCtx& L, int mode, const DevModel<T>* model, const DevParams<T>& prm, const SweepArgs<T>& a);
// observer_kernel<T>: the momentum-observer update as its own kernel (large observer-on batches, second stream)
template <class T> hipError_t k_observer(const LaunchCtx& L, const DevModel<T>* model, const DevParams<T>& prm, const SweepArgs<T>& a);
// sweep_obs_kernel<T, W>: k_observer and the observer-free k_dyn_sweep(SW_MATS | SW_STEP | SW_NOB) as the two roles of ONE launch (mid-size observer-on batches)
template <class T> hipError_t k_sweep_obs(const LaunchCtx& L, const DevModel<T>* model, const DevParams<T>& prm, const SweepArgs<T>& a);
// tile_tick_kernel<T, W, NS>: the whole tick as one launch of `states`-state workgroups (tile_tick.hip.hpp); the sizes and ranges: plan_consts.hpp, tile_tick_states*()
template <class T> hipError_t k_tile_prepare();   // raises the dynamic-LDS limit of the tile_tick kernels (once per process and device)
template <class T> hipError_t k_qp_prepare();     // ... of the staged QP tile kernels
template <class T> hipError_t k_tile_tick(const LaunchCtx& L, bool observer, int states, const DevModel<T>* model, const DevParams<T>& prm, const SweepArgs<T>& a, const QpArgs<T>& qa, const QpJidx& jmap);
// GRF QP + torque map; rhat = the observer estimate arrives through the workspace (k_observer ran).
// tile = 0: qp_group16_kernel, one wavefront per workgroup, four consecutive states per wavefront;
// tile = 64 | 128 | 256 | 512: qp_tile_kernel, workgroups of four wavefronts deal a tile of that many states by predicted work
// list (optional): solve the states list[4 .. 4 + list[0]) instead of the whole batch (qp_list_kernel; the count is reset by the
// NEXT tick's front-half kernel, SweepArgs::qp_todo -- not here)
// warm (tile = 0, no list): qp_group16_kernel<.., WARM>, every state starts from its active set in a.aset_in
// tile = 0 runs the structured body (qp_struct16.hip.hpp) whatever the kernel's name says.
// body (tiles): 0 structured body on gathered inputs (qp_tile_kernel), 1 the orthogonal-factor fp32 body instead (qp_group16.hip.hpp: fp32 only, tiles of
// 64 ... 128 states, from WBC_F32_DENSE_TILE_MIN states on), 2 STAGED tiles --
// qp_stile_kernel, the tile's inputs through LDS, twelve wavefronts per workgroup, tile <= STILE_MAX_TILE (a multiple of 4)
template <class T> hipError_t k_qp(const LaunchCtx& L, bool rhat, int tile, const DevParams<T>& prm, const QpArgs<T>& a, const QpJidx& jmap,
                                  int* list = nullptr, bool warm = false, int body = 0);
// qp_lane_kernel<T, RHAT>: the GRF QP one state per LANE (semismooth Newton on the 6-dimensional residual wrench); states it
// does not finish are appended to todo (todo[0] = count, todo[4 ...] = indices) for k_qp(..., list = todo); the count must be
// zero when this kernel starts: the front-half kernel of the tick empties it (SweepArgs::qp_todo)
template <class T> hipError_t k_qp_lane(const LaunchCtx& L, bool rhat, const DevParams<T>& prm, const QpArgs<T>& a, const QpJidx& jmap, int* todo, bool warm = false);
// fused_tick_kernel<T, OBSERVER, MATS>: the whole tick of a small batch as one launch
template <class T> hipError_t k_fused_tick(const LaunchCtx& L, bool observer, bool mats, const DevModel<T>* model, const DevParams<T>& prm,
                                          const SweepArgs<T>& a, const QpArgs<T>& qa, const QpJidx& jmap, bool warm = false);
// fused_pair_kernel<T>: two 16-state tick workgroups as ONE twelve-wavefront workgroup of 32 states (the ranges and their measurements: plan_consts.hpp, WBC_FUSED_PAIR_*)
template <class T> hipError_t k_fused_pair(const LaunchCtx& L, const DevModel<T>* model, const DevParams<T>& prm, const SweepArgs<T>& a, const QpArgs<T>& qa, const QpJidx& jmap);
// The rollout family: `horizon` dependent ticks incl. forward dynamics as one launch, rollout_kernel<T, OBSERVER, TRACK, SPW, WARM, PAYLOAD> or -- with the
// running cost accumulated on chip (score.hip.hpp), always warm -- rollout_scored_kernel<T, OBSERVER, TRACK, SPW, PAYLOAD>.  What one launch carries:
template <class T> struct RolloutLaunch {
  bool observer; int spw;   // states per workgroup, 4 | 16
  const DevModel<T>* model; DevParams<T> prm;
  SweepArgs<T> a; QpArgs<T> qa; QpJidx jmap; IntegrateArgs<T> ia; int horizon;
  const DevRefParams<T>* G; RefArgs<T> ra;   // ra.plan non-null: TRACK, the planner in the loop
  bool warm;                                 // the unscored kernels' WARM
  const T* payload;                          // non-null, [10][N]: PAYLOAD, the plant carries it on its trunk
  const ScoreArgs<T>* score;                 // non-null: the scored kernels
};
// one variant's launcher; k_rollout.hip compiled with the variant's flags defines it (csrc/Makefile, ROLLOUT_UNITS)
template <class T, bool TRACK, bool PAYLOAD, bool SCORE> hipError_t rollout_launch(const LaunchCtx& L, const RolloutLaunch<T>& r);
// picks the variant from r.ra.plan, r.payload, r.score
template <class T> hipError_t k_rollout(const LaunchCtx& L, const RolloutLaunch<T>& r);
// score_tick_kernel<T>: one tick's cost l_k of every state into sc.cost / sc.fail (the per-tick path of the scored rollouts, wbc_score_batch)
template <class T> hipError_t k_score_tick(const LaunchCtx& L, const ScoreArgs<T>& sc, const T* q, const T* v, const T* tau, const T* f, const int* status, int is_last);
// rollout_select_kernel<T, BLOCK>: per group of `group` consecutive costs the best index, its cost and the MPPI weights (one workgroup per group)
template <class T> hipError_t k_rollout_select(hipStream_t st, size_t n_groups, size_t group, const T* cost, T lambda, int* best, T* best_cost, T* weights);
// qp_general_kernel<T>: dense QPs of run-time size (n <= 36 variables, m <= 64 rows, the first meq of them equalities), one per wavefront
template <class T> hipError_t k_qp_general(const LaunchCtx& L, const QpGeneralArgs<T>& a);
// the torque-limit post-pass behind a tick (limit.hip.hpp): limit_scan_kernel<T> lists the states with a stance-leg torque beyond its limit and clips
// swing-leg torques; limit_qp_kernel<T> re-solves the listed states' GRF QPs with the limits as rows on `workgroups` workgroups (limit_qp_grid: one
// resident round for a device of that many compute units)
template <class T> hipError_t k_limit_scan(const LaunchCtx& L, const LimitArgs<T>& a);
template <class T> hipError_t k_limit_qp(const LaunchCtx& L, const LimitArgs<T>& a, int workgroups);
// One resident round of wavefronts, from the kernel's LDS footprint.  A wavefront's slice holds the limited QP at its largest (LIMIT_QP_N = 12 variables,
// LIMIT_QP_M = 48 rows) in fp64 for both scalar types: qpg_lds_scalars(12, 48) = 1076 doubles = 8608 bytes; a workgroup of LIMIT_QP_WPB = 4 wavefronts takes
// 34 432 bytes, so floor(163 840 / 34 432) = 4 workgroups = 16 wavefronts share a compute unit's 160 KB (at most 128 registers each, four per SIMD):
//     grid = compute units x floor(LDS per compute unit / (LIMIT_QP_WPB x 8608)) workgroups  =  256 x 4 = 1024 workgroups = 4096 wavefronts on MI355X.
// The list is walked with a grid stride, so a larger list takes further trips of the same wavefronts and a wrong guess costs time, never correctness.
// The 160 KB are specific to gfx950 (CDNA4), the only target this library is built for: a constant, not read from the device properties.
constexpr size_t GFX950_LDS_PER_CU = 160 * 1024;
inline int limit_qp_grid(int compute_units) {
  const size_t wg_bytes = (size_t)LIMIT_QP_WPB * qpg_lds_scalars(LIMIT_QP_N, LIMIT_QP_M) * sizeof(double);
  const size_t per_cu = GFX950_LDS_PER_CU / wg_bytes;
  return compute_units * (int)(per_cu < 1 ? 1 : per_cu);
}
// one thread: *ptr = value, system scope (the completion ticket of the flag-polled single-robot tick)
hipError_t k_flag(hipStream_t st, unsigned* ptr, unsigned value);
// the peer gather of wbc_multi_*: ONE launch copies `bytes` bytes at src to each of the nd <= 64 destinations (this device's or peer-mapped memory)
hipError_t k_gather_push(hipStream_t st, const void* src, void* const* dst, int nd, size_t bytes);
template <class T> hipError_t k_integrate(const LaunchCtx& L, const DevModel<T>* model, const IntegrateArgs<T>& a);
// integrate_kernel<T, true>: k_integrate with a payload [10][N] on the plant's trunk (integrate.hip.hpp, PAYLOAD; defined in the payload unit of k_rollout.hip)
template <class T> hipError_t k_integrate_plant(const LaunchCtx& L, const DevModel<T>* model, const IntegrateArgs<T>& a, const T* payload);
template <class T> hipError_t k_reference(const LaunchCtx& L, const DevModel<T>* model, const DevRefParams<T>* G, const RefArgs<T>& a);
// swing-foot references (swing_ref.hip.hpp): swing_reference_kernel<T> rewrites the swing legs' rows of a.vdot_des from its base rows as they stand;
// com_swing_reference_kernel<T> is k_reference with the same law applied before its joint rows are stored -- one launch
template <class T> hipError_t k_swing_reference(const LaunchCtx& L, const DevModel<T>* model, const SwingRefArgs<T>& a);
template <class T> hipError_t k_reference_swing(const LaunchCtx& L, const DevModel<T>* model, const DevRefParams<T>* G, const RefArgs<T>& a, const SwingArgs<T>& sa);
// gait scheduler (gait.hip.hpp): gait_kernel<T> advances phase, rewrites mask and the lifted feet's plan words of swing, in place
template <class T> hipError_t k_gait(const LaunchCtx& L, const DevModel<T>* model, const GaitArgs<T>& a);
// ground-contact plant (ground.hip.hpp): ground_force_kernel<T> is the contact law alone (f_gr, contact, gap from q, v, Jc and the terrain);
// ground_integrate_kernel<T> is the same law followed by k_integrate with f = f_gr handed over in registers -- one launch
template <class T> hipError_t k_ground_force(const LaunchCtx& L, const DevModel<T>* model, const GroundArgs<T>& a);
template <class T> hipError_t k_ground_integrate(const LaunchCtx& L, const DevModel<T>* model, const GroundIntegrateArgs<T>& a);
// stiction on the ground plant (stick.hip.hpp): stick_force_kernel<T> is the contact law with the per-foot anchor spring (anchor, stick advance in
// place); stick_integrate_kernel<T> is that law followed by k_integrate with f = f_gr handed over in registers -- one launch
template <class T> hipError_t k_stick_force(const LaunchCtx& L, const DevModel<T>* model, const StickArgs<T>& a);
template <class T> hipError_t k_stick_integrate(const LaunchCtx& L, const DevModel<T>* model, const StickIntegrateArgs<T>& a);
// contact sensing from the observer's residual (contact_est.hip.hpp): contact_estimate_kernel<T> is the law alone (f_est, fn_est, singular and the
// contact word, in place, from Jc, r, f_prev and the normals); gait_estimated_kernel<T> is the same law followed by k_gait with the word handed over in
// registers -- one launch
template <class T> hipError_t k_contact_estimate(const LaunchCtx& L, const DevModel<T>* model, const ContactArgs<T>& a);
template <class T> hipError_t k_gait_estimated(const LaunchCtx& L, const DevModel<T>* model, const GaitEstimatedArgs<T>& a);
// terrain heightfield (terrain.hip.hpp): terrain_sample_kernel<T> is the sampling law at caller-given points; terrain_feet_kernel<T> the law under the
// four feet of every state (normals, height, surf, and p1_z of the lifted feet's plans); gait_terrain_kernel<T> / gait_estimated_terrain_kernel<T> are
// k_gait / k_gait_estimated followed by k_terrain_feet on the mask and swing they leave -- one launch each
template <class T> hipError_t k_terrain_sample(const LaunchCtx& L, const TerrainSampleArgs<T>& a);
template <class T> hipError_t k_terrain_feet(const LaunchCtx& L, const DevModel<T>* model, const TerrainFeetArgs<T>& a);
template <class T> hipError_t k_gait_terrain(const LaunchCtx& L, const DevModel<T>* model, const GaitTerrainArgs<T>& a);
template <class T> hipError_t k_gait_estimated_terrain(const LaunchCtx& L, const DevModel<T>* model, const GaitEstimatedTerrainArgs<T>& a);
// foothold selection (foothold.hip.hpp): terrain_cost_kernel<T> writes the cost of every node of a map (set-up time); foothold_select_kernel<T> is the
// selection law alone on the mask and swing a gait call left; gait_terrain_select_kernel<T> / gait_estimated_terrain_select_kernel<T> are k_gait /
// k_gait_estimated, then that law, then k_terrain_feet -- one launch each
template <class T> hipError_t k_terrain_cost(const LaunchCtx& L, const TerrainCostArgs<T>& a, unsigned n_tiles);
template <class T> hipError_t k_foothold_select(const LaunchCtx& L, const FootholdSelectArgs<T>& a);
template <class T> hipError_t k_gait_terrain_select(const LaunchCtx& L, const DevModel<T>* model, const GaitTerrainSelectArgs<T>& a);
template <class T> hipError_t k_gait_estimated_terrain_select(const LaunchCtx& L, const DevModel<T>* model, const GaitEstimatedTerrainSelectArgs<T>& a);
// base state from leg odometry (odom.hip.hpp): base_estimate_kernel<T> is the law alone (base, anchor, odo in place; q_est, v_est); gait_estimated_odom_kernel<T>
// is that law, then k_gait_estimated with the estimated base rows handed over in registers -- one launch
template <class T> hipError_t k_base_estimate(const LaunchCtx& L, const DevModel<T>* model, const OdomArgs<T>& a);
template <class T> hipError_t k_gait_estimated_odom(const LaunchCtx& L, const DevModel<T>* model, const GaitEstimatedOdomArgs<T>& a);
// trunk reference from the velocity command (cmd_ref.hip.hpp): cmd_reference_kernel<T> is k_reference with the plan formed on the device from cmd and
// the foot planes (trunk advances in place); cmd_swing_reference_kernel<T> is the same with the swing law applied before the joint rows are stored
template <class T> hipError_t k_reference_cmd(const LaunchCtx& L, const DevModel<T>* model, const DevRefParams<T>* G, const CmdRefArgs<T>& a);
template <class T> hipError_t k_reference_cmd_swing(const LaunchCtx& L, const DevModel<T>* model, const DevRefParams<T>* G, const CmdRefArgs<T>& a,
                                                    const SwingArgs<T>& sa);

}  // namespace wbc
