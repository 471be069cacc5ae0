// The tick planner: which kernels a tick of N states runs with a solver's options.  No device and no HIP header is needed (tick_plan.cpp links with
// error.cpp alone: tools/plan_sweep.cpp walks every batch size with it); step_impl (api_tick.cpp) launches what plan_tick says, wbc_plan_tick /
// wbc_dispatch_thresholds report it.  The thresholds themselves: plan_consts.hpp.
#pragma once
#include <cstddef>
#include "../../include/wbc_hip.h"

namespace wbc {

// the thresholds between kernel variants after the options are applied (resolve_options); (size_t)-1 as a minimum / 0 as a maximum: never
struct Resolved { size_t fused_max, fused_max_noobs, fused_max_obs, obs_split_min, obs_split_min_nomats, tile_min, lane_min, warm_tile_min, warm_lane_min, colaunch_min, colaunch_max, stile_min, stile_max, tt_min, tt_max, tt_first_min, tt_max_obs, tt_max_noobs32, pair_min, pair_max; };
Resolved resolve_options(int dtype, const wbc_solver_options& o);

// the values of wbc_tick_plan's fields of the same names (include/wbc_hip.h documents them)
enum PlanFused { FUSED_NONE = 0, FUSED_TICK = 1, FUSED_TILE_TICK = 2, FUSED_PAIR = 3 };
enum PlanFront { FRONT_SWEEP = 0, FRONT_RNEA = 1, FRONT_OBS_THEN_SWEEP = 2, FRONT_OBS_THEN_RNEA = 3, FRONT_SWEEP_OBS_ROLES = 4 };
enum PlanQp { QP_GROUP16 = 0, QP_TILES = 1, QP_LANE_PAIR = 2 };
enum PlanQpBody { QP_BODY_STRUCTURED = 0, QP_BODY_DENSE_F32 = 1, QP_BODY_STAGED = 2 };

struct TickPlan {
  PlanFused fused; PlanFront front; PlanQp qp; int tile; PlanQpBody qp_body; int pack2, sweep_block, qp_warm;
  bool obs_split, lane;   // not public: the QP completes b with rhat from the workspace; the per-lane pair (qp == QP_LANE_PAIR)
};
TickPlan plan_tick(int dtype, int observer_order, const wbc_solver_options& o, const Resolved& r, size_t N, bool mats, bool pf, bool warm = false);

int options_from_caller(const wbc_solver_options* opt, wbc_solver_options& o);   // NULL = the defaults; checks struct_size
void plan_to_public(const TickPlan& p, wbc_tick_plan* out);

}  // namespace wbc
