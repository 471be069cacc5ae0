// Which kernels run a tick.  The measured switches between kernel variants, in ONE place: step_impl launches what plan_tick says, wbc_plan_tick /
// wbc_dispatch_thresholds report it (tests/test_gpu_parity.py straddles every switch with it, so a moved threshold moves the test).  Every number N is
// compared with is a name of plan_consts.hpp, where its measurement is written down.  Plain C++: no HIP header, no device.
#include "tick_plan.hpp"

#include <cstring>

#include "host_internal.hpp"
#include "plan_consts.hpp"

namespace wbc {

constexpr size_t NEVER_MIN = (size_t)-1, ALWAYS_MAX = (size_t)-1;   // a minimum no N reaches; a maximum every N stays below

Resolved resolve_options(int dtype, const wbc_solver_options& o) {
  Resolved r;
  const bool f32 = dtype == WBC_F32;
  // the one-launch rollout and the one-launch tick
  r.fused_max = WBC_FUSED_MAX_ROLLOUT; r.fused_max_noobs = WBC_FUSED_MAX_NOOBS; r.fused_max_obs = WBC_FUSED_MAX_OBS;
  if (o.fused_max >= 0) r.fused_max = r.fused_max_noobs = r.fused_max_obs = (size_t)o.fused_max;
  // observer as its own kernel before the sweep: >= 0 the caller's size, -1 auto, below never; ticks without M / h / Jc outputs have their own auto size
  r.obs_split_min = NEVER_MIN;
  if (o.obs_split_min >= 0) r.obs_split_min = (size_t)o.obs_split_min;
  else if (o.obs_split_min == -1) r.obs_split_min = f32 ? WBC_OBS_SPLIT_MIN_F32 : WBC_OBS_SPLIT_MIN_F64;
  r.obs_split_min_nomats = o.obs_split_min >= 0 ? (size_t)o.obs_split_min
                           : (o.obs_split_min == -1 ? (size_t)(f32 ? WBC_OBS_SPLIT_MIN_NOMATS_F32 : WBC_OBS_SPLIT_MIN_NOMATS_F64) : NEVER_MIN);
  // tiles dealt by predicted work (auto); per-lane QP pair (auto); staged tiles (fp32 solvers)
  r.tile_min = f32 ? WBC_QP_TILE_MIN_F32 : WBC_QP_TILE_MIN_F64;
  r.lane_min = f32 ? WBC_QP_LANE_MIN_F32 : WBC_QP_LANE_MIN_F64;
  r.stile_min = f32 ? (size_t)WBC_STILE_MIN_F32 : NEVER_MIN;
  r.stile_max = f32 ? STILE_MAX_STATES : 0;
  // the whole tick as one launch of 64 / 96 / 128-state workgroups (tile_tick_kernel)
  // (auto only while the kernel-selection options of the two-launch tick are at auto themselves: a caller who names a QP kernel or a front half gets it)
  const bool tt_auto_ok = o.qp_tile == 0 && o.qp_lane == 0 && o.obs_colaunch == 0 && o.obs_split_min == -1;
  r.tt_min = NEVER_MIN; r.tt_max = 0; r.tt_first_min = NEVER_MIN; r.tt_max_noobs32 = 0; r.tt_max_obs = 0;
  if (o.tile_tick > 0 || (o.tile_tick == 0 && tt_auto_ok)) {
    const bool forced = o.tile_tick > 0;
    r.tt_min = forced ? WBC_TILE_TICK_FORCED_MIN : (f32 ? WBC_TILE_TICK_MIN : WBC_TILE_TICK_MIN_F64);
    if (!forced && o.fused_max < 0) r.tt_first_min = r.tt_min;   // in front of the one-launch tick while fused_max is at auto
    if (f32) {
      r.tt_max = ALWAYS_MAX;                          // observer on: every size measured, no upper limit
      r.tt_max_noobs32 = forced ? ALWAYS_MAX : 0;     // observer off: forced only
    } else {
      r.tt_max = forced ? ALWAYS_MAX : (size_t)WBC_TILE_TICK_MAX_F64;          // observer off
      r.tt_max_obs = forced ? ALWAYS_MAX : (size_t)WBC_TILE_TICK_MAX_F64_OBS;  // observer on
    }
  }
  // the one-launch tick as 32-state, twelve-wavefront workgroups (fused_pair_kernel, fused_tick.hip.hpp): observer off, cold, M / h / Jc outputs, N >= 64.
  // Both halves of a pair are resident together, so a round of workgroups is 8 192 states instead of 4 096 -- at the price of the rnea role's spill (168 registers).
  r.pair_min = NEVER_MIN; r.pair_max = 0;
  if (o.fused_pair > 0) { r.pair_min = WBC_FUSED_PAIR_FORCED_MIN; r.pair_max = WBC_FUSED_PAIR_FORCED_MAX; }
  else if (o.fused_pair == 0 && o.fused_max < 0 && o.tile_tick == 0 && tt_auto_ok) { r.pair_min = (size_t)WBC_FUSED_PAIR_MIN; r.pair_max = (size_t)(f32 ? WBC_FUSED_PAIR_MAX_F32 : WBC_FUSED_PAIR_MAX); }
  r.warm_tile_min = f32 ? r.tile_min : (size_t)WBC_WARM_TILE_MIN_F64;
  r.warm_lane_min = f32 ? WBC_WARM_LANE_MIN_F32 : WBC_WARM_LANE_MIN_F64;
  // observer update + observer-free sweep as the two roles of ONE launch (sweep_obs_kernel, observer.hip.hpp)
  r.colaunch_min = NEVER_MIN; r.colaunch_max = 0;
  if (o.obs_colaunch > 0) { r.colaunch_min = 0; r.colaunch_max = ALWAYS_MAX; }
  else if (o.obs_colaunch == 0) { r.colaunch_min = f32 ? WBC_COLAUNCH_MIN_F32 : WBC_COLAUNCH_MIN_F64; r.colaunch_max = f32 ? WBC_COLAUNCH_MAX_F32 : WBC_COLAUNCH_MAX_F64; }
  return r;
}

TickPlan plan_tick(int dtype, int observer_order, const wbc_solver_options& o, const Resolved& r, size_t N, bool mats, bool pf, bool warm) {
  TickPlan p{};
  const bool ob = observer_order > 0, f32 = dtype == WBC_F32;
  const bool dense32 = f32 && N >= (size_t)WBC_F32_DENSE_TILE_MIN;   // the fp32 12 x 12 body's batch sizes
  // (warm ticks: behind the one-launch warm tick and below the warm per-lane pair the COLD tile tick -- its staged tiles report the sets -- beats the two-launch
  //  warm plans: WBC_TT_WARM_MAX_F32; fp64: up to warm_lane_min)
  const bool tt_warm_ok = !warm || (N < (f32 ? (size_t)WBC_TT_WARM_MAX_F32 : r.warm_lane_min) && o.qp_lane <= 0);
  const bool tt64 = mats && !ob && !f32 && tt_warm_ok && N >= r.tt_min && N <= r.tt_max;   // fp64, observer off (configs[1]'s shape): sweep wavefronts, then the staged QP tile of their states
  // fp64, observer on (configs[2]'s shape): NS sweep + NS observer wavefronts, then the staged QP tile; 64-state workgroups in rounds beyond 16 384 states
  const bool tt64o = mats && ob && !f32 && tt_warm_ok && N >= r.tt_min && N <= r.tt_max_obs;
  // fp32, observer on (configs[3]'s shape), even batches: packed sweep + observer wavefronts, staged QP tile
  const bool tt32 = mats && ob && f32 && (N & 1) == 0 && o.f32_pack2 >= 0 && N >= r.tt_min && N <= r.tt_max && tt_warm_ok;
  const bool tt32n = mats && !ob && f32 && (N & 1) == 0 && o.f32_pack2 >= 0 && N >= r.tt_min && N <= r.tt_max_noobs32 && tt_warm_ok;   // ... observer off
  if (mats && !ob && !warm && N >= r.pair_min && N <= r.pair_max) {   // observer off, cold: 32-state workgroups of the one-launch tick
    p.fused = FUSED_PAIR;
    return p;
  }
  // the tile tick's plan, stated once (at most one of the four holds: they differ in scalar type and observer).  Observer on: the sweep | observer roles in
  // front; fp32: the packed sweep; the states per workgroup are the kernel's own.  It goes in front of the one-launch tick from tt_first_min on, behind it otherwise.
  TickPlan tt{};
  const bool tile_tick = tt32n || tt32 || tt64 || tt64o;
  if (tile_tick) {
    tt.fused = FUSED_TILE_TICK; tt.front = ob ? FRONT_SWEEP_OBS_ROLES : FRONT_SWEEP; tt.obs_split = ob; tt.pack2 = f32; tt.sweep_block = 64; tt.qp = QP_TILES; tt.qp_body = QP_BODY_STAGED;
    tt.tile = f32 ? tile_tick_states(N) : (ob ? tile_tick_states_f64_obs(N) : tile_tick_states_f64(N));
  }
  if (tile_tick && !warm && N >= r.tt_first_min) return tt;
  if ((mats || !pf) && N <= (ob ? r.fused_max_obs : r.fused_max_noobs)) {
    // small batch: one launch, 16 states per workgroup, rnea_step | mass_jac | [observer] | QP as wavefront roles and the
    // workspace through LDS (fused_tick.hip.hpp)
    p.fused = FUSED_TICK;
    p.qp_warm = warm;
    return p;
  }
  // tt32: mid-size fp32 observer-on batch: sweep | observer roles and the staged QP tile of the same 128 states per workgroup, one launch (tile_tick.hip.hpp).
  // (warm ticks: only where the cold tiles are the plan anyway -- the kernel reports the sets; from warm_lane_min on the warm per-lane pair stays faster:
  //  230 against 250 us at 262 144 states)
  if (tile_tick) return tt;
  // Large batches solve the QPs one state per lane first, with the dense kernel behind it for what is left (WBC_QP_LANE_MIN_*; warm ticks: WBC_WARM_LANE_MIN_*)
  p.lane = warm ? (o.qp_lane > 0 || (o.qp_lane == 0 && N >= r.warm_lane_min)) : (o.qp_lane > 0 || (o.qp_lane == 0 && N >= r.lane_min));
  if (!mats) {   // no M, h, Jc wanted: the CRBA-free rnea_step kernel is the front half -- large observer-on batches: observer kernel + observer-free rnea_step
    p.obs_split = ob && N >= r.obs_split_min_nomats;
    p.front = p.obs_split ? FRONT_OBS_THEN_RNEA : FRONT_RNEA;
  }
  else if (ob && N >= r.colaunch_min && N <= r.colaunch_max && (!f32 || o.obs_colaunch > 0 || ((N & 1) == 0 && o.f32_pack2 >= 0))) { p.front = FRONT_SWEEP_OBS_ROLES; p.obs_split = true; }   // ... as the two roles of one launch
  else if (ob && N >= r.obs_split_min) { p.front = FRONT_OBS_THEN_SWEEP; p.obs_split = true; }   // observer kernel + observer-free sweep
  else p.front = FRONT_SWEEP;
  if (p.front != FRONT_RNEA && p.front != FRONT_OBS_THEN_RNEA) {   // what the dyn_sweep launcher picks (k_sweep.hip)
    const bool obs_variant = p.front == FRONT_SWEEP && ob;
    p.pack2 = f32 && (N & 1) == 0 && o.f32_pack2 >= 0 && (o.f32_pack2 > 0 || N >= (size_t)WBC_PACK2_MIN_STATES || p.front == FRONT_SWEEP_OBS_ROLES);   // (the two-role launch packs every even fp32 batch)
    const size_t threads = ((N + (p.pack2 ? 2 : 1) - 1) / (p.pack2 ? 2 : 1)) * 4;
    p.sweep_block = (!obs_variant && p.front != FRONT_SWEEP_OBS_ROLES && threads >= BIG_GRID_THREADS) ? 256 : 64;
  }
  // two-kernel ticks deal tiles of states to the wavefronts by predicted work (qp_tile_kernel).  Measured on MI355X, fp64,
  // QP kernel alone, one-wavefront workgroups -> tiles: 34.7 -> 32.7 us at 12 288 states (tiles of 32), 62.4 -> 48.3 at
  // 32 768, 109.6 -> 93.1 at 65 536, 408 -> 350 at 262 144 (tiles of 64; 128 and 256 lose to the workgroup lifetime);
  // below 12 288 states the tiles do not fill the device
  // (round 3, structured QP body, QP stage in us.  fp64 standing batch: one-wave 19.0 / tiles-of-32 19.6 at 12 288; 22.2 / 20.0 / 64: 23.9 at
  //  16 384; 31.2 / 24.6 / 30.3 at 24 576; 32.4 / 31.9 / 29.9 at 28 672; 35.9 / 34.7 / 30.4 at 32 768.  fp32 -- whose tile kernel holds 180
  //  registers, two workgroups per CU, where the one-wave kernel runs four wavefronts per SIMD -- trot batch: 17.0 / 20.8 / 20.5 at 16 384,
  //  19.6 / 31.2 / 20.5 at 24 576, 22.1 / 33.4 / 22.0 at 28 672, 24.3 / 35.7 / 22.7 at 32 768; standing batch 31.3 / 44.1 / 37.2 at 24 576)
  // ONE ROUND OF RESIDENT WORKGROUPS: the tile kernel keeps three workgroups on a CU (146 registers in fp64, 159 in fp32; 768 on the device),
  // and a launch with a few workgroups more than that runs a second, nearly empty round -- QP stage at 36 864 fp64 states: tiles of
  // 64 (576 workgroups, 2.25 per CU) 37.8 us, of 48 (768) 30.8 us; fp32 at 40 960: 64 -> 36.7, 80 (512 workgroups) -> 27.2.  So the tile is the
  // smallest size (steps of 4 / 8: k_qp.hip) that fits the batch into one round.
  int tile = warm ? (o.qp_tile == 0 && N >= r.warm_tile_min && !dense32 ? 0 : -1) : o.qp_tile;   // (warm: the auto tiles only, and never the fp32 12 x 12 body, which reports no set)
  bool staged = false;
  if (tile == 0) {
    if (f32) {
      if (N >= (warm ? r.warm_tile_min : r.stile_min) && N <= r.stile_max) { tile = (int)(((N + 255) / 256 + 3) / 4 * 4); staged = true; }   // one workgroup per CU
      else if (N >= r.tile_min && !dense32) { tile = (int)(((N + 767) / 768 + 7) / 8 * 8); tile = tile < 64 ? 64 : tile; }   // (159 registers since the QP weights stay scalar: three workgroups per CU, but 64-state tiles at two per CU beat 44-state ones at three: 22.2 vs 24.1 us at 32 768)
      else if (dense32) {                      // (beyond: the leaner fp32 body, FOUR workgroups per CU -- k_qp.hip: one round is 1 024 tiles)
        tile = (int)(((N + 1023) / 1024 + 7) / 8 * 8);
        tile = tile > 128 ? 64 : tile;         // (more than one round of 128-state tiles: many rounds of 64-state ones)
      }
    } else if (N >= r.tile_min) {
      tile = (int)(((N + 767) / 768 + 3) / 4 * 4);
      tile = tile < 32 ? 32 : (tile > 64 ? 64 : tile);
    }
  }
  if (tile < 0) tile = 0;
  if (p.lane) { p.qp = QP_LANE_PAIR; p.tile = 0; }
  else { p.qp = tile > 0 ? QP_TILES : QP_GROUP16; p.tile = tile; }
  p.qp_warm = warm && p.qp != QP_TILES;
  if (!warm && o.qp_tile > 0 && f32 && tile <= STILE_MAX_TILE && tile % 4 == 0 && !dense32) staged = true;   // (an explicit qp_tile: staged where the kernel exists)
  p.qp_body = (p.qp == QP_TILES && staged) ? QP_BODY_STAGED : ((p.qp == QP_TILES && dense32 && tile >= 64 && tile <= 128) ? QP_BODY_DENSE_F32 : QP_BODY_STRUCTURED);
  return p;
}

int options_from_caller(const wbc_solver_options* opt, wbc_solver_options& o) {
  wbc_solver_options_default(&o);
  if (opt) {
    if (opt->struct_size == 0 || opt->struct_size > sizeof(o)) return fail(WBC_E_INVALID, "wbc_solver_options.struct_size is not set (call wbc_solver_options_default first)");
    std::memcpy(&o, opt, opt->struct_size);   // a caller built against an older, shorter struct keeps the newer defaults
    o.struct_size = sizeof(o);
  }
  return WBC_OK;
}

void plan_to_public(const TickPlan& p, wbc_tick_plan* out) {
  wbc_tick_plan t;
  std::memset(&t, 0, sizeof(t));
  t.struct_size = sizeof(t);
  t.fused = (int)p.fused; t.front = (int)p.front; t.qp = (int)p.qp; t.qp_tile = p.tile; t.qp_body = (int)p.qp_body; t.sweep_pack2 = p.pack2; t.sweep_block = p.sweep_block;
  t.qp_warm = p.qp_warm;
  const size_t n = out->struct_size && out->struct_size < sizeof(t) ? out->struct_size : sizeof(t);
  std::memcpy(out, &t, n);
  out->struct_size = n;
}

}  // namespace wbc

using namespace wbc;

extern "C" void wbc_solver_options_default(wbc_solver_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(*o);
  o->fused_max = -1;
  o->rollout_persistent = 1;
  o->rollout_spw = 0;
  o->obs_split_min = -1;   // auto
  o->one_zerocopy = 3;   // measured p50 of a one-robot tick on the image (us): 0: 23.0, 1: 20.6, 2: 18.8, 3: 17.1
  o->timing_mode = WBC_TIMING_DISPATCH;
  o->qp_tile = 0;
  o->obs_split_serial = 1;
  o->qp_lane = 0;
  o->f32_pack2 = 0;
  o->keep_structural = 0;
  o->rollout_warm = 1;
  o->multi_threads = 0;
  o->multi_spin_us = 200;
  o->obs_colaunch = 0;
  o->tile_tick = 0;
  o->fused_pair = 0;
}

extern "C" int wbc_plan_tick(int dtype, int observer_order, const wbc_solver_options* opt, size_t N, int with_mats, int with_pf, int warm,
                             wbc_tick_plan* plan) {
  if (!plan || (dtype != WBC_F64 && dtype != WBC_F32) || observer_order < 0 || observer_order > 2) return fail(WBC_E_INVALID, "bad argument");
  wbc_solver_options o;
  const int rc = options_from_caller(opt, o);
  if (rc) return rc;
  plan_to_public(plan_tick(dtype, observer_order, o, resolve_options(dtype, o), N, with_mats != 0, with_pf != 0, warm != 0), plan);
  return WBC_OK;
}

// the batch sizes N at which plan(N) differs from plan(N - 1), ascending (the one-round tile SIZE is not a switch of kernel family
// and is left out: it steps every 3 072 / 6 144 / 8 192 states)
extern "C" int wbc_dispatch_thresholds(int dtype, int observer_order, const wbc_solver_options* opt, int flags, size_t* out, int cap, int* n) {
  const int with_mats = flags & WBC_PLAN_WITH_MATS;
  const bool warm = (flags & WBC_PLAN_WARM) != 0;
  if (!n || (cap > 0 && !out) || (dtype != WBC_F64 && dtype != WBC_F32) || observer_order < 0 || observer_order > 2) return fail(WBC_E_INVALID, "bad argument");
  wbc_solver_options o;
  const int rc = options_from_caller(opt, o);
  if (rc) return rc;
  const Resolved r = resolve_options(dtype, o);
  // candidates: every constant the planner compares N with (+ 1 where the comparison is <=); kept when the plan really changes there.
  // tools/plan_sweep.cpp --check walks every N and fails when a switch is missing here
  const size_t cand[] = {r.pair_min, r.pair_max ? r.pair_max + 1 : NEVER_MIN, (size_t)WBC_TT_WARM_MAX_F32, r.tt_min, r.tt_max + 1, r.tt_max_obs + 1, r.tt_max_noobs32 + 1, r.stile_min, r.stile_max + 1, r.fused_max_noobs + 1, r.fused_max_obs + 1, r.tile_min, r.obs_split_min, r.lane_min, r.warm_tile_min, r.warm_lane_min, r.obs_split_min_nomats, (size_t)WBC_PACK2_MIN_STATES, (size_t)WBC_F32_DENSE_TILE_MIN,
                         BIG_GRID_THREADS / 4, BIG_GRID_THREADS / 2, r.colaunch_min, r.colaunch_max + 1};
  constexpr int NCAND = (int)(sizeof(cand) / sizeof(cand[0]));
  size_t keep[NCAND]; int k = 0;
  for (size_t c : cand) {
    if (c < 2 || c == NEVER_MIN || c > ((size_t)1 << 21)) continue;
    // an odd N never packs: compare like with like (both even) for the fp32 sweep, plain neighbours otherwise
    auto same = [&](size_t a, size_t b) {
      const TickPlan x = plan_tick(dtype, observer_order, o, r, a, with_mats != 0, true, warm), y = plan_tick(dtype, observer_order, o, r, b, with_mats != 0, true, warm);
      return x.fused == y.fused && x.front == y.front && x.qp == y.qp && x.qp_body == y.qp_body && x.pack2 == y.pack2 && x.sweep_block == y.sweep_block && x.qp_warm == y.qp_warm;
    };
    const bool changes = (c % 2 == 0) ? !same(c - 2, c) : !same(c - 1, c + 1);
    if (!changes) continue;
    bool dup = false;
    for (int i = 0; i < k; ++i) dup = dup || keep[i] == c;
    if (!dup) keep[k++] = c;
  }
  for (int i = 0; i < k; ++i) for (int j = i + 1; j < k; ++j) if (keep[j] < keep[i]) { const size_t t = keep[i]; keep[i] = keep[j]; keep[j] = t; }
  // (an even candidate right behind a kept odd one is the same switch seen from the even side -- the plans of fp32 batches are compared even with even)
  for (int i = 1; i < k; ++i) if (keep[i] % 2 == 0 && keep[i - 1] + 1 == keep[i]) { for (int j = i; j + 1 < k; ++j) keep[j] = keep[j + 1]; --k; --i; }
  *n = k;
  for (int i = 0; i < k && i < cap; ++i) out[i] = keep[i];
  return WBC_OK;
}
