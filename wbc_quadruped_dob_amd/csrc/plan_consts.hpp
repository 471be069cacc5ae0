// Every batch size at which a tick changes kernel variant, in ONE table, with the measurement that fixed each number.  Plain C++, no HIP header: the
// tick planner (tick_plan.cpp) compares N with these names and nothing else, and launch.hpp includes this header, so the launchers in k_*.hip switch at
// exactly the values that wbc_plan_tick reports.
#pragma once
#include <cstddef>

namespace wbc {

// ---- what the launchers themselves switch on (k_sweep.hip, k_rnea.hip, k_misc.hip, k_qp.hip, k_tile.hip)
// 256-thread workgroups (one constant table for four wavefronts) from two full rounds of 8 waves per CU on
constexpr size_t BIG_GRID_THREADS = (size_t)256 * 8 * 64 * 2;
// fp32 sweep, even N: two states per lane as packed pairs.  Below this the batch does not fill the SIMDs with one state per lane
// either, and the shorter dependent chain per state of the unpacked form wins
constexpr long long WBC_PACK2_MIN_STATES = 32768;
// fp32 tiles of 64 ... 128 states from this batch size on run the leaner dense fp32 body (four workgroups per CU).  Up to one state below it
// (65 536) the gathered fp32 tiles and the warm auto tiles end: the 12 x 12 body reports no active set
constexpr long long WBC_F32_DENSE_TILE_MIN = 65537;

// staged tiles (qp_stile_kernel, fp32 solvers): one workgroup of twelve wavefronts per CU holds ceil(N / 256) states, up to 192 (three 64-column chunks:
// image 80 kB + twelve wavefronts' solver tables 70 kB of the CU's 160 kB of LDS) -- i.e. one round of workgroups up to 49 152 states
constexpr int STILE_MAX_TILE = 192;
constexpr size_t STILE_MAX_STATES = (size_t)STILE_MAX_TILE * 256;
// staged tiles (round 6, fp32 solvers; qp_stile_kernel): ONE workgroup of twelve wavefronts per CU holds the CU's share of the batch and its inputs in LDS.
// Measured on MI355X (profiles/r06b_ab_staged_tiles.log; QP stage in us, one-wavefront workgroups or gathered tiles -> staged): fp32 trot batch 16 384: 17.5 -> 16.2,
// 20 480: 19.9 -> 17.8, 24 576: 20.1 -> 15.6, 28 672: 22.5 -> 17.1, 32 768 (configs[3]'s shard): 22.6 -> 17.2, 40 960: 26.5 -> 20.8, 49 152: 26.9 -> 21.6
constexpr long long WBC_STILE_MIN_F32 = 16384;

// tile_tick_kernel<T, W, NS>: the whole tick of a mid-size observer-on fp32 batch (even N, M / h / Jc outputs) as one launch of `states`-state workgroups
// (64 | 96 | 128: NS = 2 | 3 | 4 packed sweep wavefronts + as many observer wavefronts): sweep | observer roles, then the staged QP tile of the same
// states (tile_tick.hip.hpp).  The host picks the smallest size that makes ONE round of workgroups on the 256 CUs.
constexpr int TILE_TICK_STATES = 128;
// Beyond one round (N > 32 768) 64-state workgroups again, two resident per CU: they drift apart over the rounds, so that one's QP stage (latency-bound) shares the SIMDs with
// the other's roles (issue-bound) -- 49 152 states: 895 -> 960 M steps/s, 262 144: 1 051 -> 1 088; a tie at 65 536 (profiles/r06h_ab_tile_tick_states.log)
inline int tile_tick_states(size_t N) { return N <= 64 * 256 ? 64 : (N <= 96 * 256 ? 96 : (N <= 128 * 256 ? 128 : 64)); }   // (32-state workgroups for <= 8 192 states: measured, no faster -- the tick's floor is ~22 us; r06o)
// fp64, observer off: NS = 2 ... 7 sweep wavefronts of 16 states (a CU's LDS holds seven wavefronts' parking lots), again the smallest one-round size
inline int tile_tick_states_f64(size_t N) { const size_t ns = (N + 4095) / 4096; return 16 * (int)(ns < 2 ? 2 : (ns > 7 ? 7 : ns)); }
// fp64, observer on: NS = 2 ... 4 sweep + as many observer wavefronts of 16 states -- one round of workgroups holds 64 x 256 states, larger batches take several
inline int tile_tick_states_f64_obs(size_t N) { const size_t ns = (N + 4095) / 4096; return 16 * (int)(ns < 2 ? 2 : (ns > 4 ? 4 : ns)); }

// ---- the tile tick's ranges (resolve_options: tt_min, tt_max, tt_first_min, tt_max_obs, tt_max_noobs32)
// fp32, observer on, M / h / Jc outputs, even N (round 6).  Measured on MI355X
// (profiles/r06c_ab_tile_tick.log; M steps/s, sweep_obs / observer + sweep -> staged or gathered tiles / per-lane pair against the tile tick): 12 800: 445 -> 492,
// 16 384: 521 -> 613, 24 576: 750 -> 843, 32 768 (configs[3]'s shard): 913 -> 1 059, 36 864 (a second, nearly empty round of workgroups): 694 -> 719, 49 152: 851 -> 892,
// 65 536: 910 -> 1 123, 98 304: 1 045 -> 1 132, 131 072: 1 002 -> 1 038, 196 608: 927 -> 1 078, 262 144: 993 -> 1 049 -- every size measured, so: no upper limit
// (fp32 below the one-launch tick's limit, profiles/r06o_tile_tick_f32_small.log, one-launch -> tile tick: 8 192: 347 -> 335 but 8 704: 337 -> 353, 10 240: 357 -> 434, 12 288: 413 -> 490:
//  from 8 194 states the tile tick goes in front of the one-launch tick while fused_max is at auto -- tt_first_min, as for fp64 below)
// fp32, observer off: forced only.  Measured on the standing batch (profiles/r06q_tile_tick_f32_noobs.log; M steps/s, default -> tile tick): 16 384: 490 -> 484,
// 24 576: 610 -> 633, 32 768: 688 -> 800, but 49 152: 807 -> 738, 10 240: 343 -> 307, 262 144: 1 254 -> 850 -- no range worth a default
constexpr long long WBC_TILE_TICK_MIN = 8194;
// fp64 observer-off batches (32 ... 112-state workgroups: NS = 2 ... 7 sweep wavefronts; small tiles get helper wavefronts for the QP stage).  fp64 QPs of
// the standing batch iterate 2.5 times per state against the trot batches' 0.5, so the QP stage weighs more and the gain is small, and only while the batch is ONE
// round of workgroups (profiles/r06d_ab_tile_tick_f64.log; M steps/s, default -> tile tick): 11 264: 333 -> 355, 12 288: 347 -> 379, 16 384: 425 -> 475, 24 576: 531 -> 550,
// 28 672: 541 -> 568; but 8 192: 343 -> 287 (the fused tick's role split overlaps QP and dynamics), 32 768: 602 -> 376 (a second round), 262 144: 790 -> 550
// With tau_partial handed over in LDS (profiles/r06j_ab_tile_tick_lds_handover.log, r06k_tile_tick_f64_range.log, r06m_tile_tick_f64_small.log; default -> tile tick): 9 216: 303 -> 324,
// 10 240: 319 -> 350, 11 264: 333 -> 378, 12 288: 348 -> 404, 16 384: 427 -> 501, 24 576: 532 -> 575, 28 672: 546 -> 596; 8 192 (two full rounds of the one-launch tick): 342 -> 305.
// So from 8 193 states on the tile tick also goes IN FRONT of the one-launch tick (tt_first_min) -- while the caller leaves fused_max at auto.
constexpr long long WBC_TILE_TICK_MIN_F64 = 8193;
constexpr long long WBC_TILE_TICK_MAX_F64 = 7 * 16 * 256;   // one round of the largest (112-state) workgroups
// fp64 observer on (NS sweep + NS observer wavefronts of 16 states: 32 / 48 / 64-state workgroups, 64 in rounds beyond 16 384 states), profiles/r06n_tile_tick_f64_obs.log,
// M steps/s default -> tile tick: 8 192: 358 -> 326 (one-launch tick, two full rounds) but 8 704: 311 -> 350, 10 240: 358 -> 398, 12 288: 388 -> 461; against the
// two-launch ticks 12 800: 355 -> 399, 16 384: 416 -> 567, 24 576: 499 -> 525, 32 768: 532 -> 639, 49 152: 614 -> 656, 65 536: 553 -> 578, 98 304: 557 -> 597,
// 131 072: 580 -> 586, 196 608: 571 -> 598, but 262 144: 611 -> 574
constexpr long long WBC_TILE_TICK_MAX_F64_OBS = 196608;
constexpr long long WBC_TILE_TICK_FORCED_MIN = 2;   // wbc_solver_options.tile_tick > 0: every batch the kernel can run
// (warm ticks: behind the one-launch warm tick and below the warm per-lane pair the COLD tile tick -- its staged tiles report the sets -- beats the two-launch warm plans:
//  closed loops of 16 384 drifting states, wall us per tick, warm one-wavefront kernels -> tile tick: fp64 observer off 41.8 -> 38.8, on 44.8 -> 37.1, fp32 37.8 -> 34.4;
//  profiles/r06zz_warm_loop_large.log, r06t_warm_loop_tile_tick.log)
//  fp32 against the warm per-lane pair: 49 152: 75.6 -> 66.5, 65 536: 80.8 -> 76.6, 81 920: 94.0 / 95.4, 98 304: 101 / 108 -- so up to 81 920 states; fp64: up to warm_lane_min)
constexpr long long WBC_TT_WARM_MAX_F32 = 81920;   // warm fp32 observer-on ticks below this run the (cold, set-reporting) tile tick: plan_tick

// ---- the one-launch tick (fused_tick.hip.hpp) and the one-launch rollout
// rollouts of at most fused_max states run as ONE persistent launch (rollout_kernel); ticks of at most fused_max_noobs / fused_max_obs states run as
// ONE kernel (fused_tick.hip.hpp): it still wins with two rounds of workgroups -- since round 3 also with the observer on in fp64
// (M steps/s, two-kernel -> fused: 5 120 states 175 -> 233, 6 144: 220 -> 287, 8 192: 258 -> 331) -- and loses from 12 288 on
// End of round 4 (the observer-on tick's QP no longer waits for rhat, warm ticks end with the dynamics roles): the one-launch tick still wins with THREE
// rounds of workgroups.  M steps/s, two-kernel -> fused: fp64 observer on 9 216: 291 -> 318, 10 240: 317 -> 351, 12 288: 347 -> 377, but 13 312: 384 -> 353;
// fp32 observer on 9 216: 281 -> 344, 12 288: 380 -> 406, 13 312: 360 -> 376, 14 336: 385 -> 347; fp64 observer off 9 216: 295 -> 301, 11 264: 309 -> 328,
// 12 288: 348 -> 342 (warm ticks in a closed loop, kernels in us: observer off 10 240: 30.9 -> 27.6, 12 288: 32.7 -> 30.2; on 10 240: 34.8 -> 32.7).
constexpr long long WBC_FUSED_MAX_ROLLOUT = 4096, WBC_FUSED_MAX_NOOBS = 11264, WBC_FUSED_MAX_OBS = 12288;
// fused_pair_kernel<T>: two 16-state tick workgroups as ONE twelve-wavefront workgroup of 32 states at 168 registers (fp64: the rnea / mass_jac roles spill; fp32: no spill) -- both halves
// resident on a CU together -- for observer-off, cold, M/h/Jc-writing ticks of N >= 64 states
// auto range (wbc_solver_options.fused_pair = 0), measured on MI355X: profiles/r06v_ab_fused_pair.log
// (just above 4 096 states the 16-state workgroups' second round is a handful of workgroups and the pair's tail workgroup costs ~0.9 us: 4 097: 18.7 against 19.7 us, 4 128: 19.0 / 18.8,
//  4 352: 20.0 / 18.5, 5 000: 21.3 / 19.6, 6 000: 24.4 / 20.5, 7 500: 24.4 / 20.3, 8 191: 27.4 / 21.1 -- profiles/r06y3_ab_fused_pair_ragged.log)
// fp32 (observer off): the pair holds 168 registers WITHOUT a spill (the six-wavefront workgroup 152), a pair lasts 15.3 us against 12.4 -- ahead of every other plan from one round of
// 16-state workgroups up to two rounds of pairs (profiles/r06zzz_ab_pair_f32.log, M steps/s default -> pair: 5 000: 245 -> 283, 6 144: 285 -> 352, 8 192: 364 -> 457, 10 240: 341 -> 364,
// 12 288: 369 -> 432, 16 384: 485 -> 527; 24 576: 608 -> 507-549)
constexpr long long WBC_FUSED_PAIR_MIN = 4225, WBC_FUSED_PAIR_MAX = 8192, WBC_FUSED_PAIR_MAX_F32 = 16384;
// wbc_solver_options.fused_pair > 0 (from 64 states: the QP wavefronts of a tail workgroup test their unshifted slots 16 p + 16 .. 31 against N, fused_tick.hip.hpp)
constexpr long long WBC_FUSED_PAIR_FORCED_MIN = 64, WBC_FUSED_PAIR_FORCED_MAX = 65536;

// ---- the two-launch tick's front half
// observer as its own kernel before the sweep (the all-in-one observer sweep runs one wavefront per SIMD).  Measured on
// MI355X, front half of the tick, all-in-one -> observer kernel + observer-free sweep (us): fp64 464 -> 112 + 279 at
// 262 144 states, 111 -> 34 + 57 at 65 536, but 48 -> 25 + 33 at 32 768; fp32 298 -> 57 + 168 at 262 144, 45 -> 17 + 27 at
// 65 536 (a tie per tick), 26 -> 13 + 16 at 32 768.  At the final kernels (observer-free sweep without the w_des forwarding,
// both observer forms with their inputs requested up front) per tick, all-in-one -> split (M steps/s): fp64 437 -> 472 at
// 65 536, 428 -> 446 at 49 152, 405 -> 439 at 40 960, 451 -> 460 at 32 768, 360 -> 398 at 24 576, 308 -> 341 at 20 480, but
// 330 -> 289 at 16 384; fp32 855 -> 934 at 98 304, 784 -> 798 at 65 536, 681 -> 717 at 49 152, 594 -> 629 at 40 960, but
// 625 -> 587 at 32 768.  Round 3 (M steps/s): fp32 570 -> 593 at 34 816, 599 -> 614 at 36 864, 612 -> 638 at 38 912 (past 32 768 states the
// all-in-one fp32 sweep needs a second round of wavefronts: 23.7 -> 37 us).  Default: fp64 from 20 480 states on, fp32 from 33 792.
constexpr long long WBC_OBS_SPLIT_MIN_F64 = 20480, WBC_OBS_SPLIT_MIN_F32 = 33792;
// ticks without M / h / Jc outputs: the all-in-one observer form of rnea_step against observer kernel + observer-free rnea_step.  Measured
// (tools/ab_sweep.sh with AB_EXTRA=--no-mats, M steps/s, all-in-one -> split): fp64 trot batch 12 288: 460 -> 409, 16 384: 393 -> 449, 24 576: 528 -> 581,
// 32 768: 542 -> 648, 65 536: 580 -> 792, 131 072: 649 -> 940, 262 144: 606 -> 967 (rnea_step with the observer inside 332 us; observer kernel 100 +
// observer-free rnea_step 68); fp32 24 576: 688 -> 637, 32 768: 720 -> 759, 65 536: 966 -> 1 163, 131 072: 1 160 -> 1 441, 262 144: 1 149 -> 1 539.
// (The two kernels on two streams lose to one after the other at every size, as with the sweep.)
constexpr long long WBC_OBS_SPLIT_MIN_NOMATS_F64 = 16384;
constexpr long long WBC_OBS_SPLIT_MIN_NOMATS_F32 = 32768;
// observer update + observer-free sweep as the two roles of ONE launch (sweep_obs_kernel, observer.hip.hpp): while both roles' wavefronts are resident
// together -- fp32 with two states per lane: 2 x N / 32 <= 2 048 wavefronts, i.e. up to 32 768 states, BASELINE's configs[3] shard; fp64 (228 registers,
// 21 kB of LDS per one-wavefront workgroup: seven per CU, 1 792 on the device) up to 14 336 states.  Measured (profiles/r05b_ab_colaunch_*.log, M steps/s,
// all-in-one observer sweep -> two roles): fp32 12 290: 351 -> 393, 16 384: 445 -> 498, 20 480: 498 -> 551, 24 576: 586 -> 651, 28 672: 639 -> 679,
// 32 768: 732 -> 779 (the two bodies as two kernels one after the other: 315 / 411 / 467 / 536 / 594 / 630); fp64 12 800: 321 -> 352, 13 312: 385 -> 420,
// 14 336: 386 -> 448, but 16 384 (two rounds): 418 -> 405.
constexpr long long WBC_COLAUNCH_MIN_F32 = 12289;
constexpr long long WBC_COLAUNCH_MAX_F32 = 32768;
constexpr long long WBC_COLAUNCH_MIN_F64 = 12289;
constexpr long long WBC_COLAUNCH_MAX_F64 = 14336;

// ---- the two-launch tick's QP stage
// tiles dealt by predicted work (auto): fp64 from 14 336 states, fp32 from 30 720 (the measurements: plan_tick, at the tile's size)
constexpr long long WBC_QP_TILE_MIN_F64 = 14336, WBC_QP_TILE_MIN_F32 = 30720;
// Large batches solve the QPs ONE STATE PER LANE first (qp_lane_kernel: semismooth Newton on the residual wrench, 64 QPs
// per wavefront, no cross-lane traffic); the few per cent it does not finish go through a device-side list to the dense
// active-set kernel.  No host read: the list length stays on the device, the second launch is grid-stride over it.
// End of round 3, tiles with the predictor hand-over and the scalar weights against the per-lane pair, M steps/s.  fp64 standing batch: a tie from
// 53 248 to 98 304 states (605 / 605, 608 / 605, 606 / 604, 621 / 625, 638 / 639), then the pair: 636 / 690 at 114 688, 644 / 730 at 131 072; fp64 trot
// batch: tiles 531 / 483 at 53 248, 533 / 463 at 57 344, 537 / 503 at 65 536, 554 / 520 at 81 920, 546 / 534 at 98 304, pair 527 / 554 at 114 688.
// fp32 trot batch: tiles 1 043 / 919 at 98 304, 992 / 909 at 131 072, 934 / 911 at 196 608, pair 907 / 951 at 229 376.
// Hence the default: fp64 from 106 496 states on, fp32 from 212 992 (history of the threshold: docs/DESIGN_R04.md 4.3a).
constexpr long long WBC_QP_LANE_MIN_F64 = 106496, WBC_QP_LANE_MIN_F32 = 212992;
// wbc_step_batch_warm (dependent ticks), beyond the fused size.  Below warm_tile_min (fp64 24 576 states, fp32 the cold tile_min) the
// one-wavefront kernel with the block set-up (qp_struct16.hip.hpp); from warm_lane_min on the per-lane kernel started from the previous FACES (one Newton step confirms them;
// qp_lane.hip.hpp) with the hand-over list behind it; in between the COLD tiles, which only report the sets (qp_warm = 0): the warm
// one-wavefront kernel holds 232-252 registers and loses to them there, and the per-lane pair has a floor of two dependent launches (a
// wavefront of the lane kernel 14-19 us, then the hardest handed-over state's cold solve, 11-15 us).  Closed loops of drifting states on
// MI355X, tick in us, cold tiles / warm one-wavefront / warm per-lane: fp64 observer on 36 864: 82.6 / 91.0 / 89.7, 49 152: 102.4 / 110.5 /
// 104.8, 57 344: 124.2 / 133.3 / 121.4, 65 536: 135 / 148 / 129, 262 144: 474 / 533 / 414; fp64 observer off 32 768: 63.8 / 61.9 / 71.7,
// 49 152: 88.3 / 85.5 / 87.9, 65 536: 120 / 115 / 108, 98 304: 168 / 170 / 153; fp32 (QP stage alone) 36 864: 35.5 / 36.3 / 32.4,
// 57 344: 42.7 / 50.6 / 34.2, 98 304: 64.9 / 80.6 / 41.4, whole tick 262 144: 300 / 378 / 230.  wbc_solver_options.qp_lane = -1 / 1 forces either.
// Since the set-up drops rows with negative multipliers instead of restarting cold, the warm one-wavefront kernel against the cold tiles
// (tick in us, cold / warm one-wavefront): fp64 observer off 16 384: 45.4 / 42.2, 24 576: 52.9 / 49.4, 32 768: 61.8 / 58.0, 49 152: 82.6 / 78.7;
// fp64 observer on (a trot batch whose cold solves need 0.9 iterations) 16 384: 46.8 / 45.6, 24 576: 61.8 / 62.2, 32 768: 71.3 / 76.4,
// 49 152: 98.2 / 105.0; fp32 16 384: 45.2 / 43.4, 24 576: 53.0 / 52.6, 32 768: 58.0 / 57.8, 49 152: 78.5 / 82.3 -- it depends on how hard
// the batch's cold solves are; the default takes it up to 24 576 fp64 states, where it wins or ties on both.
constexpr long long WBC_WARM_TILE_MIN_F64 = 24576;   // (warm ticks: the one-wavefront kernel with the block set-up up to here; fp32: the cold WBC_QP_TILE_MIN_F32)
constexpr long long WBC_WARM_LANE_MIN_F64 = 53248;   // (measured: tools/warm_loop.py with WARM_LOOP_LANE=1)
constexpr long long WBC_WARM_LANE_MIN_F32 = 36864;

}  // namespace wbc
