// The one-launch control tick: the whole tick of a batch that fits one round of workgroups as ONE kernel instead of {dyn_sweep -> QP}.  A workgroup owns 16
// consecutive states; its wavefronts are ROLES that hand the 66-word step workspace over in LDS (no launch boundary, no round trip of the workspace through
// memory), and the M / h / Jc stores -- which no role reads back -- drain behind the QP.  At these sizes (the bench default: 4 096 fp64 states = 256 CUs x 16)
// every stage is latency-bound: the kernel lasts as long as the dependent chain of its workgroup's hardest QP.
// Which batches take it: the planner (tick_plan.cpp; the table of DESIGN.md 5); above it the pair tick below and the tile
// tick (tile_tick.hip.hpp) take over, and large batches keep the two-launch tick, whose sweep is bandwidth-bound and wants every lane of eight wavefronts per CU.
// History of the layout and of what was measured on the way: docs/DESIGN_R04.md, docs/DESIGN_R05.md, docs/DESIGN_HISTORY.md.
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "dyn_split.hip.hpp"
#include "qp_struct16.hip.hpp"
#include "integrate.hip.hpp"
#include "com_ref.hip.hpp"
#include "observer.hip.hpp"

namespace wbc {

// fused tick, observer on: the observer role (observer_body: the register-only body of observer.hip.hpp, no LDS parking) is TWO wavefronts -- base rows -> rhat_base,
// which the QP's b waits for; joint rows -> rhat_joint, needed only in the torque map.  (One wavefront doing both, and rnea_step_body as the observer role, were the
// forms of rounds 2-3: docs/DESIGN_R04.md.)  The structural zeros / ones of M and Jc are written by the four QP wavefronts while they wait for the lever arms, not by
// the mass_jac role (~55 store instructions = ~4 us of store issue off that role's path).
constexpr int FUSED_OBS_WAVES = 2;

// The front half is SPLIT by consumer.  Six wavefronts per workgroup of
// 16 states: wave 4 runs rnea_step_body (bias forces h, and the 66-word step workspace -- all the QP needs -- into LDS),
// wave 5 runs mass_jac_body (M, Jc, pf: 3.2 kB/state that nobody on the GPU reads), waves 0..3 wait for wave 4's flag
// and run the GRF QP.  The QP therefore starts after the ~1/3 of the dynamics it depends on, and the CRBA and its
// stores overlap with it on otherwise idle issue slots.  No barrier after the table staging: the hand-over is an
// LDS flag (the four QP waves poll it; all waves of a workgroup are resident, so the producer always runs).
// OBSERVER on: two more wavefronts take the observer role (observer_body: velocities, momenta, gravity terms,
// beta = C^T v - g, the update of {integ, r}), split by rows: wave 6 the base rows (rhat_base -> LDS, flag `oready`; the
// QP's b waits for it), wave 7 the joint rows (rhat_joint -> LDS, counted on `ready`; needed in the torque map only).
// The QP waves subtract rhat from b and tau_partial themselves.
// MATS = false (the caller wants tau, f only): no mass_jac role, and the rnea role runs the single merged force chain.
// Staged hand-over (QpSync, qp_row16.hip.hpp): the rnea role publishes the four lever arms right after its state
// loads and w_des right behind them (`gready` counts both) -- H and its factor need the former only, b the latter --
// rhat follows from the observer role (`oready`,
// first needed for g = -A^T S b) and tau_partial + the own-leg Jacobian blocks when the force recursions are done
// (`ready`, first needed in the torque map).  Observer off, N = 4 096: 25.5 -> 22.5 us per tick.
// WARM ticks, observer off, M/h/Jc wanted, fp64 (fused_split_h): the rnea role is TWO wavefronts (a seventh wavefront; with the observer on the CU's eight slots
// are taken).  Wave 4 runs the ONE merged force recursion RNEA(q, v, vdot_des) -- tau_partial, all the QP's torque map waits for -- and wave 6 the bias-force
// recursion whose only consumer is the caller's h buffer.  The COLD tick keeps both chains on wave 4: there the QP, not the rnea role, ends the tick.
// 1 (default, round 5): the observer role stores r only after the QP wavefronts have read r_prev (QpSync::rp_ack); 0: the unordered read of round 4 (A/B)
// (fp64 only: the fp32 tick fits two six-wavefront workgroups on a CU -- 147 VGPRs, 49 kB LDS -- and a seventh wavefront would end that)
// WARM ticks are another matter: the block set-up ends the QP at about +5.5 us, so the tick ends with the rnea role and its torque map, and taking
// the bias-force chain off that role shows: tick kernel 12.0 -> 11.0 us at 1 024 states, 13.2 -> 12.6 at 4 096, 22.2 -> 21.3 at 8 192 in a closed
// loop of drifting states (13.5 -> 13.2 on the bench's own batch; tools/ab_libs.sh with --closed-loop).  On by default for the warm instantiation.
// (the fp32 WARM instantiation holds 254 registers -- one workgroup per CU whatever the wavefront count; with the split 12.4 -> 12.1 us at 4 096 drifting states: too little
//  to carry another instantiation, so fp64 only)
template <class T, bool OBSERVER, bool MATS, bool WARM = false> constexpr bool fused_split_h() {
  return !OBSERVER && MATS && WARM && sizeof(T) == 8;
}
// Store policy of M, h, Jc, pf (device_types.hpp, store_out): the COLD fp64 tick that writes them stores them write-through, observer off and on.
// 4 096 fp64 states: kernel 13.23 -> 12.15 us, 309 -> 340 M steps/s -- what the tick reaches when it writes no M, h, Jc at all;
// observer on 314 -> 339 M (profiles/r07_store_policy_measure.log).  Warm ticks end with the rnea role, not the QP, and keep plain stores.  So does the pair tick
// (fused_pair_kernel): two runs at 8 192 states gave 397 - 400 -> 412 M, but 6 144 states were not measured, and it takes both to turn it on there.
// fp32 keeps plain stores: with other stores in the role bodies the compiler packs other pairs of fp32 multiplies (v_pk_mul_f32 in place of fused multiply-adds: 49 fewer
// fmas in the fp32 tick), so M came out with other last bits than the warm tick, the two-launch tick and every earlier build give -- and those are compared bit for bit
// (tests/test_gpu_warm.py).  fp64 has no packed arithmetic: its instruction mix, and its bits, are those of the plain-store build.
template <class T, bool MATS, bool WARM> constexpr int fused_store() { return (MATS && !WARM && sizeof(T) == 8) ? ST_WT : ST_PLAIN; }
// The QP wavefronts' own stores -- tau, f, status, iters, the active set: the tick's LAST stores -- are plain stores in the observer-on and warm ticks: write-through
// there gave +1.5 % at 4 096 fp64 states, short of the gain rule on its own, and cost the observer-on tick 1 % (docs/DESIGN_HISTORY.md).
// The cold fp64 observer-off tick is the one whose QP ends the kernel.  Its trips branch around the add-commit that no live row of the wavefront needs (qp_struct16.hip.hpp,
// SKIP), and with the same flag its QP runs the same arithmetic in fewer instructions and stores its results write-through (DIET there; tools/chain_count.py counts the chain).
template <class T, bool OBSERVER, bool WARM> constexpr bool fused_trip_skip() { return !OBSERVER && !WARM && sizeof(T) == 8; }
template <class T, bool OBSERVER, bool MATS, bool WARM = false> constexpr int fused_threads() { return OBSERVER ? 384 + 64 * FUSED_OBS_WAVES : (fused_split_h<T, OBSERVER, MATS, WARM>() ? 448 : 384); }
// WARM: the QP of every state starts from the active set in qa.aset_in (wbc_step_batch_warm: dependent ticks of a closed loop)
// LEAD (observer off: the nine types launch_fused_tick names, k_fused.hip; observer on: empty): leading arguments, ordered by first use, for what the wavefronts need in front of their
// first memory instruction -- q, v, N, the packed joint indices, vdot_des, w_des (the roles' first loads), mask, normals, mu (the QP wavefronts').  The unit is compiled
// with kernel-argument preload (csrc/Makefile): the first 14 dwords behind the segment pointer -- model ... w_des -- arrive in scalar registers at wave launch, so the
// state loads and the table staging no longer start one scalar-memory round trip late; the rest and the structs behind them come by scalar loads that are waited
// for where first used.  The role bodies keep reading the structs: their fields are patched from the leading arguments (the host passes the same values in both
// places).  Measured, 4 096 fp64 states, cold, observer off: 339.2 -> 346.3 M steps/s, kernel 12.17 -> 11.86 us.
// Observer on: no leading arguments.  Those instantiations sit at 251 ... 255 registers, the fourteen more live scalar registers went to vector-register lanes
// (v_readlane 190 -> 474 in the cold fp64 one) and the tick lost 1 % (docs/DESIGN_HISTORY.md).
// (after the patch the struct copies of these eleven fields, as loaded from the argument segment, are dead: nothing reads them, and the compiler drops their loads)
template <class T> WBC_DEV void fused_patch_args(SweepArgs<T>&, QpArgs<T>&) {}
template <class T> WBC_DEV void fused_patch_args(SweepArgs<T>& a, QpArgs<T>& qa, const T* q, const T* v, size_t N, unsigned long long jpack, const T* vdot_des,
                                                 const T* w_des, const int* mask, const T* normals, const T* mu) {
  a.q = q; a.v = v; a.N = N; a.jpack = jpack; a.vdot_des = vdot_des; a.w_des = w_des;
  qa.N = N; qa.jpack = jpack; qa.mask = mask; qa.normals = normals; qa.mu = mu;
}
template <class T, bool OBSERVER, bool MATS, bool WARM = false, class... LEAD>
__global__ __launch_bounds__((fused_threads<T, OBSERVER, MATS, WARM>()), 1) void fused_tick_kernel(const DevModel<T>* __restrict__ model, LEAD... lead, DevParams<T> prm,
                                                                            SweepArgs<T> a, QpArgs<T> qa, QpJidx jmap) {
  fused_patch_args<T>(a, qa, lead...);
  __shared__ __attribute__((aligned(512))) T cst[CST_WORDS];   // (the alignment puts the table FIRST in the workgroup's LDS: within reach of the 16-bit ds_read offset, see dyn_sweep.hip.hpp)
  __shared__ int zidx_s[64];
  __shared__ T wsl[WS_LDS_WORDS * 16];
  __shared__ int ready, gready, oready;   // rnea role done / its lever arms are out / observer role done
  __shared__ int rpack;                   // QP wavefronts that have read r_prev (speculative start): the observer role stores r behind all four
  constexpr bool SPEC_ORDER = OBSERVER && !WARM;
  const int wave = (int)(threadIdx.x >> 6);
  // (issue priorities for the QP wavefronts / the rnea role / everybody above the mass_jac role: 13.2 -> 13.4 ... 13.5 us, DESIGN_R05.md section 9)
#ifdef WBC_FUSED_STAMP   // diagnostic build: the pf output carries the role timestamps (slot, workgroup) instead of foot positions
  double* const stamp = (double*)a.pf;
  const unsigned stampN = (unsigned)a.N;
  a.pf = nullptr;
#define FSTAMP(slot) do { if (stamp) WBC_FSTAMP(stamp, stampN, slot); } while (0)
  if (wave == 0) FSTAMP(0);
#else
#define FSTAMP(slot) do {} while (0)
#endif
  // The four QP wavefronts stage the tables; the producers issue their state loads first and join the ONE workgroup
  // barrier from inside their bodies (EXT = 2), so table staging and state loads share a memory round trip.
  if (wave == 4) {
    int* const gflag = &gready;
    constexpr int RMODE = ((MATS && !fused_split_h<T, OBSERVER, MATS, WARM>()) ? (RS_STEP | RS_H) : RS_STEP) | (fused_store<T, MATS, WARM>() == ST_WT ? RS_WT : 0);
    auto geom_out = [=] __device__() {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(gflag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      FSTAMP(7);
    };
    // (tau_partial handed to the QP wavefronts before the base rows of h are summed, rotated and stored: measured neutral here, profiles/r05*_ab_*taup_first*.log)
    rnea_step_body<T, RMODE, 64, 2>(model, prm, a, cst, wsl, NoWait(), geom_out);
    FSTAMP(8);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");     // my LDS writes first (lgkmcnt only) ...
    if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&ready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // ... then the flag
  } else if (wave == 5) {
    if constexpr (MATS) mass_jac_body<T, 64, 2, 16, (0), MjNoHook, fused_store<T, MATS, WARM>()>(model, a, cst, zidx_s);   // (2: the role writes them LAST)
    else __syncthreads();
    FSTAMP(9);
  } else if (fused_split_h<T, OBSERVER, MATS, WARM>() && wave == 6) {
    if constexpr (fused_split_h<T, OBSERVER, MATS, WARM>()) rnea_step_body<T, RS_H, 64, 2>(model, prm, a, cst, wsl);   // bias forces h -> HBM only
  } else if (OBSERVER && wave == 6) {
    if constexpr (OBSERVER) {
      int* const ack = &rpack;
      auto wait_ack = [ack] __device__() {   // (see QpSync::rp_ack; the QP wavefronts count at about +2.6 us, this role gets here at about +6)
        if constexpr (SPEC_ORDER) { while (__hip_atomic_load(ack, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < 4) __builtin_amdgcn_s_sleep(1); }
      };
      observer_body<T, 64, 2, 1, 16, decltype(wait_ack)>(model, prm, a, cst, wsl, wait_ack);   // base rows
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&oready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      FSTAMP(10);      // (observer builds: slot 10 is the observer role's end, otherwise QP wave 3's)
    }
  } else if (OBSERVER && FUSED_OBS_WAVES == 2 && wave == 7) {
    if constexpr (OBSERVER && FUSED_OBS_WAVES == 2) {
      observer_body<T, 64, 2, 2>(model, prm, a, cst, wsl);                                      // joint rows
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&ready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // counts with the rnea role: both feed the torque map
    }
  } else {
    for (int i = threadIdx.x; i < CST_WORDS; i += 256) cst[i] = model->cst[i];
    if (threadIdx.x < 64) zidx_s[threadIdx.x] = model->zidx[threadIdx.x];
    if (threadIdx.x == 0) { ready = 0; gready = 0; oready = 0; rpack = 0; }
    __syncthreads();
    constexpr int NFIN = (OBSERVER && FUSED_OBS_WAVES == 2) ? 2 : 1;   // rnea role (+ the observer's joint-row wavefront)
#ifdef WBC_FUSED_STAMP
    QpSync sy{&gready, &oready, &ready, 1, 2, 1, NFIN, stamp, stampN};
#else
    QpSync sy{&gready, &oready, &ready, 1, 2, 1, NFIN};   // the QP waits for each piece where it first needs it
#endif
    if constexpr (SPEC_ORDER) sy.rp_ack = &rpack;
    if constexpr (MATS) {
      const int* const zs = zidx_s;
      const unsigned tq = threadIdx.x;
      auto idle = [=] __device__() { if (!a.skip_consts) structural_consts_quarter<T, fused_store<T, MATS, WARM>()>(model, a, zs, tq); };
      qp_body<T, true, OBSERVER, 16, false, 4, decltype(idle), false, WARM ? 1 : 0, 0, fused_trip_skip<T, OBSERVER, WARM>()>(prm, qa, jmap, wsl, &sy, QpWho{0, false}, idle);
    } else
    qp_body<T, true, OBSERVER, 16, false, 4, QpNoIdle, false, WARM ? 1 : 0, 0, fused_trip_skip<T, OBSERVER, WARM>()>(prm, qa, jmap, wsl, &sy);
  }
}

// fused_pair_kernel (round 6): TWO of the observer-off, cold, M/h/Jc-writing tick workgroups above as ONE workgroup of twelve wavefronts and 32 states, for batches
// between one round of the 16-state workgroups and one (fp64) or two (fp32) rounds of pairs.  Why a pair and not launch bounds: the fp64 six-wavefront workgroup holds 214
// registers, so a CU takes one of them and 6 144 states cost two full rounds (23.9 us against 13.3 for 4 096).  Compiled to 168 registers (three wavefronts per SIMD) two of
// them still do NOT share a CU: the dispatcher deals a workgroup's wavefronts to the SIMDs round robin from SIMD 0 -- 2 + 2 + 1 + 1, twice = 4 on SIMD 0 (tools/cores_probe.hip:
// 512 six-wavefront workgroups of 168 registers take 1.5 T, not T; profiles/r06u_cores_probe_168.log; the tick itself, 8 192 states 23.9 -> 26.2 us:
// profiles/r06u_ab_fused_two_per_cu_by_launch_bounds_not_kept.log).
// Twelve wavefronts of ONE workgroup land 3 + 3 + 3 + 3: wavefronts 0 .. 3 / 4 .. 7 the QPs of the first / second 16 states, 8 / 9 their rnea roles, 10 / 11 their mass_jac
// roles -- every SIMD holds two QP wavefronts and one role.  The bodies are those of fused_tick_kernel, untouched: they address state blockIdx.x * 16 + slot, so the second
// half works on the batch's upper half through argument pointers advanced by that many states (scalar registers: `half` is wave-uniform); its QP wavefronts are threads
// 256 .. 511, whose slots 16 .. 31 are folded into the same shift (and into the workspace pointer).  Every lane is live and the component stride N is the same for both
// halves; a batch that is not a multiple of 32 gets one more workgroup anchored at its end (below).
// The price in fp64: the rnea and mass_jac roles spill (52 / 36 dwords per lane at 168 registers; 22 MB of scratch traffic per launch at 8 192 states by PMC) and the halves share
// issue slots -- a pair lasts 18.3 us where a lone workgroup lasts 13.3 (fp32, which does not spill: 15.3 against 12.4) -- so the host runs this form only where it saves a
// round: fp64 4 225 ... 8 192 states (6 144: 23.9 -> 20.0 us, 257 -> 307 M steps/s; 8 192: 24.0 -> 20.4 us, 342 -> 402 M), fp32 4 225 ... 16 384 (8 192: 364 -> 457 M);
// profiles/r06v_ab_fused_pair.log, r06y3_ab_fused_pair_ragged.log, r06zzz_ab_pair_f32.log.  Measured on top and not kept (profiles/r06v_pair_variants.log,
// r06y5_pair_knock_and_layout_not_kept.log): issue priorities, the bias-force recursion behind the mass_jac role, the roles of a half on one SIMD.
// The role bodies park joint transforms and forces in static LDS arrays [word][BLOCK] indexed by the thread within BLOCK: the pair instantiates them with BLOCK = 128, so
// that the role wavefronts of the two halves (threads 512 .. 639 and 640 .. 767: 0 .. 63 and 64 .. 127 within 128) own disjoint columns.
template <class P> WBC_DEV void shift_ptr(P*& p, int off) { if (p) p += off; }
template <class T> WBC_DEV void shift_states(SweepArgs<T>& a, int off) {
  shift_ptr(a.q, off); shift_ptr(a.v, off); shift_ptr(a.M, off); shift_ptr(a.h, off); shift_ptr(a.Jc, off); shift_ptr(a.pf, off); shift_ptr(a.p, off); shift_ptr(a.beta, off);
  shift_ptr(a.w_des, off); shift_ptr(a.vdot_des, off); shift_ptr(a.tau_prev, off); shift_ptr(a.f_prev, off); shift_ptr(a.obs_integ, off); shift_ptr(a.obs_r, off); shift_ptr(a.ws, off);
}
template <class T> WBC_DEV void shift_states(QpArgs<T>& a, int off) {
  shift_ptr(a.ws, off); shift_ptr(a.normals, off); shift_ptr(a.mu, off); shift_ptr(a.mask, off); shift_ptr(a.Jc, off); shift_ptr(a.wdes, off);
  shift_ptr(a.tau, off); shift_ptr(a.f, off); shift_ptr(a.status, off); shift_ptr(a.iters, off); shift_ptr(a.aset_in, off); shift_ptr(a.aset_out, off); shift_ptr(a.rprev, off);
}
constexpr int FUSED_PAIR_THREADS = 768;
template <class T>
__global__ __launch_bounds__(FUSED_PAIR_THREADS) void fused_pair_kernel(const DevModel<T>* __restrict__ model, DevParams<T> prm, SweepArgs<T> a, QpArgs<T> qa, QpJidx jmap) {
  __shared__ __attribute__((aligned(512))) T cst[CST_WORDS];   // one constant table for both halves (first in LDS: see fused_tick_kernel)
  __shared__ int zidx_s[64];
  __shared__ T wsl2[2 * WS_LDS_WORDS * 16];
  __shared__ int flags[2][4];   // per half: rnea role done / its lever arms, w_des are out / (observer: unused)
  const int wave = (int)(threadIdx.x >> 6);
  const int half = __builtin_amdgcn_readfirstlane(wave < 8 ? (wave >> 2) : (wave & 1));
  // Workgroups 0 .. N / 32 - 1: the lower half of the first 32 (N / 32) states on the first half's wavefronts, the upper half on the second's.  N not a multiple of 32: one
  // more workgroup, anchored at the END of the batch -- states N - 32 .. N - 17 and N - 16 .. N - 1.  It recomputes up to 31 states a regular workgroup also owns and stores
  // the same bits (same bodies, same inputs, no observer state to advance): every lane of every workgroup is live.  N >= 64: the bodies test their UNSHIFTED state index
  // against N -- the role wavefronts blockIdx.x * 16 + slot <= 16 pairs + 15, the QP wavefronts of a second half 16 pairs + 31 at most, both < N from two pairs on.
  const int pairs = (int)(a.N >> 5);
  const bool tail = (int)blockIdx.x == pairs;
  const int off = tail ? (int)a.N - 32 + 16 * half - 16 * pairs : (half ? 16 * pairs : 0);   // what the bodies' blockIdx.x * 16 + slot lacks
  T* const wsl = wsl2 + half * (WS_LDS_WORDS * 16);
  int* const ready = &flags[half][0];
  int* const gready = &flags[half][1];
  int* const oready = &flags[half][2];
  if (wave >= 8) {
    shift_states(a, off);
    if (wave < 10) {
      auto geom_out = [=] __device__() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(gready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      };
      rnea_step_body<T, RS_STEP | RS_H, 128, 2>(model, prm, a, cst, wsl, NoWait(), geom_out);   // (128: the role's parking lot has a half per role wavefront -- threads 512 .. 639, 640 .. 767)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(ready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      mass_jac_body<T, 128, 2, 16, (0)>(model, a, cst, zidx_s);
    }
  } else {
    for (int i = threadIdx.x; i < CST_WORDS; i += 512) cst[i] = model->cst[i];
    if (threadIdx.x < 64) zidx_s[threadIdx.x] = model->zidx[threadIdx.x];
    if (threadIdx.x < 8) (&flags[0][0])[threadIdx.x] = 0;
    __syncthreads();
    shift_states(a, off);
    shift_states(qa, half ? off - 16 : off);   // (QP slots 16 .. 31 of threads 256 .. 511: see above; `off` >= 16 for every second half)
#ifdef WBC_FUSED_STAMP
    QpSync sy{gready, oready, ready, 1, 2, 1, 1, nullptr, 0};
#else
    QpSync sy{gready, oready, ready, 1, 2, 1, 1};
#endif
    const int* const zs = zidx_s;
    const unsigned tq = threadIdx.x & 255u;
    auto idle = [=] __device__() { if (!a.skip_consts) structural_consts_quarter<T>(model, a, zs, tq); };
    qp_body<T, true, false, 16, false, 8, decltype(idle), false, 0>(prm, qa, jmap, wsl - (half ? 16 : 0), &sy, QpWho{0, false}, idle);
  }
}

// Persistent rollout (BASELINE.json configs[4]): `horizon` dependent ticks of {tick roles as above, forward
// dynamics + integrator} in ONE launch.  A workgroup owns its 4 or 16 states for the whole horizon, so no tick boundary ever
// leaves the CU: no launch, no HBM round trip of the workspace.
// Layout (round 5; DESIGN.md 4.7 -- the layouts of rounds 1-4, with an integrator wavefront of its own and two barriers per tick, and every placement
// tried on the way are in docs/DESIGN_R04.md 8.0a and profiles/r05*_ab_rollout_*.log; their code went in round 6): the integrator's factorisation
// (phase 1) runs on the mass_jac wavefront behind its LDS image, its right-hand sides / solves / state update (phase 2) on QP wavefront 0 right behind
// the torque map; ONE barrier per tick; the states, this tick's tau / f / h, the planner's references and plans live in LDS images from tick to tick,
// and the caller's buffers are written in the launch's last tick only.
//   SPW = 4 (up to 1 024 rollouts: every CU gets a workgroup and a tick waits for the slowest of 4 QPs): FOUR wavefronts, one per SIMD --
//     wavefront 0  [planner,] QP of the 4 states, then phase 2        wavefront 1  rnea role, its two force recursions side by side in the lanes (RS_LANE2)
//     wavefront 2  mass_jac role, then phase 1 on its own image       wavefront 3  observer, ONE pass over both sets of rows (rhat_base handed to the QP first)
//   SPW = 16: QP x 4 (phase 2 on wavefront 0 behind all four), rnea (tau_partial handed to the QPs before the base rows of h), mass_jac + phase 1,
//     observer base rows and, on a wavefront of their own, joint rows: six / eight wavefronts, two per SIMD.
// tau_prev / f_prev of the observer are the result image's rows of the previous tick (first tick: the caller's buffers).
// TRACK: the CoM planner in the loop (wbc_rollout_tracking_batch): QP wavefront 0 first runs the reference generator (com_reference_body: w_des, vdot_des
// of this tick -> LDS image, optional CoM record) and raises a flag; the rnea role issues its state loads, then waits for that flag.
// WARM: every tick after the first starts its QPs from the previous tick's active set, carried in an LDS word per state (wbc_solver_options.rollout_warm;
// the QP body of these instantiations is the block set-up of qp_struct16.hip.hpp for EVERY tick -- tick 0 from the empty set, or from qa.aset_in when
// the caller continues an earlier rollout).
__host__ __device__ constexpr int rollout_threads(bool observer, int spw) {
  return (spw == 4) ? (256)
       : (spw == 16) ? (observer ? 512 : 384)   // QP x 4, rnea, mass_jac [, observer base rows, joint rows]: no integrator wavefront
       : (observer ? 512 : 448);
}
// PAYLOAD: the plant carries a payload on its trunk (integrate.hip.hpp, PAYLOAD: phase 1 on the mass_jac wavefront, phase 2 on wavefront 0; the controller's
// roles keep the nominal model); `ia` is then a PlantIntegrateArgs.  false: the kernels of round 6, argument layout and code unchanged.
// SCORE (wbc_rollout_scored_batch, score.hip.hpp): phase 2 of the integrator also forms its leg row's share of the tick's cost l_k and keeps the running sum in
// an LDS word per lane of wavefront 0 (a register would be live through the QP, which runs at the full register file); the rows are summed once, behind the
// last tick.  The QP wavefronts leave the tick's status in an LDS word per state beside the result image (QpSync::stat, in front of the fence and flag that
// already hand tau and f over); the goals and q_nom are parked in LDS for the whole launch.  No barrier, flag or store is added to the tick.
// The body is ONE text, rollout_body.inc.hpp, included into both kernels (WBC_RB_SCORE 0 / 1): as a device function shared by the two it changed the register
// allocation of the unscored kernels, which are to stay the code they were.  The scored kernels are instantiated in units of their own (k_rollout.hip,
// -DWBC_ROLLOUT_SCORE=1).
template <class T, bool OBSERVER, bool TRACK, int SPW = 16, bool WARM = false, bool PAYLOAD = false>
__global__ __launch_bounds__(rollout_threads(OBSERVER, SPW), 1) void rollout_kernel(const DevModel<T>* __restrict__ model, DevParams<T> prm,
                                                                         SweepArgs<T> a, QpArgs<T> qa, QpJidx jmap, IntegrateArgsP<T, PAYLOAD> ia,
                                                                         int horizon, const DevRefParams<T>* __restrict__ G, RefArgs<T> ra) {
#define WBC_RB_SCORE 0
#include "rollout_body.inc.hpp"
#undef WBC_RB_SCORE
}
// the scored sibling (always warm: the results do not depend on it, include/wbc_hip.h, and the instantiations stay at T x OBSERVER x TRACK x SPW x PAYLOAD)
template <class T, bool OBSERVER, bool TRACK, int SPW = 16, bool PAYLOAD = false>
__global__ __launch_bounds__(rollout_threads(OBSERVER, SPW), 1) void rollout_scored_kernel(const DevModel<T>* __restrict__ model, DevParams<T> prm,
                                                                         SweepArgs<T> a, QpArgs<T> qa, QpJidx jmap, IntegrateArgsP<T, PAYLOAD> ia,
                                                                         int horizon, const DevRefParams<T>* __restrict__ G, RefArgs<T> ra, ScoreArgs<T> sc) {
  constexpr bool WARM = true;
  const ScoreArgs<T>* const sca = &sc;
#define WBC_RB_SCORE 1
#include "rollout_body.inc.hpp"
#undef WBC_RB_SCORE
}

}  // namespace wbc
