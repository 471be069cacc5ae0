// The body of the persistent rollout kernels (fused_tick.hip.hpp): included into rollout_kernel with WBC_RB_SCORE 0 and into rollout_scored_kernel with
// WBC_RB_SCORE 1 (there `sca` is the launch's ScoreArgs).  No include guard: it is program text of two functions.
  __shared__ __attribute__((aligned(512))) T cst[CST_WORDS];   // (the alignment puts the table FIRST in the workgroup's LDS: within reach of the 16-bit ds_read offset, see dyn_sweep.hip.hpp)
  __shared__ int zidx_s[64];
  __shared__ T wsl[WS_LDS_WORDS * 16];
  __shared__ int ready, gready, oready, mready, rready, fready, qdone, hready;   // (hready, TAUP_FIRST: the rnea role's h is complete in the result image)   // (qdone: QP wavefronts whose tau, f of this tick are in the result image)
  __shared__ int rpack;   // (QpSync::rp_ack: QP wavefronts that have read r_prev in this tick, counted over the ticks)
  // (four wavefronts, one per SIMD: each may use the SIMD's whole register file -- 512 with the accumulation registers; an eight-wavefront form sat at 256 and spilled)
  static_assert(SPW == 4 || SPW == 16, "4 or 16 states per workgroup");
  constexpr int REXT = 3;   // the roles' EXT: 3 = states from the LDS image (dyn_split.hip.hpp, WBC_STATE_MACROS)
  // 4 states: the observer wavefront runs the WHOLE update in one pass (PART 0: both sets of rows share the sweeps; as two passes the joint rows arrived behind
  // the rnea role: 11.8 against 11.1 us per tick, profiles/r05o_ab_rollout_merge.log)
  constexpr bool OBS_ONE = SPW == 4;
  constexpr bool OBS_FIFTH = OBSERVER && FUSED_OBS_WAVES == 2 && (SPW == 16);   // joint rows on their own wavefront
  constexpr int W_JOINT = SPW == 16 ? 7 : 4;
  // the fp64 rnea role does not propagate the own-leg Jacobian blocks -- the torque map takes them from the mass_jac role's image (RS_NOJC): 9.33 -> 9.23 us per
  // tick at 1 024 robots; fp32 7.57 -> 7.62 and cold 15.75 -> 15.86, hence fp64 only (profiles/r05s_ab_rollout_nojc_refimg.log)
  constexpr bool NOJC = sizeof(T) == 8;
  constexpr bool SPEC_ORDER = OBSERVER && !WARM;
  constexpr int QP_WAVES = SPW / 4;
  for (int i = threadIdx.x; i < CST_WORDS; i += blockDim.x) cst[i] = model->cst[i];
  if (threadIdx.x < 64) zidx_s[threadIdx.x] = model->zidx[threadIdx.x];
  if (threadIdx.x == 0) { ready = 0; gready = 0; oready = 0; mready = 0; rready = 0; fready = 0; qdone = 0; hready = 0; rpack = 0; }
  __syncthreads();
  const int wave = (int)(threadIdx.x >> 6);
  // -DWBC_RO_PRIO=1: the rnea role -- the chain a rollout tick waits for (tools/ro_knock.sh) -- at a higher issue priority than QP wavefront 0, its SIMD-mate
  constexpr int W_RNEA = (SPW == 4) ? 1 : 4, W_MJ = (SPW == 4) ? 2 : 5, W_OBS = (SPW == 4) ? 3 : 6;
  // (where the idle QP wavefronts of a 4-state workgroup were tried as hosts of the observer's joint rows, the bias-force recursion and the integrator: docs/DESIGN_R04.md 8.0a,
  //  DESIGN.md 4.7 -- all measured slower than the four-wavefront layout below and removed in round 6; the A/B logs are profiles/r05b_ab_rollout_*.log)
  constexpr int PLAN_WAVE = (TRACK) ? 0 : ((TRACK && SPW == 4) ? 3 : -1);   // (in front of the QP, whose first input -- the lever arms -- the rnea role
                                                                                         // publishes only after it has waited for these references)
  T* const traj0 = ia.tau_traj;
  T* const com0 = ra.com;
  const T* payload = nullptr;   // (PAYLOAD) [10][N], read by both phases of the integrator every tick (L2-resident)
  if constexpr (PAYLOAD) payload = ia.payload;
  // (WARM) the active set of each of the workgroup's states, from tick to tick: one LDS word per state, read and written by the state's own
  // QP row only (a register of the QP wavefronts would be live through every role's code of this 256-register kernel)
  __shared__ int aset_sh[16];
  // what the integrator's factorisation needs of M and Jc, handed over by the mass_jac role in LDS (dyn_split.hip.hpp): with the QP warm-started
  // the tick's barrier waits for that factorisation, not for the QP, and its operands should neither wait for the role's stores to drain
  // nor come back through L2
  __shared__ T mj_hand[MJ_HAND_WORDS * 64];
  // 1: the factorisation (phase 1 of the integrator) runs on the mass_jac wavefront, right behind its image; the integrator wavefront runs the observer's
  // joint rows, waits at the tick barrier and does phase 2 with the factors from an LDS image.  In the stamp build the tick's barrier moves from +10.3 to
  // +9.2 us (profiles/r05g_rollout_timeline_spw4.txt); WITHOUT stamps the tick gets slower -- 12.5 -> 13.1 us at 1 024 robots, fp32 10.6 -> 11.2
  // (profiles/r05g_ab_rollout_*.log): measured, not kept.  0 (default): phase 1 on the integrator wavefront behind the joint rows
// the integrator's state stores without their `if (live)` (integrate.hip.hpp, UNGUARD)
  // (round 5) this tick's tau, f (QP wavefronts) and h (rnea role) for the integrator ALSO in LDS, the tick's first barrier ordering LDS only (the global
  // stores drain until barrier B) and phase 2 reading them there instead of through L2.  Measured (profiles/r05f_ab_rollout_reslds_*.log, us per tick at
  // 1 024 robots, off -> on): fp32 10.57 -> 10.01, fp64 12.51 -> 12.80 (128 robots 12.30 -> 12.67, planner in the loop 15.15 -> 15.6) -- round 4 had seen the
  // same sign for fp64.  1 (default): fp32 kernels only; 0: never; 2: both scalar types (A/B)
  constexpr bool RES_LDS = true;
  __shared__ T fact_sh[true ? INT_FACT_WORDS * 64 : 1];   // the integrator's phase 1 -> phase 2 hand-over (integrate.hip.hpp, PHASE)
  __shared__ T st_sh[SIMG_WORDS * 16];             // the workgroup's states
  __shared__ T ref_sh[(TRACK) ? 24 * 16 : 1];         // (planner in the loop) this tick's references: planner role -> rnea role
  __shared__ T plan_sh[(TRACK) ? PLAN_WORDS * 16 : 1];   // ... and the plans of the workgroup's states
  {
    for (int i = threadIdx.x; i < SIMG_WORDS * 16; i += blockDim.x) {
      const int comp = i >> 4, slot = i & 15;
      size_t st = (size_t)blockIdx.x * SPW + (slot < SPW ? slot : 0);
      st = st < a.N ? st : a.N - 1;
      st_sh[i] = comp < SIMG_V ? a.q[(size_t)comp * a.N + st] : a.v[(size_t)(comp - SIMG_V) * a.N + st];
    }
    if constexpr (TRACK) {
      for (int i = threadIdx.x; i < PLAN_WORDS * 16; i += blockDim.x) {
        const int comp = i >> 4, slot = i & 15;
        size_t st = (size_t)blockIdx.x * SPW + (slot < SPW ? slot : 0);
        st = st < a.N ? st : a.N - 1;
        plan_sh[i] = ra.plan[(size_t)comp * a.N + st];
      }
    }
    if constexpr (!RES_LDS) __syncthreads();
  }
  __shared__ T res_sh[RES_LDS ? (RES_WORDS + 18) * 16 : 1];   // (+ 18 rows: the external torques of the workgroup's states, parked once)
  T* const res_img = RES_LDS ? res_sh : nullptr;
  if constexpr (RES_LDS) {
    for (int i = threadIdx.x; i < 18 * 16; i += blockDim.x) {
      const int comp = i >> 4, slot = i & 15;
      size_t st = (size_t)blockIdx.x * SPW + (slot < SPW ? slot : 0);
      st = st < a.N ? st : a.N - 1;
      res_sh[(RES_WORDS + comp) * 16 + slot] = ia.tau_ext ? ia.tau_ext[(size_t)comp * a.N + st] : (T)0;
    }
    if constexpr (OBSERVER) {   // tau_prev, f_prev of the first tick: the caller's; of every later tick: what the QP left in these rows
      for (int i = threadIdx.x; i < 24 * 16; i += blockDim.x) {
        const int comp = i >> 4, slot = i & 15;
        size_t st = (size_t)blockIdx.x * SPW + (slot < SPW ? slot : 0);
        st = st < a.N ? st : a.N - 1;
        res_sh[i] = comp < 12 ? (a.tau_prev ? a.tau_prev[(size_t)comp * a.N + st] : (T)0) : (a.f_prev ? a.f_prev[(size_t)(comp - 12) * a.N + st] : (T)0);
      }
    }
    __syncthreads();
  }
#if WBC_RB_SCORE
  __shared__ T goal_sh[GOAL_WORDS * 16];   // the goals of the workgroup's states, the weights, the running cost per lane of wavefront 0,
  __shared__ DevScoreW<T> wsc_sh;          // the weights (from LDS they cost phase 2 no scalar registers across the tick), its failed ticks, this tick's status per state
  __shared__ ScoreOut<T> sout_sh;          // where the sums go (read once, behind the last tick)
  __shared__ T cost_sh[64];
  __shared__ int nfail_sh[64];
  __shared__ int stat_sh[16];
  {
    for (int i = threadIdx.x; i < GOAL_WORDS * 16; i += blockDim.x) {
      const int comp = i >> 4, slot = i & 15;
      size_t st = (size_t)blockIdx.x * SPW + (slot < SPW ? slot : 0);
      st = st < a.N ? st : a.N - 1;
      goal_sh[i] = sca->goal[(size_t)comp * a.N + st];
    }
    if (threadIdx.x == 64) { sout_sh.cost = sca->cost; sout_sh.fail = sca->fail; sout_sh.accumulate = sca->accumulate; }
    static_assert(sizeof(DevScoreW<T>) % sizeof(T) == 0, "a struct of scalars");
    if (threadIdx.x < sizeof(DevScoreW<T>) / sizeof(T)) ((T*)&wsc_sh)[threadIdx.x] = ((const T*)&sca->w)[threadIdx.x];
    __syncthreads();
  }
#endif
  auto barrier_A = [] __device__() {
    if constexpr (RES_LDS) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");   // my LDS writes (lgkmcnt only): the global stores keep draining
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    } else __syncthreads();
  };
  if constexpr (WARM) {
    if (threadIdx.x < 16) {
      const size_t sq = (size_t)blockIdx.x * SPW + threadIdx.x;
      aset_sh[threadIdx.x] = (qa.aset_in && sq < a.N && (int)threadIdx.x < SPW) ? qa.aset_in[sq] : 0;
    }
    __syncthreads();
  }
  for (int t = 0; t < horizon; ++t) {
    // The batch size is laundered through an empty asm once per tick: every per-lane address in the role bodies derives
    // from it, so none of that (tick-invariant) address arithmetic is hoisted out of the horizon loop -- hoisted, it
    // occupied ~250 registers for the whole kernel and spilled 1-2 kB per lane.
    unsigned long long n_tick = a.N;
    asm volatile("" : "+s"(n_tick) : : "memory");
    SweepArgs<T> at = a;
    QpArgs<T> qat = qa;
    IntegrateArgs<T> iat = ia;
    at.N = qat.N = iat.N = (size_t)n_tick;
    at.simg = st_sh; iat.simg = st_sh; at.resimg = res_sh; at.refimg = ref_sh;
// 0: every tick stores its q, v (A/B)
    iat.skip_state = (1 && t < horizon - 1) ? 1 : 0;   // q, v of the LAST tick are what the caller finds (the roles read the LDS image)
// 0: every tick stores its M / Jc / pf (A/B)
    at.skip_mats = (1 && t < horizon - 1) ? 1 : 0;   // M, Jc, pf of the LAST tick are what the caller finds in its buffers (as with per-tick launches)
    if (t > 0) at.skip_consts = 1;   // the structural zeros / ones of M, Jc were written by tick 0 of THIS launch into the same buffers (the mass_jac role's
                                     // ~55 store instructions per tick sit in front of the integrator's factorisation: api_rollout.cpp, rollout_persistent)
#ifdef WBC_FUSED_STAMP   // diagnostic build: the last tick's role timestamps go out through the pf output
    double* const rstamp = (t == horizon - 1) ? (double*)a.pf : nullptr;
    const unsigned rstampN = (unsigned)n_tick;
    at.pf = nullptr;
#define RSTAMP(slot) do { if (rstamp) WBC_FSTAMP_S(rstamp, rstampN, slot, SPW); } while (0)
    if (wave == 0) RSTAMP(0);
#else
#define RSTAMP(slot) do {} while (0)
#endif
    auto planner_role = [&]() __attribute__((always_inline)) {   // this tick's references
      if constexpr (TRACK) {
        RefArgs<T> rt = ra;
        rt.N = (size_t)n_tick;
        rt.simg = st_sh; rt.refimg = ref_sh; rt.planimg = plan_sh;
        rt.skip_out = (t < horizon - 1) ? 1 : 0;   // (the caller finds the LAST tick's references in its w_des / vdot_des buffers)
        rt.t = (T)t * prm.dt + ra.t;
        rt.com = com0 ? com0 + (size_t)t * 6 * (size_t)n_tick : nullptr;
        com_reference_body<T, true, SPW, true>(model, G, rt, cst);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");   // w_des, vdot_des are in L2 ...
        if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&rready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // ... then the flag
      }
    };
    auto joint_rows_role = [&]() __attribute__((always_inline)) {
      if constexpr (OBSERVER && FUSED_OBS_WAVES == 2) {
        // the JOINT rows of the observer update (rhat_joint, which the QP needs only in its torque map); wave 6 is left with the base rows,
        // whose rhat_base the QP's b waits for
        observer_body<T, 64, REXT, 2, SPW>(model, prm, at, cst, wsl);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&ready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    };
    if (wave == W_RNEA) {
      int* const rflag = &rready;
      const int rneed = t + 1;
      int* const gflag = &gready;
      // (4-state workgroups: the bias and the acceleration recursion side by side in the lanes -- RS_LANE2, device_types.hpp; -DWBC_RO_LANE2=0: one after the other)
      constexpr int RNEA_MODE = (SPW == 4 ? (RS_STEP | RS_H | RS_LANE2) : (RS_STEP | RS_H)) | (NOJC ? RS_NOJC : 0) | ((TRACK) ? RS_REFIMG : 0);
      auto wait_refs = [rflag, rneed] __device__() {
        if constexpr (TRACK) {
          while (__hip_atomic_load(rflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < rneed) __builtin_amdgcn_s_sleep(1);
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
      };
      auto geom_out = [gflag] __device__() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(gflag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      };
      // (16-state workgroups) tau_partial is handed to the QP BEFORE the base rows of h are summed, rotated and written: only phase 2 of the integrator,
      // behind the torque map, needs those -- it waits for `hready`.  Measured (profiles/r05zz_ab_rollout_taup_first.log): 2 048 rollouts 12.33 -> 12.11 us
      // per tick; the 4-state workgroups LOSE with it (8.84 -> 8.96, planner in the loop 11.39 -> 11.51) and keep the one flag behind the whole body
      // (-DWBC_RO_TAUP_FIRST=2: both; 0: neither)
      constexpr bool TAUP_FIRST = ((SPW == 16));
      if constexpr (TAUP_FIRST) {
        int* const finflag = &ready;
        auto taup_out = [finflag] __device__() {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
          if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(finflag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };
        rnea_step_body<T, RNEA_MODE, 64, REXT, SPW>(model, prm, at, cst, wsl, wait_refs, geom_out, res_img ? res_img + RES_H * 16 : nullptr, taup_out);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&hready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else {
      rnea_step_body<T, RNEA_MODE, 64, REXT, SPW>(model, prm, at, cst, wsl, wait_refs, geom_out, res_img ? res_img + RES_H * 16 : nullptr);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&ready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      RSTAMP(3);   // (WBC_RO_STAMP_ALT) rnea: done
    } else if (wave == W_MJ) {
      int* const mflag = &mready;
      int* const fflag = &fready;
      T* const factp = fact_sh;
      T* const handp = mj_hand;
      const IntegrateArgs<T> ia1 = iat;
      auto publish = [=] __device__() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");   // the hand-over image is in LDS ...
        if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(mflag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // ... then the flag
        RSTAMP(1);   // (WBC_RO_STAMP_ALT) mass_jac: image published
        // phase 1 of the integrator, on my own image (my own LDS words: program order of one lane); the factors are complete when this wavefront
        // reaches the tick barrier, behind which the integrator wavefront reads them
        integrate_body<T, SPW, IntegrateNoWait, 1, true, true, false, IntegrateNoWait, true, PAYLOAD>(model, ia1, IntegrateNoWait(), handp, nullptr, factp,
                                                                                                       IntegrateNoWait(), payload);
           // the factors are in LDS: wavefront 0 may start phase 2
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
          if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(fflag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        
      };
      // (the M / Jc / pf stores to HBM come BEHIND the flag, from the image, and only in the launch's last tick: nothing in this kernel reads them)
      mass_jac_body<T, 64, REXT, SPW, true, decltype(publish)>(model, at, cst, zidx_s, mj_hand, publish);
    } else if (OBSERVER && wave == W_OBS) {
      if constexpr (OBSERVER) {
        int* const ack = &rpack;
        const int ack_need = QP_WAVES * (t + 1);
        const bool ack_on = qa.rprev != nullptr;   // (null: the QP waits for rhat and reads nothing this role writes)
        auto wait_ack = [ack, ack_need, ack_on] __device__() {
          if constexpr (SPEC_ORDER) { if (ack_on) { while (__hip_atomic_load(ack, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < ack_need) __builtin_amdgcn_s_sleep(1); } }
        };
        if constexpr (OBS_ONE) {   // one pass over both sets of rows; rhat_base is handed to the QP as soon as it exists, the joint rows count as a finisher
          int* const oflag = &oready;
          int* const jflag = &ready;
          auto rows_out = [oflag, jflag] __device__(int stage) {   // 0: rhat_base is in the image, 1: rhat_joint is
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(stage == 0 ? oflag : jflag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          };
          observer_body<T, 64, REXT, 0, SPW, decltype(wait_ack), decltype(rows_out)>(model, prm, at, cst, wsl, wait_ack, rows_out);
          RSTAMP(10);
        } else {
        if constexpr (FUSED_OBS_WAVES == 2) observer_body<T, 64, REXT, 1, SPW, decltype(wait_ack)>(model, prm, at, cst, wsl, wait_ack);   // base rows
        else observer_body<T, 64, REXT, 0, SPW, decltype(wait_ack)>(model, prm, at, cst, wsl, wait_ack);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&oready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        RSTAMP(10);
        }
        if constexpr (FUSED_OBS_WAVES == 2 && !OBS_ONE && !OBS_FIFTH) joint_rows_role();   // (-DWBC_RO_MERGE_OBS=2) ... then the joint rows, which the torque map needs ~3 us later
      }
    } else if (OBS_FIFTH && wave == W_JOINT) {
      joint_rows_role();
    } else {
      constexpr int NFIN = (OBSERVER && (FUSED_OBS_WAVES == 2 || OBS_ONE)) ? 2 : 1;   // rnea role (+ the observer's joint rows, run by the integrator wavefront)
#ifdef WBC_FUSED_STAMP
      QpSync sy{&gready, &oready, &ready, 2 * t + 1, 2 * t + 2, t + 1, NFIN * (t + 1), rstamp, rstampN};
#else
      QpSync sy{&gready, &oready, &ready, 2 * t + 1, 2 * t + 2, t + 1, NFIN * (t + 1)};
#endif
      if constexpr (SPEC_ORDER) { if (qa.rprev) sy.rp_ack = &rpack; }
      sy.res = res_img;
#if WBC_RB_SCORE
      sy.stat = stat_sh;
#endif
// 0: every tick stores its tau, f, status, iters (A/B)
      if constexpr (NOJC) { sy.hand = mj_hand; sy.hand_flag = &mready; sy.need_hand = t + 1; }
      sy.skip_out = 1 && t < horizon - 1;   // (the LAST tick's are what the caller finds, as with per-tick launches)
      if constexpr (PLAN_WAVE >= 0) { if (wave == PLAN_WAVE) planner_role(); }
      if constexpr (WARM) {
        qat.aset_out = (t == horizon - 1) ? qa.aset_out : nullptr;   // the set goes out once, behind the last tick
        if (wave * 4 < SPW) qp_body<T, true, OBSERVER, SPW, false, 4, QpNoIdle, false, 2>(prm, qat, jmap, wsl, &sy, QpWho{0, false}, QpNoIdle(), &aset_sh[(threadIdx.x & 255) >> 4]);
      } else
      if (wave * 4 < SPW) qp_body<T, true, OBSERVER, SPW>(prm, qat, jmap, wsl, &sy);   // (SPW = 4: QP wavefront 0 only)
      if constexpr (QP_WAVES > 1) {   // (16 states: four QP wavefronts fill the result image; phase 2 runs behind all of them)
        if (wave * 4 < SPW) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
          if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&qdone, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
              if (wave == 0) {   // phase 2 of the integrator, on the wavefront that has just written tau and f to the LDS image (its own LDS traffic: program order)
          if constexpr (QP_WAVES > 1) { while (__hip_atomic_load(&qdone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < QP_WAVES * (t + 1)) __builtin_amdgcn_s_sleep(1); }
          while (__hip_atomic_load(&fready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < t + 1) __builtin_amdgcn_s_sleep(1);   // M's blocks and the factors
          if constexpr (((SPW == 16))) { while (__hip_atomic_load(&hready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < t + 1) __builtin_amdgcn_s_sleep(1); }   // h
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
          iat.tau_traj = traj0 ? traj0 + (size_t)t * 12 * (size_t)n_tick : nullptr;
#ifdef WBC_FUSED_STAMP
          iat.istamp = rstamp; iat.istampN = rstampN;
          RSTAMP(7);   // phase 2 starts (the factors are there)
#endif
// 1: the tick's barrier in FRONT of this wavefront's stores (integrate.hip.hpp, after_state: measured, not kept)
#if WBC_RB_SCORE
          {
            const ScoreTick<T> stk{&sout_sh, &wsc_sh, goal_sh, cost_sh, nfail_sh, stat_sh, t == 0, t == horizon - 1};
            integrate_body<T, SPW, IntegrateNoWait, 2, true, true, true, IntegrateNoWait, true, PAYLOAD, true>(model, iat, IntegrateNoWait(), mj_hand, res_img,
                                                                                                                     fact_sh, IntegrateNoWait(), payload, &stk);
          }
#else
                      integrate_body<T, SPW, IntegrateNoWait, 2, true, true, true, IntegrateNoWait, true, PAYLOAD>(model, iat, IntegrateNoWait(), mj_hand, res_img,
                                                                                                                   fact_sh, IntegrateNoWait(), payload);
#endif
            RSTAMP(8);
          
        }
      
    }
    __syncthreads(); continue;   // the tick's only barrier: the new state (LDS image), tau, f (memory: the next tick's observer reads them)
    barrier_A();       // barrier A: tau, f (waves 0..3), h (wave 4) are visible to the integrator (round 5: in LDS)
    __syncthreads();   // barrier B: q, v of the next tick -- and this tick's tau, f, h in memory (the next tick's observer role reads tau, f as tau_prev, f_prev)
  }
