// cda_policy_step.inc - k_policy_step for ONE history depth of the observation (the network's input width): included from cda_kernels.inc (256-order tile only)
// once per compiled depth with  CDA_MLP_HIST = the depth (include/cda_mlp.h's layout macros follow it),  PS_NS = the namespace csrc/cda_mlp_dev.inc was included
// into at that depth,  PS_NAME(x) = x with the depth's suffix.  The kernel itself is described at its first inclusion (cda_kernels.inc).
// Included for TWO kernel families:  PS_NET = 0, PS_KERNEL = k_policy_step, PS_KERNARGS = PolicyStepKernArgs  (the tanh network with its own value network, fixed at
// compile time: forward16) and  PS_NET = 1, PS_KERNEL = k_net_step, PS_KERNARGS = NetStepKernArgs  (activation and trunk read from the arguments: forward16_net).
#if !PS_NET
__host__ __device__ constexpr int PS_NAME(policy_step_lds_bytes)(int agents, int n_hist) {
    return DEC_TABLE_BYTES + ZIG_LDS_BYTES + PS_WPB * lds_bytes_per_wave(agents, n_hist) + 16 + PS_NS::F16_LDS_BYTES;
}
#endif
template <bool TALLY>
__global__ __launch_bounds__(64 * PS_WPB, 1) void PS_NAME(PS_KERNEL)(PS_KERNARGS KA) {
    uint8_t* const arena = KA.K.arena;
    const Params& P = KA.K.P;
    const StepArgs& S = KA.K.S;
    const PolicyArgs& F = KA.F;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
    const int mi = S.first_market + (int)blockIdx.x * PS_WPB + wave;
    const bool live = mi < S.end_market;
    const int A = P.cfg.num_agents;
    unsigned long long* ph = nullptr;
#ifdef CDA_PHASE_TIMING
    ph = (S.phase_cycles && live) ? S.phase_cycles + (size_t)mi * 40 : nullptr;     // (tools/policy_step_phases.py: stamps 34 .. 37 = entry, tile staged, forward done, sampled)
#endif
    PH_MARK(ph, 34);
    // the sampling's scalars (rollout counter, log_std), requested at entry: read where the sampling starts they were two dependent memory round trips on the
    // step's critical path (tools/policy_step_phases.py: the sampling segment 2.9 us mean, 6 us for the slowest wave)
    const long long ctr0 = F.counter[0];
    const float ls0 = F.theta[CDA_MLP_OFF_LS], ls1 = F.theta[CDA_MLP_OFF_LS + 1];
    // the tables: the 256-thread staging of k_step, by the first four waves (the others only meet the barrier)
    TablePrefetch tq; tq.wi = tq.ki = tq.jump = 0; tq.rcp = 0.0; tq.pow10 = 0;
    if (wave < 4) tq = stage_tables_issue();
    __builtin_amdgcn_sched_barrier(0);
    const int mc = live ? mi : S.first_market;
    MarketPtrs mp = market_ptrs(arena, P, mc);
    const MarketPrefetch mq = load_market_issue<true>(mp, P, lane);     // the record's requests fly under the whole forward pass
    // this wave's observation row -> the workgroup's bf16 tile
    unsigned char* fwd_base = cda_smem + ((DEC_TABLE_BYTES + ZIG_LDS_BYTES + PS_WPB * lds_bytes_per_wave(A, P.cfg.n_hist) + 15) & ~15);
    const PS_NS::Fwd16Lds T = PS_NS::fwd16_lds(fwd_base);
    {
        constexpr int CH = PS_NS::KX / PS_NS::VW, REAL = PS_NS::OBS / PS_NS::VW, PER = (CH + 63) / 64;    // chunks of VW values per row: REAL of them data, the rest the zero padding to KX
        PS_NS::obsvec v[PER];
        #pragma unroll
        for (int u = 0; u < PER; u++) {
            const int c = lane + 64 * u;
            v[u] = PS_NS::obs_zero();
            if (c < REAL) v[u] = *reinterpret_cast<const PS_NS::obsvec*>(F.obs_in + (size_t)mc * PS_NS::OBS + c * PS_NS::VW);
        }
        PS_NS::WRing<1, PS_NS::KX / 16, PS_PF, false> R1;
        const int half = wave >> 3, grp = (wave >> 1) & 3, jt = wave & 1;
#if PS_NET
        if (!(KA.N.shared_trunk && half))                          // (a shared trunk has no value half: waves 8 .. 15 only meet the forward's barriers)
#endif
        R1.prime(reinterpret_cast<const __bf16*>(F.wb) + CDA_MLP_WB_W1 + (size_t)(256 * half + 64 * grp) * PS_NS::KX + (size_t)jt * (PS_NS::KX / 16) * 512, PS_NS::KX, lane);
        #pragma unroll
        for (int u = 0; u < PER; u++) { const int c = lane + 64 * u; if (c < CH) PS_NS::obs_to_bf16(T.xs + wave * PS_NS::XS_LD + c * PS_NS::VW, v[u], false); }
        if (wave < 4) stage_tables_commit(tq); else __syncthreads();   // (one barrier either way: the tables and the observation tile are in LDS)
        PH_MARK(ph, 35);
#if PS_NET
        PS_NS::forward16_net<PS_PF>(reinterpret_cast<const __bf16*>(F.wb), F.theta, T, wave, lane, R1, KA.N.activation, KA.N.shared_trunk != 0);
#else
        PS_NS::forward16<PS_PF>(reinterpret_cast<const __bf16*>(F.wb), F.theta, T, wave, lane, R1);
#endif
        PH_MARK(ph, 36);
    }
    if (!live) return;
    // sampling: lane a < A draws agent a's action from this market's row of outputs
    LaneAction in;
    in.pres = false; in.ord = 1; in.cat = 0; in.level = 0; in.off = 0; in.mean = 0.0f; in.sigma = 0.0f;
    {
        float l[PS_NS::N_LOGITS];
        #pragma unroll
        for (int q = 0; q < PS_NS::N_LOGITS; q++) l[q] = T.outs[wave * PS_NS::OUTS_LD + q];
        const unsigned long long key = PS_NS::rollout_key(F.seed, ctr0, F.draw);
        const long long i = (long long)mi * A + (lane < A ? lane : 0);
        // (log-std = the free vector + the row's outputs 25, 26: the state-dependent head's offsets, zero in a network without it - as k_mlp_fwd<SAMPLE>)
        const float lsr0 = ls0 + T.outs[wave * PS_NS::OUTS_LD + PS_NS::N_LOGITS + 1], lsr1 = ls1 + T.outs[wave * PS_NS::OUTS_LD + PS_NS::N_LOGITS + 2];
        const PS_NS::SampledAction sa = PS_NS::sample_action(l, key, i, lsr0, lsr1);
        if (lane < A) {
            in.cat = sa.cat; in.level = sa.price; in.off = sa.off; in.mean = sa.size_mean; in.sigma = sa.size_sigma;
            F.category[i] = sa.cat; F.price[i] = sa.price; F.price_offset[i] = sa.off; F.size_mean[i] = sa.size_mean; F.size_sigma[i] = sa.size_sigma;
            F.a_cont[2 * i] = sa.x0; F.a_cont[2 * i + 1] = sa.x1;
            F.logp[i] = sa.logp;
            if (F.rec) {
                float4* rp = reinterpret_cast<float4*>(F.rec + 8 * i);
                rp[0] = make_float4(__int_as_float(sa.cat), __int_as_float(sa.price), __int_as_float(sa.off), sa.x0);
                *reinterpret_cast<float2*>(F.rec + 8 * i + 4) = make_float2(sa.x1, sa.logp);
            }
        }
        if (lane == 0) F.value[mi] = T.outs[wave * PS_NS::OUTS_LD + PS_NS::N_LOGITS];
        if (F.dist) {
            float o24[PS_NS::N_LOGITS];
            PS_NS::dist_row(l, o24);
            float v = 0.0f;
            #pragma unroll
            for (int q = 0; q < PS_NS::N_LOGITS; q++) v = lane == q ? o24[q] : v;
            v = lane == PS_NS::N_LOGITS ? lsr0 : (lane == PS_NS::N_LOGITS + 1 ? lsr1 : v);            // the log-stds the row was sampled with | 2 zeros
            if (lane < CDA_MLP_DIST_LD) F.dist[(size_t)mi * CDA_MLP_DIST_LD + lane] = v;
        }
    }
    PH_MARK(ph, 37);
    // the step: k_step<false> from here on
    Lds& L = wave_lds(P, wave, ZIG_LDS_BYTES);
    const unsigned long long* zig_wi = reinterpret_cast<const unsigned long long*>(cda_smem + DEC_TABLE_BYTES);
    const unsigned long long* zig_ki = zig_wi + 256;
    Mkt m;
#ifdef CDA_PHASE_TIMING
    for (int i = 0; i < 30; i++) m.tacc[i] = 0;
#endif
    load_market_finish<true, false>(mp, P, L, m, mq, lane);
#ifdef CDA_DEBUG_SKIP
    m.dbg = S.dbg_skip;
#endif
    if (__builtin_expect(market_is_cold(m, P), 0)) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");          // the general build reads this step's actions back from the arrays written above
        const int over = slow_step<false>((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave);
        if (over) {
            if constexpr (TALLY) episode_end_after_step((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave, over == 2);
            else reset_after_step((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave);
        }
        return;
    }
    step_loaded<false, false, TALLY ? 1 : 0>(P, S, mp, L, m, in, 1, zig_wi, zig_ki, mi, lane, ph);
    if (__builtin_expect(S.done_out != nullptr && episode_over(m, P, mi), 0)) {
        if constexpr (TALLY) episode_end_after_step((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave, true);
        else reset_after_step((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave);
    }
}
