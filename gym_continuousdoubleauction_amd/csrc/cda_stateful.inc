// cda_stateful.inc - scripted opponents with memory on the device (include/cda.h cda_stateful_*; the laws: include/cda_stateful_agents.h), included at the very end of
// cda_hip.hip (behind every other kernel: theirs keep their places in the code object).
//
// k_stateful_actions is a READER of the arena in k_script_actions' style, and a copy of its walk, not shared code (the sibling stays instruction for instruction what it
// is): one wave per market, lane a = agent a, both sides of the book in queue order - the tile's orders and then the ring's, 64 per pass (BookSide of
// cda_book_report.inc).  The laws read no volume, so there is no level scan and no quantity load: per side the walk gathers the best price and, in lane a, agent a's own
// order count and the price of its first own order.  Lane a issues the loads of its slot's 32 state bytes (two 16-byte loads) and of its profile's fields BEFORE the walk,
// which hides their latency.  Then the lane reads its net position, builds the view, advances the state (cda_stateful_advance), asks the law (cda_stateful_decide), stores
// the five action words (and a_cont, logp and the sample record, as k_script_actions writes them for a scripted slot) and the state (two 16-byte stores).  Lanes whose slot
// the table does not name write nothing: no action, no state.  Integer state, no atomics, no LDS.

__global__ __launch_bounds__(64 * CDA_WPB) void k_stateful_actions(const uint8_t* arena, Params P, int cap, int first, int n, StatefulArgs S, const long long* counter, long long draw,
                                                                  int32_t* env_cat, float* env_mean, float* env_sigma, int32_t* env_price, int32_t* env_off,
                                                                  float* a_cont, float* logp, float* rec) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w, A = P.cfg.num_agents;
    const long long slot_ix = (long long)mi * A + lane;
    int pidx = -1;
    if (lane < A) { const int s = S.slot[slot_ix]; if (s >= 1 && s <= S.n_profiles) pidx = s - 1; }
    if (__ballot(pidx >= 0) == 0ull) return;                         // (uniform) no stateful slot in this market
    const bool on = pidx >= 0;
    // the slot's state and its profile, requested ahead of the walk (field by field, and the view below likewise: the structs then live in registers - a block copy of
    // the 64 bytes would pin them to scratch)
    longlong2* sp = reinterpret_cast<longlong2*>(S.state + CDA_STATEFUL_WORDS * (on ? slot_ix : 0));
    longlong2 s01 = make_longlong2(0, 0), s23 = make_longlong2(0, 0);
    if (on) { s01 = sp[0]; s23 = sp[1]; }
    const cda_stateful_profile* gp = S.profiles + (on ? pidx : 0);
    cda_stateful_profile pf;
    pf.law = on ? gp->law : 0; pf.size_mean = on ? gp->size_mean : 0.0f; pf.size_sigma = on ? gp->size_sigma : 0.0f; pf.max_position = on ? gp->max_position : 0;
    pf.fast_shift = on ? gp->fast_shift : 0; pf.slow_shift = on ? gp->slow_shift : 1; pf.band_ticks = on ? gp->band_ticks : 0; pf.direction = on ? gp->direction : 1;
    pf.warmup = on ? gp->warmup : 0; pf.patience = on ? gp->patience : 0; pf.p_move_q32 = on ? gp->p_move_q32 : 0ull;
    pf.target = on ? gp->target : 1; pf.start_step = on ? gp->start_step : 0; pf.duration = on ? gp->duration : 1;
    cda_script_view v;
#pragma unroll
    for (int sd = 0; sd < 2; sd++) {
        const BookSide b = book_side(arena, P, cap, mi, sd);
        int32_t bestp = 0, own_best = 0;
        int own_cnt = 0;
        for (int base = 0; base < b.n; base += WAVE) {
            const int i = base + lane;
            const bool valid = i < b.n;
            int32_t p = 0, owner = -1;
            if (valid) { p = b.get(0, i); owner = b.get(2, i) & 15; }
            if (base == 0) bestp = __shfl(p, 0);
            for (int a = 0; a < A; a++) {
                const unsigned long long mk = __ballot(valid && owner == a);
                if (mk == 0ull) continue;                            // (uniform)
                const int32_t pf0 = __shfl(p, __ffsll((long long)mk) - 1);
                if (lane == a) { if (own_cnt == 0) own_best = pf0; own_cnt += __popcll(mk); }
            }
        }
        if (sd == 0) { v.best_bid = bestp; v.own_orders[0] = own_cnt; v.own_best[0] = own_best; }
        else { v.best_ask = bestp; v.own_orders[1] = own_cnt; v.own_best[1] = own_best; }
    }
    if (!on) return;
    const uint8_t* mrec = arena + (size_t)mi * (size_t)P.lay.stride;
    v.t_step = (int32_t)reinterpret_cast<const uint32_t*>(mrec)[H_T_STEP];
    v.net_position = reinterpret_cast<const Acc*>(mrec + P.lay.acc_off)[lane].net_position;
    v.tick = mrow_lane(P, mi).tick_size;
    v.vol[0] = 0; v.vol[1] = 0;                                      // (no law here reads volume)
    int64_t st[CDA_STATEFUL_WORDS] = {(int64_t)s01.x, (int64_t)s01.y, (int64_t)s23.x, (int64_t)s23.y};
    cda_stateful_advance(&pf, pidx, &v, S.seed, counter ? (uint64_t)counter[0] : 0ull, S.market_base + (uint64_t)mi, (uint32_t)draw, (uint32_t)lane, st);
    int32_t c, pr, o; float sm, ss;
    cda_stateful_decide(&pf, &v, st, &c, &sm, &ss, &pr, &o);
    env_cat[slot_ix] = c; env_price[slot_ix] = pr; env_off[slot_ix] = o; env_mean[slot_ix] = sm; env_sigma[slot_ix] = ss;
    if (a_cont) { a_cont[2 * slot_ix] = 0.0f; a_cont[2 * slot_ix + 1] = 0.0f; }
    if (logp) logp[slot_ix] = 0.0f;
    if (rec) {
        float4* rp = reinterpret_cast<float4*>(rec + 8 * slot_ix);
        rp[0] = make_float4(__int_as_float(c), __int_as_float(pr), __int_as_float(o), 0.0f);
        *reinterpret_cast<float2*>(rec + 8 * slot_ix + 4) = make_float2(0.0f, 0.0f);
    }
    sp[0] = make_longlong2((long long)st[0], (long long)st[1]);
    sp[1] = make_longlong2((long long)st[2], (long long)st[3]);
}

extern "C" {

int cda_stateful_attach(cda_env* e, const int32_t* slot_dev, const void* profiles_dev, int32_t n_profiles, int64_t* state_dev, uint64_t seed, uint64_t market_index_base) {
    if (!e || !slot_dev || !profiles_dev || !state_dev || n_profiles < 1 || n_profiles > CDA_STATEFUL_MAX_PROFILES || ((uintptr_t)slot_dev & 3) != 0 ||
        ((uintptr_t)profiles_dev & 7) != 0 || ((uintptr_t)state_dev & 31) != 0) return CDA_ERR_INVALID;      // (the state: 32-byte rows, moved by 16-byte loads and stores)
    if (e->P.cfg.num_agents < 1 || e->P.cfg.num_agents > CDA_MAX_AGENTS) return CDA_ERR_INVALID;
    // both tables are read back and vetted before the env changes: an invalid profile or a slot value outside 0 .. n_profiles changes nothing
    HIPCHK(hipSetDevice(e->device));
    cda_stateful_profile host[CDA_STATEFUL_MAX_PROFILES];
    HIPCHK(hipMemcpy(host, profiles_dev, (size_t)n_profiles * sizeof(cda_stateful_profile), hipMemcpyDeviceToHost));
    for (int k = 0; k < n_profiles; k++) if (!cda_stateful_profile_valid(&host[k])) return CDA_ERR_INVALID;
    const size_t slots = (size_t)e->P.n_markets * (size_t)e->P.cfg.num_agents;
    HostBuf<int32_t> sl(slots);
    if (!sl) return CDA_ERR_NOMEM;
    const hipError_t he = hipMemcpy(sl, slot_dev, slots * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return hip_fail(he, "hipMemcpy(stateful slots)");
    for (size_t i = 0; i < slots; i++) if (sl[i] < 0 || sl[i] > n_profiles) return CDA_ERR_INVALID;
    e->stateful = StatefulArgs{slot_dev, (const cda_stateful_profile*)profiles_dev, state_dev, n_profiles, 0, seed, market_index_base};
    e->stateful_epoch++;
    return CDA_OK;
}
int cda_stateful_detach(cda_env* e) {
    if (!e) return CDA_ERR_INVALID;
    e->stateful = StatefulArgs{};
    e->stateful_epoch++;
    return CDA_OK;
}
int64_t cda_stateful_epoch(const cda_env* e) { return e ? e->stateful_epoch : 0; }
int cda_stateful_attached(const cda_env* e) { return e && e->stateful.slot ? 1 : 0; }

int cda_stateful_actions(cda_env* e, int32_t first_market, int32_t n_markets, const int64_t* counter_dev, int64_t draw,
                         int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset,
                         float* a_cont, float* logp, float* record, void* stream) {
    if (!e || !category || !size_mean || !size_sigma || !price || !price_offset || first_market < 0 || n_markets < 1 || ((uintptr_t)record & 15) != 0 ||
        ((uintptr_t)counter_dev & 7) != 0) return CDA_ERR_INVALID;
    if (!range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->stateful.slot) return CDA_OK;                            // nothing attached: nothing to launch
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_stateful_actions, grid_for(n_markets), dim3(64 * CDA_WPB), 0, (hipStream_t)stream, (const uint8_t*)e->arena, e->P, (int)e->cap, (int)first_market,
                       (int)n_markets, e->stateful, (const long long*)counter_dev, (long long)draw, category, size_mean, size_sigma, price, price_offset, a_cont, logp, record);
    return launch_status();
}

int cda_stateful_advance_host(const void* profiles_host, int32_t n_profiles, const int32_t* profile_index_host, const void* views_host, int64_t n,
                              uint64_t seed, uint64_t counter, const uint64_t* market_host, const uint32_t* draw_host, const uint32_t* agent_host, int64_t* state_inout,
                              int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset) {
    if (!profiles_host || n_profiles < 1 || !profile_index_host || !views_host || n < 0 || !market_host || !draw_host || !agent_host || !state_inout || !category ||
        !size_mean || !size_sigma || !price || !price_offset) return CDA_ERR_INVALID;
    const cda_stateful_profile* pf = (const cda_stateful_profile*)profiles_host;
    const cda_script_view* vw = (const cda_script_view*)views_host;
    for (int32_t k = 0; k < n_profiles; k++) if (!cda_stateful_profile_valid(&pf[k])) return CDA_ERR_INVALID;
    for (int64_t i = 0; i < n; i++) if (profile_index_host[i] < 0 || profile_index_host[i] >= n_profiles) return CDA_ERR_INVALID;
    for (int64_t i = 0; i < n; i++) {
        int64_t* st = state_inout + CDA_STATEFUL_WORDS * i;
        cda_stateful_advance(&pf[profile_index_host[i]], profile_index_host[i], &vw[i], seed, counter, market_host[i], draw_host[i], agent_host[i], st);
        cda_stateful_decide(&pf[profile_index_host[i]], &vw[i], st, &category[i], &size_mean[i], &size_sigma[i], &price[i], &price_offset[i]);
    }
    return CDA_OK;
}
int cda_stateful_profile_check_host(const void* profiles_host, int32_t n_profiles) {
    if (!profiles_host || n_profiles < 1) return CDA_ERR_INVALID;
    for (int32_t k = 0; k < n_profiles; k++) if (!cda_stateful_profile_valid(&((const cda_stateful_profile*)profiles_host)[k])) return CDA_ERR_INVALID;
    return CDA_OK;
}

}  // extern "C"
