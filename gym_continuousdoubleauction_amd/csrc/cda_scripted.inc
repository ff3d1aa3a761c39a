// cda_scripted.inc - scripted opponents on the device (include/cda.h cda_scripted_*; the laws: include/cda_scripted_agents.h), included at the end of cda_hip.hip.
//
// k_script_actions is a READER of the arena: one wave per market walks both sides of the market's book, one after the other, in queue order - the tile's
// orders and then the ring's, 64 per pass (BookSide of cda_book_report.inc) - and gathers, in one walk per side, what k_book_levels and k_book_agents gather in
// two: the side's best price, the volume of the first depth_levels levels (level boundaries: price changes between neighbours, __shfl_up and __ballot, the
// previous pass's last price and level index carried in uniform registers) and, in lane a, agent a's own order count and the price of its first own order.
// Volume is summed only while the walk is inside the largest depth_levels any profile of the market's slots asks for; the own-order counts need the whole
// side.  Then lane a reads its net position, builds the view and asks the law; the five action words (and a_cont, logp and the sample record, as the league's
// random branch writes them) are stored only where slot_script names a profile.  Integer sums, no atomics, no LDS.

__global__ __launch_bounds__(64 * CDA_WPB) void k_script_actions(const uint8_t* arena, Params P, int cap, int first, int n, ScriptArgs S, const long long* counter, long long draw,
                                                                int32_t* env_cat, float* env_mean, float* env_sigma, int32_t* env_price, int32_t* env_off,
                                                                float* a_cont, float* logp, float* rec) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w, A = P.cfg.num_agents;
    const long long slot_ix = (long long)mi * A + lane;
    int pidx = -1;
    if (lane < A) { const int s = S.slot[slot_ix]; if (s >= 1 && s <= S.n_profiles) pidx = s - 1; }
    if (__ballot(pidx >= 0) == 0ull) return;                         // (uniform) no scripted slot in this market
    // (field by field, and the view below likewise: both structs then live in registers - a block copy of the 64 bytes would pin them to scratch)
    const cda_script_profile* gp = S.profiles + (pidx >= 0 ? pidx : 0);
    const bool on = pidx >= 0;
    cda_script_profile pf;
    pf.law = on ? gp->law : 0; pf.size_mean = on ? gp->size_mean : 0.0f; pf.size_sigma = on ? gp->size_sigma : 0.0f;
    pf.max_position = on ? gp->max_position : 0; pf.skew_position = on ? gp->skew_position : 0; pf.max_orders = on ? gp->max_orders : 1;
    pf.depth_levels = on ? gp->depth_levels : 1; pf.imb_num = on ? gp->imb_num : 1; pf.imb_den = on ? gp->imb_den : 1;
    pf.p_trade_q32 = on ? gp->p_trade_q32 : 0ull;
    const int depth = pidx >= 0 ? (pf.depth_levels < 1 ? 1 : (pf.depth_levels > CDA_SCRIPT_MAX_DEPTH ? CDA_SCRIPT_MAX_DEPTH : pf.depth_levels)) : 0;
    int dmax = 0;
    for (int d = 1; d <= CDA_SCRIPT_MAX_DEPTH; d++) if (__ballot(depth == d) != 0ull) dmax = d;
    cda_script_view v;
#pragma unroll
    for (int sd = 0; sd < 2; sd++) {
        const BookSide b = book_side(arena, P, cap, mi, sd);
        int lv = -1;                                                 // the carry: level index and price of the previous pass's last order
        int32_t cp = 0, bestp = 0, own_best = 0;
        int own_cnt = 0;
        long long vol = 0;
        for (int base = 0; base < b.n; base += WAVE) {
            const int i = base + lane;
            const bool valid = i < b.n;
            int32_t p = 0, q = 0, owner = -1;
            if (valid) { p = b.get(0, i); q = b.get(1, i); owner = b.get(2, i) & 15; }
            if (base == 0) bestp = __shfl(p, 0);
            if (lv < dmax) {                                         // (uniform) still inside the deepest ladder asked for
                const int32_t up = __shfl_up(p, 1);
                const unsigned long long heads = __ballot(valid && (lane == 0 ? (lv < 0 || p != cp) : p != up));
                const int level = lv + __popcll(heads & lanes_le(lane));
                const long long vq = wave_scan_sum((long long)q, lane);
                for (int d = 1; d <= dmax; d++) {                    // levels never decrease along the queue: the orders of levels < d are a prefix of the pass
                    const int k = __popcll(__ballot(valid && level < d));
                    if (k == 0) continue;                            // (uniform)
                    const long long sum = __shfl(vq, k - 1);
                    if (depth == d) vol += sum;
                }
                const int lastv = 63 - __clzll((long long)__ballot(valid));
                lv = __shfl(level, lastv); cp = __shfl(p, lastv);
            }
            for (int a = 0; a < A; a++) {
                const unsigned long long mk = __ballot(valid && owner == a);
                if (mk == 0ull) continue;                            // (uniform)
                const int32_t pf0 = __shfl(p, __ffsll((long long)mk) - 1);
                if (lane == a) { if (own_cnt == 0) own_best = pf0; own_cnt += __popcll(mk); }
            }
        }
        if (sd == 0) { v.best_bid = bestp; v.own_orders[0] = own_cnt; v.own_best[0] = own_best; v.vol[0] = vol; }
        else { v.best_ask = bestp; v.own_orders[1] = own_cnt; v.own_best[1] = own_best; v.vol[1] = vol; }
    }
    if (pidx < 0) return;
    const uint8_t* mrec = arena + (size_t)mi * (size_t)P.lay.stride;
    v.t_step = (int32_t)reinterpret_cast<const uint32_t*>(mrec)[H_T_STEP];
    v.net_position = reinterpret_cast<const Acc*>(mrec + P.lay.acc_off)[lane].net_position;
    v.tick = mrow_lane(P, mi).tick_size;
    int32_t c, pr, o; float sm, ss;
    cda_scripted_decide(&pf, &v, S.seed, counter ? (uint64_t)counter[0] : 0ull, S.market_base + (uint64_t)mi, (uint32_t)draw, (uint32_t)lane, &c, &sm, &ss, &pr, &o);
    env_cat[slot_ix] = c; env_price[slot_ix] = pr; env_off[slot_ix] = o; env_mean[slot_ix] = sm; env_sigma[slot_ix] = ss;
    if (a_cont) { a_cont[2 * slot_ix] = 0.0f; a_cont[2 * slot_ix + 1] = 0.0f; }
    if (logp) logp[slot_ix] = 0.0f;
    if (rec) {
        float4* rp = reinterpret_cast<float4*>(rec + 8 * slot_ix);
        rp[0] = make_float4(__int_as_float(c), __int_as_float(pr), __int_as_float(o), 0.0f);
        *reinterpret_cast<float2*>(rec + 8 * slot_ix + 4) = make_float2(0.0f, 0.0f);
    }
}

extern "C" {

int cda_scripted_attach(cda_env* e, const int32_t* slot_script_dev, const void* profiles_dev, int32_t n_profiles, uint64_t seed, uint64_t market_index_base) {
    if (!e || !slot_script_dev || !profiles_dev || n_profiles < 1 || n_profiles > CDA_SCRIPT_MAX_PROFILES || ((uintptr_t)slot_script_dev & 3) != 0 ||
        ((uintptr_t)profiles_dev & 7) != 0) return CDA_ERR_INVALID;
    if (e->P.cfg.num_agents < 1 || e->P.cfg.num_agents > CDA_MAX_AGENTS) return CDA_ERR_INVALID;
    // both tables are read back and vetted before the env changes: an invalid profile or a slot value outside 0 .. n_profiles changes nothing
    HIPCHK(hipSetDevice(e->device));
    cda_script_profile host[CDA_SCRIPT_MAX_PROFILES];
    HIPCHK(hipMemcpy(host, profiles_dev, (size_t)n_profiles * sizeof(cda_script_profile), hipMemcpyDeviceToHost));
    for (int k = 0; k < n_profiles; k++) if (!cda_script_profile_valid(&host[k])) return CDA_ERR_INVALID;
    const size_t slots = (size_t)e->P.n_markets * (size_t)e->P.cfg.num_agents;
    HostBuf<int32_t> sl(slots);
    if (!sl) return CDA_ERR_NOMEM;
    const hipError_t he = hipMemcpy(sl, slot_script_dev, slots * sizeof(int32_t), hipMemcpyDeviceToHost);
    bool ok = he == hipSuccess;
    for (size_t i = 0; ok && i < slots; i++) ok = sl[i] >= 0 && sl[i] <= n_profiles;
    if (he != hipSuccess) return hip_fail(he, "hipMemcpy(slot_script)");
    if (!ok) return CDA_ERR_INVALID;
    e->script.slot = slot_script_dev; e->script.profiles = (const cda_script_profile*)profiles_dev; e->script.n_profiles = n_profiles;
    e->script.seed = seed; e->script.market_base = market_index_base;
    e->script.epoch++;
    return CDA_OK;
}
int cda_scripted_detach(cda_env* e) {
    if (!e) return CDA_ERR_INVALID;
    e->script.slot = NULL; e->script.profiles = NULL; e->script.n_profiles = 0; e->script.seed = 0; e->script.market_base = 0;
    e->script.epoch++;
    return CDA_OK;
}
int64_t cda_scripted_epoch(const cda_env* e) { return e ? e->script.epoch : 0; }
int cda_scripted_attached(const cda_env* e) { return e && e->script.slot ? 1 : 0; }

int cda_scripted_actions(cda_env* e, int32_t first_market, int32_t n_markets, const int64_t* counter_dev, int64_t draw,
                         int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset,
                         float* a_cont, float* logp, float* record, void* stream) {
    if (!e || !category || !size_mean || !size_sigma || !price || !price_offset || first_market < 0 || n_markets < 1 || ((uintptr_t)record & 15) != 0 ||
        ((uintptr_t)counter_dev & 7) != 0) return CDA_ERR_INVALID;
    if (!range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->script.slot) return CDA_OK;                              // nothing attached: nothing to launch
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_script_actions, grid_for(n_markets), dim3(64 * CDA_WPB), 0, (hipStream_t)stream, (const uint8_t*)e->arena, e->P, (int)e->cap, (int)first_market,
                       (int)n_markets, e->script, (const long long*)counter_dev, (long long)draw, category, size_mean, size_sigma, price, price_offset, a_cont, logp, record);
    return launch_status();
}

int cda_scripted_decide_host(const void* profiles_host, int32_t n_profiles, const int32_t* profile_index_host, const void* views_host, int64_t n,
                             uint64_t seed, uint64_t counter, const uint64_t* market_host, const uint32_t* draw_host, const uint32_t* agent_host,
                             int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset) {
    if (!profiles_host || n_profiles < 1 || !profile_index_host || !views_host || n < 0 || !market_host || !draw_host || !agent_host || !category || !size_mean ||
        !size_sigma || !price || !price_offset) return CDA_ERR_INVALID;
    const cda_script_profile* pf = (const cda_script_profile*)profiles_host;
    const cda_script_view* vw = (const cda_script_view*)views_host;
    for (int32_t k = 0; k < n_profiles; k++) if (!cda_script_profile_valid(&pf[k])) return CDA_ERR_INVALID;
    for (int64_t i = 0; i < n; i++) if (profile_index_host[i] < 0 || profile_index_host[i] >= n_profiles) return CDA_ERR_INVALID;
    for (int64_t i = 0; i < n; i++)
        cda_scripted_decide(&pf[profile_index_host[i]], &vw[i], seed, counter, market_host[i], draw_host[i], agent_host[i], &category[i], &size_mean[i], &size_sigma[i],
                            &price[i], &price_offset[i]);
    return CDA_OK;
}
int cda_scripted_profile_check_host(const void* profiles_host, int32_t n_profiles) {
    if (!profiles_host || n_profiles < 1) return CDA_ERR_INVALID;
    for (int32_t k = 0; k < n_profiles; k++) if (!cda_script_profile_valid(&((const cda_script_profile*)profiles_host)[k])) return CDA_ERR_INVALID;
    return CDA_OK;
}

}  // extern "C"
