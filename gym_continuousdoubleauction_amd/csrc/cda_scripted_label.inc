// cda_scripted_label.inc - the label tap: a law's answer for slots it does not play (include/cda.h cda_label_*), included at the very end of cda_hip.hip (behind every
// other kernel: theirs keep their places in the code object).  DAgger asks an expert about the LEARNER's state: its inventory, its resting orders, its place in the queue.
//
// k_script_label is k_script_actions with a second table.  One wave per market, lane a = agent a; the walk is the sibling's, copied as k_sched_orders' is (the
// sibling stays instruction for instruction what it is): both sides of the book in queue order, the tile's orders and then the ring's, 64 per pass, level heads
// by __shfl_up / __ballot, the previous pass's last price and level index carried in uniform registers - once per side, whatever the tables ask.  Per lane there
// are two optional profiles: the ATTACHED one (the env's ScriptArgs; S.slot == NULL: none) and the LABEL one (LabelArgs: a slot table, profiles, seed and market
// base of its own).  Their depth_levels may differ, so a lane carries two volume sums, and volume is summed while the walk is inside the deepest ladder either
// table asks for in this market; every other field of the view is shared.  cda_scripted_decide is called once per table that names a profile for the slot:
//   attached slot   the five env action words, a_cont, logp and the sample record, exactly as k_script_actions writes them
//   labelled slot   the law's five words to the label buffers (the step's row: the host passes the row's base), 0 / 1 to `played`
//   neither         nothing is written anywhere
// Mixing (a labelled slot that is NOT attached): w = cda_script_mix_draw(label seed, counter, market, draw, agent); if its low 32 bits lie below *mix_q32 - a
// word in device memory, so a captured graph follows a beta the host changes between replays - the label also becomes the slot's env action, written as a
// scripted slot's is (a_cont = 0, logp = 0, the record), and played = 1.  A slot that is attached and labelled plays its attached law and is never mixed.
// Integer sums, no atomics, no LDS.

// what a scripted slot's action looks like in a rollout's buffers (k_script_actions' tail, word for word)
__device__ __forceinline__ void label_store_env(long long slot_ix, int32_t c, float sm, float ss, int32_t pr, int32_t o, int32_t* env_cat, float* env_mean, float* env_sigma,
                                                int32_t* env_price, int32_t* env_off, float* a_cont, float* logp, float* rec) {
    env_cat[slot_ix] = c; env_price[slot_ix] = pr; env_off[slot_ix] = o; env_mean[slot_ix] = sm; env_sigma[slot_ix] = ss;
    if (a_cont) { a_cont[2 * slot_ix] = 0.0f; a_cont[2 * slot_ix + 1] = 0.0f; }
    if (logp) logp[slot_ix] = 0.0f;
    if (rec) {
        float4* rp = reinterpret_cast<float4*>(rec + 8 * slot_ix);
        rp[0] = make_float4(__int_as_float(c), __int_as_float(pr), __int_as_float(o), 0.0f);
        *reinterpret_cast<float2*>(rec + 8 * slot_ix + 4) = make_float2(0.0f, 0.0f);
    }
}

// (field by field, as the sibling explains: the struct then lives in registers - a block copy of the 64 bytes would pin it to scratch)
__device__ __forceinline__ void label_load_profile(cda_script_profile& pf, const cda_script_profile* gp, bool on) {
    pf.law = on ? gp->law : 0; pf.size_mean = on ? gp->size_mean : 0.0f; pf.size_sigma = on ? gp->size_sigma : 0.0f;
    pf.max_position = on ? gp->max_position : 0; pf.skew_position = on ? gp->skew_position : 0; pf.max_orders = on ? gp->max_orders : 1;
    pf.depth_levels = on ? gp->depth_levels : 1; pf.imb_num = on ? gp->imb_num : 1; pf.imb_den = on ? gp->imb_den : 1;
    pf.p_trade_q32 = on ? gp->p_trade_q32 : 0ull;
}
__device__ __forceinline__ int label_depth(const cda_script_profile& pf, bool on) {
    return on ? (pf.depth_levels < 1 ? 1 : (pf.depth_levels > CDA_SCRIPT_MAX_DEPTH ? CDA_SCRIPT_MAX_DEPTH : pf.depth_levels)) : 0;
}

__global__ __launch_bounds__(64 * CDA_WPB) void k_script_label(const uint8_t* arena, Params P, int cap, int first, int n, ScriptArgs S, LabelArgs Lb, const long long* counter,
                                                              long long draw, int32_t* env_cat, float* env_mean, float* env_sigma, int32_t* env_price, int32_t* env_off,
                                                              float* a_cont, float* logp, float* rec) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w, A = P.cfg.num_agents;
    const long long slot_ix = (long long)mi * A + lane;
    int pa = -1, pl = -1;                                            // the attached / the label profile of this lane's slot
    if (lane < A) {
        if (S.slot) { const int s = S.slot[slot_ix]; if (s >= 1 && s <= S.n_profiles) pa = s - 1; }
        const int s = Lb.slot[slot_ix]; if (s >= 1 && s <= Lb.n_profiles) pl = s - 1;
    }
    if (__ballot(pa >= 0 || pl >= 0) == 0ull) return;                // (uniform) no slot of this market is named in either table
    cda_script_profile pfa, pfl;
    label_load_profile(pfa, S.profiles + (pa >= 0 ? pa : 0), pa >= 0);
    label_load_profile(pfl, Lb.profiles + (pl >= 0 ? pl : 0), pl >= 0);
    const int depth_a = label_depth(pfa, pa >= 0), depth_l = label_depth(pfl, pl >= 0);
    int dmax = 0;
    for (int d = 1; d <= CDA_SCRIPT_MAX_DEPTH; d++) if (__ballot(depth_a == d || depth_l == d) != 0ull) dmax = d;
    cda_script_view v;
    long long vol_a[2], vol_l[2];
#pragma unroll
    for (int sd = 0; sd < 2; sd++) {
        const BookSide b = book_side(arena, P, cap, mi, sd);
        int lv = -1;                                                 // the carry: level index and price of the previous pass's last order
        int32_t cp = 0, bestp = 0, own_best = 0;
        int own_cnt = 0;
        long long va = 0, vl = 0;
        for (int base = 0; base < b.n; base += WAVE) {
            const int i = base + lane;
            const bool valid = i < b.n;
            int32_t p = 0, q = 0, owner = -1;
            if (valid) { p = b.get(0, i); q = b.get(1, i); owner = b.get(2, i) & 15; }
            if (base == 0) bestp = __shfl(p, 0);
            if (lv < dmax) {                                         // (uniform) still inside the deepest ladder either table asks for
                const int32_t up = __shfl_up(p, 1);
                const unsigned long long heads = __ballot(valid && (lane == 0 ? (lv < 0 || p != cp) : p != up));
                const int level = lv + __popcll(heads & lanes_le(lane));
                const long long vq = wave_scan_sum((long long)q, lane);
                for (int d = 1; d <= dmax; d++) {                    // levels never decrease along the queue: the orders of levels < d are a prefix of the pass
                    const int k = __popcll(__ballot(valid && level < d));
                    if (k == 0) continue;                            // (uniform)
                    const long long sum = __shfl(vq, k - 1);
                    if (depth_a == d) va += sum;
                    if (depth_l == d) vl += sum;
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
        if (sd == 0) { v.best_bid = bestp; v.own_orders[0] = own_cnt; v.own_best[0] = own_best; vol_a[0] = va; vol_l[0] = vl; }
        else { v.best_ask = bestp; v.own_orders[1] = own_cnt; v.own_best[1] = own_best; vol_a[1] = va; vol_l[1] = vl; }
    }
    if (pa < 0 && pl < 0) return;
    const uint8_t* mrec = arena + (size_t)mi * (size_t)P.lay.stride;
    v.t_step = (int32_t)reinterpret_cast<const uint32_t*>(mrec)[H_T_STEP];
    v.net_position = reinterpret_cast<const Acc*>(mrec + P.lay.acc_off)[lane].net_position;
    v.tick = mrow_lane(P, mi).tick_size;
    const uint64_t ctr = counter ? (uint64_t)counter[0] : 0ull;
    int32_t c, pr, o; float sm, ss;
    if (pa >= 0) {
        v.vol[0] = vol_a[0]; v.vol[1] = vol_a[1];
        cda_scripted_decide(&pfa, &v, S.seed, ctr, S.market_base + (uint64_t)mi, (uint32_t)draw, (uint32_t)lane, &c, &sm, &ss, &pr, &o);
        label_store_env(slot_ix, c, sm, ss, pr, o, env_cat, env_mean, env_sigma, env_price, env_off, a_cont, logp, rec);
    }
    if (pl < 0) return;
    v.vol[0] = vol_l[0]; v.vol[1] = vol_l[1];
    cda_scripted_decide(&pfl, &v, Lb.seed, ctr, Lb.market_base + (uint64_t)mi, (uint32_t)draw, (uint32_t)lane, &c, &sm, &ss, &pr, &o);
    Lb.cat[slot_ix] = c; Lb.price[slot_ix] = pr; Lb.off[slot_ix] = o; Lb.mean[slot_ix] = sm; Lb.sigma[slot_ix] = ss;
    int32_t played = 0;
    if (pa < 0 && Lb.mix_q32) {
        const uint64_t wd = cda_script_mix_draw(Lb.seed, ctr, Lb.market_base + (uint64_t)mi, (uint32_t)draw, (uint32_t)lane);
        if ((wd & 0xffffffffULL) < Lb.mix_q32[0]) {
            played = 1;
            label_store_env(slot_ix, c, sm, ss, pr, o, env_cat, env_mean, env_sigma, env_price, env_off, a_cont, logp, rec);
        }
    }
    if (Lb.played) Lb.played[slot_ix] = played;
}

extern "C" {

// the two tables read back and vetted, as cda_scripted_attach vets its own: CDA_OK, or the error to return
static int label_tables_ok(const cda_env* e, const int32_t* slot_dev, const void* profiles_dev, int32_t n_profiles) {
    cda_script_profile host[CDA_SCRIPT_MAX_PROFILES];
    HIPCHK(hipMemcpy(host, profiles_dev, (size_t)n_profiles * sizeof(cda_script_profile), hipMemcpyDeviceToHost));
    for (int k = 0; k < n_profiles; k++) if (!cda_script_profile_valid(&host[k])) return CDA_ERR_INVALID;
    const size_t slots = (size_t)e->P.n_markets * (size_t)e->P.cfg.num_agents;
    HostBuf<int32_t> sl(slots);
    if (!sl) return CDA_ERR_NOMEM;
    const hipError_t he = hipMemcpy(sl, slot_dev, slots * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return hip_fail(he, "hipMemcpy(slot_label)");
    for (size_t i = 0; i < slots; i++) if (sl[i] < 0 || sl[i] > n_profiles) return CDA_ERR_INVALID;
    return CDA_OK;
}
static bool label_table_args_ok(const cda_env* e, const int32_t* slot_dev, const void* profiles_dev, int32_t n_profiles) {
    return e && slot_dev && profiles_dev && n_profiles >= 1 && n_profiles <= CDA_SCRIPT_MAX_PROFILES && ((uintptr_t)slot_dev & 3) == 0 && ((uintptr_t)profiles_dev & 7) == 0 &&
           e->P.cfg.num_agents >= 1 && e->P.cfg.num_agents <= CDA_MAX_AGENTS;
}
static bool label_outputs_ok(const int32_t* category, const float* size_mean, const float* size_sigma, const int32_t* price, const int32_t* price_offset) {
    return category && size_mean && size_sigma && price && price_offset &&
           (((uintptr_t)category | (uintptr_t)size_mean | (uintptr_t)size_sigma | (uintptr_t)price | (uintptr_t)price_offset) & 3) == 0;
}

int cda_label_tap_attach(cda_env* e, const int32_t* slot_label_dev, const void* profiles_dev, int32_t n_profiles, uint64_t seed, uint64_t market_index_base,
                         const uint64_t* mix_q32_dev, int32_t rows, int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset,
                         int32_t* played) {
    if (!label_table_args_ok(e, slot_label_dev, profiles_dev, n_profiles) || !mix_q32_dev || ((uintptr_t)mix_q32_dev & 7) != 0 || rows < 1 ||
        !label_outputs_ok(category, size_mean, size_sigma, price, price_offset) || !played || ((uintptr_t)played & 3) != 0) return CDA_ERR_INVALID;
    // both tables (and the mix word) are read back and vetted before the env changes
    HIPCHK(hipSetDevice(e->device));
    const int rc = label_tables_ok(e, slot_label_dev, profiles_dev, n_profiles);
    if (rc != CDA_OK) return rc;
    uint64_t q = 0;
    HIPCHK(hipMemcpy(&q, mix_q32_dev, sizeof q, hipMemcpyDeviceToHost));
    if (q > 0x100000000ULL) return CDA_ERR_INVALID;
    e->label = LabelArgs{slot_label_dev, (const cda_script_profile*)profiles_dev, n_profiles, rows, seed, market_index_base, mix_q32_dev,
                         category, size_mean, size_sigma, price, price_offset, played};
    e->label_epoch++;
    return CDA_OK;
}
int cda_label_tap_detach(cda_env* e) {
    if (!e) return CDA_ERR_INVALID;
    e->label = LabelArgs{};
    e->label_epoch++;
    return CDA_OK;
}
int64_t cda_label_tap_epoch(const cda_env* e) { return e ? e->label_epoch : 0; }
int cda_label_tap_attached(const cda_env* e) { return e && e->label.slot ? 1 : 0; }

// what cda_scripted_step_actions issues for the stateless family: the scripted launch, the label tap's, or none
static int scripted_step_launch(cda_env* e, int32_t first_market, int32_t n_markets, const int64_t* counter_dev, int32_t t,
                                int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset,
                                float* a_cont, float* logp, float* record, void* stream) {
    if (!e || t < 0) return CDA_ERR_INVALID;
    if (!e->label.slot)                                              // no tap: this IS cda_scripted_actions - the same kernel and launch, or none
        return cda_scripted_actions(e, first_market, n_markets, counter_dev, t, category, size_mean, size_sigma, price, price_offset, a_cont, logp, record, stream);
    if (!category || !size_mean || !size_sigma || !price || !price_offset || first_market < 0 || n_markets < 1 || ((uintptr_t)record & 15) != 0 ||
        ((uintptr_t)counter_dev & 7) != 0 || t >= e->label.rows) return CDA_ERR_INVALID;
    if (!range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    LabelArgs Lb = e->label;                                         // the step's row of the label buffers
    const size_t o = (size_t)t * (size_t)e->P.n_markets * (size_t)e->P.cfg.num_agents;
    Lb.cat += o; Lb.mean += o; Lb.sigma += o; Lb.price += o; Lb.off += o; Lb.played += o;
    hipLaunchKernelGGL(k_script_label, grid_for(n_markets), dim3(64 * CDA_WPB), 0, (hipStream_t)stream, (const uint8_t*)e->arena, e->P, (int)e->cap, (int)first_market,
                       (int)n_markets, e->script, Lb, (const long long*)counter_dev, (long long)t, category, size_mean, size_sigma, price, price_offset, a_cont, logp, record);
    return launch_status();
}
int cda_scripted_step_actions(cda_env* e, int32_t first_market, int32_t n_markets, const int64_t* counter_dev, int32_t t,
                              int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset,
                              float* a_cont, float* logp, float* record, void* stream) {
    const int rc = scripted_step_launch(e, first_market, n_markets, counter_dev, t, category, size_mean, size_sigma, price, price_offset, a_cont, logp, record, stream);
    if (rc != CDA_OK || !e->stateful.slot) return rc;
    // ... and behind it the stateful family's launch (csrc/cda_stateful.inc), with draw = t: a slot both tables name plays its stateful law
    return cda_stateful_actions(e, first_market, n_markets, counter_dev, t, category, size_mean, size_sigma, price, price_offset, a_cont, logp, record, stream);
}

int cda_label_actions(cda_env* e, int32_t first_market, int32_t n_markets, const int32_t* slot_label_dev, const void* profiles_dev, int32_t n_profiles, uint64_t seed,
                      uint64_t market_index_base, const int64_t* counter_dev, int64_t draw, int32_t* category, float* size_mean, float* size_sigma, int32_t* price,
                      int32_t* price_offset, void* stream) {
    if (!label_table_args_ok(e, slot_label_dev, profiles_dev, n_profiles) || !label_outputs_ok(category, size_mean, size_sigma, price, price_offset) ||
        ((uintptr_t)counter_dev & 7) != 0 || first_market < 0 || n_markets < 1 || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    // (asynchronous: the tables are the caller's to keep valid - the kernel ignores a slot value outside 1 .. n_profiles)
    ScriptArgs none; memset(&none, 0, sizeof none);                  // no attached table, no mix word, no `played`, no env action buffers: the labels alone
    const LabelArgs Lb{slot_label_dev, (const cda_script_profile*)profiles_dev, n_profiles, 1, seed, market_index_base, NULL, category, size_mean, size_sigma, price,
                       price_offset, NULL};
    hipLaunchKernelGGL(k_script_label, grid_for(n_markets), dim3(64 * CDA_WPB), 0, (hipStream_t)stream, (const uint8_t*)e->arena, e->P, (int)e->cap, (int)first_market,
                       (int)n_markets, none, Lb, (const long long*)counter_dev, (long long)draw, (int32_t*)NULL, (float*)NULL, (float*)NULL, (int32_t*)NULL, (int32_t*)NULL,
                       (float*)NULL, (float*)NULL, (float*)NULL);
    return launch_status();
}

int cda_label_mix_host(uint64_t seed, uint64_t counter, const uint64_t* market_host, const uint32_t* draw_host, const uint32_t* agent_host, int64_t n, uint64_t mix_q32,
                       int32_t* played_out) {
    if (!market_host || !draw_host || !agent_host || n < 0 || mix_q32 > 0x100000000ULL || !played_out) return CDA_ERR_INVALID;
    for (int64_t i = 0; i < n; i++)
        played_out[i] = (cda_script_mix_draw(seed, counter, market_host[i], draw_host[i], agent_host[i]) & 0xffffffffULL) < mix_q32 ? 1 : 0;
    return CDA_OK;
}

}  // extern "C"
