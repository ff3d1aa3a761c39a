// cda_schedule.inc - order schedules (include/cda.h cda_schedule_*): per market and per step of the market's episode a window of explicit messages, played by
// every step entry point ahead of the step.  Included like cda_orders.inc - behind it once per book capacity (CDA_CAP defined: the two kernels), and once at the
// end of cda_hip.hip (the entry points).
//
// k_sched_orders / k_tsched_orders: CDA_WPB waves per workgroup, one wave per market.  A wave first CHOOSES its window - the market's schedule row (sched_of), the
// record's first 32 header words in one 128-byte vector load (t_step and the done mask made uniform with readlane), the market's horizon from its parameter row,
// then the two offsets of window t_step - and leaves at once where nothing plays: no row, the episode over, t_step beyond the schedule, an empty window.  That is
// the common case of sparse flow and costs those small reads, not a record load.  A window that holds messages then runs sched_walk: the walk of
// the order streams (cda_orders.inc), same LDS stage, same register recipe - the record's loads are issued there, behind the choice, together with the first chunk's.
#ifdef CDA_CAP
#ifndef CDA_SCHED_ARGS
#define CDA_SCHED_ARGS
namespace cda {
struct SchedArgs {
    const int32_t* sched_of;     // [n_markets]: the market's schedule row, < 0 = none (NULL: nothing attached)
    const long long* offsets;    // [n_sched][n_steps + 1]: row r owns, for step t, messages offsets[r][t] .. offsets[r][t + 1]
    const uint4* msgs;           // cda_order_msg[]
    long long* counts;           // [n_markets][4], env-owned: messages done, rejected, invalid, fills - cumulative since the attach
    long long n_msgs;            // messages behind `msgs`: a window that reaches beyond them plays nothing
    int32_t n_sched, n_steps;
    uint32_t flags;              // CDA_SCHEDULE_*
    int32_t pad;
};
}
#endif
namespace cda { namespace CDA_CAPNS {

// The message walk of order_stream<TAPE> (cda_orders.inc), restated: the messages msgs[b .. b + rem), rem >= 1, into market mi - its record loaded once and stored
// once, the same LDS stage (order_stage / stage_chunk), the same own_lane / pin_market discipline, 16-byte vector loads, chunks of 64; no result records leave.
// `report(n_done, n_rej, n_inv, fills, ln)` runs once behind the last message and before the store, for every lane (ln: a lane index of its own).  The walk is a
// copy and not a function the two share: with order_stream split into "choose" and "walk" the compiler scheduled k_order_stream / k_tape_order_stream differently
// (tools/kernel_identity.py: 4 functions, 29 - 70 instructions fewer each), and those kernels stay the parent's instruction for instruction.
// -DCDA_SCHED_LOADS_FIRST (a measurement build only, tools/order_schedule_cost.py --alt-root): the record's requests are issued AHEAD of the window's choice and
// handed to the walk - what an empty window then pays for nothing, against what a played window saves (DESIGN.md: which won).
#ifdef CDA_SCHED_LOADS_FIRST
#define CDA_SCHED_EARLY_PARAM , const MarketPrefetch& early
#define CDA_SCHED_EARLY_ARG , early
#else
#define CDA_SCHED_EARLY_PARAM
#define CDA_SCHED_EARLY_ARG
#endif
template <bool TAPE, class Report>
__device__ __forceinline__ void sched_walk(uint8_t* arena, const Params& P, int mi, const uint4* msgs, long long b, long long rem, uint32_t flags,
                                           const TapeArgs* T, int wave, int lane, Report report CDA_SCHED_EARLY_PARAM) {
    const int A = P.cfg.num_agents;
    const uint4* mp_msgs = msgs + b;
    Lds& L = wave_lds(P, wave);
    uint4* stage = order_stage(P, wave);
    MarketPtrs mp = market_ptrs(arena, P, mi);
    Mkt m;
    unsigned long long vmask;
    {
        // the record's requests and the first chunk's are in flight together: ONE round trip before the first message runs
#ifdef CDA_SCHED_LOADS_FIRST
        const MarketPrefetch& pre = early;
#else
        const MarketPrefetch pre = load_market_issue<false>(mp, P, lane);
#endif
        const uint4 q = mp_msgs[(long long)lane < rem ? lane : 0];   // (every lane asks: no branch, hence no wait, around the load)
        load_market_finish<false, true>(mp, P, L, m, pre, lane);
        vmask = stage_chunk(stage, q, rem < WAVE ? (int)rem : WAVE, A);
    }
    if constexpr (TAPE) tape_begin(*T, mi, m);
    int n_done = 0, n_rej = 0, n_inv = 0;
    bool placed = false;
    for (long long base = 0; base < rem; base += WAVE) {
        const int cnt = rem - base < WAVE ? (int)(rem - base) : WAVE;
        n_inv += cnt - __popcll(vmask);
        for (int k = 0; k < cnt; k++) {
            if (!((vmask >> k) & 1ull)) continue;                    // (uniform) skipped: outside the hook's domain
            // A lane index of the iteration's own (own_lane): the hook's body is straight-line code, and so it stays here.  With the kernel's one `lane` the
            // compiler hoists the body's lane predicates (owner lane, helper group) out of the walk as 0 / 1 words and spills them across it.
            const int ln = own_lane(k);
            const uint4 q = stage[k];                                // one address for the wave: a broadcast read, made scalar below
            const uint32_t tts = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.z);
            const int type = (int)((tts >> 16) & 0xffu);
            const int fills0 = m.fills, rest0 = __builtin_amdgcn_readfirstlane(total_orders(L, m));
            int32_t status = CDA_ORD_DONE, dpos = 0;
            if (type == CDA_OP_MARK) mark_to_mkt(L, m, A, ln);
            else {
                const int tr = (int)(tts & 0xffffu), side = (int)(tts >> 24);
                const int32_t price = __builtin_amdgcn_readfirstlane((int)q.x), size = __builtin_amdgcn_readfirstlane((int)q.y);
                const int32_t pos0 = __builtin_amdgcn_readfirstlane(L.acc[tr].net_position), rej0 = __builtin_amdgcn_readfirstlane(L.acc[tr].num_rejected_step);
                place_order<true, false, TAPE>(L, m, tr, type, side, size, price, ln);
                CDA_WSYNC();
                dpos = __builtin_amdgcn_readfirstlane(L.acc[tr].net_position) - pos0;
                if (__builtin_amdgcn_readfirstlane(L.acc[tr].num_rejected_step) != rej0) status = CDA_ORD_REJECTED;
                placed = true;
            }
            if (status == CDA_ORD_DONE) n_done += 1; else n_rej += 1;
            const int32_t drest = __builtin_amdgcn_readfirstlane(total_orders(L, m)) - rest0;
            pin_market<TAPE>(m);
            if (ln == 0) stage[k] = make_uint4((uint32_t)status, (uint32_t)(m.fills - fills0), (uint32_t)dpos, (uint32_t)drest);
        }
        CDA_WSYNC();
        // Lane-indexed addresses are formed HERE, from a lane index the compiler cannot hoist above the walk (own_lane): computed once before the loop they
        // would be held - in the end spilled - across every message's body.
        const int ln = own_lane((int)base);
        const long long nb = base + WAVE;
        if (nb < rem) {                                              // (uniform) the next chunk: one exposed round trip per 64 messages
            const int ncnt = rem - nb < WAVE ? (int)(rem - nb) : WAVE;
            vmask = stage_chunk(stage, mp_msgs[nb + (ln < ncnt ? ln : 0)], ncnt, A);
        }
    }
    const int ln = own_lane(n_done);                                 // (the record's lane addresses are formed here, not held across the walk)
    report(n_done, n_rej, n_inv, m.fills, ln);
    if (n_done + n_rej == 0) return;                                 // nothing but invalid messages: as if the hooks had never been called
    if constexpr (TAPE) tape_finish(*T, mi, m, false, ln);
    if (placed) m.status &= ~ST_LEVELS_VALID;                        // the cached aggregation no longer describes the book (as k_place_order)
    if ((flags & CDA_ORDERS_CLEAR_STEP_COUNTERS) && ln < A) clear_step_counters(L.acc[ln]);
    store_market(market_ptrs(arena, P, mi), P, L, m, ln);
}

template <bool TAPE>
__device__ __forceinline__ void sched_orders(uint8_t* arena, const Params& P, const SchedArgs& C, int first, int n, const TapeArgs* T) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
    const int w = (int)blockIdx.x * CDA_WPB + wave;
    dec_tables_init();                                               // workgroup-wide (one __syncthreads): before any early exit
    if (w >= n) return;
    const int mi = first + w;
    const int r = __builtin_amdgcn_readfirstlane(C.sched_of[mi]);
    if (r < 0 || r >= C.n_sched) return;                             // no schedule for this market
#ifdef CDA_SCHED_LOADS_FIRST
    const MarketPrefetch early = load_market_issue<false>(market_ptrs(arena, P, mi), P, lane);
#endif
    // the header's leading words, one per lane: what episode_over asks (the done mask, t_step) without the record
    const uint32_t hw = lane < 32 ? market_ptrs(arena, P, mi).hdr[lane] : 0u;
    const uint32_t done_mask = (uint32_t)__builtin_amdgcn_readlane((int)hw, H_DONE_MASK);
    int t = __builtin_amdgcn_readlane((int)hw, H_T_STEP);
    if (__popc(done_mask) == P.cfg.num_agents || t >= mrow(P, mi).max_step || t < 0) return;      // the episode is over: the step will not run it either
    if (C.flags & CDA_SCHEDULE_LOOP) t %= C.n_steps;
    else if (t >= C.n_steps) return;                                 // beyond the schedule
    const long long* row = C.offsets + (long long)r * (long long)(C.n_steps + 1) + t;
    const long long b = uniform_i64(row[0]), rem = uniform_i64(row[1]) - b;
    if (rem <= 0 || b < 0 || b + rem > C.n_msgs) return;             // an empty window: the market is neither loaded nor stored, its counters stay
    sched_walk<TAPE>(arena, P, mi, C.msgs, b, rem, (C.flags & CDA_SCHEDULE_CLEAR_STEP_COUNTERS) ? CDA_ORDERS_CLEAR_STEP_COUNTERS : 0u, T, wave, lane,
                     [&](int n_done, int n_rej, int n_inv, int fills, int ln) {
        // the market's row of the counters table: lanes 0 .. 3 own one 64-bit counter each - one vector load and one vector store per market and launch
        if (ln < 4) {
            const int add = ln == 0 ? n_done : (ln == 1 ? n_rej : (ln == 2 ? n_inv : fills));
            long long* c = C.counts + (long long)mi * 4 + ln;
            *c = *c + (long long)add;
        }
    } CDA_SCHED_EARLY_ARG);
}
#undef CDA_SCHED_EARLY_PARAM
#undef CDA_SCHED_EARLY_ARG

__global__ __launch_bounds__(64 * CDA_WPB, CDA_MIN_WAVES) void k_sched_orders(uint8_t* arena, Params P, SchedArgs C, int first, int n) {
    sched_orders<false>(arena, P, C, first, n, nullptr);
}
__global__ __launch_bounds__(64 * CDA_WPB, CDA_MIN_WAVES) void k_tsched_orders(uint8_t* arena, Params P, SchedArgs C, int first, int n, TapeArgs T) {
    sched_orders<true>(arena, P, C, first, n, &T);
}

} }  // namespace cda::CDA_CAPNS
#else

// the launch every step entry point issues first (launch_step); arguments validated by the callers
static int schedule_play(cda_env* e, int32_t first, int32_t n, hipStream_t stream) {
    if (!e->sched.sched_of) return CDA_OK;
    const cda::Launch l = waves_for(e, n, (size_t)CDA_WPB * cda::ORDER_STAGE_BYTES, stream);
    if (e->tape.ring) launch(e->k->tsched_orders, l, e->arena, e->P, e->sched, (int)first, (int)n, e->tape);
    else launch(e->k->sched_orders, l, e->arena, e->P, e->sched, (int)first, (int)n);
    return launch_status();
}
static void schedule_free(cda_env* e) {
    if (e->sched.counts) (void)hipFree(e->sched.counts);
    memset(&e->sched, 0, sizeof e->sched);
}

extern "C" {

int cda_schedule_check_host(int32_t num_agents, int32_t n_markets, const int32_t* sched_of, const int64_t* step_offsets, int32_t n_sched, int32_t n_steps, int64_t n_msgs) {
    if (num_agents < 1 || num_agents > CDA_MAX_AGENTS || n_markets < 1 || !sched_of || !step_offsets || n_sched < 1 || n_steps < 1 || n_msgs < 0) return CDA_ERR_INVALID;
    for (int32_t i = 0; i < n_markets; i++) if (sched_of[i] < -1 || sched_of[i] >= n_sched) return CDA_SCHEDULE_BAD_SCHED_OF;
    for (int32_t r = 0; r < n_sched; r++) {
        const int64_t* row = step_offsets + (size_t)r * (size_t)(n_steps + 1);
        if (row[0] < 0) return CDA_SCHEDULE_BAD_START;
        for (int32_t t = 0; t < n_steps; t++) if (row[t + 1] < row[t]) return CDA_SCHEDULE_BAD_ROW;
        if (row[n_steps] > n_msgs) return CDA_SCHEDULE_BAD_END;
    }
    return CDA_OK;
}

int cda_schedule_attach(cda_env* e, const int32_t* sched_of_dev, const int64_t* step_offsets_dev, int32_t n_sched, int32_t n_steps, const cda_order_msg* msgs_dev,
                        int64_t n_msgs, uint32_t flags) {
    if (!e || !sched_of_dev || !step_offsets_dev || n_sched < 1 || n_steps < 1 || n_msgs < 0 || (n_msgs > 0 && !msgs_dev)) return CDA_ERR_INVALID;
    if (((uintptr_t)sched_of_dev & 3) != 0 || ((uintptr_t)step_offsets_dev & 7) != 0 || ((uintptr_t)msgs_dev & 15) != 0) return CDA_ERR_INVALID;
    if ((flags & ~(CDA_SCHEDULE_LOOP | CDA_SCHEDULE_CLEAR_STEP_COUNTERS)) != 0) return CDA_ERR_INVALID;
    // both index tables are read back and vetted before the env changes: one fault changes nothing
    HIPCHK(hipSetDevice(e->device));
    const size_t n_off = (size_t)n_sched * (size_t)(n_steps + 1), N = (size_t)e->P.n_markets;
    HostBuf<int32_t> so(N);
    HostBuf<int64_t> off(n_off);
    if (!so || !off) return CDA_ERR_NOMEM;
    hipError_t he = hipMemcpy(so, sched_of_dev, N * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(off, step_offsets_dev, n_off * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return hip_fail(he, "hipMemcpy(schedule tables)");
    if (cda_schedule_check_host(e->P.cfg.num_agents, e->P.n_markets, so, off, n_sched, n_steps, n_msgs)) return CDA_ERR_INVALID;
    // a launch in flight reads the schedule it started with: the counters are cleared and the attachment changes once the device is idle
    HIPCHK(hipDeviceSynchronize());
    DevBuf<long long> fresh;                                         // the counters table of a first attach: the env's (schedule_free) once it is cleared
    long long* counts = e->sched.counts;
    if (!counts) { HIPCHK(fresh.alloc(N * 4 * sizeof(long long))); counts = fresh; }
    he = hipMemset(counts, 0, N * 4 * sizeof(long long));
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he != hipSuccess) return hip_fail(he, "hipMemset(schedule counters)");
    (void)fresh.release();
    e->sched.sched_of = sched_of_dev; e->sched.offsets = (const long long*)step_offsets_dev; e->sched.msgs = (const uint4*)msgs_dev; e->sched.counts = counts;
    e->sched.n_msgs = n_msgs; e->sched.n_sched = n_sched; e->sched.n_steps = n_steps; e->sched.flags = flags; e->sched.pad = 0;
    e->sched_epoch++;
    return CDA_OK;
}
int cda_schedule_detach(cda_env* e) {
    if (!e) return CDA_ERR_INVALID;
    // (the counters table stays, with what the schedule counted, until the next attach clears it)
    e->sched.sched_of = NULL; e->sched.offsets = NULL; e->sched.msgs = NULL; e->sched.n_msgs = 0; e->sched.n_sched = 0; e->sched.n_steps = 0; e->sched.flags = 0;
    e->sched_epoch++;
    return CDA_OK;
}
int64_t cda_schedule_epoch(const cda_env* e) { return e ? e->sched_epoch : 0; }
int cda_schedule_attached(const cda_env* e) { return e && e->sched.sched_of ? 1 : 0; }

int cda_schedule_counts(cda_env* e, int32_t first_market, int32_t n_markets, int64_t* out_dev, void* stream) {
    if (!e || !out_dev || ((uintptr_t)out_dev & 7) != 0 || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    const size_t bytes = (size_t)n_markets * 4 * sizeof(long long);
    if (!e->sched.counts) HIPCHK(hipMemsetAsync(out_dev, 0, bytes, (hipStream_t)stream));                 // never attached: nothing was ever counted
    else HIPCHK(hipMemcpyAsync(out_dev, e->sched.counts + (size_t)first_market * 4, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CDA_OK;
}

int cda_schedule_play(cda_env* e, int32_t first_market, int32_t n_markets, void* stream) {
    if (!e || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    return schedule_play(e, first_market, n_markets, (hipStream_t)stream);
}

}  // extern "C"
#endif
