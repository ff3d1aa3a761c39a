// cda_orders.inc - order streams (include/cda.h cda_submit_orders): a whole per-market list of explicit messages - market, limit, modify, cancel orders
// and mark_to_mkt - played into every market of a range in ONE asynchronous launch.  cda_hip.hip includes this file three times: behind cda_kernels.inc
// once per book capacity (CDA_CAP defined: the two kernels, in `namespace cda::CDA_CAPNS`), and once at its end (the entry points).
//
// k_order_stream / k_tape_order_stream: CDA_WPB waves per workgroup, one wave per market.  The market record is loaded once (load_market: the general
// form, tile + HBM ring), the messages run through the hook's own bodies - place_order<true, false[, true]> and mark_to_mkt, one call site each -
// in stream order, the record is stored once.  A message is 16 bytes: lane l loads message base + l of the current chunk of 64 with one vector load
// (1 KiB per wave, coalesced), all 64 are validated lane-parallel, one ballot forms the valid mask.  The wave then walks k = 0 .. cnt - 1, takes the
// k-th message's words as scalars - as the hook's kernel arguments are - and leaves the message's result where the message was; a chunk's results
// leave as one coalesced 16-byte store per lane.  The first chunk's load is issued with the record's; a later chunk's (one exposed round trip per 64
// messages) behind the walk of the one before.
//
// Registers.  place_order's inlined body takes 116 - 119 VGPRs in the hooks, and the kernels here keep four waves per SIMD (128) without a spill: whatever
// a lane holds ACROSS that body comes on top.  Three things therefore stay out of its way (each was measured in the compiler's output: 31 - 48 spilled
// VGPRs with all three, 8 - 16 with the first two dealt with, 0 now, at 121 / 124 VGPRs):
//   - the chunk waits in 1 KiB of LDS per wave, not in registers (slot k is read through one address - a broadcast - and pinned with readfirstlane); the
//     same slot takes the result.  Messages, a register-prefetched next chunk and results held in lanes were 12 VGPRs across every body.
//   - lane-indexed addresses and the bodies' own lane predicates (owner lane, helper group) are formed from a lane index taken afresh where it is used
//     (own_lane): from the kernel's one `lane` the optimiser hoists them out of the walk and holds - spills - them across it.
//   - the market scalars a message changes go back to SGPRs behind every message (pin_market).
#ifdef CDA_CAP
#ifndef CDA_ORDER_STREAM_ARGS
#define CDA_ORDER_STREAM_ARGS
namespace cda {
struct OrderStreamArgs {
    const long long* offsets;    // [n + 1]: market first + w owns messages offsets[w] .. offsets[w + 1]
    const uint4* msgs;           // cda_order_msg[]
    uint4* results;              // cda_order_result[], indexed like msgs; NULL = not wanted
    uint4* summary;              // [n] x (executed, rejected, invalid, fills); NULL = not wanted
    long long n_msgs;            // messages behind `msgs` (< 0: not known): a market whose offsets reach beyond them runs nothing
    long long skip, limit;       // this launch plays, of every market's stream, the messages [skip, skip + limit)
    int first, n;
    uint32_t flags;              // CDA_ORDERS_*
};
constexpr int ORDER_STAGE_BYTES = 64 * 16;
}
#endif
namespace cda { namespace CDA_CAPNS {

__device__ __forceinline__ long long uniform_i64(long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(unsigned long long)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
// the hook's accepted domain (cda_place_order; CDA_OP_MARK carries nothing but its type), by the lane that holds the message
__device__ __forceinline__ bool order_msg_valid(const uint4& q, int A) {
    const int32_t price = (int32_t)q.x, size = (int32_t)q.y;
    const int trader = (int)(int16_t)(q.z & 0xffffu), type = (int)(int8_t)((q.z >> 16) & 0xffu), side = (int)(int8_t)(q.z >> 24);
    if (type == CDA_OP_MARK) return true;
    return trader >= 0 && trader < A && type >= 0 && type <= 3 && side >= 0 && side <= 1 && size >= 1 && (type == 0 || price >= 1);
}

// the wave's message chunk: 64 x 16 bytes of the workgroup's dynamic LDS behind the CDA_WPB market images (ORDER_STAGE_BYTES per wave on top of the images)
__device__ __forceinline__ uint4* order_stage(const Params& P, int wave) {
    return reinterpret_cast<uint4*>(cda_smem + DEC_TABLE_BYTES + (size_t)CDA_WPB * (size_t)lds_bytes_per_wave(P.cfg.num_agents, P.cfg.n_hist) + (size_t)wave * ORDER_STAGE_BYTES);
}

// The market scalars a message can change, back in SGPRs.  place_order updates them under branches the compiler treats as divergent, so behind a message they
// live in VGPRs - every lane the same value; carried around the walk like that they would occupy a dozen VGPRs at the top of the next message's body, which
// the hook's straight-line code never pays.
template <bool TAPE>
__device__ __forceinline__ void pin_market(Mkt& m) {
    #define CDA_PIN(f) m.f = (decltype(m.f))__builtin_amdgcn_readfirstlane((int)m.f)
    CDA_PIN(lob_time); CDA_PIN(next_oid); CDA_PIN(last_price); CDA_PIN(has_trade); CDA_PIN(last_trade_price); CDA_PIN(flags);
    CDA_PIN(nb); CDA_PIN(na); CDA_PIN(status); CDA_PIN(peak_orders); CDA_PIN(fills);
    if constexpr (TAPE) { CDA_PIN(tape_pos); CDA_PIN(tape_new); }
    #undef CDA_PIN
}
// The lane index, formed where it is used: mbcnt counts the lanes below this one ON TOP of `seed`, and the caller passes a seed that changes from one use to the
// next (the message's index, the chunk's base) - so the optimiser can neither fold the sum nor hoist it, and what is computed from it stays where it is written.
// The mask gives the result lane_id()'s known range, 0 .. 63.  It is not decoration: without it (and likewise with an empty asm statement in mbcnt's place)
// the build scheduled a few instructions of the EXISTING kernels that inline the same bodies differently (tools/kernel_identity.py: 50 functions); with it every
// one of them is the parent's, instruction for instruction.
__device__ __forceinline__ int own_lane(int seed) {
    return ((int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (uint32_t)seed)) - seed) & (WAVE - 1);
}
// lane l hands the chunk's l-th message (or, for one outside the domain, its result) to the stage; the mask of the valid ones
__device__ __forceinline__ unsigned long long stage_chunk(uint4* stage, const uint4& q, int cnt, int A) {
    const int ln = own_lane(cnt);
    const bool ok = ln < cnt && order_msg_valid(q, A);
    stage[ln] = ok ? q : make_uint4((uint32_t)CDA_ORD_INVALID, 0u, 0u, 0u);               // slot l: the message - and, once the walk has passed it, its RESULT
    CDA_WSYNC();
    return __ballot(ok);
}

template <bool TAPE>
__device__ __forceinline__ void order_stream(uint8_t* arena, const Params& P, const OrderStreamArgs& S, const TapeArgs* T) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
    const int w = (int)blockIdx.x * CDA_WPB + wave;
    dec_tables_init();                                               // workgroup-wide (one __syncthreads): before any early exit
    if (w >= S.n) return;
    const int mi = S.first + w, A = P.cfg.num_agents;
    const long long o0 = uniform_i64(S.offsets[w]), o1 = uniform_i64(S.offsets[w + 1]);
    if (o0 < 0 || o1 < o0 || (S.n_msgs >= 0 && o1 > S.n_msgs)) {     // not a stream: nothing runs, the summary says so
        if (S.summary && lane == 0) S.summary[w] = make_uint4(0u, 0u, 0xffffffffu, 0u);
        return;
    }
    const long long b = o0 + S.skip;                                 // this launch's window of the stream
    long long rem = o1 - b;
    if (rem > S.limit) rem = S.limit;
    if (rem <= 0) {                                                  // an empty stream: the market is neither loaded nor stored
        if (S.summary && lane == 0) S.summary[w] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint4* mp_msgs = S.msgs + b;
    Lds& L = wave_lds(P, wave);
    uint4* stage = order_stage(P, wave);
    MarketPtrs mp = market_ptrs(arena, P, mi);
    Mkt m;
    unsigned long long vmask;
    {
        // the record's requests and the first chunk's are in flight together: ONE round trip before the first message runs
        const MarketPrefetch pre = load_market_issue<false>(mp, P, lane);
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
        if (S.results && ln < cnt) S.results[b + base + ln] = stage[ln];               // the chunk's results: one coalesced 16-byte store per lane
        CDA_WSYNC();
        const long long nb = base + WAVE;
        if (nb < rem) {                                              // (uniform) the next chunk: one exposed round trip per 64 messages
            const int ncnt = rem - nb < WAVE ? (int)(rem - nb) : WAVE;
            vmask = stage_chunk(stage, mp_msgs[nb + (ln < ncnt ? ln : 0)], ncnt, A);
        }
    }
    const int ln = own_lane(n_done);                                 // (the record's lane addresses are formed here, not held across the walk)
    if (S.summary && ln == 0) S.summary[w] = make_uint4((uint32_t)n_done, (uint32_t)n_rej, (uint32_t)n_inv, (uint32_t)m.fills);
    if (n_done + n_rej == 0) return;                                 // nothing but invalid messages: as if the hooks had never been called
    if constexpr (TAPE) tape_finish(*T, mi, m, false, ln);
    if (placed) m.status &= ~ST_LEVELS_VALID;                        // the cached aggregation no longer describes the book (as k_place_order)
    if ((S.flags & CDA_ORDERS_CLEAR_STEP_COUNTERS) && ln < A) clear_step_counters(L.acc[ln]);
    store_market(market_ptrs(arena, P, mi), P, L, m, ln);
}

__global__ __launch_bounds__(64 * CDA_WPB, CDA_MIN_WAVES) void k_order_stream(uint8_t* arena, Params P, OrderStreamArgs S) {
    order_stream<false>(arena, P, S, nullptr);
}
__global__ __launch_bounds__(64 * CDA_WPB, CDA_MIN_WAVES) void k_tape_order_stream(uint8_t* arena, Params P, OrderStreamArgs S, TapeArgs T) {
    order_stream<true>(arena, P, S, &T);
}

} }  // namespace cda::CDA_CAPNS
#else

static inline bool order_msg_ok_host(const cda_order_msg& q, int32_t A) {
    if (q.type == CDA_OP_MARK) return true;
    return q.trader >= 0 && q.trader < A && q.type >= 0 && q.type <= 3 && q.side >= 0 && q.side <= 1 && q.size >= 1 && (q.type == 0 || q.price >= 1);
}
static_assert(sizeof(cda_order_msg) == 16 && sizeof(cda_order_result) == 16, "one 16-byte vector access per message / result");

extern "C" {

int cda_order_msgs_check_agents_host(int32_t num_agents, const cda_order_msg* msgs_host, int64_t n, int64_t* first_bad_out) {
    if (num_agents < 1 || num_agents > CDA_MAX_AGENTS || n < 0 || (n > 0 && !msgs_host) || !first_bad_out) return CDA_ERR_INVALID;
    *first_bad_out = -1;
    for (int64_t i = 0; i < n; i++) if (!order_msg_ok_host(msgs_host[i], num_agents)) { *first_bad_out = i; break; }
    return CDA_OK;
}
int cda_order_msgs_check_host(const cda_env* e, const cda_order_msg* msgs_host, int64_t n, int64_t* first_bad_out) {
    return cda_order_msgs_check_agents_host(e ? e->P.cfg.num_agents : CDA_MAX_AGENTS, msgs_host, n, first_bad_out);
}

int cda_submit_orders_window(cda_env* e, int32_t first_market, int32_t n_markets, const int64_t* offsets_dev, const cda_order_msg* msgs_dev, int64_t n_msgs,
                             int64_t skip, int64_t limit, cda_order_result* results_dev, int32_t* summary_dev, uint32_t flags, void* stream) {
    if (!e || !offsets_dev || !msgs_dev || first_market < 0 || n_markets < 1 || skip < 0 || limit < 1 || (flags & ~CDA_ORDERS_CLEAR_STEP_COUNTERS) != 0) return CDA_ERR_INVALID;
    if (((uintptr_t)offsets_dev & 7) != 0 || ((uintptr_t)msgs_dev & 15) != 0 || ((uintptr_t)results_dev & 15) != 0 || ((uintptr_t)summary_dev & 15) != 0) return CDA_ERR_INVALID;
    if (!range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    cda::OrderStreamArgs S;
    S.offsets = (const long long*)offsets_dev; S.msgs = (const uint4*)msgs_dev; S.results = (uint4*)results_dev; S.summary = (uint4*)summary_dev;
    S.n_msgs = n_msgs; S.skip = skip; S.limit = limit; S.first = first_market; S.n = n_markets; S.flags = flags;
    const cda::Launch l = waves_for(e, n_markets, (size_t)CDA_WPB * cda::ORDER_STAGE_BYTES, (hipStream_t)stream);
    if (e->tape.ring) launch(e->k->tape_order_stream, l, e->arena, e->P, S, e->tape);
    else launch(e->k->order_stream, l, e->arena, e->P, S);
    return launch_status();
}
int cda_submit_orders(cda_env* e, int32_t first_market, int32_t n_markets, const int64_t* offsets_dev, const cda_order_msg* msgs_dev, cda_order_result* results_dev,
                      int32_t* summary_dev, uint32_t flags, void* stream) {
    return cda_submit_orders_window(e, first_market, n_markets, offsets_dev, msgs_dev, -1, 0, INT64_MAX, results_dev, summary_dev, flags, stream);
}

}  // extern "C"
#endif
