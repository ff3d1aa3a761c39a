// cda_order_tape.inc - the order tape (include/cda.h cda_order_tape_*, cda_order_flow, cda_order_fills): every decoded order of a step and its execution rank,
// recorded on the device, and two order-flow reductions over it.  Included at the end of cda_hip.hip, behind cda_depth.inc (DepthArgs, depth_ring, depth_meta_now,
// k_depth_meta, k_depth_series: a record of 1 + A words in a ring with a QuoteMeta row IS a depth ring of `levels` = A, so the meta and series readers are the depth
// tape's kernels, launched over this service's buffers), cda_quotes.inc (the episode rule) and cda_tape.inc (tape_span, tape_load).  order_tape.py states every
// word in numpy.
//
// The WRITER is k_order_record, which launch_step issues behind the depth recorder's launch and ahead of the step kernel while the tape is on: k_depth_record's
// frame (one wave per market, the header in one 256-byte load, gone at once where the episode is over), then phases 2 and 3 of step_market (cda_kernels.inc)
// restated on a PRIVATE COPY of the generator: present / dict-order keys, one normal per present agent in key order, the clamps, the float32 scale product and the
// float64 sample (the library is built with -ffp-contract=off), rint(fabs()), min_size, _set_price, the arrival list and the nibble Fisher-Yates.  The normals are
// drawn one after the other, wave-uniform, with rng_std_normal: that IS the stream - the step's lane-speculative jump computes the same draws and falls back to
// exactly this loop whenever a candidate is rejected.  The ten level prices per side are the header's cache while ST_LEVELS_VALID is set, else a walk of the side
// (order_levels: depth_side's scheme, prices only).  Nothing of the market record is written: the step that follows draws from the state it would have drawn from.
// Only the market's own wave writes its ring slot and its meta row, with ordinary per-lane vector stores; every word of the slot is written on every visit.
// The recorder and its walk count bits with __builtin_popcount / __builtin_popcountll, not HIP's __popc / __popcll: the compiler propagates value ranges across
// functions BEFORE it inlines those wrappers, and one more caller of them changed the range it proves for an argument of the step's cold_aggregate (one compare of
// it came out signed, not unsigned).  With the builtins every device function of the parent build is instruction for instruction what it was.

static_assert(sizeof(cda_order_head) == 16 && sizeof(cda_order_slot) == 16, "an order record is 1 + num_agents 16-byte words");
static_assert(CDA_MAX_AGENTS == 16 && CDA_MAX_AGENTS <= CDA_DEPTH_MAX_LEVELS, "an order ring is a depth ring of `levels` = num_agents");
static_assert(CDA_K_ROWS == 10 && H_LEVELS + 2 * CDA_K_ROWS <= H_WORDS, "the header's level cache: bid prices, then ask prices");
static_assert(CDA_ORDER_FLOW_WORDS == 32 && CDA_ORDER_FILL_WORDS == 24, "report rows");
enum { OF_PRESENT = 0, OF_PASSES, OF_ABSENT, OF_PAIRS, OF_CROSSING = OF_PAIRS + 16, OF_INSIDE, OF_AT_TOUCH, OF_BEHIND, OF_BEHIND_TICKS, OF_NO_REFERENCE };
enum { OX_TYPES = 0, OX_MAKER_FILLS = 16, OX_MAKER_QTY, OX_SELF_FILLS, OX_SELF_QTY, OX_UNMATCHED_FILLS, OX_UNMATCHED_QTY };
static_assert(OF_NO_REFERENCE < CDA_ORDER_FLOW_WORDS && OX_UNMATCHED_QTY < CDA_ORDER_FILL_WORDS, "report rows");

// THE LAYOUT OF A RECORD, as the readers see it: word 0 `h` = cda_order_head, word 1 + a `r` = cda_order_slot of agent a (include/cda.h)
static_assert(offsetof(cda_order_head, flags) == 4 && offsetof(cda_order_head, best_bid) == 8 && offsetof(cda_order_head, best_ask) == 12, "h = (step, flags, best_bid, best_ask)");
static_assert(offsetof(cda_order_slot, size) == 4 && offsetof(cda_order_slot, price) == 8 && offsetof(cda_order_slot, action) == 12, "r = (code, size, price, action)");
#define order_code(r) ((int)(r).x)
#define order_type(r) ((int)((r).x & 3u))
#define order_side(r) ((int)(((r).x >> 2) & 3u))
#define order_size(r) ((long long)(int)(r).y)
#define order_price(r) ((long long)(int)(r).z)
#define order_sent(r) (order_code(r) >= 0 && order_side(r) != S_NONE)

struct OrderActs { const int32_t* category; const float* size_mean; const float* size_sigma; const int32_t* price; const int32_t* price_offset; const uint8_t* present; };

// the best CDA_K_ROWS level prices of one side, walked in queue order: lane l ends with the price of level l (0: the side has no such level)
__device__ __forceinline__ int32_t order_levels(const BookSide& b, int lane) {
    int lv = -1;                                                     // the level the last order of the pass before belongs to, and its price
    int32_t cp = 0, mine = 0;
    for (int base = 0; base < b.n; base += WAVE) {
        const int i = base + lane;
        const bool valid = i < b.n;
        int32_t p = 0;
        if (valid) p = b.get(0, i);
        const int32_t up = __shfl_up(p, 1);
        unsigned long long heads = __ballot(valid && (lane == 0 ? (lv < 0 || p != cp) : p != up));
        const int level = lv + __builtin_popcountll(heads & lanes_le(lane));
        while (heads != 0ull) {                                       // (uniform) every level that starts in this pass hands its price to the lane of its index
            const int src = __ffsll((long long)heads) - 1;
            heads &= heads - 1ull;
            const int l = __shfl(level, src);
            const int32_t pp = __shfl(p, src);
            if (lane == l) mine = pp;
        }
        const int lastv = 63 - __clzll((long long)__ballot(valid));
        lv = __shfl(level, lastv); cp = __shfl(p, lastv);
        if (lv >= CDA_K_ROWS - 1) break;                             // the tenth level's head has been seen
    }
    return lane < CDA_K_ROWS ? mine : 0;
}

__global__ __launch_bounds__(64 * CDA_WPB) void k_order_record(const uint8_t* arena, Params P, DepthArgs O, OrderActs X, int cap, int first, int n) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w;
    const int A = P.cfg.num_agents;
    // the whole header, one word per lane: the clock and the done mask (episode_over), the generator, last_price, the status and the level cache
    const uint32_t hw = reinterpret_cast<const uint32_t*>(arena + (size_t)mi * (size_t)P.lay.stride)[lane];
    Mkt m;                                                           // a private copy: nothing of it is stored
    decode_header(hw, m);
    const int t = m.t_step;
    if (__builtin_popcount(m.done_mask) == A || t >= mrow(P, mi).max_step || t < 0) return;      // the episode is over: the step will not run it either
    QuoteMeta h = quote_roll(quote_meta_load(O.meta, mi, lane), t);
    // the step's pre-step snapshot: level prices per side, lanes 0 .. 9
    int32_t bpx, apx;
    if (m.status & ST_LEVELS_VALID) {
        bpx = (int32_t)__shfl((int)hw, H_LEVELS + (lane < CDA_K_ROWS ? lane : 0));
        apx = (int32_t)__shfl((int)hw, H_LEVELS + CDA_K_ROWS + (lane < CDA_K_ROWS ? lane : 0));
    } else {
        bpx = order_levels(book_side(arena, P, cap, mi, 0), lane);
        apx = order_levels(book_side(arena, P, cap, mi, 1), lane);
    }
    const int32_t best_bid = m.nb > 0 ? __shfl(bpx, 0) : 0, best_ask = m.na > 0 ? __shfl(apx, 0) : 0;
    // lane a: agent a's five action words and its `present` word, as k_step reads them
    const size_t ab = (size_t)mi * (size_t)A + (size_t)(lane < A ? lane : 0);
    const int in_cat = X.category[ab], in_level = X.price[ab], in_off = X.price_offset[ab];
    const float in_mean = X.size_mean[ab], in_sigma = X.size_sigma[ab];
    const uint8_t present = X.present ? X.present[ab] : (uint8_t)1;
    const bool pres = lane < A && present != 0;
    const int ord = X.present ? (int)present : 1;
    const int tick = mrow(P, mi).tick_size;
    // 2. set_actions: the k-th key of the caller's dict draws the k-th normal
    const unsigned long long pm = __ballot(pres);
    int k = __builtin_popcountll(pm & ((1ull << lane) - 1ull));
    const bool ordered = __ballot(pres && ord != 1) != 0ull;
    if (ordered) {
        const int key = pres ? ord : 0x7fffffff;
        k = 0;
        for (int b = 0; b < A; b++) { const int kb = __shfl(key, b); k += (kb < key || (kb == key && b < lane)) ? 1 : 0; }
    }
    const int n_pres = __builtin_popcountll(pm);
    double z = 0.0;
    for (int r = 0; r < n_pres; r++) {
        const int a = __ffsll((long long)__ballot(pres && k == r)) - 1;
        const double za = rng_std_normal(m);
        if (lane == a) z = za;
    }
    bool ovf = false;
    int side = S_NONE, type = T_MARKET, action = 0;
    int32_t size = -1, pr = -1;
    if (pres) {
        const int cat = clampi(in_cat, 0, 8);
        const float mean = clampf(in_mean, -1.0f, 1.0f), sigma = clampf(in_sigma, 0.0f, 1.0f);
        const int level = clampi(in_level, 0, CDA_K_ROWS - 1), off = clampi(in_off, 0, 2) - 1;
        action = cat | (level << 4) | ((off + 1) << 8);
        side = cat == 0 ? S_NONE : (cat <= 4 ? S_BID : S_ASK);
        type = cat == 0 ? T_MARKET : ((cat - 1) & 3);
        const float mul = type == T_MARKET ? mrow(P, mi).mkt_mul : mrow(P, mi).lim_mul;
        const float locf = mul * mean;                                // float32 product (numpy NEP 50)
        const double prod = (double)sigma * z;
        const double sample = (double)locf + prod;
        double rs = rint(fabs(sample));
        if (rs > 1.0e9) { rs = 1.0e9; ovf = true; }
        size = (int32_t)rs + mrow(P, mi).min_size;
    }
    // _set_price: the level's price of the agent's side (a per-lane index into lanes 0 .. 9: every lane takes part in the exchange)
    {
        const int level = clampi(in_level, 0, CDA_K_ROWS - 1), off = clampi(in_off, 0, 2) - 1;
        const int32_t pb = __shfl(bpx, level), pa = __shfl(apx, level);
        if (pres && side != S_NONE && type != T_MARKET) {
            const int32_t p = side == S_BID ? pb : pa;
            if (side == S_BID) pr = (p == 0 ? m.last_price - (level + 1) * tick : p) + off * tick;
            else pr = (p == 0 ? m.last_price + (level + 1) * tick : p) - off * tick;
            if (pr < tick) pr = tick;
            if (pr >= (1 << 24)) { pr = (1 << 24) - 1; ovf = true; }
        }
    }
    const bool acts = pres && side != S_NONE;
    const uint32_t act_mask = (uint32_t)__ballot(acts), pass_mask = (uint32_t)__ballot(pres && side == S_NONE);
    int arrival = __builtin_popcount(act_mask & ((1u << (lane & 31)) - 1u));
    if (ordered) {
        const int key = acts ? k : 0x7fffffff;
        arrival = 0;
        for (int b = 0; b < A; b++) arrival += __shfl(key, b) < key ? 1 : 0;
    }
    // 3. rand_exec_seq: Fisher-Yates over the n non-pass orders, nibble-packed
    const int n_acts = __builtin_popcount(act_mask);
    uint64_t perm = 0xFEDCBA9876543210ull;
    for (int i = n_acts - 1; i >= 1; i--) {
        const int j = (int)rng_interval(m, (uint32_t)i);
        const uint64_t vi = (perm >> (4 * i)) & 0xFull, vj = (perm >> (4 * j)) & 0xFull;
        perm &= ~((0xFull << (4 * i)) | (0xFull << (4 * j)));
        perm |= (vj << (4 * i)) | (vi << (4 * j));
    }
    int rank = 0;                                                    // the shuffle's i-th pick from the arrival list executes i-th
    for (int i = 0; i < n_acts; i++) if (acts && (int)((perm >> (4 * i)) & 0xFull) == arrival) rank = i;
    const uint32_t slot = (uint32_t)((unsigned long long)h.n_total % (unsigned long long)O.cap);
    uint4* rec = depth_ring(O, mi) + (size_t)slot * (size_t)(1 + A);
    h.n_total += 1; h.n_episode += 1;
    if (lane < A) {
        const int code = !pres ? -1 : (type | (side << 2) | (rank << 4) | (ovf ? CDA_ORDER_CLAMPED : 0));
        if (!acts) { size = -1; pr = -1; }                            // (a pass, or not present)
        rec[1 + lane] = make_uint4((uint32_t)code, (uint32_t)size, (uint32_t)pr, (uint32_t)(pres ? action : 0));
    }
    if (lane == 0) {
        const int flags = (m.nb > 0 ? CDA_QUOTE_BID : 0) | (m.na > 0 ? CDA_QUOTE_ASK : 0) | (n_acts << 8) | (__builtin_popcount(pass_mask) << 16);
        rec[0] = make_uint4((uint32_t)t, (uint32_t)flags, (uint32_t)best_bid, (uint32_t)best_ask);
    }
    if (lane < 8) reinterpret_cast<int32_t*>(O.meta + mi)[lane] = quote_meta_word(h, lane);
}

// Order flow per agent.  Lanes over (record, agent): G = 64 / A consecutive records per pass, lane = rl x A + a, so a lane serves one agent over all passes; a
// lane reads its record's head and its own slot.  LDS per wave: A x CDA_ORDER_FLOW_WORDS 64-bit words (at most 4 KiB).
__global__ __launch_bounds__(64 * CDA_WPB) void k_order_flow(const uint8_t* arena, Params P, DepthArgs O, int first, int n, int which, int agents, long long* out, int32_t* info) {
    extern __shared__ __align__(16) unsigned long long order_flow_lds[];
    READER_WAVE_IN_GROUP(CDA_WPB);
    const bool live = w < n;
    const int n_words = agents * CDA_ORDER_FLOW_WORDS, W = 1 + agents;
    unsigned long long* tb = order_flow_lds + (size_t)wib * (size_t)n_words;
    for (int i = lane; i < n_words; i += WAVE) tb[i] = 0ull;
    __syncthreads();
    QuoteSpan sp = {0, 0, 0, 0, 0, 0u};
    if (live) {
        const int mi = first + w;
        sp = quote_span(depth_meta_now(O, arena, P, mi, lane), O.cap, which);
        const uint4* ring = depth_ring(O, mi);
        const int tk = mrow(P, mi).tick_size;
        const long long tick = tk < 1 ? 1ll : (long long)tk;
        const int G = WAVE / agents, rl = lane / agents, a = lane - rl * agents;
        unsigned long long* row = tb + (size_t)a * CDA_ORDER_FLOW_WORDS;
        for (int base = 0; base < sp.count; base += G) {
            const int idx = base + rl;
            if (rl >= G || idx >= sp.count) continue;
            const uint4* rp = ring + (size_t)quote_slot(sp, O.cap, idx) * (size_t)W;
            const uint4 hd = rp[0], r = rp[1 + a];
            if (order_code(r) < 0) { lds_add(row + OF_ABSENT, 1ll); continue; }
            lds_add(row + OF_PRESENT, 1ll);
            const int side = order_side(r), type = order_type(r);
            if (side == S_NONE) { lds_add(row + OF_PASSES, 1ll); continue; }
            lds_add(row + OF_PAIRS + 2 * (type * 2 + side), 1ll);
            lds_add(row + OF_PAIRS + 2 * (type * 2 + side) + 1, order_size(r));
            if (type != T_LIMIT) continue;
            const bool has_bid = (hd.y & CDA_QUOTE_BID) != 0u, has_ask = (hd.y & CDA_QUOTE_ASK) != 0u;
            const long long bb = (long long)(int)hd.z, ba = (long long)(int)hd.w, p = order_price(r);
            const bool crossing = side == S_BID ? (has_ask && p >= ba) : (has_bid && p <= bb);
            const bool own = side == S_BID ? has_bid : has_ask;
            const long long d = side == S_BID ? bb - p : p - ba;       // > 0: behind the own best
            if (crossing) lds_add(row + OF_CROSSING, 1ll);
            else if (!own) lds_add(row + OF_NO_REFERENCE, 1ll);
            else if (d < 0) lds_add(row + OF_INSIDE, 1ll);
            else if (d == 0) lds_add(row + OF_AT_TOUCH, 1ll);
            else { lds_add(row + OF_BEHIND, 1ll); lds_add(row + OF_BEHIND_TICKS, d / tick); }
        }
    }
    __syncthreads();
    if (!live) return;
    for (int i = lane; i < n_words; i += WAVE) out[(size_t)w * (size_t)n_words + i] = (long long)tb[i];
    if (info && lane == 0) reader_info(info, w, sp.count, sp.lost, sp.step0, sp.partial);
}

// Fills against orders.  First the held order records, laid over the lanes as in k_order_flow: orders and submitted quantity per type.  Then the episode's held
// tape records, 64 per pass (k_tape_spreads' frame): the order record of the fill's step is read at its slot - indexed directly, no search.  An order counts as
// filled once: at the first held fill of its (initiator, step) - a step's fills are consecutive in the tape, so a lane looks back over the records of its own step.
// LDS per wave: A x CDA_ORDER_FILL_WORDS 64-bit words (at most 3 KiB).
__global__ __launch_bounds__(64 * CDA_WPB) void k_order_fills(const uint8_t* arena, Params P, TapeArgs T, DepthArgs O, int first, int n, int which, int agents, long long* out,
                                                              int32_t* info) {
    extern __shared__ __align__(16) unsigned long long order_fill_lds[];
    READER_WAVE_IN_GROUP(CDA_WPB);
    const bool live = w < n;
    const int n_words = agents * CDA_ORDER_FILL_WORDS, W = 1 + agents;
    unsigned long long* tb = order_fill_lds + (size_t)wib * (size_t)n_words;
    for (int i = lane; i < n_words; i += WAVE) tb[i] = 0ull;
    __syncthreads();
    TapeSpan ts = {0, 0, 0, 0};
    QuoteSpan sp = {0, 0, 0, 0, 0, 0u};
    int step_first_fill = -1;
    if (live) {
        const int mi = first + w;
        ts = tape_span(T.meta[mi], T.cap, which);
        sp = quote_span(depth_meta_now(O, arena, P, mi, lane), O.cap, which);
        const uint4* ring = depth_ring(O, mi);
        {
            const int G = WAVE / agents, rl = lane / agents, a = lane - rl * agents;
            unsigned long long* row = tb + (size_t)a * CDA_ORDER_FILL_WORDS;
            for (int base = 0; base < sp.count; base += G) {
                const int idx = base + rl;
                if (rl >= G || idx >= sp.count) continue;
                const uint4 r = ring[(size_t)quote_slot(sp, O.cap, idx) * (size_t)W + (size_t)(1 + a)];
                if (!order_sent(r)) continue;
                lds_add(row + OX_TYPES + 4 * order_type(r), 1ll);
                lds_add(row + OX_TYPES + 4 * order_type(r) + 1, order_size(r));
            }
        }
        const uint4* tring = T.ring + (size_t)mi * (size_t)T.cap * 2;
        const uint32_t tmask = T.cap - 1u, t0 = (uint32_t)ts.start & tmask;
        const int count = (int)ts.count;
        const long long o_first = (long long)sp.step0, o_last = sp.count > 0 ? o_first + (long long)sp.count - 1 : -1ll;
        for (int base = 0; base < count; base += WAVE) {
            const int idx = base + lane;
            const bool in = idx < count;
            uint4 r0, r1;
            tape_load(tring, tmask, t0, idx, in, r0, r1);
            if (idx == 0 && in) step_first_fill = (int)tape_step(r1);
            const uint32_t cid = tape_counter_id(r0), iid = tape_init_id(r1);
            if (!in || cid >= (uint32_t)agents || iid >= (uint32_t)agents) continue;      // (ids outside the env's agents cannot index the table)
            const long long step = (long long)tape_step(r1), qty = (long long)tape_qty(r0);
            unsigned long long* rm = tb + (size_t)cid * CDA_ORDER_FILL_WORDS;
            unsigned long long* ri = tb + (size_t)iid * CDA_ORDER_FILL_WORDS;
            lds_add(rm + OX_MAKER_FILLS, 1ll); lds_add(rm + OX_MAKER_QTY, qty);
            if (cid == iid) { lds_add(ri + OX_SELF_FILLS, 1ll); lds_add(ri + OX_SELF_QTY, qty); }
            uint4 r = make_uint4(0xffffffffu, 0u, 0u, 0u);
            if (step >= o_first && step <= o_last) r = ring[(size_t)quote_slot(sp, O.cap, (int)(step - o_first)) * (size_t)W + (size_t)(1u + iid)];
            if (!order_sent(r)) { lds_add(ri + OX_UNMATCHED_FILLS, 1ll); lds_add(ri + OX_UNMATCHED_QTY, qty); continue; }
            bool is_first = true;                                    // no earlier held fill of this step has this initiator
            for (int j = idx - 1; j >= 0; j--) {
                const uint32_t slot = (t0 + (uint32_t)j) & tmask;
                const uint4 q1 = tring[2 * (size_t)slot + 1];
                if ((long long)tape_step(q1) != step) break;
                if (tape_init_id(q1) == iid) { is_first = false; break; }
            }
            if (is_first) lds_add(ri + OX_TYPES + 4 * order_type(r) + 2, 1ll);
            lds_add(ri + OX_TYPES + 4 * order_type(r) + 3, qty);
        }
    }
    __syncthreads();
    if (!live) return;
    for (int i = lane; i < n_words; i += WAVE) out[(size_t)w * (size_t)n_words + i] = (long long)tb[i];
    if (info && lane == 0) {
        reader_info(info, 2 * w, sp.count, sp.lost, sp.step0, sp.partial);
        reader_info(info, 2 * w + 1, (int32_t)ts.count, (int32_t)ts.lost, step_first_fill, ts.partial);
    }
}

// the launch every step entry point issues behind the depth recorder's and ahead of the step (launch_step); arguments validated by the callers
static int order_tape_record(cda_env* e, int32_t first, int32_t n, const StepArgs& S, hipStream_t stream) {
    if (!e->otape.ring) return CDA_OK;
    const OrderActs X = {S.category, S.size_mean, S.size_sigma, S.price, S.price_offset, S.present};
    hipLaunchKernelGGL(k_order_record, grid_for(n), dim3(64 * CDA_WPB), 0, stream, (const uint8_t*)e->arena, e->P, e->otape, X, (int)e->cap, (int)first, (int)n);
    return launch_status();
}
static void order_tape_free(cda_env* e) {
    if (e->otape.ring) (void)hipFree(e->otape.ring);
    if (e->otape.meta) (void)hipFree(e->otape.meta);
    memset(&e->otape, 0, sizeof e->otape);
}

extern "C" {

int cda_order_tape_check_host(int32_t kind, int32_t num_agents, int64_t a, int32_t b) {
    if (num_agents < 1 || num_agents > CDA_MAX_AGENTS) return CDA_ERR_INVALID;
    if (kind == CDA_ORDER_CHECK_ENABLE) return a >= 1 && a <= CDA_QUOTE_CAP_MAX && (a & (a - 1)) == 0 ? CDA_OK : CDA_ERR_INVALID;
    if (kind == CDA_ORDER_CHECK_SERIES) return (a == CDA_TAPE_CURRENT || a == CDA_TAPE_PREVIOUS) && b >= 1 ? CDA_OK : CDA_ERR_INVALID;
    if (kind == CDA_ORDER_CHECK_REPORT) return a == CDA_TAPE_CURRENT || a == CDA_TAPE_PREVIOUS ? CDA_OK : CDA_ERR_INVALID;
    return CDA_ERR_INVALID;
}

int cda_order_tape_enable(cda_env* e, int64_t capacity_steps) {
    if (!e || cda_order_tape_check_host(CDA_ORDER_CHECK_ENABLE, e->P.cfg.num_agents, capacity_steps, 0) != CDA_OK) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    const size_t n = (size_t)e->P.n_markets, bytes = n * (size_t)capacity_steps * (size_t)(1 + e->P.cfg.num_agents) * sizeof(uint4);
    DevBuf<uint4> ring; DevBuf<QuoteMeta> meta;                       // (the env keeps what it has until both allocations stand)
    if (ring.alloc(bytes) != hipSuccess || meta.alloc(n * sizeof(QuoteMeta)) != hipSuccess) { (void)hipGetLastError(); return CDA_ERR_NOMEM; }
    hipError_t he = hipMemset(ring, 0, bytes);
    if (he == hipSuccess) he = hipMemset(meta, 0, n * sizeof(QuoteMeta));
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he != hipSuccess) return hip_fail(he, "cda_order_tape_enable");
    order_tape_free(e);
    e->otape.ring = ring.release(); e->otape.meta = meta.release(); e->otape.cap = (uint32_t)capacity_steps; e->otape.levels = (uint32_t)e->P.cfg.num_agents;
    return CDA_OK;
}
int cda_order_tape_disable(cda_env* e) {
    if (!e) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    order_tape_free(e);
    return CDA_OK;
}
int64_t cda_order_tape_capacity(const cda_env* e) { return e && e->otape.ring ? (int64_t)e->otape.cap : 0; }

int cda_order_tape_meta(cda_env* e, int32_t first_market, int32_t n_markets, int32_t* meta_out_dev, void* stream) {
    if (!reader_args_ok(e, meta_out_dev, first_market, n_markets) || !aligned(meta_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->otape.ring) return CDA_ERR_UNSUPPORTED;
    return reader_launch(e, k_depth_meta, n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, e->otape, (int)first_market, (int)n_markets, meta_out_dev);
}
int cda_order_tape_series(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, int32_t k, void* records_out_dev, int32_t* counts_out_dev, int32_t* info_out_dev,
                          void* stream) {
    if (!reader_args_ok(e, records_out_dev, first_market, n_markets) || !agents_ok(e) || cda_order_tape_check_host(CDA_ORDER_CHECK_SERIES, e->P.cfg.num_agents, which, k) != CDA_OK ||
        !aligned(records_out_dev, 16) || !aligned(counts_out_dev, 4) || !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->otape.ring) return CDA_ERR_UNSUPPORTED;
    return reader_launch(e, k_depth_series, n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, e->otape, (int)first_market, (int)n_markets, (int)which, (int)k,
                         (uint4*)records_out_dev, counts_out_dev, info_out_dev);
}
int cda_order_flow(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, int64_t* flow_out_dev, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, flow_out_dev, first_market, n_markets) || !agents_ok(e) || cda_order_tape_check_host(CDA_ORDER_CHECK_REPORT, e->P.cfg.num_agents, which, 0) != CDA_OK ||
        !aligned(flow_out_dev, 8) || !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->otape.ring) return CDA_ERR_UNSUPPORTED;
    const size_t lds = (size_t)CDA_WPB * (size_t)e->P.cfg.num_agents * CDA_ORDER_FLOW_WORDS * sizeof(unsigned long long);      // <= 4 x 16 x 32 x 8 B = 16 KiB
    return reader_launch(e, k_order_flow, n_markets, CDA_WPB, lds, stream, (const uint8_t*)e->arena, e->P, e->otape, (int)first_market, (int)n_markets, (int)which,
                         (int)e->P.cfg.num_agents, (long long*)flow_out_dev, info_out_dev);
}
int cda_order_fills(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, int64_t* fills_out_dev, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, fills_out_dev, first_market, n_markets) || !agents_ok(e) || cda_order_tape_check_host(CDA_ORDER_CHECK_REPORT, e->P.cfg.num_agents, which, 0) != CDA_OK ||
        !aligned(fills_out_dev, 8) || !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->tape.ring || !e->otape.ring) return CDA_ERR_UNSUPPORTED;
    const size_t lds = (size_t)CDA_WPB * (size_t)e->P.cfg.num_agents * CDA_ORDER_FILL_WORDS * sizeof(unsigned long long);      // <= 4 x 16 x 24 x 8 B = 12 KiB
    return reader_launch(e, k_order_fills, n_markets, CDA_WPB, lds, stream, (const uint8_t*)e->arena, e->P, e->tape, e->otape, (int)first_market, (int)n_markets, (int)which,
                         (int)e->P.cfg.num_agents, (long long*)fills_out_dev, info_out_dev);
}

}  // extern "C"
