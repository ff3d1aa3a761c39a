// cda_quotes.inc - the quote tape (include/cda.h cda_quotes_*, cda_quote_*, cda_tape_spreads): the top of the book per step of an episode, recorded on the device,
// and the reductions over it.  Included at the end of cda_hip.hip, behind cda_book_report.inc (the walk of a side: BookSide) and cda_tape.inc (tape_span,
// tape_load); the wave toolkit is cda_wave.hpp.  The record's layout as the readers see it - quote_two_sided, quote_m2 and their kin - stands beside QuoteSpan.
//
// Per market a ring of `capacity` records (cda_quote_record, eight int32 words = two 16-byte words) in a buffer of its own beside the arena, and one QuoteMeta
// row: neither the market record, nor the state dump, nor the snapshot blob know of either.  The WRITER is k_quote_record, which launch_step issues behind the
// order schedule's launch and ahead of the step kernel while quotes are on: one wave per market; the header's leading words in one 128-byte load (t_step and the
// done mask by readlane, as the schedule's choice stage), gone at once where the episode is over; else the head of each side read where it lies (the tile and,
// behind it, the HBM ring).  Only the market's own wave writes its ring slot and its meta row, with ordinary per-lane vector stores: no atomics anywhere.
//
// THE EPISODE RULE (quote_roll; quotes.py roll is the same statement in numpy).  Nothing tells the recorder of a reset or a restore: it and every reader derive
// the episode from the meta row and the market's current t_step alone.  The current episode holds n_episode records, of the steps first .. first + n_episode - 1:
//   t_step == first + n_episode      the expected next step (a complete episode has first == 0: t_step == n_episode): nothing changes.
//   t_step == 0 and n_episode > 0    the market was reset: the held episode becomes "previous" (n_prev, prev_first, its partial bit), the current one starts empty.
//   anything else                    a snapshot restore (or a set_state) moved the clock: the current episode restarts at t_step, empty, partial unless t_step == 0;
//                                    the records it held stay in the ring as a gap between the previous episode and the new current one.
// The recorder applies the rule and stores the row; the readers apply it to their copy (the roll is lazy: right behind the step whose in-kernel auto reset ended
// an episode, "previous" already names that episode, as the trade tape's does).  The ring is never cleared: in record numbers it holds [n_total - capacity,
// n_total), the current episode is [n_total - n_episode, n_total), the previous one the n_prev records before n_total - n_episode - gap (quote_span).

static_assert(sizeof(cda_quote_record) == CDA_QUOTE_WORDS * 4 && sizeof(cda_quote_record) == 32, "cda_quote_record layout");
static_assert(CDA_QUOTE_STAT_WORDS == 16 && CDA_TAPE_MAX_HORIZONS == 8, "cda_quote_stats / cda_tape_spreads layout");
static_assert(sizeof(QuoteMeta) == 32, "QuoteMeta layout");
enum { QM_PARTIAL = 1, QM_PREV_PARTIAL = 2 };
enum { QS_STEPS = 0, QS_TWO_SIDED, QS_BID_ONLY, QS_ASK_ONLY, QS_EMPTY, QS_SPREAD_SUM, QS_SPREAD_SQ, QS_SPREAD_MIN, QS_SPREAD_MAX, QS_M2_SUM, QS_BID_VOL, QS_ASK_VOL,
       QS_PAIRS, QS_M2_CHANGES, QS_ABS_DM2, QS_DM2_SQ };
enum { SP_COST_NOW = 0, SP_COST_LATER, SP_QTY, SP_FILLS, SP_OPEN, SP_UNQUOTED, SP_WORDS };

__device__ __forceinline__ QuoteMeta quote_roll(QuoteMeta h, int t_step) {
    if (t_step == h.first + h.n_episode) return h;
    if (t_step == 0 && h.n_episode > 0) {
        h.n_prev = h.n_episode; h.prev_first = h.first; h.gap = 0;
        h.flags = (h.flags & QM_PARTIAL) ? QM_PREV_PARTIAL : 0;
        h.n_episode = 0; h.first = 0;
        return h;
    }
    h.gap = h.gap + h.n_episode > CDA_QUOTE_CAP_MAX ? CDA_QUOTE_CAP_MAX : h.gap + h.n_episode;       // (a gap of the ring's size or more: the previous episode is gone)
    h.n_episode = 0; h.first = t_step;
    h.flags = (h.flags & QM_PREV_PARTIAL) | (t_step != 0 ? QM_PARTIAL : 0);
    return h;
}
// the market's meta row, one word per lane (lanes 0 .. 7), made uniform
__device__ __forceinline__ QuoteMeta quote_meta_load(const QuoteMeta* meta, int mi, int lane) {
    const int32_t w = lane < 8 ? reinterpret_cast<const int32_t*>(meta + mi)[lane] : 0;
    QuoteMeta h;
    h.n_total = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane(w, 1) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane(w, 0));
    h.n_episode = __builtin_amdgcn_readlane(w, 2); h.n_prev = __builtin_amdgcn_readlane(w, 3); h.first = __builtin_amdgcn_readlane(w, 4);
    h.prev_first = __builtin_amdgcn_readlane(w, 5); h.gap = __builtin_amdgcn_readlane(w, 6); h.flags = __builtin_amdgcn_readlane(w, 7);
    return h;
}
__device__ __forceinline__ int32_t quote_meta_word(const QuoteMeta& h, int k) {
    return k == 0 ? (int32_t)(uint32_t)(uint64_t)h.n_total : k == 1 ? (int32_t)(uint32_t)((uint64_t)h.n_total >> 32) : k == 2 ? h.n_episode : k == 3 ? h.n_prev :
           k == 4 ? h.first : k == 5 ? h.prev_first : k == 6 ? h.gap : h.flags;
}
// the market's t_step as its header holds it (uniform)
__device__ __forceinline__ int quote_t_step(const uint8_t* arena, const Params& P, int mi) {
    return __builtin_amdgcn_readfirstlane((int)reinterpret_cast<const uint32_t*>(arena + (size_t)mi * (size_t)P.lay.stride)[H_T_STEP]);
}
// what a reader sees: the stored row, rolled to the market's clock
__device__ __forceinline__ QuoteMeta quote_meta_now(const QuoteArgs& Q, const uint8_t* arena, const Params& P, int mi, int lane) {
    const QuoteMeta h = quote_meta_load(Q.meta, mi, lane);
    const int t = quote_t_step(arena, P, mi);
    return t < 0 ? h : quote_roll(h, t);
}
// One of the two remembered episodes in record numbers (tape_span's scheme): `start` / `count` what the ring still holds of it, `lost` the records of its head that
// are overwritten, `step0` the step of record `start` (the record of step s is start + s - step0), `slot0` = start % capacity.
struct QuoteSpan { long long start; int count, lost, step0, partial; uint32_t slot0; };
__device__ __forceinline__ QuoteSpan quote_span(const QuoteMeta& h, uint32_t cap, int which) {
    const bool prev = which == CDA_TAPE_PREVIOUS;
    long long hi = h.n_total - (prev ? (long long)h.n_episode + (long long)h.gap : 0ll);
    long long lo = hi - (long long)(prev ? h.n_prev : h.n_episode);
    if (lo < 0) lo = 0;
    if (hi < lo) hi = lo;
    long long floor = h.n_total - (long long)cap;
    if (floor < lo) floor = lo;
    if (floor > hi) floor = hi;
    QuoteSpan s;
    s.start = floor; s.count = (int)(hi - floor); s.lost = (int)(floor - lo); s.step0 = (prev ? h.prev_first : h.first) + s.lost;
    s.partial = (h.flags & (prev ? QM_PREV_PARTIAL : QM_PARTIAL)) ? 1 : 0;
    s.slot0 = (uint32_t)((unsigned long long)floor % (unsigned long long)cap);
    return s;
}
// the ring slot of record start + i, 0 <= i < capacity
__device__ __forceinline__ uint32_t quote_slot(const QuoteSpan& s, uint32_t cap, int i) {
    const uint32_t x = s.slot0 + (uint32_t)i;                        // < 2 x capacity <= 2^21
    return x >= cap ? x - cap : x;
}
// THE LAYOUT OF A RECORD, as the readers see it: two 16-byte words r0, r1 of the ring = cda_quote_record (include/cda.h).  The writer is k_quote_record below (one
// word per lane, in the struct's order); every reader decodes through these accessors and nowhere else.  m2 = bid + ask: the mid in half price units.
static_assert(offsetof(cda_quote_record, flags) == 4 && offsetof(cda_quote_record, bid_price) == 8 && offsetof(cda_quote_record, ask_price) == 12,
              "r0 = (step, flags, bid_price, ask_price)");
static_assert(offsetof(cda_quote_record, bid_volume) == 16 && offsetof(cda_quote_record, ask_volume) == 20, "r1 = (bid_volume, ask_volume, bid_orders, ask_orders)");
// (macros for the reason given beside the tape's accessors in cda_tape.inc; quote_m2_i32: the same sum in 32 bits, as styl_stage keeps it in LDS)
#define quote_sides(r0) ((int)((r0).y & 3u))
#define quote_two_sided(r0) (((r0).y & 3u) == 3u)
#define quote_bid(r0) ((long long)(int)(r0).z)
#define quote_ask(r0) ((long long)(int)(r0).w)
#define quote_m2(r0) (quote_bid(r0) + quote_ask(r0))
#define quote_m2_i32(r0) ((int32_t)(r0).z + (int32_t)(r0).w)

// the best level of one side: its price, the summed quantity and the number of its orders.  The side is walked in queue order, 64 orders per pass: the level is the
// run of orders from the first on that carry the first order's price - it ends inside a pass, or continues (a level deeper than the tile: into the HBM ring).
__device__ __forceinline__ void quote_head(const BookSide& b, int lane, int32_t& price, long long& volume, long long& orders) {
    price = 0; volume = 0; orders = 0;
    for (int base = 0; base < b.n; base += WAVE) {
        const int i = base + lane;
        const bool valid = i < b.n;
        int32_t p = 0, q = 0;
        if (valid) { p = b.get(0, i); q = b.get(1, i); }
        if (base == 0) price = __shfl(p, 0);
        const bool in = valid && p == price;
        const unsigned long long m = __ballot(in);
        volume += wave_sum(in ? (long long)q : 0ll);
        orders += (long long)__popcll(m);
        if (m != ~0ull) break;                                       // (uniform) the level ended inside this pass
    }
}

// (the record's layout is stated once, for every reader, by the accessors beside QuoteSpan above: quote_two_sided, quote_m2)
__global__ __launch_bounds__(64 * CDA_WPB) void k_quote_record(const uint8_t* arena, Params P, QuoteArgs Q, int cap, int first, int n) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w;
    // the header's leading words, one per lane: what episode_over asks (the done mask, t_step) without the record
    const uint32_t hw = lane < 32 ? reinterpret_cast<const uint32_t*>(arena + (size_t)mi * (size_t)P.lay.stride)[lane] : 0u;
    const uint32_t done_mask = (uint32_t)__builtin_amdgcn_readlane((int)hw, H_DONE_MASK);
    const int t = __builtin_amdgcn_readlane((int)hw, H_T_STEP);
    if (__popc(done_mask) == P.cfg.num_agents || t >= mrow(P, mi).max_step || t < 0) return;      // the episode is over: the step will not run it either
    QuoteMeta h = quote_roll(quote_meta_load(Q.meta, mi, lane), t);
    int32_t bp, ap;
    long long bv, bo, av, ao;
    quote_head(book_side(arena, P, cap, mi, 0), lane, bp, bv, bo);
    quote_head(book_side(arena, P, cap, mi, 1), lane, ap, av, ao);
    const long long top = 0x7fffffffll;
    int32_t flags = (bo > 0 ? CDA_QUOTE_BID : 0) | (ao > 0 ? CDA_QUOTE_ASK : 0);
    if (bv > top || av > top || bo > top || ao > top) flags |= CDA_QUOTE_SATURATED;              // never wrapped silently
    const int32_t word = lane == 0 ? t : lane == 1 ? flags : lane == 2 ? bp : lane == 3 ? ap : lane == 4 ? (int32_t)(bv > top ? top : bv) :
                         lane == 5 ? (int32_t)(av > top ? top : av) : lane == 6 ? (int32_t)(bo > top ? top : bo) : (int32_t)(ao > top ? top : ao);
    const uint32_t slot = (uint32_t)((unsigned long long)h.n_total % (unsigned long long)Q.cap);
    h.n_total += 1; h.n_episode += 1;
    if (lane < 8) {
        reinterpret_cast<int32_t*>(Q.ring + 2 * ((size_t)mi * (size_t)Q.cap + (size_t)slot))[lane] = word;
        reinterpret_cast<int32_t*>(Q.meta + mi)[lane] = quote_meta_word(h, lane);
    }
}

// the rolled meta rows of a range, as the readers see them: out i32 [n][8]
__global__ __launch_bounds__(64 * CDA_WPB) void k_quote_meta(const uint8_t* arena, Params P, QuoteArgs Q, int first, int n, int32_t* out) {
    READER_WAVE();
    if (w >= n) return;
    const QuoteMeta h = quote_meta_now(Q, arena, P, first + w, lane);
    if (lane < 8) out[8 * (size_t)w + lane] = quote_meta_word(h, lane);
}

// the last kmax held records of an episode, oldest first; rows beyond the count are zero.  info: {records copied, records of the episode that are not among
// them because the ring overwrote them, step of the first copied record, partial}
__global__ __launch_bounds__(64 * CDA_WPB) void k_quote_series(const uint8_t* arena, Params P, QuoteArgs Q, int first, int n, int which, int kmax, uint4* out,
                                                               int32_t* counts, int32_t* info) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w;
    const QuoteSpan sp = quote_span(quote_meta_now(Q, arena, P, mi, lane), Q.cap, which);
    const int cnt = sp.count > kmax ? kmax : sp.count, skip = sp.count - cnt;
    const uint4* ring = Q.ring + 2 * (size_t)mi * (size_t)Q.cap;
    uint4* dst = out + 2 * (size_t)w * (size_t)kmax;
    for (int x = lane; x < 2 * cnt; x += WAVE) dst[x] = ring[2 * (size_t)quote_slot(sp, Q.cap, skip + (x >> 1)) + (size_t)(x & 1)];
    for (long long x = 2ll * cnt + lane; x < 2ll * (long long)kmax; x += WAVE) dst[x] = make_uint4(0u, 0u, 0u, 0u);
    if (lane == 0) {
        if (counts) counts[w] = cnt;
        if (info) reader_info(info, w, cnt, sp.lost, sp.step0 + skip, sp.partial);
    }
}

// the statistics of an episode's held records: out i64 [n][CDA_QUOTE_STAT_WORDS].  64 steps per pass, lane l reads record base + l; the left neighbour comes by
// __shfl_up, lane 0's from the carry of the pass before (uniform registers); wave reductions finish every sum.
__global__ __launch_bounds__(64 * CDA_WPB) void k_quote_stats(const uint8_t* arena, Params P, QuoteArgs Q, int first, int n, int which, long long* out, int32_t* info) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w;
    const QuoteSpan sp = quote_span(quote_meta_now(Q, arena, P, mi, lane), Q.cap, which);
    const uint4* ring = Q.ring + 2 * (size_t)mi * (size_t)Q.cap;
    long long s_two = 0, s_bid = 0, s_ask = 0, s_empty = 0, s_sp = 0, s_sq = 0, s_m2 = 0, s_bv = 0, s_av = 0, s_pairs = 0, s_chg = 0, s_abs = 0, s_d2 = 0;
    long long s_min = 0x7fffffffffffffffll, s_max = -0x7fffffffffffffffll - 1;
    int c_two = 0;                                                   // the carry: the last record of the pass before
    long long c_m2 = 0;
    for (int base = 0; base < sp.count; base += WAVE) {
        const int idx = base + lane;
        const bool in = idx < sp.count;
        uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0;
        if (in) { const uint32_t slot = quote_slot(sp, Q.cap, idx); r0 = ring[2 * (size_t)slot]; r1 = ring[2 * (size_t)slot + 1]; }
        const int side = quote_sides(r0);
        const int two = in && side == 3 ? 1 : 0;
        const long long bid = quote_bid(r0), ask = quote_ask(r0), m2 = bid + ask, spread = ask - bid;
        int p_two = __shfl_up(two, 1);
        long long p_m2 = __shfl_up(m2, 1);
        if (lane == 0) { p_two = c_two; p_m2 = c_m2; }
        const bool pair = two && p_two;
        const long long d = pair ? m2 - p_m2 : 0ll;
        s_two += (long long)__popcll(__ballot(two != 0));
        s_bid += (long long)__popcll(__ballot(in && side == 1));
        s_ask += (long long)__popcll(__ballot(in && side == 2));
        s_empty += (long long)__popcll(__ballot(in && side == 0));
        s_sp += wave_sum(two ? spread : 0ll); s_sq += wave_sum(two ? spread * spread : 0ll); s_m2 += wave_sum(two ? m2 : 0ll);
        s_bv += wave_sum(two ? (long long)(int)r1.x : 0ll); s_av += wave_sum(two ? (long long)(int)r1.y : 0ll);
        const long long lo = wave_min(two ? spread : 0x7fffffffffffffffll), hi = wave_max(two ? spread : -0x7fffffffffffffffll - 1);
        s_min = lo < s_min ? lo : s_min; s_max = hi > s_max ? hi : s_max;
        s_pairs += (long long)__popcll(__ballot(pair));
        s_chg += (long long)__popcll(__ballot(pair && d != 0));
        s_abs += wave_sum(d < 0 ? -d : d); s_d2 += wave_sum(d * d);
        c_two = __shfl(two, 63); c_m2 = __shfl(m2, 63);
    }
    if (s_two == 0) { s_min = 0; s_max = 0; }
    if (lane < CDA_QUOTE_STAT_WORDS) {
        const long long v = lane == QS_STEPS ? (long long)sp.count : lane == QS_TWO_SIDED ? s_two : lane == QS_BID_ONLY ? s_bid : lane == QS_ASK_ONLY ? s_ask :
                            lane == QS_EMPTY ? s_empty : lane == QS_SPREAD_SUM ? s_sp : lane == QS_SPREAD_SQ ? s_sq : lane == QS_SPREAD_MIN ? s_min :
                            lane == QS_SPREAD_MAX ? s_max : lane == QS_M2_SUM ? s_m2 : lane == QS_BID_VOL ? s_bv : lane == QS_ASK_VOL ? s_av :
                            lane == QS_PAIRS ? s_pairs : lane == QS_M2_CHANGES ? s_chg : lane == QS_ABS_DM2 ? s_abs : s_d2;
        out[(size_t)w * CDA_QUOTE_STAT_WORDS + lane] = v;
    }
    if (info && lane == 0) reader_info(info, w, sp.count, sp.lost, sp.step0, sp.partial);
}

// Spread reports: the trade tape joined to the quotes, by step.  One wave per market, lanes over the episode's tape records, 64 per pass (k_tape_exec's frame);
// per fill and horizon the quotes of step s and of step s + k are read at their slots - indexed directly, no search - and the six words of (agent, horizon, role)
// are integer adds on the wave's own slice of dynamic LDS, written out once, dense.
struct SpreadHorizons { int32_t k[CDA_TAPE_MAX_HORIZONS]; };
__global__ __launch_bounds__(64 * CDA_WPB) void k_tape_spreads(const uint8_t* arena, Params P, TapeArgs T, QuoteArgs Q, int first, int n, int which, int agents, int nh,
                                                               SpreadHorizons hz, long long* out, int32_t* info) {
    extern __shared__ __align__(16) unsigned long long spread_lds[];  // per wave: agents x nh x 2 roles x SP_WORDS
    READER_WAVE_IN_GROUP(CDA_WPB);
    const bool live = w < n;
    const int n_words = agents * nh * 2 * SP_WORDS;
    unsigned long long* tb = spread_lds + (size_t)wib * (size_t)n_words;
    for (int i = lane; i < n_words; i += WAVE) tb[i] = 0ull;
    __syncthreads();
    int used = 0;
    TapeSpan ts = {0, 0, 0, 0};
    QuoteSpan qs = {0, 0, 0, 0, 0, 0u};
    if (live) {
        const int mi = first + w;
        ts = tape_span(T.meta[mi], T.cap, which);
        qs = quote_span(quote_meta_now(Q, arena, P, mi, lane), Q.cap, which);
        const uint4* tring = T.ring + (size_t)mi * (size_t)T.cap * 2;
        const uint4* qring = Q.ring + 2 * (size_t)mi * (size_t)Q.cap;
        const uint32_t tmask = T.cap - 1u, t0 = (uint32_t)ts.start & tmask;
        const int count = (int)ts.count;
        const long long q_first = (long long)qs.step0, q_last = qs.count > 0 ? q_first + (long long)qs.count - 1 : -1ll;      // no quote held: every fill is open
        for (int base = 0; base < count; base += WAVE) {
            const int idx = base + lane;
            const bool in = idx < count;
            uint4 r0, r1;
            tape_load(tring, tmask, t0, idx, in, r0, r1);
            const uint32_t cid = tape_counter_id(r0), iid = tape_init_id(r1);
            const long long step = (long long)tape_step(r1);
            const int cside = tape_counter_side(r1), iside = tape_init_side(r1);
            const long long price = (long long)tape_price(r0), qty = (long long)tape_qty(r0);
            const bool ok = in && cid < (uint32_t)agents && iid < (uint32_t)agents;      // (ids outside the env's agents cannot index the table)
            const bool ev = ok && cid != iid;
            used += __popcll(__ballot(ok));
            // the quote of the fill's own step: held iff q_first <= s <= q_last
            const bool now_held = ev && step >= q_first && step <= q_last;
            uint4 qa = make_uint4(0u, 0u, 0u, 0u);
            if (now_held) qa = qring[2 * (size_t)quote_slot(qs, Q.cap, (int)(step - q_first))];
            const bool now_two = now_held && quote_two_sided(qa);
            const long long now = 2 * price - quote_m2(qa);
            for (int h = 0; h < nh; h++) {
                const long long due = step + (long long)hz.k[h];
                const bool open = ev && due > q_last;
                const bool later_held = ev && !open && due >= q_first;                   // (due >= step: held whenever the fill's own step is)
                uint4 qb = make_uint4(0u, 0u, 0u, 0u);
                if (later_held) qb = qring[2 * (size_t)quote_slot(qs, Q.cap, (int)(due - q_first))];
                const bool scored = now_two && later_held && quote_two_sided(qb);
                if (!ev) continue;
                unsigned long long* cm = tb + (((int)cid * nh + h) * 2) * SP_WORDS;          // [agent][horizon][role 0 = maker][6]
                unsigned long long* ct = tb + (((int)iid * nh + h) * 2 + 1) * SP_WORDS;      // ... [role 1 = taker]
                if (scored) {
                    const long long later = 2 * price - quote_m2(qb);
                    lds_add(cm + SP_COST_NOW, (cside ? -now : now) * qty); lds_add(cm + SP_COST_LATER, (cside ? -later : later) * qty);
                    lds_add(cm + SP_QTY, qty); lds_add(cm + SP_FILLS, 1ll);
                    lds_add(ct + SP_COST_NOW, (iside ? -now : now) * qty); lds_add(ct + SP_COST_LATER, (iside ? -later : later) * qty);
                    lds_add(ct + SP_QTY, qty); lds_add(ct + SP_FILLS, 1ll);
                } else {
                    const int word = open ? SP_OPEN : SP_UNQUOTED;
                    lds_add(cm + word, 1ll); lds_add(ct + word, 1ll);
                }
            }
        }
    }
    __syncthreads();
    if (!live) return;
    long long* o = out + (size_t)w * (size_t)n_words;
    for (int i = lane; i < n_words; i += WAVE) o[i] = (long long)tb[i];
    if (info && lane == 0) reader_info(info, w, (int32_t)used, (int32_t)ts.lost, (int32_t)qs.lost, (int32_t)(ts.partial | (qs.partial << 1)));
}

// the launch every step entry point issues behind the order schedule's and ahead of the step (launch_step); arguments validated by the callers
static int quotes_record(cda_env* e, int32_t first, int32_t n, hipStream_t stream) {
    if (!e->quotes.ring) return CDA_OK;
    hipLaunchKernelGGL(k_quote_record, grid_for(n), dim3(64 * CDA_WPB), 0, stream, (const uint8_t*)e->arena, e->P, e->quotes, (int)e->cap, (int)first, (int)n);
    return launch_status();
}
static void quotes_free(cda_env* e) {
    if (e->quotes.ring) (void)hipFree(e->quotes.ring);
    if (e->quotes.meta) (void)hipFree(e->quotes.meta);
    memset(&e->quotes, 0, sizeof e->quotes);
}

extern "C" {

int cda_quotes_enable(cda_env* e, int64_t capacity_steps) {
    if (!e || capacity_steps < 1 || capacity_steps > CDA_QUOTE_CAP_MAX) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    quotes_free(e);
    const size_t n = (size_t)e->P.n_markets;
    DevBuf<uint4> ring; DevBuf<QuoteMeta> meta;
    if (ring.alloc(n * (size_t)capacity_steps * sizeof(cda_quote_record)) != hipSuccess || meta.alloc(n * sizeof(QuoteMeta)) != hipSuccess) { (void)hipGetLastError(); return CDA_ERR_NOMEM; }
    hipError_t he = hipMemset(ring, 0, n * (size_t)capacity_steps * sizeof(cda_quote_record));
    if (he == hipSuccess) he = hipMemset(meta, 0, n * sizeof(QuoteMeta));
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he != hipSuccess) return hip_fail(he, "cda_quotes_enable");
    e->quotes.ring = ring.release(); e->quotes.meta = meta.release(); e->quotes.cap = (uint32_t)capacity_steps; e->quotes.pad = 0;
    return CDA_OK;
}
int cda_quotes_disable(cda_env* e) {
    if (!e) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    quotes_free(e);
    return CDA_OK;
}
int64_t cda_quotes_capacity(const cda_env* e) { return e && e->quotes.ring ? (int64_t)e->quotes.cap : 0; }

int cda_quote_meta(cda_env* e, int32_t first_market, int32_t n_markets, int32_t* meta_out_dev, void* stream) {
    if (!reader_args_ok(e, meta_out_dev, first_market, n_markets) || !aligned(meta_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->quotes.ring) return CDA_ERR_UNSUPPORTED;
    return reader_launch(e, k_quote_meta, n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, e->quotes, (int)first_market, (int)n_markets, meta_out_dev);
}
int cda_quote_series(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, int32_t k, void* records_out_dev, int32_t* counts_out_dev, int32_t* info_out_dev,
                     void* stream) {
    if (!reader_args_ok(e, records_out_dev, first_market, n_markets) || k < 1 || !which_ok(which) || !aligned(records_out_dev, 16) || !aligned(counts_out_dev, 4) ||
        !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->quotes.ring) return CDA_ERR_UNSUPPORTED;
    return reader_launch(e, k_quote_series, n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, e->quotes, (int)first_market, (int)n_markets, (int)which, (int)k,
                         (uint4*)records_out_dev, counts_out_dev, info_out_dev);
}
int cda_quote_stats(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, int64_t* stats_out_dev, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, stats_out_dev, first_market, n_markets) || !which_ok(which) || !aligned(stats_out_dev, 8) || !aligned(info_out_dev, 4) ||
        !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->quotes.ring) return CDA_ERR_UNSUPPORTED;
    return reader_launch(e, k_quote_stats, n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, e->quotes, (int)first_market, (int)n_markets, (int)which,
                         (long long*)stats_out_dev, info_out_dev);
}
int cda_tape_spreads(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* horizons_host, int32_t n_horizons, int64_t* spreads_out_dev,
                     int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, spreads_out_dev, first_market, n_markets) || !horizons_host || n_horizons < 1 || n_horizons > CDA_TAPE_MAX_HORIZONS || !which_ok(which) ||
        !aligned(spreads_out_dev, 8) || !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    SpreadHorizons hz;
    memset(&hz, 0, sizeof hz);
    for (int h = 0; h < n_horizons; h++) {
        if (horizons_host[h] < 0) return CDA_ERR_INVALID;
        hz.k[h] = horizons_host[h];
    }
    if (!agents_ok(e)) return CDA_ERR_INVALID;
    if (!e->tape.ring || !e->quotes.ring) return CDA_ERR_UNSUPPORTED;
    const size_t lds = (size_t)CDA_WPB * (size_t)e->P.cfg.num_agents * (size_t)n_horizons * 2 * SP_WORDS * sizeof(unsigned long long);      // <= 4 x 16 x 8 x 12 x 8 = 48 KiB
    return reader_launch(e, k_tape_spreads, n_markets, CDA_WPB, lds, stream, (const uint8_t*)e->arena, e->P, e->tape, e->quotes, (int)first_market, (int)n_markets, (int)which,
                         (int)e->P.cfg.num_agents, (int)n_horizons, hz, (long long*)spreads_out_dev, info_out_dev);
}

}  // extern "C"
