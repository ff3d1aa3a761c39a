// cda_depth.inc - the depth tape (include/cda.h cda_depth_*): the Level-2 ladder per step of an episode, recorded on the device, and the book-shape reductions
// over it.  Included at the end of cda_hip.hip, behind cda_book_report.inc (the walk of a side: BookSide, k_book_levels' scheme), cda_quotes.inc (QuoteMeta,
// quote_roll, quote_span, quote_slot: the episode rule is stated THERE and only there) and cda_stylised.inc (StylLags, styl_points, styl_waves); the wave toolkit
// is cda_wave.hpp.  depth.py states every word in numpy.
//
// Per market a ring of `capacity` records of 1 + levels 16-byte words in a buffer of its own beside the arena, and one QuoteMeta row of the service's own: neither
// the market record, nor the state dump, nor the snapshot blob know of either.  The WRITER is k_depth_record, which launch_step issues behind the quote recorder's
// launch and ahead of the step kernel while depth is on: k_quote_record's frame (one wave per market, the header's leading words in one 128-byte load, gone at
// once where the episode is over), then k_book_levels' walk of each side, ended as soon as `levels` levels are complete and it is known whether another follows.
// Only the market's own wave writes its ring slot and its meta row, with ordinary per-lane vector stores; every half word of the slot is written on every visit
// (levels below the side's count by the lane that closes the level, the others as zeros): the ring is never cleared.  No atomics, no LDS, no scratch.
//
// The READERS are one wave per market.  k_depth_profile lays its lanes over the WORDS of consecutive records - lane = record of the pass x (1 + levels) + word, a
// contiguous run of the ring modulo the capacity -, so a lane serves one level index in every pass and keeps that level's sums in registers; k_depth_imbalance and
// k_depth_ofi lay them over records, 64 per pass.  Tables are integer adds on the wave's own slice of dynamic LDS (lds_add; k_depth_ofi's bar words are int32, as
// k_tape_flow_returns' Q_b), written out dense once.  Nothing is atomic on global memory.

static_assert(sizeof(cda_depth_head) == 16 && sizeof(cda_depth_level) == 16, "a depth record is 1 + levels 16-byte words");
static_assert(CDA_DEPTH_MAX_LEVELS == 16 && CDA_DEPTH_MAX_LEVELS < WAVE && CDA_DEPTH_MAX_DIST == 256 && CDA_DEPTH_MAX_DEPTHS == 4, "depth tape bounds");
static_assert(CDA_DEPTH_BID == CDA_QUOTE_BID && CDA_DEPTH_ASK == CDA_QUOTE_ASK && CDA_DEPTH_SATURATED == CDA_QUOTE_SATURATED, "the side bits are the quote tape's");
enum { DP_STEPS = 0, DP_TWO_SIDED, DP_BID_MORE, DP_ASK_MORE, DP_SATURATED, DP_BID_LEVELS, DP_ASK_LEVELS, DP_ZERO, DP_WORDS, DP_LEVEL_WORDS = 3 };
enum { DI_STEPS = 0, DI_TWO_SIDED, DI_DIFF, DI_SUM, DI_WORDS, DI_RESP_WORDS = 5 };
enum { DO_PAIRS = 0, DO_BARS_KEPT, DO_BARS_EXCLUDED, DO_SATURATED, DO_WORDS, DO_LAG_WORDS = 6 };

// THE LAYOUT OF A RECORD, as the readers see it: word 0 `h` = cda_depth_head, word 1 + l `r` = cda_depth_level l (include/cda.h).  The writer is k_depth_record
// below; every reader decodes through these accessors and nowhere else.  m2 = bid + ask of level 0: the mid in half price units.
static_assert(offsetof(cda_depth_head, flags) == 4 && offsetof(cda_depth_head, bid_levels) == 8 && offsetof(cda_depth_head, ask_levels) == 12,
              "h = (step, flags, bid_levels, ask_levels)");
static_assert(offsetof(cda_depth_level, bid_volume) == 4 && offsetof(cda_depth_level, ask_price) == 8 && offsetof(cda_depth_level, ask_volume) == 12,
              "r = (bid_price, bid_volume, ask_price, ask_volume)");
#define depth_flags(h) ((int)(h).y)
#define depth_two_sided(h) (((h).y & 3u) == 3u)
#define depth_bid_levels(h) ((int)(h).z)
#define depth_ask_levels(h) ((int)(h).w)
#define depth_bid_price(r) ((int32_t)(r).x)
#define depth_bid_volume(r) ((long long)(int)(r).y)
#define depth_ask_price(r) ((int32_t)(r).z)
#define depth_ask_volume(r) ((long long)(int)(r).w)
#define depth_m2(r) ((long long)(int)(r).x + (long long)(int)(r).z)

// market mi's ring: records of W = 1 + levels words
__device__ __forceinline__ uint4* depth_ring(const DepthArgs& D, int mi) { return D.ring + (size_t)mi * (size_t)D.cap * (size_t)(1u + D.levels); }
// what a reader sees: the service's stored row, rolled to the market's clock (the quote tape's own function over this service's rows)
__device__ __forceinline__ QuoteMeta depth_meta_now(const DepthArgs& D, const uint8_t* arena, const Params& P, int mi, int lane) {
    const QuoteArgs q = {nullptr, D.meta, D.cap, 0u};
    return quote_meta_now(q, arena, P, mi, lane);
}
// |a - b| / tick of two prices (int32 words, multiples of tick: exact), in 32 bits
__device__ __forceinline__ uint32_t depth_dist(int32_t a, int32_t b, uint32_t tick) {
    const long long d = (long long)a - (long long)b;
    return (uint32_t)(d < 0 ? -d : d) / tick;
}

// one side's half of level `level` of the record at `rec`: one 8-byte store
__device__ __forceinline__ void depth_store(int32_t* rec, int sd, int level, int32_t price, long long volume) {
    const long long top = 0x7fffffffll;
    *reinterpret_cast<int2*>(rec + 4 * (1 + level) + 2 * sd) = make_int2((int)price, (int)(volume > top ? top : volume));
}
// The best L levels of one side into the record at `rec`: k_book_levels' walk - 64 orders per pass in queue order, level heads = price changes between neighbours,
// a segmented scan leaves a level's volume in its last lane, which stores it; the level that reaches the pass's last order is carried.  The walk ends with the
// side, or with the pass in which a head of index L shows: levels 0 .. L - 1 are then complete and `more` is known.  -> the levels recorded; the half words of the
// levels behind them are stored as zeros.  sat: set where a stored volume was clamped.
__device__ __forceinline__ int depth_side(const BookSide& b, int lane, int L, int32_t* rec, int sd, int& more, int& sat) {
    const long long top = 0x7fffffffll;
    int lv = -1;                                                     // the carried (open) level: its index, price, volume
    int32_t cp = 0;
    long long cvol = 0;
    more = 0;
    for (int base = 0; base < b.n; base += WAVE) {
        const int i = base + lane;
        const bool valid = i < b.n;
        int32_t p = 0, q = 0;
        if (valid) { p = b.get(0, i); q = b.get(1, i); }
        const int32_t up = __shfl_up(p, 1);
        const unsigned long long heads = __ballot(valid && (lane == 0 ? (lv < 0 || p != cp) : p != up));
        const unsigned long long le = lanes_le(lane);
        const int level = lv + __popcll(heads & le);
        const int seg = 63 - __clzll((long long)((heads | 1ull) & le));      // first lane of this lane's run (lane 0 may continue the carried level)
        long long vol = (long long)q;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) { const long long o = __shfl_up(vol, d); if (lane - d >= seg) vol += o; }
        if (seg == 0 && (heads & 1ull) == 0ull) vol += cvol;
        if ((heads & 1ull) != 0ull && lv >= 0 && lv < L) {           // (uniform) the carried level ended with the last pass
            if (lane == 0) depth_store(rec, sd, lv, cp, cvol);
            if (cvol > top) sat = 1;
        }
        const int lastv = 63 - __clzll((long long)__ballot(valid));
        const bool tail = valid && lane < lastv && ((heads >> ((lane + 1) & 63)) & 1ull) != 0ull && level < L;
        if (tail) depth_store(rec, sd, level, p, vol);
        if (__ballot(tail && vol > top) != 0ull) sat = 1;
        lv = __shfl(level, lastv); cp = __shfl(p, lastv); cvol = __shfl(vol, lastv);
        if (lv >= L) { more = 1; break; }                            // levels 0 .. L - 1 are stored; the open level lies behind them
    }
    if (lv >= 0 && lv < L) {
        if (lane == 0) depth_store(rec, sd, lv, cp, cvol);
        if (cvol > top) sat = 1;
    }
    const int count = lv + 1 > L ? L : lv + 1;
    if (lane >= count && lane < L) depth_store(rec, sd, lane, 0, 0ll);
    return count;
}

__global__ __launch_bounds__(64 * CDA_WPB) void k_depth_record(const uint8_t* arena, Params P, DepthArgs D, int cap, int first, int n) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w;
    // the header's leading words, one per lane: what episode_over asks (the done mask, t_step) without the record
    const uint32_t hw = lane < 32 ? reinterpret_cast<const uint32_t*>(arena + (size_t)mi * (size_t)P.lay.stride)[lane] : 0u;
    const uint32_t done_mask = (uint32_t)__builtin_amdgcn_readlane((int)hw, H_DONE_MASK);
    const int t = __builtin_amdgcn_readlane((int)hw, H_T_STEP);
    if (__popc(done_mask) == P.cfg.num_agents || t >= mrow(P, mi).max_step || t < 0) return;      // the episode is over: the step will not run it either
    QuoteMeta h = quote_roll(quote_meta_load(D.meta, mi, lane), t);
    const int L = (int)D.levels;
    const uint32_t slot = (uint32_t)((unsigned long long)h.n_total % (unsigned long long)D.cap);
    int32_t* rec = reinterpret_cast<int32_t*>(depth_ring(D, mi) + (size_t)slot * (size_t)(1 + L));
    int bmore, amore, sat = 0;
    const int nb = depth_side(book_side(arena, P, cap, mi, 0), lane, L, rec, 0, bmore, sat);
    const int na = depth_side(book_side(arena, P, cap, mi, 1), lane, L, rec, 1, amore, sat);
    const int32_t flags = (nb > 0 ? CDA_DEPTH_BID : 0) | (na > 0 ? CDA_DEPTH_ASK : 0) | (sat ? CDA_DEPTH_SATURATED : 0) | (bmore ? CDA_DEPTH_BID_MORE : 0) |
                          (amore ? CDA_DEPTH_ASK_MORE : 0);
    h.n_total += 1; h.n_episode += 1;
    if (lane < 4) rec[lane] = lane == 0 ? t : lane == 1 ? flags : lane == 2 ? nb : na;
    if (lane < 8) reinterpret_cast<int32_t*>(D.meta + mi)[lane] = quote_meta_word(h, lane);
}

// the rolled meta rows of a range, as the readers see them: out i32 [n][8]
__global__ __launch_bounds__(64 * CDA_WPB) void k_depth_meta(const uint8_t* arena, Params P, DepthArgs D, int first, int n, int32_t* out) {
    READER_WAVE();
    if (w >= n) return;
    const QuoteMeta h = depth_meta_now(D, arena, P, first + w, lane);
    if (lane < 8) out[8 * (size_t)w + lane] = quote_meta_word(h, lane);
}

// the last kmax held records of an episode, oldest first; rows beyond the count are zero.  info as k_quote_series
__global__ __launch_bounds__(64 * CDA_WPB) void k_depth_series(const uint8_t* arena, Params P, DepthArgs D, int first, int n, int which, int kmax, uint4* out,
                                                               int32_t* counts, int32_t* info) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w;
    const uint32_t W = 1u + D.levels;
    const QuoteSpan sp = quote_span(depth_meta_now(D, arena, P, mi, lane), D.cap, which);
    const int cnt = sp.count > kmax ? kmax : sp.count, skip = sp.count - cnt;
    const uint4* ring = depth_ring(D, mi);
    uint4* dst = out + (size_t)w * (size_t)kmax * (size_t)W;
    const uint32_t words = (uint32_t)cnt * W;                        // <= 2^20 x 17
    for (uint32_t x = (uint32_t)lane; x < words; x += WAVE) {
        const uint32_t r = x / W, c = x - r * W;
        dst[x] = ring[(size_t)quote_slot(sp, D.cap, skip + (int)r) * (size_t)W + (size_t)c];
    }
    for (long long x = (long long)words + lane; x < (long long)kmax * (long long)W; x += WAVE) dst[x] = make_uint4(0u, 0u, 0u, 0u);
    if (lane == 0) {
        if (counts) counts[w] = cnt;
        if (info) reader_info(info, w, cnt, sp.lost, sp.step0 + skip, sp.partial);
    }
}

// The average shape of the book.  Lanes over the words of G = 64 / W consecutive records per pass: lane = rl x W + word, so `word` - the head, or level word - 1 - is
// the lane's own over all passes.  A level lane reads its word, its record's head and its record's level 0; its six sums stay in registers.  LDS per wave:
// DP_WORDS + 6 L + 2 (md + 1) 64-bit words.
__global__ __launch_bounds__(64 * CDA_WPB) void k_depth_profile(const uint8_t* arena, Params P, DepthArgs D, int first, int n, int which, int md, long long* base_out,
                                                                long long* lev_out, long long* shape_out, int32_t* info) {
    extern __shared__ __align__(16) unsigned long long depth_prof_lds[];
    READER_WAVE_IN_GROUP(CDA_WPB);
    const bool live = w < n;
    const int L = (int)D.levels, W = 1 + L, n_lev = 2 * L * DP_LEVEL_WORDS, n_shape = 2 * (md + 1), n_words = DP_WORDS + n_lev + n_shape;
    unsigned long long* tb = depth_prof_lds + (size_t)wib * (size_t)n_words;
    unsigned long long* lev = tb + DP_WORDS;
    unsigned long long* shape = lev + n_lev;
    for (int i = lane; i < n_words; i += WAVE) tb[i] = 0ull;
    __syncthreads();
    QuoteSpan sp = {0, 0, 0, 0, 0, 0u};
    if (live) {
        const int mi = first + w;
        sp = quote_span(depth_meta_now(D, arena, P, mi, lane), D.cap, which);
        const uint4* ring = depth_ring(D, mi);
        const int tk = mrow(P, mi).tick_size;
        const uint32_t tick = tk < 1 ? 1u : (uint32_t)tk;
        const int G = WAVE / W;                                       // records per pass: 3 (levels 16) .. 32 (levels 1)
        const int rl = lane / W, word = lane - rl * W, l = word - 1;
        const bool on = rl < G;
        long long a[2][DP_LEVEL_WORDS] = {};                          // a level lane's sums: per side steps, volume, distance
        long long c_two = 0, c_bm = 0, c_am = 0, c_sat = 0, c_bl = 0, c_al = 0;      // a head lane's
        for (int base = 0; base < sp.count; base += G) {
            const int idx = base + rl;
            if (!on || idx >= sp.count) continue;
            const uint4* rp = ring + (size_t)quote_slot(sp, D.cap, idx) * (size_t)W;
            const uint4 hd = rp[0];
            if (word == 0) {
                const int f = depth_flags(hd);
                c_two += depth_two_sided(hd) ? 1 : 0; c_bm += (f & CDA_DEPTH_BID_MORE) ? 1 : 0; c_am += (f & CDA_DEPTH_ASK_MORE) ? 1 : 0;
                c_sat += (f & CDA_DEPTH_SATURATED) ? 1 : 0; c_bl += (long long)depth_bid_levels(hd); c_al += (long long)depth_ask_levels(hd);
                continue;
            }
            const uint4 best = rp[1], r = rp[word];
            if (l < depth_bid_levels(hd)) {
                const uint32_t d = depth_dist(depth_bid_price(r), depth_bid_price(best), tick);
                a[0][0] += 1; a[0][1] += depth_bid_volume(r); a[0][2] += (long long)d;
                lds_add(shape + (d > (uint32_t)md ? (uint32_t)md : d), depth_bid_volume(r));
            }
            if (l < depth_ask_levels(hd)) {
                const uint32_t d = depth_dist(depth_ask_price(r), depth_ask_price(best), tick);
                a[1][0] += 1; a[1][1] += depth_ask_volume(r); a[1][2] += (long long)d;
                lds_add(shape + (md + 1) + (d > (uint32_t)md ? (uint32_t)md : d), depth_ask_volume(r));
            }
        }
        if (on && word == 0) {
            lds_add(tb + DP_TWO_SIDED, c_two); lds_add(tb + DP_BID_MORE, c_bm); lds_add(tb + DP_ASK_MORE, c_am); lds_add(tb + DP_SATURATED, c_sat);
            lds_add(tb + DP_BID_LEVELS, c_bl); lds_add(tb + DP_ASK_LEVELS, c_al);
        }
        if (on && word > 0) {
#pragma unroll
            for (int sd = 0; sd < 2; sd++)
#pragma unroll
                for (int j = 0; j < DP_LEVEL_WORDS; j++) lds_add(lev + (sd * L + l) * DP_LEVEL_WORDS + j, a[sd][j]);
        }
    }
    __syncthreads();
    if (!live) return;
    if (lane < DP_WORDS) base_out[(size_t)w * DP_WORDS + lane] = lane == DP_STEPS ? (long long)sp.count : (long long)tb[lane];
    for (int i = lane; i < n_lev; i += WAVE) lev_out[(size_t)w * (size_t)n_lev + i] = (long long)lev[i];
    for (int i = lane; i < n_shape; i += WAVE) shape_out[(size_t)w * (size_t)n_shape + i] = (long long)shape[i];
    if (info && lane == 0) reader_info(info, w, sp.count, sp.lost, sp.step0, sp.partial);
}

// the head and level 0 of the held record idx of a span: is it two-sided, and its m2
__device__ __forceinline__ bool depth_mid(const uint4* ring, const QuoteSpan& sp, uint32_t cap, int W, int idx, long long& m2) {
    const uint4* rp = ring + (size_t)quote_slot(sp, cap, idx) * (size_t)W;
    const uint4 hd = rp[0];
    m2 = depth_m2(rp[1]);
    return depth_two_sided(hd);
}

// The response curve: the future mid move given today's depth imbalance.  Lanes over records, 64 per pass; the partner record s + lag is read at its slot (a span is
// consecutive steps: held iff idx + lag < count).  LDS per wave: nl x 2 half x 5 64-bit words (at most 40 KiB: the host sizes the workgroup).
__global__ __launch_bounds__(64 * CDA_WPB) void k_depth_imbalance(const uint8_t* arena, Params P, DepthArgs D, int first, int n, int which, int nl, StylLags lg, int k,
                                                                  int half, long long* resp_out, long long* base_out, int32_t* info) {
    extern __shared__ __align__(16) unsigned long long depth_imb_lds[];
    READER_WAVE_IN_GROUP((int)(blockDim.x >> 6));
    const bool live = w < n;
    const int W = 1 + (int)D.levels, n_words = nl * 2 * half * DI_RESP_WORDS;
    unsigned long long* tb = depth_imb_lds + (size_t)wib * (size_t)n_words;
    for (int i = lane; i < n_words; i += WAVE) tb[i] = 0ull;
    __syncthreads();
    QuoteSpan sp = {0, 0, 0, 0, 0, 0u};
    long long c_two = 0, s_diff = 0, s_sum = 0;
    if (live) {
        const int mi = first + w;
        sp = quote_span(depth_meta_now(D, arena, P, mi, lane), D.cap, which);
        const uint4* ring = depth_ring(D, mi);
        for (int base = 0; base < sp.count; base += WAVE) {
            const int idx = base + lane;
            if (idx >= sp.count) continue;
            const uint4* rp = ring + (size_t)quote_slot(sp, D.cap, idx) * (size_t)W;
            if (!depth_two_sided(rp[0])) continue;
            long long B = 0, A = 0;                                   // (rows at or beyond a side's count are zero: absent levels add nothing)
            for (int m = 0; m < k; m++) { const uint4 r = rp[1 + m]; B += depth_bid_volume(r); A += depth_ask_volume(r); }
            const long long m2 = depth_m2(rp[1]), den = B + A;
            int bin = den > 0 ? (int)((unsigned long long)(2 * B * (long long)half) / (unsigned long long)den) : 0;
            bin = bin > 2 * half - 1 ? 2 * half - 1 : bin;
            c_two += 1; s_diff += B - A; s_sum += den;
            for (int h = 0; h < nl; h++) {
                const long long j = (long long)idx + (long long)lg.k[h];
                long long m2b;
                if (j >= (long long)sp.count || !depth_mid(ring, sp, D.cap, W, (int)j, m2b)) continue;
                const long long r = m2b - m2;
                unsigned long long* cell = tb + ((size_t)h * (size_t)(2 * half) + (size_t)bin) * DI_RESP_WORDS;
                lds_add(cell, 1ll); lds_add(cell + 1, r); lds_add(cell + 2, r * r);
                if (r > 0) lds_add(cell + 3, 1ll);
                if (r < 0) lds_add(cell + 4, 1ll);
            }
        }
    }
    __syncthreads();
    if (!live) return;
    const long long t_two = wave_sum(c_two), t_diff = wave_sum(s_diff), t_sum = wave_sum(s_sum);
    if (lane < DI_WORDS) base_out[(size_t)w * DI_WORDS + lane] = lane == DI_STEPS ? (long long)sp.count : lane == DI_TWO_SIDED ? t_two : lane == DI_DIFF ? t_diff : t_sum;
    for (int i = lane; i < n_words; i += WAVE) resp_out[(size_t)w * (size_t)n_words + i] = (long long)tb[i];
    if (info && lane == 0) reader_info(info, w, sp.count, sp.lost, sp.step0, sp.partial);
}

// r_p = m2((p + 1) bar) - m2(p bar) of this tape; defined iff both points are held and two-sided (styl_return's statement, read from the ring)
__device__ __forceinline__ bool depth_return(const uint4* ring, const QuoteSpan& sp, uint32_t cap, int W, int bar, StylPoints pt, long long p, long long& r) {
    r = 0;
    if (p < (long long)pt.lo || p >= (long long)pt.hi) return false;
    long long a, b;
    const bool ta = depth_mid(ring, sp, cap, W, (int)p * bar - sp.step0, a), tb = depth_mid(ring, sp, cap, W, ((int)p + 1) * bar - sp.step0, b);
    if (!ta || !tb) return false;
    r = b - a;
    return true;
}

// Multi-level order-flow imbalance against returns, bar by bar: k_tape_flow_returns with the tape walk replaced by a walk of the depth ring.  First the pairs: lanes
// over records, 64 per pass, lane idx reads records idx - 1 and idx level by level, the running sum over the levels is OFI_K at K = m + 1, added to bar word
// [j][b] for every asked depth K_j (int32 adds in LDS: their order cannot matter).  Then per lag the products over the kept bars, 64 per pass; the returns come
// from the ring.  LDS per wave: nd x cap_pts int32 words (at most 64 KiB: one market-wave per workgroup then).
struct DepthDepths { int32_t k[CDA_DEPTH_MAX_DEPTHS]; };
__global__ __launch_bounds__(64 * CDA_WPB) void k_depth_ofi(const uint8_t* arena, Params P, DepthArgs D, int first, int n, int which, int bar, int nl, StylLags lg, int nd,
                                                            DepthDepths dp, int cap_pts, long long* lag_out, long long* base_out, int32_t* info) {
    extern __shared__ __align__(16) int32_t depth_ofi_lds[];
    READER_WAVE_IN_GROUP((int)(blockDim.x >> 6));
    const bool live = w < n;
    const int W = 1 + (int)D.levels;
    int32_t* qbar = depth_ofi_lds + (size_t)wib * (size_t)nd * (size_t)cap_pts;
    for (int i = lane; i < nd * cap_pts; i += WAVE) qbar[i] = 0;
    __syncthreads();
    QuoteSpan sp = {0, 0, 0, 0, 0, 0u};
    StylPoints pt = {0, -1};
    const uint4* ring = depth_ring(D, live ? first + w : first);
    long long b_first = 0, b_end = 0;                                 // the kept bars that are complete: [b_first, b_end)
    long long c_pairs = 0, c_sat = 0;
    if (live) {
        sp = quote_span(depth_meta_now(D, arena, P, first + w, lane), D.cap, which);
        pt = styl_points(sp, bar, cap_pts);
        if (sp.count > 0 && (sp.lost > 0 || sp.partial)) b_first = (long long)(sp.step0 / bar) + 1;      // (nothing held: nothing to exclude, every word is zero)
        b_end = sp.count > 0 ? ((long long)sp.step0 + (long long)sp.count) / (long long)bar : 0ll;
        int top = 0;
        for (int j = 0; j < nd; j++) top = dp.k[j] > top ? dp.k[j] : top;
        for (int base = 0; base < sp.count; base += WAVE) {
            const int idx = base + lane;
            if (idx >= sp.count) continue;
            const uint4* rc = ring + (size_t)quote_slot(sp, D.cap, idx) * (size_t)W;
            const uint4 hc = rc[0];
            c_sat += (depth_flags(hc) & CDA_DEPTH_SATURATED) ? 1 : 0;
            if (idx == 0) continue;                                   // (the first held record has no pair)
            const uint4* rv = ring + (size_t)quote_slot(sp, D.cap, idx - 1) * (size_t)W;
            const uint4 hv = rv[0];
            const long long b = ((long long)sp.step0 + (long long)idx) / (long long)bar;
            c_pairs += b >= b_first && b < b_end ? 1 : 0;
            if (b >= (long long)cap_pts) continue;                    // (never: a step lies below the range's largest max_step)
            long long run = 0;
            for (int m = 0; m < top; m++) {
                const uint4 c = rc[1 + m], v = rv[1 + m];
                const int32_t pb = depth_bid_price(c), pbv = depth_bid_price(v);                 // (an absent bid level is a zero row: price 0, volume 0)
                const int32_t pa = m < depth_ask_levels(hc) ? depth_ask_price(c) : 0x7fffffff, pav = m < depth_ask_levels(hv) ? depth_ask_price(v) : 0x7fffffff;
                run += (pb >= pbv ? depth_bid_volume(c) : 0ll) - (pb <= pbv ? depth_bid_volume(v) : 0ll) - (pa <= pav ? depth_ask_volume(c) : 0ll) +
                       (pa >= pav ? depth_ask_volume(v) : 0ll);
                for (int j = 0; j < nd; j++)
                    if (dp.k[j] == m + 1) atomicAdd(qbar + (size_t)j * (size_t)cap_pts + (size_t)b, (int32_t)(uint32_t)(unsigned long long)run);
            }
        }
    }
    __syncthreads();
    if (!live) return;
    for (int h = 0; h < nl; h++) {
        long long acc[CDA_DEPTH_MAX_DEPTHS][DO_LAG_WORDS] = {};
        for (long long b0 = b_first; b0 < (long long)pt.hi; b0 += WAVE) {            // (bar b <= hi - 1 < cap_pts: r_(b + lag) needs the point behind it)
            const long long b = b0 + lane;
            long long r;
            if (b >= (long long)pt.hi || !depth_return(ring, sp, D.cap, W, bar, pt, b + (long long)lg.k[h], r)) continue;
#pragma unroll
            for (int j = 0; j < CDA_DEPTH_MAX_DEPTHS; j++) {
                if (j >= nd) break;
                const long long q = (long long)qbar[(size_t)j * (size_t)cap_pts + (size_t)b];
                acc[j][0] += 1; acc[j][1] += q; acc[j][2] += r; acc[j][3] += q * r; acc[j][4] += q * q; acc[j][5] += r * r;
            }
        }
        long long v = 0;
#pragma unroll
        for (int j = 0; j < CDA_DEPTH_MAX_DEPTHS; j++) {
            if (j >= nd) break;
#pragma unroll
            for (int x = 0; x < DO_LAG_WORDS; x++) { const long long s = wave_sum(acc[j][x]); if (lane == j * DO_LAG_WORDS + x) v = s; }
        }
        if (lane < nd * DO_LAG_WORDS)
            lag_out[(((size_t)w * (size_t)nd + (size_t)(lane / DO_LAG_WORDS)) * (size_t)nl + (size_t)h) * DO_LAG_WORDS + (size_t)(lane % DO_LAG_WORDS)] = v;
    }
    const long long t_pairs = wave_sum(c_pairs), t_sat = wave_sum(c_sat);
    if (lane < DO_WORDS)
        base_out[(size_t)w * DO_WORDS + lane] = lane == DO_PAIRS ? t_pairs : lane == DO_BARS_KEPT ? (b_end > b_first ? b_end - b_first : 0ll) : lane == DO_BARS_EXCLUDED ? b_first : t_sat;
    if (info && lane == 0) reader_info(info, w, sp.count, sp.lost, sp.step0, sp.partial);
}

// the launch every step entry point issues behind the quote recorder's and ahead of the step (launch_step); arguments validated by the callers
static int depth_record(cda_env* e, int32_t first, int32_t n, hipStream_t stream) {
    if (!e->depth.ring) return CDA_OK;
    hipLaunchKernelGGL(k_depth_record, grid_for(n), dim3(64 * CDA_WPB), 0, stream, (const uint8_t*)e->arena, e->P, e->depth, (int)e->cap, (int)first, (int)n);
    return launch_status();
}
static void depth_free(cda_env* e) {
    if (e->depth.ring) (void)hipFree(e->depth.ring);
    if (e->depth.meta) (void)hipFree(e->depth.meta);
    memset(&e->depth, 0, sizeof e->depth);
}

extern "C" {

int cda_depth_enable(cda_env* e, int64_t capacity_steps, int32_t levels) {
    if (!e || capacity_steps < 1 || capacity_steps > CDA_QUOTE_CAP_MAX || levels < 1 || levels > CDA_DEPTH_MAX_LEVELS) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    const size_t n = (size_t)e->P.n_markets, bytes = n * (size_t)capacity_steps * (size_t)(1 + levels) * sizeof(uint4);
    DevBuf<uint4> ring; DevBuf<QuoteMeta> meta;                       // (the env keeps what it has until both allocations stand)
    if (ring.alloc(bytes) != hipSuccess || meta.alloc(n * sizeof(QuoteMeta)) != hipSuccess) { (void)hipGetLastError(); return CDA_ERR_NOMEM; }
    hipError_t he = hipMemset(ring, 0, bytes);
    if (he == hipSuccess) he = hipMemset(meta, 0, n * sizeof(QuoteMeta));
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he != hipSuccess) return hip_fail(he, "cda_depth_enable");
    depth_free(e);
    e->depth.ring = ring.release(); e->depth.meta = meta.release(); e->depth.cap = (uint32_t)capacity_steps; e->depth.levels = (uint32_t)levels;
    return CDA_OK;
}
int cda_depth_disable(cda_env* e) {
    if (!e) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    depth_free(e);
    return CDA_OK;
}
int64_t cda_depth_capacity(const cda_env* e) { return e && e->depth.ring ? (int64_t)e->depth.cap : 0; }
int32_t cda_depth_levels(const cda_env* e) { return e && e->depth.ring ? (int32_t)e->depth.levels : 0; }

int cda_depth_check_host(int32_t kind, int32_t levels, const int32_t* lags_host, int32_t n_lags, int32_t a, int32_t b, const int32_t* depths_host, int32_t n_depths) {
    if (levels < 1 || levels > CDA_DEPTH_MAX_LEVELS) return CDA_ERR_INVALID;
    if (kind == CDA_DEPTH_PROFILE) return a >= 1 && a <= CDA_DEPTH_MAX_DIST ? CDA_OK : CDA_ERR_INVALID;
    if (kind == CDA_DEPTH_IMBALANCE) {
        if (cda_stylised_check_host(CDA_STYL_SIGNS, lags_host, n_lags, 1, 1, 1) != CDA_OK) return CDA_ERR_INVALID;      // (the lags' bounds: 1 .. CDA_STYL_MAX_LAG)
        return a >= 1 && a <= levels && b >= 1 && b <= CDA_STYL_MAX_HIST_HALF ? CDA_OK : CDA_ERR_INVALID;
    }
    if (kind != CDA_DEPTH_OFI) return CDA_ERR_INVALID;
    if (cda_stylised_check_host(CDA_STYL_FLOW_RETURNS, lags_host, n_lags, a, 1, b) != CDA_OK) return CDA_ERR_INVALID;   // (lags >= 0, bar_steps, the bar points)
    if (!depths_host || n_depths < 1 || n_depths > CDA_DEPTH_MAX_DEPTHS) return CDA_ERR_INVALID;
    for (int32_t j = 0; j < n_depths; j++) if (depths_host[j] < 1 || depths_host[j] > levels) return CDA_ERR_INVALID;
    return CDA_OK;
}

int cda_depth_meta(cda_env* e, int32_t first_market, int32_t n_markets, int32_t* meta_out_dev, void* stream) {
    if (!reader_args_ok(e, meta_out_dev, first_market, n_markets) || !aligned(meta_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->depth.ring) return CDA_ERR_UNSUPPORTED;
    return reader_launch(e, k_depth_meta, n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, e->depth, (int)first_market, (int)n_markets, meta_out_dev);
}
int cda_depth_series(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, int32_t k, void* records_out_dev, int32_t* counts_out_dev, int32_t* info_out_dev,
                     void* stream) {
    if (!reader_args_ok(e, records_out_dev, first_market, n_markets) || k < 1 || !which_ok(which) || !aligned(records_out_dev, 16) || !aligned(counts_out_dev, 4) ||
        !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->depth.ring) return CDA_ERR_UNSUPPORTED;
    return reader_launch(e, k_depth_series, n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, e->depth, (int)first_market, (int)n_markets, (int)which, (int)k,
                         (uint4*)records_out_dev, counts_out_dev, info_out_dev);
}
int cda_depth_profile(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, int32_t max_dist, int64_t* base_out_dev, int64_t* levels_out_dev,
                      int64_t* shape_out_dev, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, base_out_dev, first_market, n_markets) || !levels_out_dev || !shape_out_dev || !which_ok(which) || !aligned(base_out_dev, 8) ||
        !aligned(levels_out_dev, 8) || !aligned(shape_out_dev, 8) || !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    // (depth off: the bounds are still vetted first, against the largest `levels` the service could have)
    if (cda_depth_check_host(CDA_DEPTH_PROFILE, e->depth.ring ? (int32_t)e->depth.levels : CDA_DEPTH_MAX_LEVELS, NULL, 0, max_dist, 0, NULL, 0) != CDA_OK) return CDA_ERR_INVALID;
    if (!e->depth.ring) return CDA_ERR_UNSUPPORTED;
    const size_t lds = (size_t)CDA_WPB * ((size_t)DP_WORDS + 2 * (size_t)e->depth.levels * DP_LEVEL_WORDS + 2 * ((size_t)max_dist + 1)) * sizeof(unsigned long long);      // <= 4 x 618 x 8 B
    return reader_launch(e, k_depth_profile, n_markets, CDA_WPB, lds, stream, (const uint8_t*)e->arena, e->P, e->depth, (int)first_market, (int)n_markets, (int)which,
                         (int)max_dist, (long long*)base_out_dev, (long long*)levels_out_dev, (long long*)shape_out_dev, info_out_dev);
}
int cda_depth_imbalance(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* lags_host, int32_t n_lags, int32_t k, int32_t half,
                        int64_t* resp_out_dev, int64_t* base_out_dev, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, resp_out_dev, first_market, n_markets) || !base_out_dev || !which_ok(which) || !aligned(resp_out_dev, 8) || !aligned(base_out_dev, 8) ||
        !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (cda_depth_check_host(CDA_DEPTH_IMBALANCE, e->depth.ring ? (int32_t)e->depth.levels : CDA_DEPTH_MAX_LEVELS, lags_host, n_lags, k, half, NULL, 0) != CDA_OK) return CDA_ERR_INVALID;
    if (!e->depth.ring) return CDA_ERR_UNSUPPORTED;
    const StylLags lg = styl_lags(lags_host, n_lags);
    const size_t per_wave = (size_t)n_lags * 2 * (size_t)half * DI_RESP_WORDS * sizeof(unsigned long long);      // <= 8 x 128 x 5 x 8 B = 40 KiB
    const int waves = styl_waves(per_wave);
    return reader_launch(e, k_depth_imbalance, n_markets, waves, per_wave * (size_t)waves, stream, (const uint8_t*)e->arena, e->P, e->depth, (int)first_market, (int)n_markets,
                         (int)which, (int)n_lags, lg, (int)k, (int)half, (long long*)resp_out_dev, (long long*)base_out_dev, info_out_dev);
}
int cda_depth_ofi(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* lags_host, int32_t n_lags, int32_t bar_steps, const int32_t* depths_host,
                  int32_t n_depths, int64_t* lagged_out_dev, int64_t* base_out_dev, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, lagged_out_dev, first_market, n_markets) || !base_out_dev || !which_ok(which) || !aligned(lagged_out_dev, 8) || !aligned(base_out_dev, 8) ||
        !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    const int32_t top = styl_range_top(e, first_market, n_markets);
    if (cda_depth_check_host(CDA_DEPTH_OFI, e->depth.ring ? (int32_t)e->depth.levels : CDA_DEPTH_MAX_LEVELS, lags_host, n_lags, bar_steps, top, depths_host, n_depths) != CDA_OK)
        return CDA_ERR_INVALID;
    if (!e->depth.ring) return CDA_ERR_UNSUPPORTED;
    const StylLags lg = styl_lags(lags_host, n_lags);
    DepthDepths dp;
    memset(&dp, 0, sizeof dp);
    for (int32_t j = 0; j < n_depths; j++) dp.k[j] = depths_host[j];
    const int64_t pts = ((int64_t)top + (int64_t)bar_steps - 1) / (int64_t)bar_steps;      // <= CDA_STYL_MAX_BARS
    const size_t per_wave = (size_t)n_depths * (size_t)pts * sizeof(int32_t);              // <= 4 x 4096 x 4 B = 64 KiB
    const int waves = styl_waves(per_wave);
    return reader_launch(e, k_depth_ofi, n_markets, waves, per_wave * (size_t)waves, stream, (const uint8_t*)e->arena, e->P, e->depth, (int)first_market, (int)n_markets,
                         (int)which, (int)bar_steps, (int)n_lags, lg, (int)n_depths, dp, (int)pts, (long long*)lagged_out_dev, (long long*)base_out_dev, info_out_dev);
}

}  // extern "C"
