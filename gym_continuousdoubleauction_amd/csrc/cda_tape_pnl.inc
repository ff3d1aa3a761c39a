// cda_tape_pnl.inc - the P&L report (include/cda.h cda_tape_pnl): per market and agent the mark-to-mid equity curve of one remembered episode - the trade tape
// joined to the quote tape on the bar points - and what a person reads off it: drawdown, the moments of the per-bar P&L, the time under water and the split of
// the P&L into what the carried inventory gained on the mid's moves and what the trades themselves earned against each bar's closing mid.  Included behind
// cda_stylised.inc (styl_points, styl_stage, styl_waves, styl_range_top, STYL_LDS_BYTES; the scans and reductions: cda_wave.hpp); pnl.py states every word in
// numpy.  A READER: one wave per market, exact integers, nothing atomic on global memory, every requested output word written exactly once by plain vector stores.
//
// The wave's slice of dynamic LDS holds, per bar point (at most CDA_STYL_MAX_BARS): cash[b] (int64), mark[p] (int32), qty[b] (int32) - 16 bytes a point, so a
// workgroup runs four market-waves up to 1024 points, two up to 2048 and one at 4096 (styl_waves).  That leaves room for ONE agent's per-bar words: the agent
// loop is the outer loop, and the tape is walked once per agent.
//   marks    staged as k_tape_flow_returns stages m2, then carried forward IN PLACE, 64 points per pass: the index of the last two-sided point at or before p is
//            a prefix max over the wave (__shfl_up, six steps) on top of the carry of the passes before; mark[p] <- m2[that index].  A two-sided point keeps its
//            own word, so the pass may read what an earlier lane has just rewritten.  Held points are consecutive, so the marked points are first_two .. hi.
//   agent a  the held tape, 64 fills per pass: each of the agent's non-self fills adds sq to qty[bar] and -sq x price to cash[bar] (LDS integer adds: their order
//            cannot matter).  Then the points from 0 on, 64 per pass, lane l owns point p: pos(p) and C(p) are prefix sums of the bars below p (wave scan + carry),
//            E(p) = 2 C + pos x mark, the running maximum a prefix max + carry; the increment that ENDS at p takes E, pos and mark of p - 1 from the lane below
//            (lane 0: from the carry).  Lanes keep partial sums in registers over all passes; one wave reduction per word closes the agent.
// The slices are wave-private, but the phases hand words from lane to lane, so three workgroup barriers per agent separate them; `agents` is uniform and a wave
// without a market takes them too.

static_assert(CDA_PNL_WORDS == 16, "cda_tape_pnl layout");
enum { PN_POINTS = 0, PN_STALE, PN_UNMARKED, PN_BARS, PN_EQUITY_FIRST, PN_EQUITY_LAST, PN_INVENTORY, PN_TRADING, PN_SUM_D2, PN_UP, PN_DOWN, PN_UNDER_WATER,
       PN_MAX_DRAWDOWN, PN_EQUITY_MAX, PN_EQUITY_MIN, PN_OPEN_FILLS };
constexpr size_t PNL_POINT_BYTES = sizeof(long long) + 2 * sizeof(int32_t);
constexpr long long PNL_LOWEST = -0x7fffffffffffffffll - 1, PNL_HIGHEST = 0x7fffffffffffffffll;

// Four waves per SIMD asked for: left alone, the max-ilp scheduler spreads the point pass over 270 registers - one wave per SIMD, where 1000 points' LDS lets a
// CU hold two workgroups; held to 128 the kernel takes 127, spills nothing and needs no scratch.
__global__ __launch_bounds__(64 * CDA_WPB, 4) void k_tape_pnl(const uint8_t* arena, Params P, TapeArgs T, QuoteArgs Q, int first, int n, int which, int bar, int agents,
                                                           int cap_pts, int n_points, long long* stats_out, long long* equity_out, int32_t* position_out,
                                                           int32_t* marks_out, int32_t* info) {
    extern __shared__ __align__(16) long long pnl_lds[];              // per wave: cap_pts cash words, then cap_pts marks, cap_pts bar quantities
    READER_WAVE_IN_GROUP((int)(blockDim.x >> 6));
    const bool live = w < n;
    long long* cash = pnl_lds + (size_t)wib * (size_t)(2 * cap_pts);  // (16 bytes a point = two 8-byte words)
    int32_t* mark = reinterpret_cast<int32_t*>(cash + cap_pts);
    int32_t* qty = mark + cap_pts;
    TapeSpan ts = {0, 0, 0, 0};
    QuoteSpan qs = {0, 0, 0, 0, 0, 0u};
    StylPoints pt = {0, -1};
    const uint4* tring = T.ring + (size_t)(live ? first + w : first) * (size_t)T.cap * 2;
    const uint32_t tmask = T.cap - 1u;
    if (live) {
        ts = tape_span(T.meta[first + w], T.cap, which);
        qs = quote_span(quote_meta_now(Q, arena, P, first + w, lane), Q.cap, which);
        pt = styl_points(qs, bar, cap_pts);
        styl_stage(mark, Q.ring + 2 * (size_t)(first + w) * (size_t)Q.cap, qs, Q.cap, bar, pt, lane);
    }
    __syncthreads();
    // ---- the marks: carried forward over the held points, in place
    int first_two = pt.hi + 1;                                        // the first marked point (hi + 1: none)
    int c_stale = 0;
    if (live) {
        int k_last = -1;                                              // the carry: the last two-sided point of the passes before
        for (int p0 = pt.lo; p0 <= pt.hi; p0 += WAVE) {
            const int p = p0 + lane;
            const bool valid = p <= pt.hi;
            const bool two = valid && mark[p] != 0;
            const unsigned long long m = __ballot(two);
            if (k_last < 0 && m != 0ull) first_two = p0 + __ffsll((long long)m) - 1;
            int last = wave_scan_max(two ? p : -1, lane);
            last = last > k_last ? last : k_last;
            const int32_t v = last >= 0 ? mark[last] : 0;             // (a two-sided point's word is never rewritten)
            c_stale += valid && last >= 0 && !two ? 1 : 0;
            if (valid) mark[p] = v;
            k_last = __shfl(last, 63);
        }
    }
    __syncthreads();
    const bool any = first_two <= pt.hi;
    const long long n_marked = any ? (long long)(pt.hi - first_two + 1) : 0ll;
    const long long n_held = pt.hi >= pt.lo ? (long long)(pt.hi - pt.lo + 1) : 0ll;
    const long long t_stale = wave_sum((long long)c_stale);
    if (live && marks_out)
        for (int p = lane; p < n_points; p += WAVE) marks_out[(size_t)w * (size_t)n_points + p] = p >= first_two && p <= pt.hi ? mark[p] : 0;
    const uint32_t t0 = (uint32_t)ts.start & tmask;
    int used = 0;
    for (int a = 0; a < agents; a++) {                                // (uniform: every wave of the workgroup takes the barriers)
        for (int i = lane; i < cap_pts; i += WAVE) { cash[i] = 0ll; qty[i] = 0; }
        __syncthreads();
        int c_open = 0;
        if (live) {
            for (long long base = 0; base < ts.count; base += WAVE) {
                const bool in = base + lane < ts.count;
                uint4 r0, r1;
                tape_load(tring, tmask, t0, base + lane, in, r0, r1);
                const uint32_t cid = tape_counter_id(r0), iid = tape_init_id(r1);
                const bool ok = in && cid < (uint32_t)agents && iid < (uint32_t)agents;      // (ids outside the env's agents: as k_tape_exec)
                if (a == 0) used += __popcll(__ballot(ok));
                const bool mine = ok && cid != iid && (cid == (uint32_t)a || iid == (uint32_t)a);
                const int side = iid == (uint32_t)a ? tape_init_side(r1) : tape_counter_side(r1);
                const long long sq = side ? -(long long)tape_qty(r0) : (long long)tape_qty(r0), price = (long long)tape_price(r0);
                const uint32_t b = tape_step(r1) / (uint32_t)bar;
                if (mine && b < (uint32_t)cap_pts) {
                    atomicAdd(qty + b, (int32_t)sq);
                    atomicAdd(reinterpret_cast<unsigned long long*>(cash + b), (unsigned long long)(-sq * price));
                }
                c_open += mine && (!any || (long long)b >= (long long)pt.hi) ? 1 : 0;
            }
        }
        __syncthreads();
        if (live) {
            const size_t row = (size_t)w * (size_t)agents + (size_t)a;
            long long k_pos = 0, k_cash = 0, k_max = PNL_LOWEST, k_eq = 0, k_mark = 0;      // the carries: of the last point of the passes before
            long long s_inv = 0, s_trd = 0, s_d2 = 0, s_first = 0, s_last = 0, m_dd = 0, m_top = PNL_LOWEST, m_low = PNL_HIGHEST;
            int c_up = 0, c_down = 0, c_under = 0;
            for (int p0 = 0; p0 <= pt.hi; p0 += WAVE) {
                const int p = p0 + lane;
                const bool valid = p <= pt.hi, held = valid && p >= pt.lo, marked = valid && p >= first_two;
                const long long dq = valid && p >= 1 ? (long long)qty[p - 1] : 0ll, dc = valid && p >= 1 ? cash[p - 1] : 0ll;      // bar p - 1 ends at point p
                const long long pos = k_pos + wave_scan_sum(dq, lane), c = k_cash + wave_scan_sum(dc, lane);
                const long long mk = marked ? (long long)mark[p] : 0ll;
                const long long eq = marked ? 2 * c + pos * mk : 0ll;
                long long top = wave_scan_max(marked ? eq : PNL_LOWEST, lane);
                top = top > k_max ? top : k_max;
                long long e_b = __shfl_up(eq, 1), pos_b = __shfl_up(pos, 1), mk_b = __shfl_up(mk, 1);
                if (lane == 0) { e_b = k_eq; pos_b = k_pos; mk_b = k_mark; }
                const bool inc = marked && p > first_two;             // the increment of bar p - 1: both of its points are marked
                const long long d = inc ? eq - e_b : 0ll, inv = inc ? pos_b * (mk - mk_b) : 0ll, trd = inc ? dq * mk + 2 * dc : 0ll;
                s_inv += inv; s_trd += trd; s_d2 += d * d;
                c_up += d > 0 ? 1 : 0; c_down += d < 0 ? 1 : 0;
                c_under += marked && eq < top ? 1 : 0;
                if (marked) { const long long dd = top - eq; m_dd = dd > m_dd ? dd : m_dd; m_top = eq > m_top ? eq : m_top; m_low = eq < m_low ? eq : m_low; }
                if (marked && p == first_two) s_first = eq;
                if (marked && p == pt.hi) s_last = eq;
                if (equity_out && valid) equity_out[row * (size_t)n_points + p] = eq;            // (hi < cap_pts <= n_points where a series is asked for)
                if (position_out && valid) position_out[row * (size_t)n_points + p] = held ? (int32_t)pos : 0;
                k_pos = __shfl(pos, 63); k_cash = __shfl(c, 63); k_max = __shfl(top, 63); k_eq = __shfl(eq, 63); k_mark = __shfl(mk, 63);
            }
            for (int p = pt.hi + 1 + lane; p < n_points; p += WAVE) {
                if (equity_out) equity_out[row * (size_t)n_points + p] = 0ll;
                if (position_out) position_out[row * (size_t)n_points + p] = 0;
            }
            const long long t_inv = wave_sum(s_inv), t_trd = wave_sum(s_trd), t_d2 = wave_sum(s_d2), t_first = wave_sum(s_first),
                            t_last = wave_sum(s_last), t_up = wave_sum((long long)c_up), t_down = wave_sum((long long)c_down),
                            t_under = wave_sum((long long)c_under), t_open = wave_sum((long long)c_open), t_dd = wave_max(m_dd),
                            t_top = wave_max(m_top), t_low = wave_min(m_low);
            if (lane < CDA_PNL_WORDS) {
                const long long v = lane == PN_POINTS ? n_marked : lane == PN_STALE ? t_stale : lane == PN_UNMARKED ? n_held - n_marked :
                                    lane == PN_BARS ? (n_marked > 0 ? n_marked - 1 : 0ll) : lane == PN_EQUITY_FIRST ? t_first : lane == PN_EQUITY_LAST ? t_last :
                                    lane == PN_INVENTORY ? t_inv : lane == PN_TRADING ? t_trd : lane == PN_SUM_D2 ? t_d2 : lane == PN_UP ? t_up : lane == PN_DOWN ? t_down :
                                    lane == PN_UNDER_WATER ? t_under : lane == PN_MAX_DRAWDOWN ? t_dd : lane == PN_EQUITY_MAX ? (any ? t_top : 0ll) :
                                    lane == PN_EQUITY_MIN ? (any ? t_low : 0ll) : t_open;
                stats_out[row * CDA_PNL_WORDS + lane] = v;
            }
        }
        __syncthreads();
    }
    if (live && info && lane == 0) reader_info(info, w, (int32_t)used, (int32_t)ts.lost, (int32_t)qs.lost, (int32_t)(ts.partial | (qs.partial << 1)));
}

extern "C" {

int cda_tape_pnl_check_host(int32_t bar_steps, int32_t n_points, int32_t want_series, int32_t max_step) {
    if (bar_steps < 1 || max_step < 1) return CDA_ERR_INVALID;
    const int64_t pts = ((int64_t)max_step + (int64_t)bar_steps - 1) / (int64_t)bar_steps;
    if (pts > CDA_STYL_MAX_BARS) return CDA_ERR_INVALID;
    if (want_series && (int64_t)n_points < pts) return CDA_ERR_INVALID;
    return CDA_OK;
}

int cda_tape_pnl(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, int32_t bar_steps, int64_t* stats_out_dev, int64_t* equity_out_dev,
                 int32_t* position_out_dev, int32_t* marks_out_dev, int32_t n_points, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, stats_out_dev, first_market, n_markets) || !which_ok(which) || !aligned(stats_out_dev, 8) || !aligned(equity_out_dev, 8) || !aligned(position_out_dev, 4) ||
        !aligned(marks_out_dev, 4) || !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    const int want = equity_out_dev || position_out_dev || marks_out_dev ? 1 : 0;
    const int32_t top = styl_range_top(e, first_market, n_markets);
    if (cda_tape_pnl_check_host(bar_steps, n_points, want, top) != CDA_OK) return CDA_ERR_INVALID;
    if (!agents_ok(e)) return CDA_ERR_INVALID;
    if (!e->tape.ring || !e->quotes.ring) return CDA_ERR_UNSUPPORTED;
    const int64_t pts = ((int64_t)top + (int64_t)bar_steps - 1) / (int64_t)bar_steps;      // <= CDA_STYL_MAX_BARS
    const size_t per_wave = (size_t)pts * PNL_POINT_BYTES;           // <= STYL_LDS_BYTES
    const int waves = styl_waves(per_wave);
    return reader_launch(e, k_tape_pnl, n_markets, waves, per_wave * (size_t)waves, stream, (const uint8_t*)e->arena, e->P, e->tape, e->quotes, (int)first_market, (int)n_markets,
                         (int)which, (int)bar_steps, (int)e->P.cfg.num_agents, (int)pts, (int)(want ? n_points : 0), (long long*)stats_out_dev, (long long*)equity_out_dev,
                         position_out_dev, marks_out_dev, info_out_dev);
}

}  // extern "C"
