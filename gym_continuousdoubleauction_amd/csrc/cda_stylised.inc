// cda_stylised.inc - the stylised-facts report (include/cda.h cda_quote_returns, cda_tape_signs, cda_tape_flow_returns): the time-series statistics of one
// remembered episode - return autocovariances and a return histogram from the quote tape, order-flow sign autocovariances from the trade tape, and signed volume
// joined to returns bar by bar from both.  Included behind cda_quotes.inc (quote_span, quote_slot, the quote accessors) and cda_tape.inc (tape_span, the tape
// accessors; wave_sum: cda_wave.hpp); stylised.py states every word in numpy.  All three kernels are READERS: one wave per market, exact integers, every output
// word additive, nothing atomic on global memory.
// k_quote_returns, k_tape_flow_returns.  A wave first STAGES the episode's bar points in its own slice of dynamic LDS: m2[p] of point p (step p * bar_steps), 0 =
// not two-sided (a two-sided m2 is at least 2) - one 16-byte load per point, the only pass over the quote ring, whatever the number of lags.  The joined kernel
// also walks the tape once, 64 fills per pass, and adds every fill's signed quantity to its bar's word Q[b] beside the points (LDS integer adds: their order cannot
// matter).  Then the products: 64 points per pass, lane l owns point p; r_p and, per lag, r_(p + lag) come from LDS.  Every lane keeps its own partial sums in
// registers over all passes; ONE int64 wave reduction per output word closes the kernel.  The slices are wave-private; the two workgroup barriers stand outside
// every loop (a wave without a market takes them too).
// LDS: per wave 4 x points (+ the histogram's bins) bytes, or 8 x points for the joined kernel, points = ceil(largest max_step of the range / bar_steps) <=
// CDA_STYL_MAX_BARS: a workgroup holds as many market-waves, up to CDA_WPB, as fit 64 KiB (styl_waves: the joined kernel runs four up to 2048 points, three up to
// 2730, two at 4096; k_quote_returns four up to about 4000 points, three at 4096).
//
// k_tape_signs.  No LDS: 64 fills per pass, the pass behind it already in registers, so that the partner fill i + lag of every lag <= 64 is a lane of one of the
// two (__shfl); only a longer lag reads its partner's two words at their ring slot (the lines the coming passes read anyway).  Runs and steps with fills look at
// the left neighbour (__shfl_up; lane 0's is the carry of the pass before).

static_assert(CDA_STYL_MAX_LAGS == 8 && CDA_STYL_MAX_BARS == 4096 && CDA_STYL_MAX_HIST_HALF == 64 && CDA_STYL_MAX_LAG == CDA_TAPE_CAP_MAX, "stylised-facts bounds");
enum { RT_BARS = 0, RT_RETURNS, RT_MISSING, RT_SUM_R, RT_SUM_ABS, RT_SUM_R2, RT_UP, RT_DOWN, RT_WORDS, RT_LAG_WORDS = 4 };
enum { SG_FILLS = 0, SG_BUYS, SG_SELLS, SG_BUY_QTY, SG_SELL_QTY, SG_SELF, SG_RUNS, SG_STEPS, SG_WORDS, SG_LAG_WORDS = 4 };
enum { FR_FILLS = 0, FR_BARS_WITH_FILLS, FR_BARS_EXCLUDED, FR_QTY, FR_WORDS, FR_LAG_WORDS = 6 };
constexpr size_t STYL_LDS_BYTES = 64 * 1024;                         // what a workgroup may take without asking for more

struct StylLags { int32_t k[CDA_STYL_MAX_LAGS]; };
// the bar points an episode's held quotes cover: lo .. hi (hi < lo: none), point p = step p * bar; never beyond the LDS slice
struct StylPoints { int lo, hi; };
__device__ __forceinline__ StylPoints styl_points(const QuoteSpan& sp, int bar, int cap_pts) {
    StylPoints pt;
    pt.lo = (int)(((long long)sp.step0 + (long long)bar - 1) / (long long)bar);
    pt.hi = sp.count > 0 ? (sp.step0 + sp.count - 1) / bar : pt.lo - 1;
    if (pt.hi >= cap_pts) pt.hi = cap_pts - 1;
    return pt;
}
// m2[p] <- bid + ask of point p's record, 0 where it is not two-sided, for the held points (p * bar <= the last held step: no overflow)
__device__ __forceinline__ void styl_stage(int32_t* m2, const uint4* qring, const QuoteSpan& sp, uint32_t cap, int bar, StylPoints pt, int lane) {
    for (int p = pt.lo + lane; p <= pt.hi; p += WAVE) {
        const uint4 r0 = qring[2 * (size_t)quote_slot(sp, cap, p * bar - sp.step0)];
        m2[p] = quote_two_sided(r0) ? quote_m2_i32(r0) : 0;
    }
}
// r_p = m2[p + 1] - m2[p]; defined iff both points are held and two-sided
__device__ __forceinline__ bool styl_return(const int32_t* m2, StylPoints pt, int p, long long& r) {
    r = 0;
    if (p < pt.lo || p >= pt.hi) return false;
    const int32_t a = m2[p], b = m2[p + 1];
    if (a == 0 || b == 0) return false;
    r = (long long)b - (long long)a;
    return true;
}
__device__ __forceinline__ long long styl_abs(long long v) { return v < 0 ? -v : v; }

__global__ __launch_bounds__(64 * CDA_WPB) void k_quote_returns(const uint8_t* arena, Params P, QuoteArgs Q, int first, int n, int which, int bar, int nl, StylLags lg,
                                                                int hh, int cap_pts, long long* base_out, long long* lag_out, long long* hist_out, int32_t* info) {
    extern __shared__ __align__(16) int32_t styl_lds[];               // per wave: cap_pts points, 2 hh + 1 bins
    READER_WAVE_IN_GROUP((int)(blockDim.x >> 6));
    const bool live = w < n;
    const int nb = 2 * hh + 1;
    int32_t* m2 = styl_lds + (size_t)wib * (size_t)(cap_pts + nb);
    int32_t* bins = m2 + cap_pts;
    for (int i = lane; i < nb; i += WAVE) bins[i] = 0;
    QuoteSpan sp = {0, 0, 0, 0, 0, 0u};
    StylPoints pt = {0, -1};
    if (live) {
        sp = quote_span(quote_meta_now(Q, arena, P, first + w, lane), Q.cap, which);
        pt = styl_points(sp, bar, cap_pts);
        styl_stage(m2, Q.ring + 2 * (size_t)(first + w) * (size_t)Q.cap, sp, Q.cap, bar, pt, lane);
    }
    __syncthreads();
    int c_ret = 0, c_miss = 0, c_up = 0, c_down = 0;                  // this lane's share of every sum
    long long s_r = 0, s_abs = 0, s_r2 = 0;
    long long acc[CDA_STYL_MAX_LAGS][RT_LAG_WORDS] = {};
    if (live) {
        const int t = mrow(P, first + w).tick_size;
        const long long tick = t < 1 ? 1ll : (long long)t;
        for (int p0 = pt.lo; p0 < pt.hi; p0 += WAVE) {                // (the last point has no return)
            const int p = p0 + lane;
            long long r;
            const bool ok = styl_return(m2, pt, p, r);
            const long long a = styl_abs(r);
            c_ret += ok ? 1 : 0; c_miss += p < pt.hi && !ok ? 1 : 0; c_up += r > 0 ? 1 : 0; c_down += r < 0 ? 1 : 0;
            s_r += r; s_abs += a; s_r2 += r * r;
            if (ok) {
                long long b = r / tick;
                b = b < -(long long)hh ? -(long long)hh : b > (long long)hh ? (long long)hh : b;
                atomicAdd(bins + ((int)b + hh), 1);
            }
#pragma unroll
            for (int h = 0; h < CDA_STYL_MAX_LAGS; h++) {
                if (h >= nl) break;
                long long r2;
                if (!styl_return(m2, pt, p + lg.k[h], r2) || !ok) continue;
                const long long a2 = styl_abs(r2);
                acc[h][0] += 1; acc[h][1] += r * r2; acc[h][2] += a * a2; acc[h][3] += r * a2;
            }
        }
    }
    __syncthreads();
    if (!live) return;
    const long long held = pt.hi >= pt.lo ? (long long)(pt.hi - pt.lo + 1) : 0ll;
    const long long t_ret = wave_sum((long long)c_ret), t_miss = wave_sum((long long)c_miss), t_up = wave_sum((long long)c_up),
                    t_down = wave_sum((long long)c_down), t_r = wave_sum(s_r), t_abs = wave_sum(s_abs), t_r2 = wave_sum(s_r2);
    if (lane < RT_WORDS) {
        const long long v = lane == RT_BARS ? held : lane == RT_RETURNS ? t_ret : lane == RT_MISSING ? t_miss : lane == RT_SUM_R ? t_r : lane == RT_SUM_ABS ? t_abs :
                            lane == RT_SUM_R2 ? t_r2 : lane == RT_UP ? t_up : t_down;
        base_out[(size_t)w * RT_WORDS + lane] = v;
    }
    long long v = 0;
#pragma unroll
    for (int h = 0; h < CDA_STYL_MAX_LAGS; h++) {
        if (h >= nl) break;
#pragma unroll
        for (int j = 0; j < RT_LAG_WORDS; j++) { const long long s = wave_sum(acc[h][j]); if (lane == h * RT_LAG_WORDS + j) v = s; }
    }
    if (lane < nl * RT_LAG_WORDS) lag_out[(size_t)w * (size_t)(nl * RT_LAG_WORDS) + lane] = v;
    for (int i = lane; i < nb; i += WAVE) hist_out[(size_t)w * (size_t)nb + i] = (long long)bins[i];
    if (info && lane == 0) reader_info(info, w, sp.count, sp.lost, sp.step0, sp.partial);
}

// what a partner needs of a fill: its quantity and its sides_step word (bit 1: the initiator's side, bits 2..: the step); self = counter_id == init_id
struct SignFill { int32_t q; uint32_t w; int32_t self; };
__device__ __forceinline__ SignFill sign_fill(const uint4* ring, uint32_t mask, uint32_t s0, long long idx, long long count) {
    SignFill x = {0, 0u, 0};
    if (idx < count) {
        const uint32_t slot = (s0 + (uint32_t)idx) & mask;
        const uint4 r0 = ring[2 * (size_t)slot], r1 = ring[2 * (size_t)slot + 1];
        x.q = tape_qty(r0); x.w = r1.w; x.self = tape_self(r0, r1) ? 1 : 0;
    }
    return x;
}
__global__ __launch_bounds__(64 * CDA_WPB) void k_tape_signs(TapeArgs T, int first, int n, int which, int nl, StylLags lg, long long* base_out, long long* lag_out,
                                                             int32_t* info) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w;
    const TapeSpan sp = tape_span(T.meta[mi], T.cap, which);
    const uint4* ring = T.ring + (size_t)mi * (size_t)T.cap * 2;
    const uint32_t mask = T.cap - 1u, s0 = (uint32_t)sp.start & mask;
    int c_buys = 0, c_sells = 0, c_self = 0, c_runs = 0, c_steps = 0;
    long long s_bq = 0, s_sq = 0;
    long long acc[CDA_STYL_MAX_LAGS][SG_LAG_WORDS] = {};
    int k_sign = 0;                                                   // the carry: sign and step of the last fill of the pass before (0: there is none)
    uint32_t k_step = 0u;
    SignFill cur = sign_fill(ring, mask, s0, (long long)lane, sp.count);
    for (long long base = 0; base < sp.count; base += WAVE) {
        const SignFill nxt = sign_fill(ring, mask, s0, base + WAVE + lane, sp.count);
        const long long idx = base + lane;
        const bool in = idx < sp.count;
        const int s = tape_init_sells(cur.w) ? -1 : 1;
        const uint32_t step = tape_stepw(cur.w);
        const long long sq = (long long)s * (long long)cur.q;
        int p_sign = __shfl_up(s, 1);
        uint32_t p_step = __shfl_up(step, 1);
        if (lane == 0) { p_sign = k_sign; p_step = k_step; }
        c_buys += in && s > 0 ? 1 : 0; c_sells += in && s < 0 ? 1 : 0; c_self += in ? cur.self : 0;
        s_bq += in && s > 0 ? (long long)cur.q : 0ll; s_sq += in && s < 0 ? (long long)cur.q : 0ll;
        c_runs += in && p_sign != s ? 1 : 0; c_steps += in && (p_sign == 0 || p_step != step) ? 1 : 0;
#pragma unroll
        for (int h = 0; h < CDA_STYL_MAX_LAGS; h++) {
            if (h >= nl) break;
            const int l = lg.k[h];                                    // (uniform)
            int32_t pq = 0;
            uint32_t pw = 0u;
            const bool pair = idx + (long long)l < sp.count;
            if (l <= WAVE) {                                          // the partner is a lane of this pass or of the next one
                const int src = lane + l;
                const int32_t qa = __shfl(cur.q, src & 63), qb = __shfl(nxt.q, src & 63);
                const uint32_t wa = __shfl(cur.w, src & 63), wb = __shfl(nxt.w, src & 63);
                pq = src < WAVE ? qa : qb; pw = src < WAVE ? wa : wb;
            } else if (pair) {
                const uint32_t slot = (s0 + (uint32_t)(idx + (long long)l)) & mask;
                pq = tape_qty(ring[2 * (size_t)slot]); pw = ring[2 * (size_t)slot + 1].w;
            }
            if (!pair) continue;
            const int ps = tape_init_sells(pw) ? -1 : 1;
            acc[h][0] += 1; acc[h][1] += (long long)(s * ps); acc[h][2] += sq * ((long long)ps * (long long)pq); acc[h][3] += tape_stepw(pw) == step ? 1 : 0;
        }
        k_sign = __shfl(s, 63); k_step = __shfl(step, 63);
        cur = nxt;
    }
    const long long t_buys = wave_sum((long long)c_buys), t_sells = wave_sum((long long)c_sells), t_self = wave_sum((long long)c_self),
                    t_runs = wave_sum((long long)c_runs), t_steps = wave_sum((long long)c_steps), t_bq = wave_sum(s_bq), t_sq = wave_sum(s_sq);
    if (lane < SG_WORDS) {
        const long long v = lane == SG_FILLS ? sp.count : lane == SG_BUYS ? t_buys : lane == SG_SELLS ? t_sells : lane == SG_BUY_QTY ? t_bq : lane == SG_SELL_QTY ? t_sq :
                            lane == SG_SELF ? t_self : lane == SG_RUNS ? t_runs : t_steps;
        base_out[(size_t)w * SG_WORDS + lane] = v;
    }
    long long v = 0;
#pragma unroll
    for (int h = 0; h < CDA_STYL_MAX_LAGS; h++) {
        if (h >= nl) break;
#pragma unroll
        for (int j = 0; j < SG_LAG_WORDS; j++) { const long long s = wave_sum(acc[h][j]); if (lane == h * SG_LAG_WORDS + j) v = s; }
    }
    if (lane < nl * SG_LAG_WORDS) lag_out[(size_t)w * (size_t)(nl * SG_LAG_WORDS) + lane] = v;
    if (info && lane == 0) reader_info(info, w, (int32_t)sp.count, (int32_t)sp.lost, 0, (int32_t)sp.partial);
}

__global__ __launch_bounds__(64 * CDA_WPB) void k_tape_flow_returns(const uint8_t* arena, Params P, TapeArgs T, QuoteArgs Q, int first, int n, int which, int bar, int nl,
                                                                    StylLags lg, int cap_pts, long long* lag_out, long long* base_out, int32_t* info) {
    extern __shared__ __align__(16) int32_t styl_flow_lds[];          // per wave: cap_pts points, cap_pts bars
    READER_WAVE_IN_GROUP((int)(blockDim.x >> 6));
    const bool live = w < n;
    int32_t* m2 = styl_flow_lds + (size_t)wib * (size_t)(2 * cap_pts);
    int32_t* qbar = m2 + cap_pts;
    for (int i = lane; i < cap_pts; i += WAVE) qbar[i] = 0;
    TapeSpan ts = {0, 0, 0, 0};
    QuoteSpan qs = {0, 0, 0, 0, 0, 0u};
    StylPoints pt = {0, -1};
    const uint4* tring = T.ring + (size_t)(live ? first + w : first) * (size_t)T.cap * 2;
    const uint32_t tmask = T.cap - 1u;
    if (live) {
        ts = tape_span(T.meta[first + w], T.cap, which);
        qs = quote_span(quote_meta_now(Q, arena, P, first + w, lane), Q.cap, which);
        pt = styl_points(qs, bar, cap_pts);
        styl_stage(m2, Q.ring + 2 * (size_t)(first + w) * (size_t)Q.cap, qs, Q.cap, bar, pt, lane);
    }
    __syncthreads();
    const uint32_t t0 = (uint32_t)ts.start & tmask;
    long long b_first = 0;                                            // the first kept bar: behind the first held fill's where the ring has lost the episode's head
    int c_fills = 0, c_bars = 0;
    long long s_qty = 0;
    if (live) {
        if (ts.lost > 0) {
            if (ts.count > 0) b_first = (long long)(tape_step(tring[2 * (size_t)t0 + 1]) / (uint32_t)bar) + 1;
            else b_first = qs.count > 0 ? (long long)((qs.step0 + qs.count - 1) / bar) + 1 : 0ll;
        }
        uint32_t k_bar = 0xffffffffu;                                 // the carry: the bar of the last fill of the pass before (no bar has this index)
        for (long long base = 0; base < ts.count; base += WAVE) {
            const bool in = base + lane < ts.count;
            uint4 r0, r1;
            tape_load(tring, tmask, t0, base + lane, in, r0, r1);
            const uint32_t b = tape_step(r1) / (uint32_t)bar;
            const int32_t qty = tape_qty(r0);
            if (in && b < (uint32_t)cap_pts) atomicAdd(qbar + b, tape_init_sells(r1.w) ? -qty : qty);
            uint32_t p_bar = __shfl_up(b, 1);
            if (lane == 0) p_bar = k_bar;
            const bool kept = in && (long long)b >= b_first;
            c_fills += kept ? 1 : 0; c_bars += kept && p_bar != b ? 1 : 0; s_qty += kept ? (long long)qty : 0ll;
            k_bar = __shfl(b, 63);
        }
    }
    __syncthreads();
    if (!live) return;
    long long acc[CDA_STYL_MAX_LAGS][FR_LAG_WORDS] = {};
    for (long long b0 = b_first; b0 < (long long)pt.hi; b0 += WAVE) { // (bar b <= hi - 1 < cap_pts: r_(b + lag) needs the point behind it)
        const long long bl = b0 + lane;
        const int b = bl < (long long)pt.hi ? (int)bl : pt.hi;        // (a lane beyond the last bar: r_(hi + lag) is never defined)
        const long long q = (long long)qbar[b];                       // (b <= hi < cap_pts: styl_points)
#pragma unroll
        for (int h = 0; h < CDA_STYL_MAX_LAGS; h++) {
            if (h >= nl) break;
            long long r;
            if (!styl_return(m2, pt, b + lg.k[h], r)) continue;
            acc[h][0] += 1; acc[h][1] += q; acc[h][2] += r; acc[h][3] += q * r; acc[h][4] += q * q; acc[h][5] += r * r;
        }
    }
    const long long t_fills = wave_sum((long long)c_fills), t_bars = wave_sum((long long)c_bars), t_qty = wave_sum(s_qty);
    if (lane < FR_WORDS) base_out[(size_t)w * FR_WORDS + lane] = lane == FR_FILLS ? t_fills : lane == FR_BARS_WITH_FILLS ? t_bars : lane == FR_BARS_EXCLUDED ? b_first : t_qty;
    long long v = 0;
#pragma unroll
    for (int h = 0; h < CDA_STYL_MAX_LAGS; h++) {
        if (h >= nl) break;
#pragma unroll
        for (int j = 0; j < FR_LAG_WORDS; j++) { const long long s = wave_sum(acc[h][j]); if (lane == h * FR_LAG_WORDS + j) v = s; }
    }
    if (lane < nl * FR_LAG_WORDS) lag_out[(size_t)w * (size_t)(nl * FR_LAG_WORDS) + lane] = v;
    if (info && lane == 0) reader_info(info, w, (int32_t)ts.count, (int32_t)ts.lost, (int32_t)qs.lost, (int32_t)(ts.partial | (qs.partial << 1)));
}

// the longest episode of the range: its rows' largest max_step
static int32_t styl_range_top(const cda_env* e, int32_t first, int32_t n) {
    int32_t top = 1;
    for (int32_t i = 0; i < n; i++) if (e->rows_host[first + i].max_step > top) top = e->rows_host[first + i].max_step;
    return top;
}
// market-waves per workgroup: CDA_WPB, or as many as fit the LDS a workgroup may take (at least one: bytes_per_wave <= 8 x CDA_STYL_MAX_BARS)
static int styl_waves(size_t bytes_per_wave) {
    const size_t fit = STYL_LDS_BYTES / bytes_per_wave;
    return fit >= CDA_WPB ? CDA_WPB : fit < 1 ? 1 : (int)fit;
}
static StylLags styl_lags(const int32_t* lags_host, int32_t n_lags) {
    StylLags lg;
    memset(&lg, 0, sizeof lg);
    for (int32_t h = 0; h < n_lags; h++) lg.k[h] = lags_host[h];
    return lg;
}

extern "C" {

int cda_stylised_check_host(int32_t kind, const int32_t* lags_host, int32_t n_lags, int32_t bar_steps, int32_t hist_half, int32_t max_step) {
    if (kind != CDA_STYL_RETURNS && kind != CDA_STYL_SIGNS && kind != CDA_STYL_FLOW_RETURNS) return CDA_ERR_INVALID;
    if (!lags_host || n_lags < 1 || n_lags > CDA_STYL_MAX_LAGS) return CDA_ERR_INVALID;
    for (int32_t h = 0; h < n_lags; h++)
        if (lags_host[h] < (kind == CDA_STYL_FLOW_RETURNS ? 0 : 1) || lags_host[h] > CDA_STYL_MAX_LAG) return CDA_ERR_INVALID;
    if (kind == CDA_STYL_SIGNS) return CDA_OK;
    if (bar_steps < 1 || max_step < 1 || ((int64_t)max_step + (int64_t)bar_steps - 1) / (int64_t)bar_steps > CDA_STYL_MAX_BARS) return CDA_ERR_INVALID;
    if (kind == CDA_STYL_RETURNS && (hist_half < 1 || hist_half > CDA_STYL_MAX_HIST_HALF)) return CDA_ERR_INVALID;
    return CDA_OK;
}

int cda_quote_returns(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* lags_host, int32_t n_lags, int32_t bar_steps, int32_t hist_half,
                      int64_t* base_out_dev, int64_t* lagged_out_dev, int64_t* hist_out_dev, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, base_out_dev, first_market, n_markets) || !lagged_out_dev || !hist_out_dev || !which_ok(which) || !aligned(base_out_dev, 8) ||
        !aligned(lagged_out_dev, 8) || !aligned(hist_out_dev, 8) || !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    const int32_t top = styl_range_top(e, first_market, n_markets);
    if (cda_stylised_check_host(CDA_STYL_RETURNS, lags_host, n_lags, bar_steps, hist_half, top) != CDA_OK) return CDA_ERR_INVALID;
    if (!e->quotes.ring) return CDA_ERR_UNSUPPORTED;
    const StylLags lg = styl_lags(lags_host, n_lags);
    const int64_t pts = ((int64_t)top + (int64_t)bar_steps - 1) / (int64_t)bar_steps;      // <= CDA_STYL_MAX_BARS
    const size_t per_wave = ((size_t)pts + 2 * (size_t)hist_half + 1) * sizeof(int32_t);
    const int waves = styl_waves(per_wave);
    return reader_launch(e, k_quote_returns, n_markets, waves, per_wave * (size_t)waves, stream, (const uint8_t*)e->arena, e->P, e->quotes, (int)first_market, (int)n_markets,
                         (int)which, (int)bar_steps, (int)n_lags, lg, (int)hist_half, (int)pts, (long long*)base_out_dev, (long long*)lagged_out_dev, (long long*)hist_out_dev,
                         info_out_dev);
}

int cda_tape_signs(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* lags_host, int32_t n_lags, int64_t* base_out_dev,
                   int64_t* lagged_out_dev, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, base_out_dev, first_market, n_markets) || !lagged_out_dev || !which_ok(which) || !aligned(base_out_dev, 8) || !aligned(lagged_out_dev, 8) ||
        !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (cda_stylised_check_host(CDA_STYL_SIGNS, lags_host, n_lags, 1, 1, 1) != CDA_OK) return CDA_ERR_INVALID;
    if (!e->tape.ring) return CDA_ERR_UNSUPPORTED;
    const StylLags lg = styl_lags(lags_host, n_lags);
    return reader_launch(e, k_tape_signs, n_markets, CDA_WPB, 0, stream, e->tape, (int)first_market, (int)n_markets, (int)which, (int)n_lags, lg, (long long*)base_out_dev,
                         (long long*)lagged_out_dev, info_out_dev);
}

int cda_tape_flow_returns(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* lags_host, int32_t n_lags, int32_t bar_steps,
                          int64_t* lagged_out_dev, int64_t* base_out_dev, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, base_out_dev, first_market, n_markets) || !lagged_out_dev || !which_ok(which) || !aligned(base_out_dev, 8) || !aligned(lagged_out_dev, 8) ||
        !aligned(info_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    const int32_t top = styl_range_top(e, first_market, n_markets);
    if (cda_stylised_check_host(CDA_STYL_FLOW_RETURNS, lags_host, n_lags, bar_steps, 1, top) != CDA_OK) return CDA_ERR_INVALID;
    if (!e->tape.ring || !e->quotes.ring) return CDA_ERR_UNSUPPORTED;
    const StylLags lg = styl_lags(lags_host, n_lags);
    const int64_t pts = ((int64_t)top + (int64_t)bar_steps - 1) / (int64_t)bar_steps;      // <= CDA_STYL_MAX_BARS
    const size_t per_wave = 2 * (size_t)pts * sizeof(int32_t);
    const int waves = styl_waves(per_wave);
    return reader_launch(e, k_tape_flow_returns, n_markets, waves, per_wave * (size_t)waves, stream, (const uint8_t*)e->arena, e->P, e->tape, e->quotes, (int)first_market,
                         (int)n_markets, (int)which, (int)bar_steps, (int)n_lags, lg, (int)pts, (long long*)lagged_out_dev, (long long*)base_out_dev, info_out_dev);
}

}  // extern "C"
