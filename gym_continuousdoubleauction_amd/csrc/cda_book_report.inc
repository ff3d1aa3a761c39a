// cda_book_report.inc - reductions over the STANDING book of a market range (include/cda.h cda_book_counts .. cda_book_pack), included at the end of cda_hip.hip
// (the wave toolkit - READER_WAVE, wave_scan_sum, lanes_le, lds_add - is cda_wave.hpp, included ahead of every .inc).
//
// All kernels are READERS of the arena: nothing here writes a market record or a spill ring, and nothing touches the step kernels.  One wave per (market,
// side) - wave w of a launch serves side w & 1 of market first + (w >> 1), CDA_WPB waves per workgroup - walks the side in queue order (best price first, FIFO
// inside a level, the tile's orders and then the ring's: BookView::get's order), 64 consecutive orders per pass.  Lane l of a pass reads order base + l: in the
// tile that is a contiguous run of every field array (bids ascending from slot 0, asks descending from slot cap - 1), in the ring a contiguous run modulo
// spill_cap; the pass in which the side leaves the tile reads both.  What a pass hands to the next is a CARRY in uniform registers: the last price, the open
// level's volume and order count, the cumulative quantity and notional.  Level boundaries are price changes between neighbours (__shfl_up, __ballot) - the
// neighbour in the previous pass (the carry) and the tile-to-ring neighbour included.  Sums are 64-bit integers: the results are exact and do not depend on
// scheduling; the only atomics are 64-bit integer adds on the wave's own slice of LDS (k_book_agents), whose order cannot matter.
//
// A market whose header counts are inconsistent (check_invariants reports CDA_INV_BOOK_COUNT for it) reads as an empty book: no lane leaves the arrays.

struct BookSide {
    const int32_t* tile; const int32_t* ring; int cap, sd, tile_n, n; uint32_t ring_cap, base;
    // field f of order i of the side, i < n
    __device__ __forceinline__ int32_t get(int f, int i) const {
        if (i < tile_n) return tile[f * cap + book_phys_rt(cap, sd, i)];
        return ring[(size_t)f * (size_t)ring_cap + ((base + (uint32_t)(i - tile_n)) & (ring_cap - 1u))];
    }
};
__device__ __forceinline__ BookSide book_side(const uint8_t* arena, const Params& P, int cap, int mi, int sd) {
    const uint8_t* rec = arena + (size_t)mi * (size_t)P.lay.stride;
    const uint32_t* h = reinterpret_cast<const uint32_t*>(rec);
    BookSide b;
    b.tile = reinterpret_cast<const int32_t*>(rec + P.lay.book_off); b.ring = nullptr; b.cap = cap; b.sd = sd; b.ring_cap = (uint32_t)P.lay.spill_cap; b.base = 0u;
    const long long nb = (int32_t)h[H_N_BIDS], na = (int32_t)h[H_N_ASKS];
    const bool ok = nb >= 0 && na >= 0 && nb + na <= (long long)cap;
    b.tile_n = ok ? (int)(sd ? na : nb) : 0;
    int tail = 0;
    if (ok && P.lay.spill_cap > 0 && (h[H_STATUS] & (uint32_t)(ST_TAIL_BID << sd)) != 0) {
        const int32_t* sp = reinterpret_cast<const int32_t*>(arena + spill_arena_off(P) + (size_t)mi * spill_region_bytes(P.lay.spill_cap));
        const int32_t tn = sp[sd];
        if (tn > 0 && tn <= P.lay.spill_cap) { tail = tn; b.base = (uint32_t)sp[2 + sd]; b.ring = sp + 16 + (size_t)sd * BOOK_FIELDS * (size_t)P.lay.spill_cap; }
    }
    b.n = b.tile_n + tail;
    return b;
}

// resting orders and distinct price levels of every side: out i32 [n][2][2] = (orders, levels)
__global__ __launch_bounds__(64 * CDA_WPB) void k_book_counts(const uint8_t* arena, Params P, int cap, int first, int n, int32_t* out) {
    READER_WAVE();
    if (w >= 2 * n) return;
    const BookSide b = book_side(arena, P, cap, first + (w >> 1), w & 1);
    int levels = 0;
    int32_t prev = 0;
    for (int base = 0; base < b.n; base += WAVE) {
        const int i = base + lane;
        const bool valid = i < b.n;
        const int32_t p = valid ? b.get(0, i) : 0;
        const int32_t up = __shfl_up(p, 1);
        levels += __popcll(__ballot(valid && (lane == 0 ? (base == 0 || p != prev) : p != up)));
        prev = __shfl(p, 63);
    }
    if (lane == 0) { out[2 * (size_t)w] = b.n; out[2 * (size_t)w + 1] = levels; }
}

// the Level-2 ladder: out i64 [n][2][L][3] = (price, volume, orders) per level, best first; rows past the side's level count are zero.  Per pass a segmented
// inclusive scan of the quantities (six __shfl_up steps) leaves every level's volume in the level's last lane, which stores the row; the level that reaches the
// pass's last order is not stored but carried, and continued by the first run of the next pass when that has the same price.
__device__ __forceinline__ void level_store(long long* rows, int level, int32_t price, long long volume, int orders) {
    long long* r = rows + 3 * (size_t)level;
    r[0] = (long long)price; r[1] = volume; r[2] = (long long)orders;
}
__global__ __launch_bounds__(64 * CDA_WPB) void k_book_levels(const uint8_t* arena, Params P, int cap, int first, int n, int L, long long* out) {
    READER_WAVE();
    if (w >= 2 * n) return;
    const BookSide b = book_side(arena, P, cap, first + (w >> 1), w & 1);
    long long* rows = out + 3 * (size_t)w * (size_t)L;
    int lv = -1, ccnt = 0;                                           // the carried (open) level: its index, price, volume, orders
    int32_t cp = 0;
    long long cvol = 0;
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
        int cnt = lane - seg + 1;
        if (seg == 0 && (heads & 1ull) == 0ull) { vol += cvol; cnt += ccnt; }
        if ((heads & 1ull) != 0ull && lv >= 0 && lv < L && lane == 0) level_store(rows, lv, cp, cvol, ccnt);       // the carried level ended with the last pass
        const int lastv = 63 - __clzll((long long)__ballot(valid));
        const bool tail = valid && lane < lastv && ((heads >> ((lane + 1) & 63)) & 1ull) != 0ull;
        if (tail && level < L) level_store(rows, level, p, vol, cnt);
        lv = __shfl(level, lastv); cp = __shfl(p, lastv); cvol = __shfl(vol, lastv); ccnt = __shfl(cnt, lastv);
        if (lv >= L) break;                                          // rows 0 .. L - 1 are written; the open level lies behind them
    }
    if (lv >= 0 && lv < L && lane == 0) level_store(rows, lv, cp, cvol, ccnt);
    for (long long i = 3ll * ((long long)lv + 1) + lane; i < 3ll * (long long)L; i += WAVE) rows[i] = 0ll;
}

// what a market order of Q_k units pays that consumes the side by price-time priority: out i64 [n][2][K][3] = (filled, notional, last_price).  The sizes come
// by value; lane k keeps the answer for size k.  Per pass an inclusive prefix sum of quantity and of price x quantity; size k is answered in the pass whose
// cumulative quantity reaches it, by the first lane that does (its order is consumed partially).
struct BookSizes { long long q[CDA_BOOK_MAX_SIZES]; };
__global__ __launch_bounds__(64 * CDA_WPB) void k_book_impact(const uint8_t* arena, Params P, int cap, int first, int n, BookSizes S, int K, long long* out) {
    READER_WAVE();
    if (w >= 2 * n) return;
    const BookSide b = book_side(arena, P, cap, first + (w >> 1), w & 1);
    const uint32_t all = (1u << K) - 1u;
    uint32_t done = 0u;                                              // (uniform) sizes answered so far
    long long cq = 0, cn = 0, rf = 0, rn = 0;
    int32_t lastp = 0, rp = 0;
    for (int base = 0; base < b.n; base += WAVE) {
        const int i = base + lane;
        const bool valid = i < b.n;
        int32_t p = 0, q = 0;
        if (valid) { p = b.get(0, i); q = b.get(1, i); }
        const long long vq = cq + wave_scan_sum((long long)q, lane), vn = cn + wave_scan_sum((long long)p * (long long)q, lane);
        cq = __shfl(vq, 63); cn = __shfl(vn, 63);                    // (a lane without an order adds nothing: lane 63 holds the pass's end)
        for (int k = 0; k < K; k++) {
            if ((done >> k) & 1u) continue;
            const long long Q = S.q[k];
            if (cq < Q) continue;
            const int l = __ffsll((long long)__ballot(valid && vq >= Q)) - 1;        // exists: the pass's last order has vq == cq
            const long long ql = __shfl(vq, l), nl = __shfl(vn, l);
            const int32_t pl = __shfl(p, l);
            if (lane == k) { rf = Q; rn = nl - (long long)pl * (ql - Q); rp = pl; }
            done |= 1u << k;
        }
        lastp = __shfl(p, 63 - __clzll((long long)__ballot(valid)));
        if (done == all) break;
    }
    if (lane < K) {
        if (((done >> lane) & 1u) == 0u) { rf = cq; rn = cn; rp = lastp; }           // larger than the side: all of it, at the side's last price (0: empty)
        long long* r = out + 3 * ((size_t)w * (size_t)K + (size_t)lane);
        r[0] = rf; r[1] = rn; r[2] = (long long)rp;
    }
}

// every agent's resting orders: out i64 [n][2][A][6] = (orders, quantity, notional, best_price, worst_price, ahead_qty).  Lane a keeps agent a's count, the
// prices of its first and last own order in queue order and the quantity in front of the first; quantity and notional are summed in the wave's slice of LDS.
__global__ __launch_bounds__(64 * CDA_WPB) void k_book_agents(const uint8_t* arena, Params P, int cap, int first, int n, int A, long long* out) {
    __shared__ unsigned long long table[CDA_WPB][CDA_MAX_AGENTS][2];
    READER_WAVE_IN_GROUP(CDA_WPB);
    const bool live = w < 2 * n;
    unsigned long long (*t)[2] = table[wib];
    if (lane < 2 * CDA_MAX_AGENTS) t[lane >> 1][lane & 1] = 0ull;
    __syncthreads();
    int cnt = 0;
    int32_t best = 0, worst = 0;
    long long ahead = 0;
    if (live) {
        const BookSide b = book_side(arena, P, cap, first + (w >> 1), w & 1);
        long long cq = 0;
        for (int base = 0; base < b.n; base += WAVE) {
            const int i = base + lane;
            const bool valid = i < b.n;
            int32_t p = 0, q = 0, owner = -1;
            if (valid) { p = b.get(0, i); q = b.get(1, i); owner = b.get(2, i) & 15; }
            const long long vq = cq + wave_scan_sum((long long)q, lane);
            cq = __shfl(vq, 63);
            if (valid && owner < A) {
                lds_add(&t[owner][0], (long long)q);
                lds_add(&t[owner][1], (long long)p * (long long)q);
            }
            for (int a = 0; a < A; a++) {
                const unsigned long long mk = __ballot(valid && owner == a);
                if (mk == 0ull) continue;                            // (uniform)
                const int f = __ffsll((long long)mk) - 1, l = 63 - __clzll((long long)mk);
                const int32_t pf = __shfl(p, f), pl = __shfl(p, l);
                const long long before = __shfl(vq - (long long)q, f);
                if (lane == a) {
                    if (cnt == 0) { best = pf; ahead = before; }
                    worst = pl; cnt += __popcll(mk);
                }
            }
        }
    }
    __syncthreads();
    if (live && lane < A) {
        long long* r = out + 6 * ((size_t)w * (size_t)A + (size_t)lane);
        r[0] = (long long)cnt; r[1] = (long long)t[lane][0]; r[2] = (long long)t[lane][1]; r[3] = (long long)best; r[4] = (long long)worst; r[5] = ahead;
    }
}

// the Level-3 dump, first half: count + scan over the 2n sides in ONE workgroup (the scheme of k_snap_offsets / k_tape_offsets): off i64 [2n + 1]
constexpr int BOOK_SCAN_THREADS = 1024;
__global__ __launch_bounds__(BOOK_SCAN_THREADS) void k_book_offsets(const uint8_t* arena, Params P, int cap, int first, int n, long long* off) {
    __shared__ long long part[BOOK_SCAN_THREADS];
    const int t = (int)threadIdx.x, items = 2 * n, chunk = (items + BOOK_SCAN_THREADS - 1) / BOOK_SCAN_THREADS;
    const int lo = t * chunk < items ? t * chunk : items, hi = lo + chunk < items ? lo + chunk : items;
    long long s = 0;
    for (int i = lo; i < hi; i++) s += book_side(arena, P, cap, first + (i >> 1), i & 1).n;
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < BOOK_SCAN_THREADS; d <<= 1) {
        const long long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = t > 0 ? part[t - 1] : 0;
    for (int i = lo; i < hi; i++) { off[i] = run; run += book_side(arena, P, cap, first + (i >> 1), i & 1).n; }
    if (t == BOOK_SCAN_THREADS - 1) off[items] = part[t];
}
// second half: the rows cda_get_book returns - (price, qty, owner, order_id, timestamp) - side after side, dense; a side whose run does not lie inside the
// buffer as the offsets say (the book moved between the two launches, or another env's table) is left alone
__global__ __launch_bounds__(64 * CDA_WPB) void k_book_pack(const uint8_t* arena, Params P, int cap, int first, int n, const long long* off, int32_t* out, long long out_rows) {
    READER_WAVE();
    if (w >= 2 * n) return;
    const BookSide b = book_side(arena, P, cap, first + (w >> 1), w & 1);
    const long long o = off[w];
    if (o < 0 || o + (long long)b.n > out_rows || off[w + 1] - o != (long long)b.n) return;
    for (int i = lane; i < b.n; i += WAVE) {
        const int32_t p = b.get(0, i), q = b.get(1, i), oo = b.get(2, i), ts = b.get(3, i);
        int32_t* r = out + 5 * ((size_t)o + (size_t)i);
        r[0] = p; r[1] = q; r[2] = oo & 15; r[3] = (int32_t)((uint32_t)oo >> 4); r[4] = ts;
    }
}

extern "C" {

// the arguments that need no env are vetted first, then the range against the env; nothing is launched behind a refusal.  One wave per (market, side): 2 n waves.

int cda_book_counts(cda_env* e, int32_t first_market, int32_t n_markets, int32_t* counts_out_dev, void* stream) {
    if (!reader_args_ok(e, counts_out_dev, first_market, n_markets) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    return reader_launch(e, k_book_counts, 2 * n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, (int)e->cap, (int)first_market, (int)n_markets, counts_out_dev);
}
int cda_book_levels(cda_env* e, int32_t first_market, int32_t n_markets, int32_t max_levels, int64_t* levels_out_dev, void* stream) {
    if (!reader_args_ok(e, levels_out_dev, first_market, n_markets) || max_levels < 1 || max_levels > CDA_BOOK_MAX_LEVELS || !aligned(levels_out_dev, 8) ||
        !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    return reader_launch(e, k_book_levels, 2 * n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, (int)e->cap, (int)first_market, (int)n_markets, (int)max_levels,
                         (long long*)levels_out_dev);
}
int cda_book_impact(cda_env* e, int32_t first_market, int32_t n_markets, const int64_t* sizes_host, int32_t n_sizes, int64_t* impact_out_dev, void* stream) {
    if (!reader_args_ok(e, impact_out_dev, first_market, n_markets) || !sizes_host || n_sizes < 1 || n_sizes > CDA_BOOK_MAX_SIZES || !aligned(impact_out_dev, 8))
        return CDA_ERR_INVALID;
    BookSizes S;
    memset(&S, 0, sizeof S);
    for (int k = 0; k < n_sizes; k++) {
        if (sizes_host[k] < 1) return CDA_ERR_INVALID;
        S.q[k] = (long long)sizes_host[k];
    }
    if (!range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    return reader_launch(e, k_book_impact, 2 * n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, (int)e->cap, (int)first_market, (int)n_markets, S, (int)n_sizes,
                         (long long*)impact_out_dev);
}
int cda_book_agents(cda_env* e, int32_t first_market, int32_t n_markets, int64_t* agents_out_dev, void* stream) {
    if (!reader_args_ok(e, agents_out_dev, first_market, n_markets) || !aligned(agents_out_dev, 8) || !range_ok(e, first_market, n_markets) || !agents_ok(e)) return CDA_ERR_INVALID;
    return reader_launch(e, k_book_agents, 2 * n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, (int)e->cap, (int)first_market, (int)n_markets,
                         (int)e->P.cfg.num_agents, (long long*)agents_out_dev);
}
int cda_book_offsets(cda_env* e, int32_t first_market, int32_t n_markets, int64_t* offsets_dev, void* stream) {
    if (!reader_args_ok(e, offsets_dev, first_market, n_markets) || !aligned(offsets_dev, 8) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    return reader_launch(e, k_book_offsets, 1, BOOK_SCAN_THREADS / 64, 0, stream, (const uint8_t*)e->arena, e->P, (int)e->cap, (int)first_market, (int)n_markets,
                         (long long*)offsets_dev);                   // (the scan: ONE workgroup)
}
int cda_book_pack(cda_env* e, int32_t first_market, int32_t n_markets, const int64_t* offsets_dev, int64_t total_orders, void* orders_out_dev, int64_t capacity_orders,
                  void* stream) {
    if (!reader_args_ok(e, offsets_dev, first_market, n_markets) || total_orders < 0 || capacity_orders < total_orders || (capacity_orders > 0 && !orders_out_dev) ||
        !aligned(orders_out_dev, 4) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    return reader_launch(e, k_book_pack, 2 * n_markets, CDA_WPB, 0, stream, (const uint8_t*)e->arena, e->P, (int)e->cap, (int)first_market, (int)n_markets,
                         (const long long*)offsets_dev, (int32_t*)orders_out_dev, (long long)capacity_orders);
}

}  // extern "C"
