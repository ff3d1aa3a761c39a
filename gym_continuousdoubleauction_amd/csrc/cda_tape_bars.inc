// cda_tape_bars.inc - reductions over the records of one remembered episode of the trade tape (include/cda.h cda_tape_bars, cda_tape_flows), included behind
// cda_tape.inc (tape_span, tape_load; the wave toolkit: cda_wave.hpp).  Both kernels are READERS: one wave per market (CDA_WPB markets per workgroup, as
// k_tape_pack), lanes over records, 64 records per pass, two 16-byte loads per record along the ring (the slot is masked: the run wraps where the ring does).
// Only the market's own wave writes the market's rows, each row once: no atomics on global memory, nothing depends on scheduling.
//
// k_tape_bars.  Within an episode the step index never decreases, so the records of a bar are one run.  Per pass: the bar index of every lane's record, head
// flags from the left neighbour's bar index (__ballot), a segmented inclusive scan over the lanes (__shfl_up, six steps: max / min / sums), after which the last
// lane of every run holds the run's bar.  The run that reaches the pass's last record is not written but CARRIED (uniform registers) and continued by the first
// run of the next pass when that has the same bar index; every other run is a finished bar, stored by its last lane with three 16-byte stores.  The empty bars
// in front of a run are zero-filled by the whole wave (coalesced), those behind the last bar at the end.
//
// k_tape_flows.  The A x A x {quantity, notional, fills} table of a market is accumulated in the wave's own slice of LDS (64-bit integer adds: their order
// cannot matter) and written out once, dense.

static_assert(sizeof(cda_tape_bar) == 48 && CDA_TAPE_CURRENT == 0 && CDA_TAPE_PREVIOUS == 1, "cda_tape_bar layout");

struct BarAcc { int32_t open, high, low, close, n_trades, n_self; long long volume, buy_volume, notional; };
__device__ __forceinline__ void bar_store(uint4* row, const BarAcc& a) {
    row[0] = make_uint4((uint32_t)a.open, (uint32_t)a.high, (uint32_t)a.low, (uint32_t)a.close);
    row[1] = make_uint4((uint32_t)a.n_trades, (uint32_t)a.n_self, (uint32_t)a.volume, (uint32_t)((unsigned long long)a.volume >> 32));
    row[2] = make_uint4((uint32_t)a.buy_volume, (uint32_t)((unsigned long long)a.buy_volume >> 32), (uint32_t)a.notional, (uint32_t)((unsigned long long)a.notional >> 32));
}
// a <- a followed by b (b's records come later on the tape)
__device__ __forceinline__ void bar_append(BarAcc& a, const BarAcc& b) {
    a.high = a.high > b.high ? a.high : b.high; a.low = a.low < b.low ? a.low : b.low; a.close = b.close;
    a.n_trades += b.n_trades; a.n_self += b.n_self; a.volume += b.volume; a.buy_volume += b.buy_volume; a.notional += b.notional;
}
__device__ __forceinline__ BarAcc bar_shfl_up(const BarAcc& a, int d) {
    BarAcc o;
    o.open = __shfl_up(a.open, d); o.high = __shfl_up(a.high, d); o.low = __shfl_up(a.low, d); o.close = a.close;
    o.n_trades = __shfl_up(a.n_trades, d); o.n_self = __shfl_up(a.n_self, d);
    o.volume = __shfl_up(a.volume, d); o.buy_volume = __shfl_up(a.buy_volume, d); o.notional = __shfl_up(a.notional, d);
    return o;
}
__device__ __forceinline__ BarAcc bar_from_lane(const BarAcc& a, int l) {
    BarAcc o;
    o.open = __shfl(a.open, l); o.high = __shfl(a.high, l); o.low = __shfl(a.low, l); o.close = __shfl(a.close, l);
    o.n_trades = __shfl(a.n_trades, l); o.n_self = __shfl(a.n_self, l);
    o.volume = __shfl(a.volume, l); o.buy_volume = __shfl(a.buy_volume, l); o.notional = __shfl(a.notional, l);
    return o;
}

__global__ __launch_bounds__(64 * CDA_WPB) void k_tape_bars(TapeArgs T, int first, int n, int which, int bar_steps, int n_bars, uint4* out, int32_t* info) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w;
    const TapeSpan sp = tape_span(T.meta[mi], T.cap, which);
    const uint4* ring = T.ring + (size_t)mi * (size_t)T.cap * 2;
    uint4* rows = out + 3 * (size_t)w * (size_t)n_bars;               // three 16-byte words per bar
    const uint32_t mask = T.cap - 1u, s0 = (uint32_t)sp.start & mask;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    constexpr int NONE = 0x7fffffff;                                  // the bar index of a lane without a record to aggregate
    int last = -1;                                                    // bar index of the carried run; every row below it is written
    BarAcc carry = {};
    int beyond = 0;
    for (long long base = 0; base < sp.count; base += WAVE) {
        const bool in = base + lane < sp.count;
        uint4 r0, r1;
        tape_load(ring, mask, s0, base + lane, in, r0, r1);
        const uint32_t b = tape_step(r1) / (uint32_t)bar_steps;
        const bool valid = in && b < (uint32_t)n_bars;
        const int key = valid ? (int)b : NONE;
        const unsigned long long vmask = __ballot(valid);
        beyond += __popcll(__ballot(in && !valid));
        if (vmask == 0ull) continue;                                  // (uniform)
        const int lv = 63 - __clzll((long long)vmask);                // the pass's last aggregated record: its run is carried
        const int pk = __shfl_up(key, 1);
        const unsigned long long heads = __ballot(lane == 0 || key != pk);
        const int seg = 63 - __clzll((long long)(heads & lanes_le(lane)));      // first lane of this lane's run
        const bool tail = lane == 63 || ((heads >> ((lane + 1) & 63)) & 1ull) != 0;
        const int price = tape_price(r0), qty = tape_qty(r0);
        BarAcc a;
        a.open = a.high = a.low = a.close = price; a.n_trades = 1; a.n_self = tape_self(r0, r1) ? 1 : 0;
        a.volume = (long long)qty; a.buy_volume = !tape_init_sells(r1.w) ? (long long)qty : 0ll; a.notional = (long long)price * (long long)qty;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {                          // segmented inclusive scan: lane l ends with the sum over [seg, l]
            BarAcc o = bar_shfl_up(a, d);
            if (lane - d >= seg) { bar_append(o, a); a = o; }
        }
        if (seg == 0 && key == last) { BarAcc o = carry; bar_append(o, a); a = o; }     // the first run continues the carried one
        const int k0 = __shfl(key, 0);
        if (last >= 0 && k0 != last && lane == 0) bar_store(rows + 3 * (size_t)last, carry);   // ... or the carried run was a whole bar
        // empty bars in front of a run: (bar of the run before it, this run's bar), filled by the whole wave
        const int prev = seg == 0 ? last : __shfl(pk, seg);
        unsigned long long gaps = __ballot(valid && tail && prev < key - 1);
        while (gaps) {
            const int l = __ffsll((long long)gaps) - 1;
            const long long lo = 3ll * ((long long)__shfl(prev, l) + 1), hi = 3ll * (long long)__shfl(key, l);
            for (long long i = lo + lane; i < hi; i += WAVE) rows[i] = zero;
            gaps &= gaps - 1ull;
        }
        if (valid && tail && lane != lv) bar_store(rows + 3 * (size_t)key, a);
        last = __shfl(key, lv);
        carry = bar_from_lane(a, lv);
    }
    if (last >= 0 && lane == 0) bar_store(rows + 3 * (size_t)last, carry);
    for (long long i = 3ll * ((long long)last + 1) + lane; i < 3ll * (long long)n_bars; i += WAVE) rows[i] = zero;
    if (info && lane == 0) reader_info(info, w, (int32_t)(sp.count - (long long)beyond), (int32_t)sp.lost, (int32_t)beyond, (int32_t)sp.partial);
}

constexpr int FLOW_CELLS_MAX = CDA_MAX_AGENTS * CDA_MAX_AGENTS * 3;
__global__ __launch_bounds__(64 * CDA_WPB) void k_tape_flows(TapeArgs T, int first, int n, int which, int agents, long long* out, int32_t* info) {
    __shared__ unsigned long long table[CDA_WPB][FLOW_CELLS_MAX];     // 6 KB per wave
    READER_WAVE_IN_GROUP(CDA_WPB);
    const bool live = w < n;
    unsigned long long* t = table[wib];
    const int cells = agents * agents * 3;
    for (int i = lane; i < cells; i += WAVE) t[i] = 0ull;
    __syncthreads();
    int used = 0;
    TapeSpan sp = {0, 0, 0, 0};
    if (live) {
        const int mi = first + w;
        sp = tape_span(T.meta[mi], T.cap, which);
        const uint4* ring = T.ring + (size_t)mi * (size_t)T.cap * 2;
        const uint32_t mask = T.cap - 1u, s0 = (uint32_t)sp.start & mask;
        for (long long base = 0; base < sp.count; base += WAVE) {
            bool ok = false;
            if (base + lane < sp.count) {
                uint4 r0, r1;
                tape_load(ring, mask, s0, base + lane, true, r0, r1);
                ok = tape_init_id(r1) < (uint32_t)agents && tape_counter_id(r0) < (uint32_t)agents;    // (ids outside the env's agents cannot index the table)
                if (ok) {
                    unsigned long long* c = t + ((int)tape_init_id(r1) * agents + (int)tape_counter_id(r0)) * 3;       // [init_id][counter_id]
                    const long long price = (long long)tape_price(r0), qty = (long long)tape_qty(r0);
                    lds_add(c, qty);
                    lds_add(c + 1, price * qty);
                    lds_add(c + 2, 1ll);
                }
            }
            used += __popcll(__ballot(ok));
        }
    }
    __syncthreads();
    if (!live) return;
    long long* dst = out + (size_t)w * (size_t)cells;
    for (int i = lane; i < cells; i += WAVE) dst[i] = (long long)t[i];
    if (info && lane == 0) reader_info(info, w, (int32_t)used, (int32_t)sp.lost, 0, (int32_t)sp.partial);
}

extern "C" {

int cda_tape_bars(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, int32_t bar_steps, int32_t n_bars, void* bars_out_dev, int32_t* info_out_dev,
                  void* stream) {
    if (!reader_args_ok(e, bars_out_dev, first_market, n_markets) || bar_steps < 1 || n_bars < 1 || !which_ok(which) || !aligned(bars_out_dev, 16) ||
        !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->tape.ring) return CDA_ERR_UNSUPPORTED;
    return reader_launch(e, k_tape_bars, n_markets, CDA_WPB, 0, stream, e->tape, (int)first_market, (int)n_markets, (int)which, (int)bar_steps, (int)n_bars,
                         (uint4*)bars_out_dev, info_out_dev);
}
int cda_tape_flows(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, int64_t* flows_out_dev, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, flows_out_dev, first_market, n_markets) || !which_ok(which) || !aligned(flows_out_dev, 8) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->tape.ring) return CDA_ERR_UNSUPPORTED;
    if (!agents_ok(e)) return CDA_ERR_INVALID;
    return reader_launch(e, k_tape_flows, n_markets, CDA_WPB, 0, stream, e->tape, (int)first_market, (int)n_markets, (int)which, (int)e->P.cfg.num_agents,
                         (long long*)flows_out_dev, info_out_dev);
}

}  // extern "C"
