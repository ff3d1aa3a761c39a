// cda_tape_exec.inc - the execution report over the records of one remembered episode of the trade tape (include/cda.h cda_tape_exec), included behind
// cda_tape.inc (tape_span, tape_load, tape_step; the wave toolkit: cda_wave.hpp).  A READER like the two kernels there: one wave per market (CDA_WPB markets per
// workgroup), lanes over records, 64 records per pass, the slot masked along the ring.  Per market and agent it fills two tables of 64-bit integers, both
// accumulated in the wave's own slice of (dynamic) LDS and written out once, dense: only the market's own wave writes the market's rows, no atomics on global
// memory, nothing depends on scheduling.
//
//   stats    [A][CDA_TAPE_STAT_WORDS]  the additive words (quantities, notionals, fills by side and by role, self-trades) are LDS adds of the lanes' records:
//                                       integer sums, their order cannot matter.  The PATH words need the agent's running position at every one of its fills:
//                                       per pass and per agent that trades in it (a uniform loop, ballot-skipped) the signed quantities of the agent's lanes
//                                       are prefix-summed over the wave (__shfl_up, six steps, other lanes add 0) on top of the position the agent carried into
//                                       the pass; the carry is the table's own final_pos / last_step word, written by the agent's last lane of the pass.
//                                       abs_pos_steps is a sum of |position before the fill| x (steps since the agent's previous fill) - two fills inside one
//                                       step are 0 steps apart, so only the position after the LAST fill of a step is weighted - closed at S_last + 1.
//   markouts [A][H][2][4]              mark(t) = the price of the last held record whose step is <= t.  The step index never decreases inside an episode, so
//                                       for a fill at record i and horizon k that record is found by a binary search over [i, count): one probe 64 records
//                                       ahead first (short horizons end inside it, on lines the pass has just read), then halving; all lanes and up to four
//                                       horizons search in lockstep, the loads unconditional (a finished search probes its own answer again).  A fill whose
//                                       s + k lies beyond S_last, the step of the last held record, is open: counted, not marked.

static_assert(CDA_TAPE_STAT_WORDS == 16 && CDA_TAPE_MAX_HORIZONS == 8 && CDA_MAX_AGENTS <= 64, "cda_tape_exec layout");
enum { XS_BUY_QTY = 0, XS_SELL_QTY, XS_BUY_NOTIONAL, XS_SELL_NOTIONAL, XS_MAKER_QTY, XS_MAKER_FILLS, XS_TAKER_QTY, XS_TAKER_FILLS, XS_SELF_QTY, XS_SELF_FILLS,
       XS_FINAL_POS, XS_MAX_LONG, XS_MAX_SHORT, XS_ABS_POS_STEPS, XS_FIRST_STEP, XS_LAST_STEP };
struct ExecHorizons { int32_t k[CDA_TAPE_MAX_HORIZONS]; };
constexpr int EXEC_HCHUNK = 4;                                        // horizons searched side by side
constexpr int EXEC_AHEAD = 64;                                        // the first probe of a mark search

// one party of a fill: side 0 = bid (bought), 1 = ask (sold); role 0 = maker (counter_id), 1 = taker (init_id)
__device__ __forceinline__ void exec_party(unsigned long long* row, int side, int role, long long qty, long long notional) {
    lds_add(row + (side ? XS_SELL_QTY : XS_BUY_QTY), qty);
    lds_add(row + (side ? XS_SELL_NOTIONAL : XS_BUY_NOTIONAL), notional);
    lds_add(row + (role ? XS_TAKER_QTY : XS_MAKER_QTY), qty);
    lds_add(row + (role ? XS_TAKER_FILLS : XS_MAKER_FILLS), 1ll);
}

__global__ __launch_bounds__(64 * CDA_WPB) void k_tape_exec(TapeArgs T, int first, int n, int which, int agents, int nh, ExecHorizons hz, long long* stats_out,
                                                            long long* marks_out, int32_t* info) {
    extern __shared__ __align__(16) unsigned long long exec_lds[];    // per wave: agents x 16 stat words, then agents x nh x 2 x 4 mark-out words
    READER_WAVE_IN_GROUP(CDA_WPB);
    const bool live = w < n;
    const int n_stat = agents * CDA_TAPE_STAT_WORDS, n_mark = agents * nh * 8;
    unsigned long long* st = exec_lds + (size_t)wib * (size_t)(n_stat + n_mark);
    unsigned long long* mk = st + n_stat;
    for (int i = lane; i < n_stat; i += WAVE) st[i] = (i & 15) >= XS_FIRST_STEP ? ~0ull : 0ull;      // first_step = last_step = -1
    for (int i = lane; i < n_mark; i += WAVE) mk[i] = 0ull;
    __syncthreads();
    int used = 0;
    TapeSpan sp = {0, 0, 0, 0};
    if (live) {
        const int mi = first + w;
        sp = tape_span(T.meta[mi], T.cap, which);
        const uint4* ring = T.ring + (size_t)mi * (size_t)T.cap * 2;
        const uint32_t mask = T.cap - 1u, s0 = (uint32_t)sp.start & mask;
        const int count = (int)sp.count;                             // <= cap <= CDA_TAPE_CAP_MAX
        const uint32_t s_last = count > 0 ? tape_step(ring[2 * (size_t)((s0 + (uint32_t)(count - 1)) & mask) + 1]) : 0u;
        for (int base = 0; base < count; base += WAVE) {
            const int idx = base + lane;
            const bool in = idx < count;
            uint4 r0, r1;
            tape_load(ring, mask, s0, idx, in, r0, r1);
            const uint32_t cid = tape_counter_id(r0), iid = tape_init_id(r1), step = tape_step(r1);
            const int cside = tape_counter_side(r1), iside = tape_init_side(r1);
            const long long price = (long long)tape_price(r0), qty = (long long)tape_qty(r0);
            const bool ok = in && cid < (uint32_t)agents && iid < (uint32_t)agents;      // (ids outside the env's agents cannot index the tables)
            const bool ev = ok && cid != iid;                        // a fill that moves two positions
            used += __popcll(__ballot(ok));
            if (ok && !ev) { lds_add(st + iid * 16 + XS_SELF_QTY, qty); lds_add(st + iid * 16 + XS_SELF_FILLS, 1ll); }
            if (ev) {
                exec_party(st + cid * 16, cside, 0, qty, price * qty);
                exec_party(st + iid * 16, iside, 1, qty, price * qty);
            }
            // ---- mark-outs
#pragma unroll
            for (int h0 = 0; h0 < CDA_TAPE_MAX_HORIZONS; h0 += EXEC_HCHUNK) {
                if (h0 >= nh) break;                                 // (uniform)
                int lo[EXEC_HCHUNK], hi[EXEC_HCHUNK];
                uint32_t tt[EXEC_HCHUNK];
                bool scored[EXEC_HCHUNK];
#pragma unroll
                for (int j = 0; j < EXEC_HCHUNK; j++) {              // (horizons beyond nh are 0 and score nothing)
                    tt[j] = step + (uint32_t)hz.k[h0 + j];           // step < 2^30, k < 2^31
                    scored[j] = ev && h0 + j < nh && tt[j] <= s_last;
                    // the last record with step <= tt lies in [idx, count): one probe EXEC_AHEAD records on, then the halving
                    const int e = idx + EXEC_AHEAD < count ? idx + EXEC_AHEAD : count - 1;
                    const uint32_t se = tape_step(ring[2 * (size_t)((s0 + (uint32_t)(scored[j] ? e : idx)) & mask) + 1]);
                    lo[j] = idx; hi[j] = idx;
                    if (scored[j]) { if (se <= tt[j]) { lo[j] = e; hi[j] = count - 1; } else hi[j] = e - 1; }
                }
                for (;;) {
                    bool more = false;
#pragma unroll
                    for (int j = 0; j < EXEC_HCHUNK; j++) {
                        const int mid = (lo[j] + hi[j] + 1) >> 1;    // lo == hi: mid = lo, the probe changes nothing
                        const uint32_t sm = tape_step(ring[2 * (size_t)((s0 + (uint32_t)mid) & mask) + 1]);
                        if (lo[j] < hi[j]) { if (sm <= tt[j]) lo[j] = mid; else hi[j] = mid - 1; }
                        more = more || lo[j] < hi[j];
                    }
                    if (!__any(more)) break;
                }
#pragma unroll
                for (int j = 0; j < EXEC_HCHUNK; j++) {
                    if (!(ev && h0 + j < nh)) continue;
                    unsigned long long* cm = mk + ((int)cid * nh + h0 + j) * 8;           // [agent][horizon][role 0 = maker][4]
                    unsigned long long* ct = mk + ((int)iid * nh + h0 + j) * 8 + 4;       // ... [role 1 = taker]
                    if (scored[j]) {
                        const long long mark = (long long)tape_price(ring[2 * (size_t)((s0 + (uint32_t)lo[j]) & mask)]);
                        const long long v = (mark - price) * qty;
                        lds_add(cm, cside ? -v : v); lds_add(cm + 1, qty); lds_add(cm + 2, 1ll);
                        lds_add(ct, iside ? -v : v); lds_add(ct + 1, qty); lds_add(ct + 2, 1ll);
                    } else { lds_add(cm + 3, 1ll); lds_add(ct + 3, 1ll); }
                }
            }
            // ---- the running position, agent by agent
            for (int a = 0; a < agents; a++) {
                const bool mem = ev && ((int)cid == a || (int)iid == a);
                const unsigned long long m = __ballot(mem);
                if (m == 0ull) continue;                             // (uniform)
                unsigned long long* row = st + a * 16;
                const long long pos0 = (long long)row[XS_FINAL_POS], step0 = (long long)row[XS_LAST_STEP];      // what the agent carried into the pass
                const int side = (int)iid == a ? iside : cside;
                const long long d = mem ? (side ? -qty : qty) : 0ll;
                long long x = d;                                     // (wave_scan_sum(d, lane), kept open-coded: through the helper the kernel compiles one instruction shorter)
#pragma unroll
                for (int dd = 1; dd < WAVE; dd <<= 1) {
                    const long long y = __shfl_up(x, dd);
                    if (lane >= dd) x += y;
                }
                const unsigned long long below = m & ((1ull << lane) - 1ull);
                const int pl = below ? 63 - __clzll((long long)below) : lane;            // the agent's previous fill of this pass
                const long long sp_ = (long long)__shfl((int)step, pl);
                const long long after = pos0 + x, before = after - d;
                const long long prev_step = below ? sp_ : step0;     // (step0 = -1: no fill yet, and `before` is 0)
                if (mem) {
                    const long long gap = (long long)step - prev_step, mag = before < 0 ? -before : before;
                    if (mag != 0 && gap != 0) lds_add(row + XS_ABS_POS_STEPS, mag * gap);
                    if (after > 0) atomicMax((long long*)row + XS_MAX_LONG, after);
                    if (after < 0) atomicMin((long long*)row + XS_MAX_SHORT, after);
                }
                __builtin_amdgcn_wave_barrier();
                if (mem && lane == 63 - __clzll((long long)m)) { row[XS_FINAL_POS] = (unsigned long long)after; row[XS_LAST_STEP] = (unsigned long long)step; }
                if (mem && below == 0ull && step0 < 0) row[XS_FIRST_STEP] = (unsigned long long)step;
                __builtin_amdgcn_wave_barrier();
            }
        }
        // the last position is held up to and including step S_last
        if (lane < agents) {
            unsigned long long* row = st + lane * 16;
            const long long pos = (long long)row[XS_FINAL_POS], ls = (long long)row[XS_LAST_STEP];
            if (ls >= 0) row[XS_ABS_POS_STEPS] += (unsigned long long)((pos < 0 ? -pos : pos) * ((long long)s_last + 1 - ls));
        }
    }
    __syncthreads();
    if (!live) return;
    long long* so = stats_out + (size_t)w * (size_t)n_stat;
    for (int i = lane; i < n_stat; i += WAVE) so[i] = (long long)st[i];
    long long* mo = marks_out + (size_t)w * (size_t)n_mark;
    for (int i = lane; i < n_mark; i += WAVE) mo[i] = (long long)mk[i];
    if (info && lane == 0) reader_info(info, w, (int32_t)used, (int32_t)sp.lost, 0, (int32_t)sp.partial);
}

extern "C" {

int cda_tape_exec(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* horizons_dev_or_host, int32_t n_horizons, int64_t* stats_out_dev,
                  int64_t* markouts_out_dev, int32_t* info_out_dev, void* stream) {
    if (!reader_args_ok(e, stats_out_dev, first_market, n_markets) || !horizons_dev_or_host || !markouts_out_dev || n_horizons < 1 || n_horizons > CDA_TAPE_MAX_HORIZONS ||
        !which_ok(which) || !aligned(stats_out_dev, 8) || !aligned(markouts_out_dev, 8) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->tape.ring) return CDA_ERR_UNSUPPORTED;
    if (!agents_ok(e)) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));                                 // (here as well as in reader_launch: the copy of a device array of horizons below runs on it)
    ExecHorizons hz;
    memset(&hz, 0, sizeof hz);
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, horizons_dev_or_host) != hipSuccess) { (void)hipGetLastError(); at.type = hipMemoryTypeUnregistered; }
    if (at.type == hipMemoryTypeDevice) {                            // a device array: one small synchronous copy (the values are checked here, and travel as arguments)
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        HIPCHK(hipMemcpy(hz.k, horizons_dev_or_host, sizeof(int32_t) * (size_t)n_horizons, hipMemcpyDeviceToHost));
    } else memcpy(hz.k, horizons_dev_or_host, sizeof(int32_t) * (size_t)n_horizons);
    for (int h = 0; h < n_horizons; h++) if (hz.k[h] < 0) return CDA_ERR_INVALID;
    const size_t lds = (size_t)CDA_WPB * (size_t)e->P.cfg.num_agents * (size_t)(CDA_TAPE_STAT_WORDS + 8 * n_horizons) * sizeof(unsigned long long);
    return reader_launch(e, k_tape_exec, n_markets, CDA_WPB, lds, stream, e->tape, (int)first_market, (int)n_markets, (int)which, (int)e->P.cfg.num_agents, (int)n_horizons, hz,
                         (long long*)stats_out_dev, (long long*)markouts_out_dev, info_out_dev);
}

}  // extern "C"
