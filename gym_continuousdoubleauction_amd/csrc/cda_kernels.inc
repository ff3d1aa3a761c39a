// cda_kernels.inc - the kernels that own a market-wave (and the device helpers around the per-wave LDS image), compiled once
// per BOOK CAPACITY: cda_hip.hip includes this file with CDA_CAP = 256 / CDA_CAPNS = cap256 and again with 512 / cap512;
// cda_create picks the variant (cda_config.book_capacity).  Everything here lives in `namespace cda::CDA_CAPNS`.
// No include guard on purpose.
namespace cda { namespace CDA_CAPNS {
#include "cda_book.inc"
// The market record is loaded in two halves so that a kernel can put its per-workgroup table setup (global loads, LDS
// writes, one __syncthreads) BETWEEN them: every request of the record is in flight while the tables are being staged.
struct MarketPrefetch { uint32_t hv; BookPrefetch book; VecPrefetch acc, hist; };
// L.tl (cda_book.inc): where the market's HBM tier lives and - only for a side whose ST_TAIL bit is set, i.e. never on the
// BASELINE workloads - how many orders its ring holds and where they start.  The cold routines find everything through L.tl.
__device__ __forceinline__ void load_tail_meta(const MarketPtrs& mp, const Params& P, Lds& L, const Mkt& m, int lane) {
    int32_t v = 0;
    if (m.status & ST_TAIL_ANY) { if (lane < 4) v = mp.spill[lane]; }
    const uint64_t sp = (uint64_t)(uintptr_t)mp.spill;
    if (lane == TL_PTR_LO) v = (int32_t)(uint32_t)sp;
    if (lane == TL_PTR_HI) v = (int32_t)(uint32_t)(sp >> 32);
    if (lane == TL_CAP) v = P.lay.spill_cap;
    if (lane < TL_WORDS) L.tl[lane] = v;
}
__device__ __forceinline__ void store_tail_meta(const MarketPtrs& mp, const Lds& L, const Mkt& m, int lane) {
    if (m.status & ST_TAIL_ANY) { if (lane < 4) mp.spill[lane] = L.tl[lane]; }
}
template <bool WITH_HIST>
__device__ __forceinline__ MarketPrefetch load_market_issue(const MarketPtrs& mp, const Params& P, int lane) {
    MarketPrefetch q;
    q.hv = load_header_word(mp.hdr, lane);                 // all the requests are in flight together
    q.book = prefetch_book(mp.book, lane);
    q.acc = vec_prefetch(mp.acc, P.cfg.num_agents * (int)sizeof(Acc), lane);
    q.hist.has = false; q.hist.v = make_uint4(0u, 0u, 0u, 0u);
    // k_step: the observation's history ring rides along, so that phase 6 does not pay an HBM round trip of its own
    if (WITH_HIST) q.hist = vec_prefetch(mp.hist, P.cfg.n_hist * CDA_SNAPSHOT_DIM * 4, lane);
    return q;
}
template <bool WITH_HIST, bool TAILS>
__device__ __forceinline__ void load_market_finish(const MarketPtrs& mp, const Params& P, Lds& L, Mkt& m, const MarketPrefetch& q, int lane) {
    const int acc_bytes = P.cfg.num_agents * (int)sizeof(Acc), hist_bytes = P.cfg.n_hist * CDA_SNAPSHOT_DIM * 4;
    decode_header(q.hv, m);
    finish_book_load(mp.book, q.book, L.book, m, lane);
    vec_finish(&L.acc[0], mp.acc, acc_bytes, q.acc, lane);
    if (WITH_HIST) vec_finish(lds_hist(L, P.cfg.num_agents), mp.hist, hist_bytes, q.hist, lane);
    if ((m.status & ST_LEVELS_VALID) && lane >= H_LEVELS && lane < H_LEVELS + 4 * CDA_K_ROWS) (&L.lvl_px[0][0])[lane - H_LEVELS] = (int32_t)q.hv;
    if (TAILS) load_tail_meta(mp, P, L, m, lane);
    CDA_WSYNC();
}
// (the general form: a market whose book may continue in the HBM tier - test hooks, reset, the out-of-line general step)
template <bool WITH_HIST = false>
__device__ __forceinline__ void load_market(const MarketPtrs& mp, const Params& P, Lds& L, Mkt& m, int lane) {
    const MarketPrefetch q = load_market_issue<WITH_HIST>(mp, P, lane);
    load_market_finish<WITH_HIST, true>(mp, P, L, m, q, lane);
}
// The hot kernels step a market on the tile-only code (TAILS = false everywhere).  That is only right while the whole book is
// - and stays - in the tile: no side continues in the HBM tier, and the pool has room for the at most one new resting order per
// agent a step can add.  Checked once, right after the record arrived and before anything is touched; a market that fails it
// is stepped by the out-of-line general build instead (slow_step / slow_run_random below).
__device__ __forceinline__ bool market_is_cold(const Mkt& m, const Params& P) {
    return (m.status & ST_TAIL_ANY) != 0 || (P.lay.spill_cap != 0 && m.nb + m.na + P.cfg.num_agents > CAP);
}
// the level aggregation currently in LDS describes the book as it is being stored: keep it for the next step
__device__ __forceinline__ void store_levels(const MarketPtrs& mp, const Lds& L, int lane) {
    if (lane >= H_LEVELS && lane < H_LEVELS + 4 * CDA_K_ROWS) __builtin_nontemporal_store((uint32_t)(&L.lvl_px[0][0])[lane - H_LEVELS], &mp.hdr[lane]);
}
template <bool TAILS = true>
__device__ __forceinline__ void store_market(const MarketPtrs& mp, const Params& P, Lds& L, const Mkt& m, int lane) {
    CDA_WSYNC();
    store_header(mp.hdr, m, lane);
    if (TAILS) store_tail_meta(mp, L, m, lane);
    store_book(mp.book, L.book, m, lane);
    {
        const int n16 = P.cfg.num_agents * (int)(sizeof(Acc) / 16);
        for (int i = lane; i < n16; i += WAVE) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(reinterpret_cast<const u32x4*>(&L.acc[0])[i], reinterpret_cast<u32x4*>(mp.acc) + i);
        }
    }
}

__device__ __forceinline__ Lds& wave_lds(const Params& P, int wave, int extra = 0) {
    return *reinterpret_cast<Lds*>(cda_smem + DEC_TABLE_BYTES + extra + (size_t)wave * (size_t)lds_bytes_per_wave(P.cfg.num_agents, P.cfg.n_hist));
}

__device__ __forceinline__ bool episode_over(const Mkt& m, const Params& P, int mi) {      // after step_loaded: t_step already counts the step
    return __popc(m.done_mask) == P.cfg.num_agents || m.t_step >= mrow(P, mi).max_step;
}
// handback / keep_step_outputs: see cda_set_handback (include/cda.h).  keep_step_outputs = the auto-reset pass: the record keeps the
// finished step's reward and flags and only receives the new episode's first frame.
// SUMMARISE: this reset may be the one that ends an episode nobody has checked and credited yet (k_reset); false inside the step kernels, which call
// episode_summarise themselves before they reset (from their own level: see there).  Pk: P where it lies in the kernarg segment.
template <bool SUMMARISE>
__device__ __forceinline__ void reset_market(uint8_t* arena, const Params& P, Lds& L, int mi, int lane, const uint64_t* seeds, float* obs_out,
                                             uint8_t* handback, int handback_stride, int keep_step_outputs, const Params* Pk) {
    MarketPtrs mp = market_ptrs(arena, P, mi);
    Mkt m;
    load_header(mp.hdr, m, lane);
    if (seeds) { rng_seed(m, seeds[mi]); m.seeded = 1; }
    else if (!m.seeded) { rng_seed(m, (uint64_t)mi); m.seeded = 1; }
    // episode metrics: the episode this reset ends is checked and credited here - once (k_run_random has done it for the episodes it finished) -, an episode that is
    // NOT over is discarded like one the reference's callback never sees end; the conservation flag survives the device-side auto reset
    uint32_t keep_flags = keep_step_outputs ? (m.flags & CDA_FLAG_NAV_CONSERVATION) : 0u;
    if (m.status & ST_EP_ON) {
        if (!(m.status & ST_EP_SUMMARISED) && episode_over(m, P, mi)) {
            if constexpr (SUMMARISE) { if (episode_summarise(arena, Pk, mi, nullptr)) keep_flags |= CDA_FLAG_NAV_CONSERVATION; }
        } else if (!(m.status & ST_EP_SUMMARISED) && lane < P.cfg.num_agents) ep_clear(ep_stats(mp, P) + lane);      // (a summarised episode's tallies are clear already)
    }
    m.nb = 0; m.na = 0;
    m.t_step = 0; m.lob_time = 0; m.next_oid = 0; m.has_trade = 0; m.last_trade_price = 0; m.done_mask = 0; m.flags = keep_flags;
    m.peak_orders = 0;
    m.status &= ST_EP_ON;                                 // (an empty book has no tail; its spill ring is simply forgotten)
    ConstRow& R = mrow(P, mi);
    m.last_price = rng_integers(m, R.price_min, R.price_max);
    int A = P.cfg.num_agents;
    if (lane < A) {                                     // Account.reset_acc (account/account.py:55-82)
        Acc& a = L.acc[lane];
        uint32_t f = 0;
        D cash = d_from_i64(R.init_cash), z = d_zero();
        st_dec(a.cash, cash, f); st_dec(a.hold, z, f); st_dec(a.posval, z, f); st_dec(a.vwap, z, f);
        st_dec(a.nav, cash, f); st_dec(a.prev_nav, cash, f); st_dec(a.max_nav, cash, f);
        a.net_position = 0; a.num_trades = 0; a.num_trades_step = 0; a.num_passive_fills_step = 0;
        a.order_step_placed = 0; a.num_rejected_step = 0; a.pad[0] = 0; a.pad[1] = 0;
    }
    aggregate_levels<false>(L, m, lane);
    int H = P.cfg.n_hist;
    if (lane < CDA_SNAPSHOT_DIM) {
        float v = snapshot_value(L, m, R.tick_size, lane);
        for (int h = 0; h < H; h++) {
            mp.hist[h * CDA_SNAPSHOT_DIM + lane] = v;
            if (obs_out) obs_out[(size_t)mi * (size_t)(H * CDA_SNAPSHOT_DIM) + (size_t)(h * CDA_SNAPSHOT_DIM + lane)] = v;
        }
        if (handback) reinterpret_cast<float*>(handback + (size_t)mi * (size_t)handback_stride)[lane] = v;
    }
    if (handback) {
        uint8_t* rec = handback + (size_t)mi * (size_t)handback_stride;
        if (!keep_step_outputs && lane < A) reinterpret_cast<double*>(rec + CDA_SNAPSHOT_DIM * 4)[lane] = 0.0;
        if (lane == 0) {
            uint8_t* fl = rec + CDA_SNAPSHOT_DIM * 4 + A * 8;
            if (!keep_step_outputs) { fl[0] = 0; fl[1] = 0; }
            fl[2] = 1;                                        // the observation restarts from this frame
        }
    }
    m.hist_head = 0;
    m.status |= ST_LEVELS_VALID;                          // aggregate_levels above ran on the (empty) book
    store_market<false>(mp, P, L, m, lane);
    store_levels(mp, L, lane);
}
// Episode-end capture (cda_step_range_capture): a market whose episode ended with this step appends the episode's LAST observation - the one the
// auto reset is about to overwrite in obs_out - to a compact list: slot = atomicAdd(fin_count, 1), fin_obs[slot] = the H frames oldest first,
// fin_index_out[market] = slot (the caller pre-sets -1).  What a learner needs to bootstrap a time-limit truncation with V(last observation) and an
// episode record needs as the last step's observation.  Cold paths only: the auto-reset pass behind k_step<true>, reset_after_step in k_step<false>.
__device__ __forceinline__ void capture_final_obs(const FinCapture& F, const float* hist, int head, int H, int mi, int lane) {
    int idx = 0;
    if (lane == 0) idx = atomicAdd(F.count, 1);
    idx = __builtin_amdgcn_readfirstlane(idx);
    if (idx >= F.cap) return;                             // (the list is full: the index stays -1 and the consumer falls back)
    if (lane < CDA_SNAPSHOT_DIM) {
        float* dst = F.obs + (size_t)idx * (size_t)(H * CDA_SNAPSHOT_DIM);
        for (int j = 0; j < H; j++) {
            int slot = head + j; if (slot >= H) slot -= H;
            dst[j * CDA_SNAPSHOT_DIM + lane] = hist[slot * CDA_SNAPSHOT_DIM + lane];
        }
    }
    if (lane == 0) F.index_out[mi] = idx;
}
__global__ __launch_bounds__(64 * CDA_WPB) void k_reset(uint8_t* arena, Params P, const uint64_t* seeds, const uint8_t* mask, float* obs_out, int first_market, int end_market,
                                                        uint8_t* handback, int handback_stride, int keep_step_outputs, FinCapture fin) {
    int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();   // wave index pinned to an SGPR: market pointers and counts become scalar
    int mi = first_market + (int)blockIdx.x * CDA_WPB + wave;
    if (P.lay.ep_on) dec_tables_init();                   // (uniform; the episode-end check sums NAV in decimal arithmetic)
    if (mi >= end_market) return;
    if (mask && !mask[mi]) return;
    if (fin.index_out && obs_out)                         // the auto-reset pass: the step's launch left the episode's last observation in obs_out (oldest frame first)
        capture_final_obs(fin, obs_out + (size_t)mi * (size_t)(P.cfg.n_hist * CDA_SNAPSHOT_DIM), 0, P.cfg.n_hist, mi, lane);
    reset_market<true>(arena, P, wave_lds(P, wave), mi, lane, seeds, obs_out, handback, handback_stride, keep_step_outputs,
                 (const Params*)((const uint8_t*)__builtin_amdgcn_kernarg_segment_ptr() + 8));      // (arena, then P)
}


// ---- trade tape: what a tape-writing instance does around the step ------------------------------------------------------------
// tape_begin: where this market's next record goes (Mkt::tape_*); tape_finish: the records match() appended join the market's counters.  Only the
// market's own wave touches its ring and its counters, between launches nobody does: no atomics.  `reset`: the launch resets the market behind this
// step (the in-kernel auto reset) - the episode's count restarts (and is remembered as n_prev) and the episode number moves on; the ring is NOT cleared,
// the episode that just ended stays readable until new fills overwrite it.
__device__ __forceinline__ void tape_begin(const TapeArgs& T, int mi, Mkt& m) {
    m.tape_ring = T.ring + (size_t)mi * (size_t)T.cap * 2;
    m.tape_mask = T.cap - 1u;
    // (a relaxed atomic load: a vector load that sees what this wave's earlier part of the launch wrote - k_tape_run hands over mid-episode)
    m.tape_pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(reinterpret_cast<const uint32_t*>(&T.meta[mi].n_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    m.tape_new = 0;
}
__device__ __forceinline__ void tape_finish(const TapeArgs& T, int mi, const Mkt& m, bool reset, int lane) {
    if (lane == 0) {
        TapeMeta& h = T.meta[mi];
        h.n_total += (int64_t)m.tape_new;
        const int32_t n_ep = h.n_episode + m.tape_new;
        h.n_episode = reset ? 0 : n_ep;
        if (reset) { h.n_prev = n_ep; h.prev_partial = h.partial; h.episode += 1; h.partial = 0; }     // (the last step's fills belong to the episode that ends)
    }
}

// phases 1-5: everything of a step that changes the market.  Returns the mask of agents that passed.
template <bool TAILS, bool TAPE = false>
__device__ __forceinline__ uint32_t step_market(Lds& L, Mkt& m, const Params& P, int mi, const unsigned long long* zig_wi, const unsigned long long* zig_ki,
                                                const LaneAction& in, unsigned long long* ph, int lane) {
    const int A = P.cfg.num_agents, tick = mrow(P, mi).tick_size;
    // 1. pre-step snapshot (continuousDoubleAuction_env.py:274): prices of ALL orders resolve against it.  It equals the
    //    post-step aggregation of the previous step, which travels in the header; recomputed only when a test hook,
    //    set_state or reset touched the book in between.
    if (!(m.status & ST_LEVELS_VALID)) aggregate_levels<TAILS>(L, m, lane);
    PH_MARK(ph, 2);
    // 2. set_actions (exchg/action_helper.py:145-172, :241-283): one normal per present agent, in agent order; lane a
    //    decodes agent a.  Every agent's normal is first computed SPECULATIVELY in its own lane: the k-th present agent
    //    jumps the LCG ahead by k + 1 and takes the ziggurat's first candidate.  If every lane accepted (95 % of the steps at
    //    4 agents) those ARE the sequential draws; otherwise the draws are redone one after the other, wave-uniform.
    uint32_t act_mask = 0, pass_mask = 0;
    int arrival = 0;                                  // lane a: position of agent a's order in the arrival list handed to the shuffle
    {
        const bool pres = in.pres;
        const uint64_t pm = __ballot(pres);
        if (pm) {
            double z = 0.0;
            // The reference walks the caller's action dict in ITS iteration order (action_helper.py:164-170): the k-th key gets the
            // k-th normal and - unless it passes - the next place in the arrival list.  `in.ord` carries that order (the value of
            // cda_step's `present`: 1 + position in the dict; a plain 0 / 1 mask or no mask at all = ascending agent index).
            int k = __popcll(pm & ((1ull << lane) - 1ull));                       // draws that precede this agent's
            const bool ordered = __ballot(pres && in.ord != 1) != 0;             // wave-uniform; never true for mask-style callers
            if (ordered) {
                const int key = pres ? in.ord : 0x7fffffff;
                k = 0;
                for (int b = 0; b < A; b++) { const int kb = __builtin_amdgcn_readlane(key, b); k += (kb < key || (kb == key && b < lane)) ? 1 : 0; }
            }
            const int n_pres = __popcll(pm);
            {
                const u128 sj = pcg_jump_state(zig_ki + 256, k & (CDA_MAX_AGENTS - 1), m.rng_state, m.rng_inc);
                const bool ok = zig_first_candidate(pcg_output(sj), zig_wi, zig_ki, &z);
                if (__ballot(pres && !ok) == 0) {
                    const int last = __ffsll((long long)__ballot(pres && k == n_pres - 1)) - 1;      // its state is the stream's state after all draws
                    uint32_t w0 = (uint32_t)sj, w1 = (uint32_t)(sj >> 32), w2 = (uint32_t)(sj >> 64), w3 = (uint32_t)(sj >> 96);
                    w0 = (uint32_t)__builtin_amdgcn_readlane((int)w0, last); w1 = (uint32_t)__builtin_amdgcn_readlane((int)w1, last);
                    w2 = (uint32_t)__builtin_amdgcn_readlane((int)w2, last); w3 = (uint32_t)__builtin_amdgcn_readlane((int)w3, last);
                    m.rng_state = ((u128)w3 << 96) | ((u128)w2 << 64) | ((u128)w1 << 32) | (u128)w0;
                } else {
                    for (int r = 0; r < n_pres; r++) {                             // the r-th key of the dict draws the r-th normal
                        const int a = __ffsll((long long)__ballot(pres && k == r)) - 1;
                        double za = rng_std_normal(m, zig_wi, zig_ki);
                        if (lane == a) z = za;
                    }
                }
            }
            bool ovf = false;
            int side = S_NONE;
            if (pres) {
                int cat = clampi(in.cat, 0, 8);
                float mean = clampf(in.mean, -1.0f, 1.0f), sigma = clampf(in.sigma, 0.0f, 1.0f);
                int level = clampi(in.level, 0, CDA_K_ROWS - 1), off = clampi(in.off, 0, 2) - 1;
                side = cat == 0 ? S_NONE : (cat <= 4 ? S_BID : S_ASK);
                int type = cat == 0 ? T_MARKET : ((cat - 1) & 3);
                // (both factors read as SCALARS first: `cond ? P.a : P.b` on a per-lane condition makes the compiler select the kernarg ADDRESS
                //  per lane and fetch it with a vector load - a global round trip in the middle of the decode phase)
                const float mul_mkt = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mrow(P, mi).mkt_mul)));
                const float mul_lim = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mrow(P, mi).lim_mul)));
                float locf = (type == T_MARKET ? mul_mkt : mul_lim) * mean;          // float32 product (numpy NEP 50)
                double prod = (double)sigma * z;
                double sample = (double)locf + prod;                                   // built with -ffp-contract=off
                double rs = rint(fabs(sample));
                if (rs > 1.0e9) { rs = 1.0e9; ovf = true; }
                int32_t size = (int32_t)rs + mrow(P, mi).min_size;
                int32_t pr = -1;
                if (type != T_MARKET) {                                                // _set_price (action_helper.py:341-397)
                    int32_t p = L.lvl_px[side == S_BID ? 0 : 1][level];
                    if (side == S_BID) pr = (p == 0 ? m.last_price - (level + 1) * tick : p) + off * tick;
                    else pr = (p == 0 ? m.last_price + (level + 1) * tick : p) - off * tick;
                    if (pr < tick) pr = tick;
                    if (pr >= (1 << 24)) { pr = (1 << 24) - 1; ovf = true; }
                }
                L.act_tsp[lane] = type | (side << 2) | ((pr + 1) << 4);
                L.act_size[lane] = size;
            }
            const bool acts = pres && side != S_NONE;
            act_mask = (uint32_t)__ballot(acts);
            pass_mask = (uint32_t)__ballot(pres && side == S_NONE);
            arrival = __popc(act_mask & ((1u << (lane & 31)) - 1u));               // (lane & 31: every lane evaluates this; a shift count of 32+ is undefined - lanes beyond the agents are masked below)
            if (ordered) {                                                          // the non-pass keys, in dict order
                const int key = acts ? k : 0x7fffffff;
                arrival = 0;
                for (int b = 0; b < A; b++) arrival += __builtin_amdgcn_readlane(key, b) < key ? 1 : 0;
            }
            // two or more market orders: this step will most likely sweep - take the head start now (see match())
            if (__popcll(__ballot(acts && (L.act_tsp[lane] & 3) == T_MARKET)) >= 2) __builtin_amdgcn_s_setprio(1);
            if (__ballot(ovf)) m.flags |= CDA_FLAG_INT_OVERFLOW;
        }
        CDA_WSYNC();
    }
    PH_MARK(ph, 3);
    // 3. rand_exec_seq (action_helper.py:174-199): Fisher-Yates over the n non-pass orders, nibble-packed
    m.fills = 0;
    int n_acts = __popc(act_mask);
    uint64_t perm = 0xFEDCBA9876543210ull;
    for (int i = n_acts - 1; i >= 1; i--) {
        int j = (int)rng_interval(m, (uint32_t)i);
        uint64_t vi = (perm >> (4 * i)) & 0xFull, vj = (perm >> (4 * j)) & 0xFull;
        perm &= ~((0xFull << (4 * i)) | (0xFull << (4 * j)));
        perm |= (vj << (4 * i)) | (vi << (4 * j));
    }
    PH_MARK(ph, 4);
    // 4. do_actions (action_helper.py:201-239): sequential, order dependent
    for (int i = 0; i < n_acts; i++) {
        const int kk = (int)((perm >> (4 * i)) & 0xFull);                          // the shuffle's i-th pick from the arrival list
        const int tr = __ffsll((long long)__ballot(lane < CDA_MAX_AGENTS && ((act_mask >> (lane & 31)) & 1u) != 0 && arrival == kk)) - 1;
        int32_t tsp = L.act_tsp[tr], size = L.act_size[tr];
        place_order<TAILS, true, TAPE>(L, m, tr, tsp & 3, (tsp >> 2) & 3, size, (tsp >> 4) - 1, lane);     // mark_to_mkt below rewrites position_val
    }
    PH_MARK(ph, 5);
    // 5. mark_to_mkt
    mark_to_mkt(L, m, A, lane);
    PH_MARK(ph, 6);
    return pass_mask;
}

// phase 7, Reward_Helper.set_reward (exchg/reward_helper.py:35-102) and Done_Helper.set_done (done_helper.py:3-18) for
// lane a < A.  The two float(Decimal) conversions of the reward are independent: the owner lane converts nav - prev_nav
// while its helper lane (a + 16) converts max_nav - nav, in the same instruction stream.
// WITH_MAX_NAV (info outputs): a third lane (a + 32) converts max_nav itself through the same call site, so the info
// tensor float(max_nav) costs no conversion of its own.
__device__ __forceinline__ StepReward step_reward(Lds& L, const Params& P, int mi, uint32_t& ferr, int lane, bool with_max_nav = false) {
    const int A = P.cfg.num_agents;
    StepReward o; o.r = o.t0 = o.t1 = o.t2 = o.t3 = o.t4 = o.drawdown = o.max_nav = 0.0; o.bankrupt = false;
    double conv = 0.0;
    if (lane_acc(lane) < A && lane_grp(lane) < (with_max_nav ? 3 : 2)) {
        const Acc& a = L.acc[lane_acc(lane)];
        const int g = lane_grp(lane);
        const bool own = g == 0;
        D nav = ld_dec(a.nav), mx = ld_dec(a.max_nav);
        D x = own ? nav : mx, y = own ? ld_dec(a.prev_nav) : nav;
        D df = d_sub(x, y);                                  // ONE call site each, so owner and helpers stay converged
        if (g == 2) df = mx;
        if (g != 1 || d_sgn(df) > 0) conv = d_to_double(df, &ferr);
    }
    const double conv_helper = __shfl(conv, (lane + 16) & 63, WAVE);
    o.max_nav = __shfl(conv, (lane + 32) & 63, WAVE);
    if (lane < A) {
        const Acc& a = L.acc[lane];
        double nav_change = conv;
        ConstRow& R = mrow(P, mi);
        double nav_term = nav_change * (nav_change < 0 ? R.loss_multiplier : 1.0);
        o.drawdown = conv_helper;
        o.t0 = nav_term;
        o.t1 = -(R.order_penalty * (double)a.order_step_placed);
        o.t2 = -(R.trade_penalty * (double)a.num_trades_step);
        o.t3 = -(R.drawdown_penalty * o.drawdown);
        o.t4 = R.passive_bonus * (double)a.num_passive_fills_step;
        double r = 0.0; r += o.t0; r += o.t1; r += o.t2; r += o.t3; r += o.t4;   // left to right (reward_helper.py:92-94)
        o.r = r;
        o.bankrupt = d_sgn(ld_dec(a.nav)) <= 0;
    }
    return o;
}

// CDA_PHASE_TIMING, inside phase 7 (tools/phase_timing.py --info): the cycle counter's low word behind step_reward and behind the four conversions (tacc[9], low / high
// half), behind the per-agent stores and behind the lane-0 block (tacc[13]) - the two accumulator slots the order phase leaves free
#ifdef CDA_PHASE_TIMING
#define TAIL_MARK(m, slot, shift) do { (m).tacc[slot] |= (__builtin_readcyclecounter() & 0xffffffffull) << (shift); } while (0)
#else
#define TAIL_MARK(m, slot, shift) do {} while (0)
#endif

// The info pointers of a launch.  A launch with info tensors carries CDA_INFO_TENSORS VALID pointers (cda_step puts the env's sink where its caller left NULL: csrc/cda_hip.hip
// fill_step_args), so no store of the info block is tested - a test per tensor made every pointer's fetch wait behind the previous pointer's branch: one scalar-memory
// round trip per tensor, back to back, at the end of every wave.  Untested, the compiler fetches them in a few wide scalar loads (profiles/info_tail/attribution.txt; a
// per-lane vector fetch of the table ahead of phase 7 with readlane at the store sites measured SLOWER than the parent: profiles/info_tail/ab.txt).

// The kernel's arguments as ONE struct: the out-of-line general step reads them back from the kernarg segment instead of having
// them passed (which would keep them live - or copy them - in the hot kernel).
struct StepKernArgs { uint8_t* arena; Params P; StepArgs S; };

// One step of one market once its record is in LDS: phases 1-7 and the write-back.  Shared by the hot kernel (TAILS = false)
// and the out-of-line general build (TAILS = true).
// TALLY (episode metrics, include/cda.h cda_episode_metrics_enable): 0 = this instance never tallies - the kernels an env launches while the metrics are off, i.e. every
// measured number of bench.py: with the tally's code merely branched around, the hot kernels measured 1 % slower (+18 spilled scalars; profiles/r06/episode_metrics_cost.txt) -,
// 1 = it always does (the instances launched while they are on), 2 = decided by the market's ST_EP_ON bit at run time (the out-of-line general build, one instance).
template <bool INFO, bool TAILS, int TALLY, bool TAPE = false>
__device__ __forceinline__ void step_loaded(const Params& P, const StepArgs& S, const MarketPtrs& mp, Lds& L, Mkt& m, LaneAction in, uint8_t present,
                                            const unsigned long long* zig_wi, const unsigned long long* zig_ki, int mi, int lane, unsigned long long* ph) {
    const bool has_info = INFO && S.has_info != 0;   // <true> keeps the run-time test (its code is the one-kernel build's), <false> folds it away
    const int A = P.cfg.num_agents, H = P.cfg.n_hist, tick = mrow(P, mi).tick_size;
    in.pres = lane < A && (!S.present || present != 0);
    in.ord = S.present ? (int)present : 1;
    uint32_t pass_mask = 0;
    if (!CDA_DBG_HAS(S, 1)) pass_mask = step_market<TAILS, TAPE>(L, m, P, mi, zig_wi, zig_ki, in, ph, lane);
    else if (!CDA_DBG_HAS(S, 2)) mark_to_mkt(L, m, A, lane);
    // 6. prep_next_state (state_helper.py:80-92): new frame, history ring, stacked observation.  The frame is COMPUTED here and
    //    written behind the last decimal routine of phase 7: every out-of-line function starts with s_waitcnt vmcnt(0) - it would
    //    wait for these stores to be acknowledged.
    float frame_v = 0.0f;                                 // lane j < 42: value j of the new frame (kept for the hand-back record)
    if (!CDA_DBG_HAS(S, 4)) {
        aggregate_levels<TAILS>(L, m, lane);
        if (lane < CDA_SNAPSHOT_DIM) frame_v = snapshot_value(L, m, tick, lane);
    }
    PH_MARK(ph, 7);
    // 7. set_step_outputs (exchg_helper.py:93-124)
    uint32_t ferr = 0;
    StepReward rw; rw.r = rw.t0 = rw.t1 = rw.t2 = rw.t3 = rw.t4 = rw.drawdown = rw.max_nav = 0.0; rw.bankrupt = false;
    if (!CDA_DBG_HAS(S, 8)) rw = step_reward(L, P, mi, ferr, lane, has_info);
    TAIL_MARK(m, 9, 0);
    if (has_info) {                                                          // Info_Helper.set_info (info_helper.py:30-116)
        // the four float(Decimal) fields of an account are converted by four lanes (a, a+16, a+32, a+48) through ONE call site
        const int al = lane_acc(lane), g = lane_grp(lane);
        if (al < A) {
            const Acc& a = L.acc[al];
            const cda_dec& src = g == 0 ? a.vwap : (g == 1 ? a.cash : (g == 2 ? a.hold : a.posval));
            const cda_info_ptrs& I = S.info;
            double* dst = g == 0 ? I.vwap : (g == 1 ? I.cash : (g == 2 ? I.cash_on_hold : I.position_val));   // (per lane: fetched from the kernarg segment by a vector load - measured cheaper than four scalar pointers held live: 462.6 vs 443.5 M)
            const double v = d_to_double(ld_dec(src), &ferr);
            dst[(size_t)mi * (size_t)A + (size_t)al] = v;
        }
    }
    TAIL_MARK(m, 9, 32);
    if (!CDA_DBG_HAS(S, 4)) {                             // phase 6's stores (no decimal routine is called from here on)
        size_t ob = (size_t)mi * (size_t)(H * CDA_SNAPSHOT_DIM);
        if (lane < CDA_SNAPSHOT_DIM) {
            int head = m.hist_head;                       // slot of the oldest frame = the one to overwrite
            const float* hist = lds_hist(L, A);           // staged by load_market
            for (int j = 0; j < H - 1; j++) {
                int slot = head + 1 + j; if (slot >= H) slot -= H;
                __builtin_nontemporal_store(hist[slot * CDA_SNAPSHOT_DIM + lane], &S.obs_out[ob + (size_t)(j * CDA_SNAPSHOT_DIM + lane)]);
            }
            __builtin_nontemporal_store(frame_v, &S.obs_out[ob + (size_t)((H - 1) * CDA_SNAPSHOT_DIM + lane)]);
            __builtin_nontemporal_store(frame_v, &mp.hist[head * CDA_SNAPSHOT_DIM + lane]);
        }
        m.hist_head = m.hist_head + 1 >= H ? 0 : m.hist_head + 1;
    }
    if (lane < A) {
        Acc& a = L.acc[lane];
        size_t ix = (size_t)mi * (size_t)A + (size_t)lane;
        __builtin_nontemporal_store(rw.r, &S.reward_out[ix]);
        if (has_info) {
            const cda_info_ptrs& I = S.info;
            I.nav[ix] = a.nav;
            I.num_trades[ix] = a.num_trades;
            I.net_position[ix] = a.net_position;
            I.drawdown[ix] = rw.drawdown;
            I.max_nav[ix] = rw.max_nav;
            I.num_trades_step[ix] = a.num_trades_step;
            I.num_passive_fills_step[ix] = a.num_passive_fills_step;
            I.order_step_placed[ix] = a.order_step_placed;
            I.num_rejected_step[ix] = a.num_rejected_step;
            I.is_pass_action[ix] = (uint8_t)((pass_mask >> (lane & 31)) & 1u);
            { double* rt = I.reward_terms + ix * 5; rt[0] = rw.t0; rt[1] = rw.t1; rt[2] = rw.t2; rt[3] = rw.t3; rt[4] = rw.t4; }
            {                                                                  // decoded orders as the env keeps them (agent order, passes left out)
                int32_t* la = I.lob_actions + ix * 4;
                const int32_t tsp = L.act_tsp[lane];
                const bool has = in.pres && !((pass_mask >> (lane & 31)) & 1u);
                la[0] = has ? ((tsp >> 2) & 3) : -1; la[1] = has ? (tsp & 3) : -1; la[2] = has ? L.act_size[lane] : -1; la[3] = has ? (tsp >> 4) - 1 : -1;
            }
        }
        // episode metrics: the tallies live right behind the book tile - an address made of what the write-back below keeps live anyway
        if constexpr (TALLY != 0) {
            if (TALLY == 1 || (m.status & ST_EP_ON)) ep_tally(reinterpret_cast<EpStats*>(mp.book + BOOK_FIELDS * CAP) + lane, rw, a, ((pass_mask >> (lane & 31)) & 1u) != 0);
        }
        clear_step_counters(a);
    }
    TAIL_MARK(m, 13, 0);
    if (__ballot(ferr != 0)) m.flags |= CDA_FLAG_DEC_DOMAIN;
    m.done_mask |= (uint32_t)__ballot(rw.bankrupt);
    if (lane == 0) {
        if (has_info) {
            const cda_info_ptrs& I = S.info;
            double bb = m.nb ? (double)L.book.price[0][0] : __longlong_as_double(0x7ff8000000000000LL);
            double ba = m.na ? (double)L.book.price[1][0] : __longlong_as_double(0x7ff8000000000000LL);
            I.last_price[mi] = (double)m.last_price;
            I.best_bid[mi] = bb;
            I.best_ask[mi] = ba;
            I.spread[mi] = (m.nb && m.na) ? ba - bb : __longlong_as_double(0x7ff8000000000000LL);
        }
        // Done_Helper.set_all_done (done_helper.py:20-54)
        const bool term = __popc(m.done_mask) == A, trunc = m.t_step + 1 >= mrow(P, mi).max_step;
        S.terminated_out[mi] = (uint8_t)term;
        S.truncated_out[mi] = (uint8_t)trunc;
        if (S.done_out) S.done_out[mi] = (uint8_t)(term || trunc);
    }
    TAIL_MARK(m, 13, 32);
    if (S.handback) {                                     // cda_set_handback: the compact record of what is new this step (ONE test per step)
        uint8_t* rec = S.handback + (size_t)mi * (size_t)S.handback_stride;
        if (lane < CDA_SNAPSHOT_DIM) reinterpret_cast<float*>(rec)[lane] = frame_v;
        if (lane < A) reinterpret_cast<double*>(rec + CDA_SNAPSHOT_DIM * 4)[lane] = rw.r;
        if (lane == 0) {
            uint8_t* fl = rec + CDA_SNAPSHOT_DIM * 4 + A * 8;
            fl[0] = (uint8_t)(__popc(m.done_mask) == A); fl[1] = (uint8_t)(m.t_step + 1 >= mrow(P, mi).max_step); fl[2] = 0;
        }
    }
    m.t_step += 1;
    m.status |= ST_LEVELS_VALID;                          // lvl_px/lvl_sz hold the post-step aggregation (phase 6)
    PH_MARK(ph, 8);
    CDA_DBG_SKIP(S, 16, return);                                 // no write-back of the record
    store_market<TAILS>(mp, P, L, m, lane);
    store_levels(mp, L, lane);
    PH_MARK(ph, 9);
#ifdef CDA_PHASE_TIMING
    if (ph && lane == 0) for (int i = 0; i < 30; i++) ph[10 + i] = m.tacc[i];
#endif
}


// The device-side auto reset (cda_config.auto_reset): a market whose episode ended with this step starts its next one right here, as the
// INFO-LESS step kernel's last act - out of line and cold like slow_step (nothing is live across the call), instead of a k_reset launch behind
// every step (4.6 us of chain latency per step in a rollout, for a pass whose waves almost always exit at once).  reset(seed=None) semantics: the
// RNG stream continues (continuousDoubleAuction_env.py:186-188); the record was written back by the step, so it is re-read from memory
// (workgroup-scope fence: this wave's own stores, the CU's write-through L1 serves the loads).
__attribute__((noinline, cold)) __device__ void reset_after_step(const StepKernArgs* kernargs, int mi, int wave) {
    const StepKernArgs& K = *kernargs;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (K.S.fin_index_out) {                              // episode-end capture: the last observation from the record's history ring (its header names the oldest slot)
        MarketPtrs mp = market_ptrs(K.arena, K.P, mi);
        Mkt m;
        load_header(mp.hdr, m, lane_id());
        FinCapture F; F.obs = K.S.fin_obs; F.count = K.S.fin_count; F.index_out = K.S.fin_index_out; F.cap = K.S.fin_cap;
        capture_final_obs(F, mp.hist, m.hist_head, K.P.cfg.n_hist, mi, lane_id());
    }
    reset_market<false>(K.arena, K.P, wave_lds(K.P, wave, ZIG_LDS_BYTES), mi, lane_id(), nullptr, K.S.obs_out, K.S.handback, K.S.handback_stride, 1, &K.P);
}

// The general step of ONE market (its book may continue in the HBM tier).  Out of line and called as the hot kernel's last
// act, so it costs that kernel no register: nothing is live across the call.  It starts over from the market's record - the
// hot kernel has not written anything yet - with plain loads; the workgroup's tables are already staged.
// Returns 1 (info-less instance only) when the step ended the market's episode and the env resets on the device: the KERNEL then checks / credits the episode and
// resets the market, from its own level (nested here, those routines' scratch would add to this one's).
template <bool INFO>
__attribute__((noinline, cold)) __device__ int slow_step(const StepKernArgs* kernargs, int mi, int wave) {
    const StepKernArgs& K = *kernargs;
    const Params& P = K.P;
    const StepArgs& S = K.S;
    const int lane = lane_id();
    Lds& L = wave_lds(P, wave, ZIG_LDS_BYTES);
    const unsigned long long* zig_wi = reinterpret_cast<const unsigned long long*>(cda_smem + DEC_TABLE_BYTES);
    const unsigned long long* zig_ki = zig_wi + 256;
    MarketPtrs mp = market_ptrs(K.arena, P, mi);
    LaneAction in;
    const size_t ab = (size_t)mi * (size_t)P.cfg.num_agents + (size_t)(lane < P.cfg.num_agents ? lane : 0);
    in.cat = S.category[ab]; in.mean = S.size_mean[ab]; in.sigma = S.size_sigma[ab];
    in.level = S.price[ab]; in.off = S.price_offset[ab]; in.pres = false; in.ord = 1;
    const uint8_t present = *(S.present ? S.present + ab : reinterpret_cast<const uint8_t*>(S.category + ab));
    Mkt m;
#ifdef CDA_PHASE_TIMING
    for (int i = 0; i < 30; i++) m.tacc[i] = 0;
#endif
    load_market<true>(mp, P, L, m, lane);
#ifdef CDA_DEBUG_SKIP
    m.dbg = S.dbg_skip;
#endif
    step_loaded<INFO, true, 2>(P, S, mp, L, m, in, present, zig_wi, zig_ki, mi, lane, nullptr);
    if constexpr (!INFO) { if (S.done_out && episode_over(m, P, mi)) return (m.status & ST_EP_ON) ? 2 : 1; }
    return 0;
}
// slow_step of the tape-writing kernels (k_tstep below): the same, with the market's tape opened and closed around the step (a routine of its own, not a shared body:
// slow_step's code stays what it was)
struct TStepKernArgs { StepKernArgs K; TapeArgs T; };    // K first: the cold paths read StepKernArgs where the kernel's arguments lie
template <bool INFO>
__attribute__((noinline, cold)) __device__ int slow_tstep(const TStepKernArgs* kernargs, int mi, int wave) {
    const StepKernArgs& K = kernargs->K;
    const Params& P = K.P;
    const StepArgs& S = K.S;
    const int lane = lane_id();
    Lds& L = wave_lds(P, wave, ZIG_LDS_BYTES);
    const unsigned long long* zig_wi = reinterpret_cast<const unsigned long long*>(cda_smem + DEC_TABLE_BYTES);
    const unsigned long long* zig_ki = zig_wi + 256;
    MarketPtrs mp = market_ptrs(K.arena, P, mi);
    LaneAction in;
    const size_t ab = (size_t)mi * (size_t)P.cfg.num_agents + (size_t)(lane < P.cfg.num_agents ? lane : 0);
    in.cat = S.category[ab]; in.mean = S.size_mean[ab]; in.sigma = S.size_sigma[ab];
    in.level = S.price[ab]; in.off = S.price_offset[ab]; in.pres = false; in.ord = 1;
    const uint8_t present = *(S.present ? S.present + ab : reinterpret_cast<const uint8_t*>(S.category + ab));
    Mkt m;
#ifdef CDA_PHASE_TIMING
    for (int i = 0; i < 30; i++) m.tacc[i] = 0;
#endif
    load_market<true>(mp, P, L, m, lane);
#ifdef CDA_DEBUG_SKIP
    m.dbg = S.dbg_skip;
#endif
    tape_begin(kernargs->T, mi, m);
    step_loaded<INFO, true, 2, true>(P, S, mp, L, m, in, present, zig_wi, zig_ki, mi, lane, nullptr);
    int over = 0;
    if constexpr (!INFO) { if (S.done_out && episode_over(m, P, mi)) over = (m.status & ST_EP_ON) ? 2 : 1; }
    tape_finish(kernargs->T, mi, m, over != 0, lane);
    return over;
}
// what the info-less step kernels do with a market whose episode has just ended: the callback's episode end, then the reset.  Out of line and thin - ONE cold call
// site in the kernel (every call site there costs the hot code spilled scalars), and the two routines it calls one after the other share its depth of scratch
__attribute__((noinline, cold)) __device__ void episode_end_after_step(const StepKernArgs* kernargs, int mi, int wave, bool metrics) {
    if (metrics) {
        const StepKernArgs& K = *kernargs;
        episode_summarise(K.arena, &K.P, mi, &wave_lds(K.P, wave, ZIG_LDS_BYTES).acc[0]);
    }
    reset_after_step(kernargs, mi, wave);
}

// INFO = the launch emits the info tensors (StepArgs::info / has_info).  A compile-time switch: kernel arguments are fetched
// wholesale at entry, and the twenty info pointers alone are 40 SGPRs that the info-less kernel would load, spill to VGPR
// lanes and carry through every step for nothing.
// (A shape-specialised instance - agent count, history depth, record layout, tick, size multipliers and reward coefficients as compile-time
// constants - was built and measured in round 4: +0.1 % at 4096 x 4, the SGPR spills unchanged (they are the market's own scalars, not
// Params); removed again, record in profiles/r04/step_specialisation.txt.)
template <bool INFO, bool TALLY>
__global__ __launch_bounds__(64 * CDA_WPB, CDA_MIN_WAVES) CDA_VGPR_CAP_ATTR void k_step(StepKernArgs K) {
    uint8_t* const arena = K.arena;
    const Params& P = K.P;
    const StepArgs& S = K.S;
    int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();   // wave index pinned to an SGPR: market pointers and counts become scalar
    int mi = S.first_market + (int)blockIdx.x * CDA_WPB + wave;
    const bool live = mi < S.end_market;      // (a workgroup's surplus waves still take part in the table setup)
    const TablePrefetch tq = stage_tables_issue();          // table words first: their wait must not cover the record's round trip
    __builtin_amdgcn_sched_barrier(0);                      // (the scheduler would otherwise sink them below the record's requests)
    // Everything below is requested unconditionally (a surplus wave asks for the launch's first market, a lane beyond the
    // agents for agent 0): a branch around a load makes the compiler wait for it at the join.
    const int mc = live ? mi : S.first_market;
    MarketPtrs mp = market_ptrs(arena, P, mc);
    const MarketPrefetch mq = load_market_issue<true>(mp, P, lane);    // the record's requests fly while the tables are staged
    LaneAction in;                                           // ... and so do this step's actions (lane a holds agent a's)
    const size_t ab = (size_t)mc * (size_t)P.cfg.num_agents + (size_t)(lane < P.cfg.num_agents ? lane : 0);
    in.cat = S.category[ab]; in.mean = S.size_mean[ab]; in.sigma = S.size_sigma[ab];
    in.level = S.price[ab]; in.off = S.price_offset[ab]; in.pres = false; in.ord = 1;
    const uint8_t present = *(S.present ? S.present + ab : reinterpret_cast<const uint8_t*>(S.category + ab));
    CDA_DBG_SKIP(S, 64, return);                                 // nothing at all
    stage_tables_commit(tq);                  // workgroup-wide (one __syncthreads), before any early exit
    if (!live) return;
    CDA_DBG_SKIP(S, 32, return);                                 // record requested, tables staged, nothing else
    Lds& L = wave_lds(P, wave, ZIG_LDS_BYTES);
    const unsigned long long* zig_wi = reinterpret_cast<const unsigned long long*>(cda_smem + DEC_TABLE_BYTES);
    const unsigned long long* zig_ki = zig_wi + 256;
    Mkt m;
    unsigned long long* ph = nullptr;
#ifdef CDA_PHASE_TIMING
    for (int i = 0; i < 30; i++) m.tacc[i] = 0;
    ph = S.phase_cycles ? S.phase_cycles + (size_t)mi * 40 : nullptr;
#endif
    PH_MARK(ph, 0);
    load_market_finish<true, false>(mp, P, L, m, mq, lane);
#ifdef CDA_DEBUG_SKIP
    m.dbg = S.dbg_skip;
#endif
    PH_MARK(ph, 1);
    // The book may outgrow its tile: the general build steps this market (it reads the kernel's arguments where they lie).  Marked
    // unlikely / cold on purpose: measured, the register allocation of the hot code is then the round-2 one (480.9 M agent-steps/s
    // info-less against 468.6 M without the hints and 456 M with the general build inlined here; profiles/r03/slow_path_variants.txt).
    if (__builtin_expect(market_is_cold(m, P), 0)) {
        const int over = slow_step<INFO>((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave);
        if constexpr (!INFO) {
            if (over) {
                if constexpr (TALLY) episode_end_after_step((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave, over == 2);
                else reset_after_step((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave);
            }
        }
        return;
    }
    step_loaded<INFO, false, TALLY ? 1 : 0>(P, S, mp, L, m, in, present, zig_wi, zig_ki, mi, lane, ph);
    // (only in the info-less instance - the one a learner's rollout runs: in k_step<true> the extra call site cost 13-19 more spilled SGPRs and
    // 1.5 % of the headline, so an env that asks for info tensors AND auto reset keeps the k_reset launch behind the step)
    if constexpr (!INFO) {
        if (__builtin_expect(S.done_out != nullptr && episode_over(m, P, mi), 0)) {
            if constexpr (TALLY) episode_end_after_step((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave, true);
            else reset_after_step((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave);      // (the metrics are off: the instance of every measured number)
        }
    }
}

// k_step that also writes the trade tape (cda_tape_enable): what an env launches while its tape is on.  A kernel of its own name and arguments - the tape's block
// lies behind k_step's -, so that with the tape off every launch runs the very instances it ran before the tape existed.  INFO as in k_step; the episode-metric tallies
// are decided at run time by the market's ST_EP_ON bit (TALLY = 2, as in the general build): two instances per tile, not four.  Stages exactly as k_step does (see there).
template <bool INFO>
__global__ __launch_bounds__(64 * CDA_WPB, CDA_MIN_WAVES) CDA_VGPR_CAP_ATTR void k_tstep(TStepKernArgs KT) {
    uint8_t* const arena = KT.K.arena;
    const Params& P = KT.K.P;
    const StepArgs& S = KT.K.S;
    int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
    int mi = S.first_market + (int)blockIdx.x * CDA_WPB + wave;
    const bool live = mi < S.end_market;
    const TablePrefetch tq = stage_tables_issue();
    __builtin_amdgcn_sched_barrier(0);
    const int mc = live ? mi : S.first_market;
    MarketPtrs mp = market_ptrs(arena, P, mc);
    const MarketPrefetch mq = load_market_issue<true>(mp, P, lane);
    LaneAction in;
    const size_t ab = (size_t)mc * (size_t)P.cfg.num_agents + (size_t)(lane < P.cfg.num_agents ? lane : 0);
    in.cat = S.category[ab]; in.mean = S.size_mean[ab]; in.sigma = S.size_sigma[ab];
    in.level = S.price[ab]; in.off = S.price_offset[ab]; in.pres = false; in.ord = 1;
    const uint8_t present = *(S.present ? S.present + ab : reinterpret_cast<const uint8_t*>(S.category + ab));
    stage_tables_commit(tq);
    if (!live) return;
    Lds& L = wave_lds(P, wave, ZIG_LDS_BYTES);
    const unsigned long long* zig_wi = reinterpret_cast<const unsigned long long*>(cda_smem + DEC_TABLE_BYTES);
    const unsigned long long* zig_ki = zig_wi + 256;
    Mkt m;
#ifdef CDA_PHASE_TIMING
    for (int i = 0; i < 30; i++) m.tacc[i] = 0;
#endif
    load_market_finish<true, false>(mp, P, L, m, mq, lane);
#ifdef CDA_DEBUG_SKIP
    m.dbg = S.dbg_skip;
#endif
    if (__builtin_expect(market_is_cold(m, P), 0)) {
        const int over = slow_tstep<INFO>((const TStepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave);
        if constexpr (!INFO) { if (over) episode_end_after_step((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave, over == 2); }
        return;
    }
    tape_begin(KT.T, mi, m);
    step_loaded<INFO, false, 2, true>(P, S, mp, L, m, in, present, zig_wi, zig_ki, mi, lane, nullptr);
    bool over = false;
    if constexpr (!INFO) over = S.done_out != nullptr && episode_over(m, P, mi);
    tape_finish(KT.T, mi, m, over, lane);
    if constexpr (!INFO) {
        if (__builtin_expect(over, 0)) episode_end_after_step((const StepKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave, (m.status & ST_EP_ON) != 0);
    }
}

#if CDA_CAP == 256
// ------------------------------------------------------------------------------------------
// k_policy_step - the rollout's policy evaluated INSIDE the step kernel (one launch per chain and step instead of two)
// ------------------------------------------------------------------------------------------
// A workgroup is SIXTEEN market-waves.  It first runs the policy / value network on its sixteen observation rows - bf16 MFMA, the weights streamed from L2 in
// operand order, one 32-feature tile per wave and layer (cda_mlp_dev.inc forward16: bit for bit what k_mlp_fwd<SAMPLE> computes) - while the market records'
// requests are in flight; then every wave samples its own market's actions (lane a = agent a) straight into the registers the step consumes, writes the rollout's
// records of them (actions, log-probability, value, sample record, distribution row), and steps its market exactly as k_step<false> does (same code: step_loaded,
// the cold general build, the auto reset).  Against {k_mlp_fwd<SAMPLE> launch, k_step launch}: one dependent-launch edge and the policy kernel's own serial chain
// (10-12 us for any batch) leave the step's critical path, and the sampled actions no longer make an HBM round trip between two kernels.
// Sixteen waves per workgroup, not four: every workgroup streams the whole network's weights (470 KB) per step - at four markets per workgroup that is four times
// the L2 traffic per CU and 14 us of streaming.  LDS: tables | 16 market images | the forward's tiles: 138 KB at 4 agents, 148 KB at 8 - one workgroup per CU.
struct PolicyArgs {
    const float* obs_in;                 // f32 [N][OBS]: the observations the actions are sampled from (the previous step's obs_out)
    const void* wb; const float* theta;  // the policy's packed weights and parameters (include/cda_mlp.h)
    unsigned long long seed; const long long* counter; long long draw;
    int32_t* category; float* size_mean; float* size_sigma; int32_t* price; int32_t* price_offset;     // = StepArgs' action arrays, written here (the cold paths read them back)
    float* a_cont; float* logp; float* value; float* rec; float* dist;
};
struct PolicyStepKernArgs { StepKernArgs K; PolicyArgs F; };      // K first: the cold paths read StepKernArgs where the kernel's arguments lie
constexpr int PS_WPB = 16;
#ifndef CDA_PS_PF
#define CDA_PS_PF 4
#endif
constexpr int PS_PF = CDA_PS_PF;                 // weight ring depth (k-steps in flight per wave)
// one instance per compiled history depth (n_hist 4 under the plain name; the others as <name>_h<H>: include/cda_mlp.h CDA_MLP_HIST_VARIANTS)
#define PS_NS CDA_HIST_SFX(mlpdev)
#define PS_NAME(x) CDA_HIST_SFX(x)
#define CDA_HIST_BODY "cda_policy_step.inc"
#define CDA_HIST_OPEN
#define CDA_HIST_CLOSE
#define PS_NET 0
#define PS_KERNEL k_policy_step
#define PS_KERNARGS PolicyStepKernArgs
#include "cda_hist_variants.inc"
#undef PS_NET
#undef PS_KERNEL
#undef PS_KERNARGS
#undef CDA_HIST_BODY
#undef CDA_HIST_OPEN
#undef CDA_HIST_CLOSE
#undef PS_NS
#undef PS_NAME
#endif

struct RunKernArgs { uint8_t* arena; Params P; RunArgs R; };
// The episode loop of one market from iteration it0 on.  TAILS = false (the hot kernel) stops BEFORE a step its tile-only code
// may not take (market_is_cold), writes the market back as it stands and returns that iteration; the general build then takes
// over from the record (slow_run_random).  Returns -1 when the launch's work for this market is complete (outputs written).
// TAPE (k_tape_run): the episode's fills go to the market's trade tape, *T (handed down explicitly: the general build is an out-of-line function and gets the
// pointer from its caller, like its RunKernArgs)
struct TRunKernArgs { RunKernArgs K; TapeArgs T; };
template <bool TAILS, int TALLY, bool TAPE = false>
__device__ __forceinline__ int run_random_part(uint8_t* arena, const Params& P, const RunArgs& R, int mi, int wave, int lane, int it0, double& ret, int& steps,
                                               const TapeArgs* T = nullptr) {
    Lds& L = wave_lds(P, wave, ZIG_LDS_BYTES);
    const unsigned long long* zig_wi = reinterpret_cast<const unsigned long long*>(cda_smem + DEC_TABLE_BYTES);
    const unsigned long long* zig_ki = zig_wi + 256;
    MarketPtrs mp = market_ptrs(arena, P, mi);
    Mkt m;
    const int A = P.cfg.num_agents, H = P.cfg.n_hist, tick = mrow(P, mi).tick_size;
#ifdef CDA_PHASE_TIMING
    for (int i = 0; i < 30; i++) m.tacc[i] = 0;
#endif
    {
        const MarketPrefetch q = load_market_issue<true>(mp, P, lane);
        load_market_finish<true, TAILS>(mp, P, L, m, q, lane);
    }
    if constexpr (TAPE) tape_begin(*T, mi, m);
    float* hist = lds_hist(L, A);                           // the history ring stays in LDS for the whole episode
    int32_t* hist_raw = reinterpret_cast<int32_t*>(hist);
    int part_steps = 0, it = it0;
    bool term = false, trunc = false, handed = false;
    for (; it < R.n_steps; it++) {
        if (!TAILS && market_is_cold(m, P)) { handed = true; break; }
        LaneAction in;
        in.pres = lane < A; in.ord = 1; in.cat = 0; in.level = 0; in.off = 0; in.mean = 0.0f; in.sigma = 0.0f;
        if (in.pres) cda_random_action(R.seed, R.market_base + (uint64_t)mi, (uint32_t)m.t_step, (uint32_t)lane, &in.cat, &in.mean, &in.sigma, &in.level, &in.off);
        const uint32_t pass_mask = step_market<TAILS, TAPE>(L, m, P, mi, zig_wi, zig_ki, in, nullptr, lane);
        aggregate_levels<TAILS>(L, m, lane);
        // Nobody reads the observation while the episode runs: the ring keeps the RAW frame (the 2 x 2 x 10 level
        // aggregation and last_price, 41 integers) and the normalisation (f64 divisions, square roots, log, log1p) is
        // done after the loop, for the at most n_hist frames that are still in the window.
        if (lane < 4 * CDA_K_ROWS) hist_raw[m.hist_head * CDA_SNAPSHOT_DIM + lane] = (&L.lvl_px[0][0])[lane];
        else if (lane == 4 * CDA_K_ROWS) hist_raw[m.hist_head * CDA_SNAPSHOT_DIM + lane] = m.last_price;
        m.hist_head = m.hist_head + 1 >= H ? 0 : m.hist_head + 1;
        uint32_t ferr = 0;
        const StepReward rw = step_reward(L, P, mi, ferr, lane);
        if (lane < A) {
            ret += rw.r;
            if constexpr (TALLY != 0) {
                if (TALLY == 1 || (m.status & ST_EP_ON)) ep_tally(reinterpret_cast<EpStats*>(mp.book + BOOK_FIELDS * CAP) + lane, rw, L.acc[lane], ((pass_mask >> (lane & 31)) & 1u) != 0);
            }
            clear_step_counters(L.acc[lane]);
        }
        if (__ballot(ferr != 0)) m.flags |= CDA_FLAG_DEC_DOMAIN;
        m.done_mask |= (uint32_t)__ballot(rw.bankrupt);
        term = __popc(m.done_mask) == A; trunc = m.t_step + 1 >= mrow(P, mi).max_step;
        m.t_step += 1;
        m.status |= ST_LEVELS_VALID;
        steps += 1; part_steps += 1;
        CDA_WSYNC();
#ifdef CDA_RR_STALL_TICKS
        // experiment (profiles/r06/served_rollout_budget.txt): every market-wave sleeps CDA_RR_STALL_TICKS x 10 ns after each step - what a wait for an action
        // server costs the batch when the other waves of the SIMD keep running
        { const unsigned long long t0 = wall_clock64(); while (wall_clock64() - t0 < (unsigned long long)(CDA_RR_STALL_TICKS)) __builtin_amdgcn_s_sleep(4); }
#endif
        if (term || trunc) break;
    }
    {   // normalise the raw frames of this part that are still in the window, oldest first: the newest one is converted
        // last, which leaves L.lvl_* / m.last_price describing the current book again
        const int n_raw = part_steps < H ? part_steps : H;
        const int32_t last_price_now = m.last_price;
        for (int k = 0; k < n_raw; k++) {
            int slot = m.hist_head - n_raw + k; if (slot < 0) slot += H;
            CDA_WSYNC();
            if (lane < 4 * CDA_K_ROWS) (&L.lvl_px[0][0])[lane] = hist_raw[slot * CDA_SNAPSHOT_DIM + lane];
            m.last_price = hist_raw[slot * CDA_SNAPSHOT_DIM + 4 * CDA_K_ROWS];
            CDA_WSYNC();
            float v = 0.0f;
            if (lane < CDA_SNAPSHOT_DIM) v = snapshot_value(L, m, tick, lane);
            CDA_WSYNC();
            if (lane < CDA_SNAPSHOT_DIM) hist[slot * CDA_SNAPSHOT_DIM + lane] = v;
        }
        m.last_price = last_price_now;
        CDA_WSYNC();
    }
    if (!handed) {
        if (R.obs_out && lane < CDA_SNAPSHOT_DIM) {             // oldest frame first; hist_head is the oldest slot
            const size_t ob = (size_t)mi * (size_t)(H * CDA_SNAPSHOT_DIM);
            for (int j = 0; j < H; j++) {
                int slot = m.hist_head + j; if (slot >= H) slot -= H;
                R.obs_out[ob + (size_t)(j * CDA_SNAPSHOT_DIM + lane)] = hist[slot * CDA_SNAPSHOT_DIM + lane];
            }
        }
        if (R.return_out && lane < A) R.return_out[(size_t)mi * (size_t)A + (size_t)lane] = ret;
        if (lane == 0) {
            if (R.terminated_out) R.terminated_out[mi] = (uint8_t)term;
            if (R.truncated_out) R.truncated_out[mi] = (uint8_t)trunc;
            if (R.steps_out) R.steps_out[mi] = steps;
        }
    }
    const bool summarise = TALLY != 0 && (m.status & ST_EP_ON) && !handed && (term || trunc);    // the launch ended this market's episode: check and credit it here (a later reset must not)
    if (summarise) m.status |= ST_EP_SUMMARISED;
    if constexpr (TAPE) tape_finish(*T, mi, m, false, lane);
    store_market<TAILS>(mp, P, L, m, lane);
    copy_words((uint32_t*)mp.hist, (const uint32_t*)hist, H * CDA_SNAPSHOT_DIM, lane);
    store_levels(mp, L, lane);
    return handed ? it : (summarise ? -2 : -1);              // -2: the KERNEL checks and credits the episode (episode_summarise, from its own level)
}
// the rest of a market's episode on the general build (see slow_step)
__attribute__((noinline, cold)) __device__ int slow_run_random(const RunKernArgs* kernargs, int mi, int wave, int it0, int steps, double ret) {
    const RunKernArgs& K = *kernargs;
    return run_random_part<true, 2>(K.arena, K.P, K.R, mi, wave, lane_id(), it0, ret, steps);
}
template <bool TALLY>
__global__ __launch_bounds__(64 * CDA_WPB, CDA_MIN_WAVES) CDA_VGPR_CAP_ATTR void k_run_random(RunKernArgs K) {
    int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
    int mi = (int)blockIdx.x * CDA_WPB + wave;
    zig_tables_init();
    dec_tables_init();
    if (mi >= K.P.n_markets) return;
    double ret = 0.0;
    int steps = 0;
    int it = run_random_part<false, TALLY ? 1 : 0>(K.arena, K.P, K.R, mi, wave, lane, 0, ret, steps);
    if (it >= 0) {                                           // the book may outgrow its tile: the general build plays the rest
        tail_fence();                                        // (it starts from the record this wave has just written)
        it = slow_run_random((const RunKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave, it, steps, ret);
    }
    if (__builtin_expect(it == -2, 0)) {                     // episode metrics: the launch ended this market's episode
        tail_fence();                                        // (the summary reads the header just written)
        const RunKernArgs* ka = (const RunKernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        episode_summarise(ka->arena, &ka->P, mi, &wave_lds(ka->P, wave, ZIG_LDS_BYTES).acc[0]);
    }
}

// k_run_random with the trade tape (cda_tape_enable); the tallies by the market's ST_EP_ON bit, as in k_tstep
__attribute__((noinline, cold)) __device__ int slow_tape_run(const TRunKernArgs* kernargs, int mi, int wave, int it0, int steps, double ret) {
    const TRunKernArgs& KT = *kernargs;
    return run_random_part<true, 2, true>(KT.K.arena, KT.K.P, KT.K.R, mi, wave, lane_id(), it0, ret, steps, &KT.T);
}
__global__ __launch_bounds__(64 * CDA_WPB, CDA_MIN_WAVES) CDA_VGPR_CAP_ATTR void k_tape_run(TRunKernArgs KT) {
    int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
    int mi = (int)blockIdx.x * CDA_WPB + wave;
    zig_tables_init();
    dec_tables_init();
    if (mi >= KT.K.P.n_markets) return;
    double ret = 0.0;
    int steps = 0;
    int it = run_random_part<false, 2, true>(KT.K.arena, KT.K.P, KT.K.R, mi, wave, lane, 0, ret, steps, &KT.T);
    if (it >= 0) {
        tail_fence();
        it = slow_tape_run((const TRunKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), mi, wave, it, steps, ret);
    }
    if (__builtin_expect(it == -2, 0)) {
        tail_fence();
        const RunKernArgs* ka = (const RunKernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        episode_summarise(ka->arena, &ka->P, mi, &wave_lds(ka->P, wave, ZIG_LDS_BYTES).acc[0]);
    }
}

// ------------------------------------------------------------------------------------------
// test hooks and small kernels
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_place_order(uint8_t* arena, Params P, int mi, int tr, int type, int side, int size, int price) {
    Lds& lds1 = wave_lds(P, 0);
    int lane = lane_id();
    dec_tables_init();
    MarketPtrs mp = market_ptrs(arena, P, mi);
    Mkt m;
    load_market(mp, P, lds1, m, lane);
    place_order<true, false>(lds1, m, tr, type, side, size, price, lane);
    m.status &= ~ST_LEVELS_VALID;                         // the cached aggregation no longer describes the book
    store_market(mp, P, lds1, m, lane);
}
__global__ __launch_bounds__(64) void k_tape_place_order(uint8_t* arena, Params P, int mi, int tr, int type, int side, int size, int price, TapeArgs T) {
    Lds& lds1 = wave_lds(P, 0);
    int lane = lane_id();
    dec_tables_init();
    MarketPtrs mp = market_ptrs(arena, P, mi);
    Mkt m;
    load_market(mp, P, lds1, m, lane);
    tape_begin(T, mi, m);
    place_order<true, false, true>(lds1, m, tr, type, side, size, price, lane);
    tape_finish(T, mi, m, false, lane);
    m.status &= ~ST_LEVELS_VALID;
    store_market(mp, P, lds1, m, lane);
}
__global__ __launch_bounds__(64) void k_mark_to_mkt(uint8_t* arena, Params P, int mi) {
    Lds& lds1 = wave_lds(P, 0);
    int lane = lane_id();
    dec_tables_init();
    MarketPtrs mp = market_ptrs(arena, P, mi);
    Mkt m;
    load_market(mp, P, lds1, m, lane);
    mark_to_mkt(lds1, m, P.cfg.num_agents, lane);
    store_market(mp, P, lds1, m, lane);
}
__global__ __launch_bounds__(64 * CDA_WPB) void k_raw_snapshot(uint8_t* arena, Params P, float* raw_out) {
    int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();   // wave index pinned to an SGPR: market pointers and counts become scalar
    int mi = (int)blockIdx.x * CDA_WPB + wave;
    if (mi >= P.n_markets) return;
    Lds& L = wave_lds(P, wave);
    MarketPtrs mp = market_ptrs(arena, P, mi);
    Mkt m;
    load_header(mp.hdr, m, lane);
    load_book(mp.book, L.book, m, lane);
    load_tail_meta(mp, P, L, m, lane);
    CDA_WSYNC();
    aggregate_levels<true>(L, m, lane);
    if (lane < CDA_RAW_DIM) raw_out[(size_t)mi * CDA_RAW_DIM + (size_t)lane] = raw_value(L, lane);
}
#if CDA_CAP == 256
// ------------------------------------------------------------------------------------------
// k_net_step - k_policy_step for every OTHER network the project trains (fcnet_activation relu / elu / linear, and vf_share_layers with any activation)
// ------------------------------------------------------------------------------------------
// The body file of k_policy_step once more: one instance per history depth, the hidden activation (csrc/cda_mlp_dev.inc ActT<> code) and the trunk chosen at run time
// by two scalars of its arguments, both uniform branches inside the forward (forward16_net: the activation in the two hidden-layer epilogues, never around the MFMA
// layers; a shared trunk idles waves 8 .. 15 through the forward).  One kernel per (activation, trunk) pair would be 7 x 14 more instances in a translation unit
// that compiles serially.  Everything behind the forward is k_policy_step's code.  The scalars live in a struct of their own behind PolicyArgs: k_policy_step's
// arguments keep their size.  (Defined behind every other kernel of the tile: the existing kernels then come out of the compiler instruction for instruction as before.)
struct NetArgs { int32_t activation; int32_t shared_trunk; };
struct NetStepKernArgs { StepKernArgs K; PolicyArgs F; NetArgs N; };      // K first, as in PolicyStepKernArgs
#define PS_NS CDA_HIST_SFX(mlpdev)
#define PS_NAME(x) CDA_HIST_SFX(x)
#define CDA_HIST_BODY "cda_policy_step.inc"
#define CDA_HIST_OPEN
#define CDA_HIST_CLOSE
#define PS_NET 1
#define PS_KERNEL k_net_step
#define PS_KERNARGS NetStepKernArgs
#include "cda_hist_variants.inc"
#undef PS_NET
#undef PS_KERNEL
#undef PS_KERNARGS
#undef CDA_HIST_BODY
#undef CDA_HIST_OPEN
#undef CDA_HIST_CLOSE
#undef PS_NS
#undef PS_NAME
#endif
} }  // namespace cda::CDA_CAPNS
