// cda_snapshot.inc - device snapshot / restore of a market range (include/cda.h cda_snapshot_*), included at the end of cda_hip.hip.
//
// A market's state between two launches is its record (header words with the PCG64 state, accounts, history frames, the book tile in its physical
// layout, the running episode tallies), its done_buf byte, its rows of the episode-metric accumulators and - for a side whose ST_TAIL bit is set -
// the ring header words and the LIVE window [base, base + n) mod spill_cap of the side's four field arrays.  The ring pointer and capacity (L.tl,
// rebuilt by load_tail_meta at every launch), the hand-back records and em_partials are not state.  The blob holds no address: a market's section
// can be unpacked into any market of any env with the same numeric config, tile, history depth, agent count and metrics setting.
//
//   blob = [cda_snapshot_header: 256 B][i64 offsets[n + 1], zero padded to 256 B][section 0][section 1] ...       (offsets[n] = total bytes)
//   section = [record: stride B][SnapMeta: 32 B][f64 em_agent[A][CDA_EM_AGENT_FIELDS]][f64 em_env[CDA_EM_ENV_FIELDS]]
//             [i32 window of side 0: 4 fields x n0][i32 window of side 1: 4 fields x n1], zero padded to 256 B
//
// Three kernels, one wave64 per market in the two that move bytes: k_snap_offsets (one workgroup: per-market sizes from the header and status words,
// scanned into the offset table), k_snap_pack, k_snap_restore (after k_snap_check has vetted every section it will read).  Records are 256-B aligned
// and so are the sections: the record and the metric rows move as 16-B per-lane accesses; a ring window is at most two contiguous runs per field.
// Nothing here touches the step kernels.

struct SnapMeta {                    // 32 B behind the record in a section
    uint32_t done;                   // the market's done_buf byte
    uint32_t tail_bits;              // H_STATUS & ST_TAIL_ANY when packed
    int32_t n[2];                    // live ring orders per side (0 for a side whose tail bit is clear); -1: the packed state was inconsistent (restore refuses it)
    int32_t base[2];                 // ring slot of each side's first tail order in the source ring
    int32_t spill_cap;               // the source ring's capacity
    uint32_t pad;
};
static_assert(sizeof(SnapMeta) == 32, "SnapMeta layout");
static_assert(sizeof(cda_snapshot_header) == 256, "cda_snapshot_header layout");

__host__ __device__ static inline int64_t snap_table_bytes(int64_t n) { return 256 + ((8 * (n + 1) + 255) & ~(int64_t)255); }
__host__ __device__ static inline int64_t snap_fixed_bytes(const Params& P) {      // a section without its ring window
    return (int64_t)P.lay.stride + (int64_t)sizeof(SnapMeta) + (int64_t)P.cfg.num_agents * CDA_EM_AGENT_FIELDS * 8 + CDA_EM_ENV_FIELDS * 8;
}
__host__ __device__ static inline int64_t snap_section_bytes(const Params& P, int n0, int n1) {
    return (snap_fixed_bytes(P) + 16 * (int64_t)(n0 + n1) + 255) & ~(int64_t)255;
}
// the live window of both sides of market mi as the kernels will see it: n < 0 = inconsistent (counted as empty, poisoned in the blob)
struct SnapTail { uint32_t bits; int32_t n[2], base[2]; bool bad; };
__device__ __forceinline__ SnapTail snap_tail(const uint8_t* arena, const Params& P, int mi) {
    SnapTail t;
    t.bits = reinterpret_cast<const uint32_t*>(arena + (size_t)mi * (size_t)P.lay.stride)[H_STATUS] & (uint32_t)ST_TAIL_ANY;
    t.n[0] = t.n[1] = 0; t.base[0] = t.base[1] = 0; t.bad = false;
    if (P.lay.spill_cap > 0 && t.bits) {
        const int32_t* sp = reinterpret_cast<const int32_t*>(arena + spill_arena_off(P) + (size_t)mi * spill_region_bytes(P.lay.spill_cap));
        for (int sd = 0; sd < 2; sd++) {
            t.base[sd] = sp[2 + sd];
            if (t.bits & (uint32_t)(ST_TAIL_BID << sd)) {
                const int32_t n = sp[sd];
                if (n < 0 || n > P.lay.spill_cap) t.bad = true; else t.n[sd] = n;
            }
        }
    } else if (t.bits) t.bad = true;                                 // (a tail bit in an env without the HBM tier)
    return t;
}

// count + scan: ONE workgroup; thread t sizes the markets of its chunk, a Hillis-Steele scan of the chunk sums gives its first offset
constexpr int SNAP_SCAN_THREADS = 1024;
__global__ __launch_bounds__(SNAP_SCAN_THREADS) void k_snap_offsets(const uint8_t* arena, Params P, int first, int n, long long* off) {
    __shared__ long long part[SNAP_SCAN_THREADS];
    const int t = (int)threadIdx.x, chunk = (n + SNAP_SCAN_THREADS - 1) / SNAP_SCAN_THREADS;
    const int lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    long long s = 0;
    for (int i = lo; i < hi; i++) { const SnapTail tl = snap_tail(arena, P, first + i); s += snap_section_bytes(P, tl.n[0], tl.n[1]); }
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < SNAP_SCAN_THREADS; d <<= 1) {
        const long long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = snap_table_bytes(n) + (t > 0 ? part[t - 1] : 0);
    for (int i = lo; i < hi; i++) { const SnapTail tl = snap_tail(arena, P, first + i); off[i] = run; run += snap_section_bytes(P, tl.n[0], tl.n[1]); }
    if (t == SNAP_SCAN_THREADS - 1) off[n] = snap_table_bytes(n) + part[t];
}

// blob stores: plain by default; -DCDA_SNAP_NT_STORES=1 (a variant build) makes them nt, for measuring the two flavours against each other
#ifndef CDA_SNAP_NT_STORES
#define CDA_SNAP_NT_STORES 0
#endif
typedef uint32_t snap_u32x4 __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ void snap_st16(void* dst, const snap_u32x4& v) {
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<snap_u32x4*>(dst)); else *reinterpret_cast<snap_u32x4*>(dst) = v;
}
template <bool NT> __device__ __forceinline__ void snap_st4(int32_t* dst, int32_t v) { if (NT) __builtin_nontemporal_store(v, dst); else *dst = v; }
// nbytes % 16 == 0, both 16-B aligned: 1 KB per wave instruction
template <bool NT> __device__ __forceinline__ void snap_copy16(void* dst, const void* src, int64_t nbytes, int lane) {
    const snap_u32x4* s = reinterpret_cast<const snap_u32x4*>(src);
    uint8_t* d = reinterpret_cast<uint8_t*>(dst);
    const int64_t n16 = nbytes >> 4;
    #pragma unroll 4
    for (int64_t i = lane; i < n16; i += WAVE) snap_st16<NT>(d + 16 * i, s[i]);
}

// pack: wave k <- market first + k.  The header words come by value (the host fills them); wave 0 writes them and the table's padding.
struct SnapPackArgs { cda_snapshot_header hdr; };
template <bool NT>
__global__ __launch_bounds__(64 * CDA_WPB) void k_snap_pack(const uint8_t* arena, Params P, int first, int n, const long long* off, uint8_t* blob, long long blob_bytes, SnapPackArgs A) {
    const int k = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = (int)(threadIdx.x & 63);
    if (k >= n) return;
    long long* table = reinterpret_cast<long long*>(blob + 256);
    if (k == 0) {
        const uint64_t total = (uint64_t)off[n];            // header words 4, 5: total_bytes, as the offset pass found it
        const uint32_t w = lane == 4 ? (uint32_t)total : (lane == 5 ? (uint32_t)(total >> 32) : reinterpret_cast<const uint32_t*>(&A.hdr)[lane]);
        reinterpret_cast<uint32_t*>(blob)[lane] = w;
        const int64_t tb = snap_table_bytes(n);
        for (int64_t b = 8 * (int64_t)(n + 1) + 4 * lane; b < tb - 256; b += 4 * WAVE) *reinterpret_cast<uint32_t*>(blob + 256 + b) = 0u;
        if (lane == 0) table[n] = off[n];
    }
    const long long o0 = off[k], o1 = off[k + 1];
    if (lane == 0) table[k] = o0;
    const int mi = first + k;
    const SnapTail tl = snap_tail(arena, P, mi);
    const int64_t fixed = snap_fixed_bytes(P), need = snap_section_bytes(P, tl.n[0], tl.n[1]);
    if (o0 < 0 || (o0 & 255) != 0 || o1 > blob_bytes || o1 - o0 < snap_section_bytes(P, 0, 0)) return;        // (an offset table this env did not produce)
    const bool bad = tl.bad || need != o1 - o0;                     // the state moved between the two passes: the section is poisoned, restore refuses it
    uint8_t* sec = blob + o0;
    snap_copy16<NT>(sec, arena + (size_t)mi * (size_t)P.lay.stride, P.lay.stride, lane);
    if (lane < 8) {
        SnapMeta m;
        m.done = reinterpret_cast<const uint8_t*>(arena + (size_t)P.n_markets * (size_t)P.lay.stride)[mi];
        m.tail_bits = tl.bits; m.n[0] = bad ? -1 : tl.n[0]; m.n[1] = bad ? -1 : tl.n[1]; m.base[0] = tl.base[0]; m.base[1] = tl.base[1];
        m.spill_cap = P.lay.spill_cap; m.pad = 0u;
        snap_st4<NT>(reinterpret_cast<int32_t*>(sec + P.lay.stride) + lane, reinterpret_cast<const int32_t*>(&m)[lane]);
    }
    const int64_t em_a = (int64_t)P.cfg.num_agents * CDA_EM_AGENT_FIELDS * 8;
    snap_copy16<NT>(sec + P.lay.stride + sizeof(SnapMeta), arena + em_agent_off(P) + (size_t)mi * (size_t)em_a, em_a, lane);
    snap_copy16<NT>(sec + P.lay.stride + sizeof(SnapMeta) + em_a, arena + em_env_off(P) + (size_t)mi * CDA_EM_ENV_FIELDS * 8, CDA_EM_ENV_FIELDS * 8, lane);
    int32_t* win = reinterpret_cast<int32_t*>(sec + fixed);
    if (!bad && (tl.n[0] | tl.n[1])) {
        const int32_t* ring = reinterpret_cast<const int32_t*>(arena + spill_arena_off(P) + (size_t)mi * spill_region_bytes(P.lay.spill_cap)) + 16;
        const uint32_t cap = (uint32_t)P.lay.spill_cap;
        for (int sd = 0; sd < 2; sd++) {
            const int nn = tl.n[sd];
            const uint32_t b0 = (uint32_t)tl.base[sd] & (cap - 1u);
            for (int f = 0; f < BOOK_FIELDS; f++) {                 // slots b0 .. cap - 1, then 0 ..: two contiguous runs
                const int32_t* src = ring + (size_t)(sd * BOOK_FIELDS + f) * cap;
                #pragma unroll 4
                for (int i = lane; i < nn; i += WAVE) snap_st4<NT>(win + i, src[(b0 + (uint32_t)i) & (cap - 1u)]);
                win += nn;
            }
        }
    }
    // zero padding to the section's end (deterministic bytes: two snapshots of one state are equal)
    uint8_t* pad0 = reinterpret_cast<uint8_t*>(win);
    for (uint8_t* p = pad0 + 4 * lane; p < sec + (o1 - o0); p += 4 * WAVE) *reinterpret_cast<uint32_t*>(p) = 0u;
}

// restore, step 1: every section the restore will read is vetted (thread per market); *bad |= 1 on anything the kernels could not take as it is
__global__ void k_snap_check(const uint8_t* blob, long long blob_bytes, int src_first, int n, Params P, int cap, uint32_t* bad) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= n) return;
    const long long* table = reinterpret_cast<const long long*>(blob + 256);
    const long long o0 = table[src_first + k], o1 = table[src_first + k + 1];
    const cda_snapshot_header* h = reinterpret_cast<const cda_snapshot_header*>(blob);
    bool ok = o0 >= snap_table_bytes(h->n_markets) && (o0 & 255) == 0 && o1 > o0 && o1 <= blob_bytes && o1 - o0 >= snap_section_bytes(P, 0, 0);
    if (ok) {
        const uint8_t* sec = blob + o0;
        const SnapMeta* m = reinterpret_cast<const SnapMeta*>(sec + P.lay.stride);
        const uint32_t* rh = reinterpret_cast<const uint32_t*>(sec);
        for (int sd = 0; sd < 2; sd++) {
            const bool has = (m->tail_bits & (uint32_t)(ST_TAIL_BID << sd)) != 0;
            ok = ok && m->n[sd] >= 0 && m->n[sd] <= P.lay.spill_cap && (has || m->n[sd] == 0);
        }
        ok = ok && (m->tail_bits & ~(uint32_t)ST_TAIL_ANY) == 0 && (rh[H_STATUS] & (uint32_t)ST_TAIL_ANY) == m->tail_bits && m->spill_cap >= 0;
        ok = ok && (m->tail_bits == 0 || P.lay.spill_cap > 0);
        ok = ok && snap_section_bytes(P, ok ? m->n[0] : 0, ok ? m->n[1] : 0) == o1 - o0;
        ok = ok && (int)rh[H_N_BIDS] >= 0 && (int)rh[H_N_ASKS] >= 0 && (int64_t)rh[H_N_BIDS] + (int64_t)rh[H_N_ASKS] <= cap && rh[H_HIST_HEAD] < (uint32_t)P.cfg.n_hist;
        ok = ok && ((rh[H_STATUS] & (uint32_t)ST_EP_ON) != 0) == (P.lay.ep_on != 0);
    }
    if (!ok) atomicOr(bad, 1u);
}

// restore, step 2: wave k -> market dst_first + k from section src_first + k.  keep_base: the rings have equal capacities - the window goes back
// where it was; otherwise it is rebased to slot 0.  The market's observation row is re-emitted from its history frames (oldest first from H_HIST_HEAD).
__global__ __launch_bounds__(64 * CDA_WPB) void k_snap_restore(uint8_t* arena, Params P, int dst_first, const uint8_t* blob, int src_first, int n, int keep_base, float* obs_out) {
    const int k = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = (int)(threadIdx.x & 63);
    if (k >= n) return;
    const long long* table = reinterpret_cast<const long long*>(blob + 256);
    const uint8_t* sec = blob + table[src_first + k];
    const int mi = dst_first + k;
    snap_copy16<false>(arena + (size_t)mi * (size_t)P.lay.stride, sec, P.lay.stride, lane);
    const SnapMeta* m = reinterpret_cast<const SnapMeta*>(sec + P.lay.stride);
    const SnapMeta mv = *m;
    if (lane == 0) (arena + (size_t)P.n_markets * (size_t)P.lay.stride)[mi] = (uint8_t)mv.done;
    const int64_t em_a = (int64_t)P.cfg.num_agents * CDA_EM_AGENT_FIELDS * 8;
    snap_copy16<false>(arena + em_agent_off(P) + (size_t)mi * (size_t)em_a, sec + P.lay.stride + sizeof(SnapMeta), em_a, lane);
    snap_copy16<false>(arena + em_env_off(P) + (size_t)mi * CDA_EM_ENV_FIELDS * 8, sec + P.lay.stride + sizeof(SnapMeta) + em_a, CDA_EM_ENV_FIELDS * 8, lane);
    if (mv.tail_bits && P.lay.spill_cap > 0) {
        int32_t* sp = reinterpret_cast<int32_t*>(arena + spill_arena_off(P) + (size_t)mi * spill_region_bytes(P.lay.spill_cap));
        const uint32_t cap = (uint32_t)P.lay.spill_cap;
        const int32_t base0 = keep_base ? mv.base[0] : 0, base1 = keep_base ? mv.base[1] : 0;       // (scalars: an indexed array would live in scratch)
        if (lane < 4) sp[lane] = lane == 0 ? mv.n[0] : (lane == 1 ? mv.n[1] : (lane == 2 ? base0 : base1));
        const int32_t* win = reinterpret_cast<const int32_t*>(sec + snap_fixed_bytes(P));
        int32_t* ring = sp + 16;
        #pragma unroll
        for (int sd = 0; sd < 2; sd++) {
            const int nn = sd ? mv.n[1] : mv.n[0];
            const uint32_t b0 = (uint32_t)(sd ? base1 : base0) & (cap - 1u);
            for (int f = 0; f < BOOK_FIELDS; f++) {
                int32_t* dst = ring + (size_t)(sd * BOOK_FIELDS + f) * cap;
                #pragma unroll 4
                for (int i = lane; i < nn; i += WAVE) dst[(b0 + (uint32_t)i) & (cap - 1u)] = win[i];
                win += nn;
            }
        }
    }
    if (obs_out && lane < CDA_SNAPSHOT_DIM) {
        const int H = P.cfg.n_hist, head = (int)reinterpret_cast<const uint32_t*>(sec)[H_HIST_HEAD];
        const float* hist = reinterpret_cast<const float*>(sec + P.lay.hist_off);
        float* o = obs_out + (size_t)mi * (size_t)(H * CDA_SNAPSHOT_DIM);
        for (int j = 0; j < H; j++) {
            int slot = head + j; if (slot >= H) slot -= H;
            o[j * CDA_SNAPSHOT_DIM + lane] = hist[slot * CDA_SNAPSHOT_DIM + lane];
        }
    }
}

extern "C" {

int64_t cda_snapshot_table_bytes(int32_t n_markets) { return n_markets >= 1 ? snap_table_bytes(n_markets) : 0; }

int cda_snapshot_offsets(cda_env* e, int32_t first_market, int32_t n_markets, int64_t* offsets_dev, void* stream) {
    if (!e || !offsets_dev || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_snap_offsets, dim3(1), dim3(SNAP_SCAN_THREADS), 0, (hipStream_t)stream, (const uint8_t*)e->arena, e->P, (int)first_market, (int)n_markets,
                       (long long*)offsets_dev);
    return launch_status();
}

int cda_snapshot_pack(cda_env* e, int32_t first_market, int32_t n_markets, const int64_t* offsets_dev, void* blob_dev, int64_t blob_bytes, void* stream) {
    if (!e || !offsets_dev || !blob_dev || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (((uintptr_t)blob_dev & 255) != 0 || blob_bytes < snap_table_bytes(n_markets)) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    SnapPackArgs A;
    memset(&A, 0, sizeof A);
    cda_snapshot_header& h = A.hdr;
    h.magic = CDA_SNAP_MAGIC; h.version = CDA_SNAP_VERSION;
    h.header_bytes = (int32_t)snap_table_bytes(n_markets); h.n_markets = n_markets; h.total_bytes = 0;      // (the kernel writes total_bytes)
    h.book_capacity = e->cap; h.record_stride = e->P.lay.stride; h.n_hist = e->P.cfg.n_hist; h.num_agents = e->P.cfg.num_agents;
    h.spill_cap = e->P.lay.spill_cap; h.episode_metrics_on = e->P.lay.ep_on; h.nav_tolerance = e->P.ep_tol;
    h.first_market = first_market; h.em_agent_fields = CDA_EM_AGENT_FIELDS; h.em_env_fields = CDA_EM_ENV_FIELDS; h.section_meta_bytes = (int32_t)sizeof(SnapMeta);
    h.cfg = e->P.cfg;
    const dim3 grid = grid_for(n_markets), block(64 * CDA_WPB);
    hipLaunchKernelGGL(k_snap_pack<CDA_SNAP_NT_STORES != 0>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)e->arena, e->P, (int)first_market, (int)n_markets,
                       (const long long*)offsets_dev, (uint8_t*)blob_dev, (long long)blob_bytes, A);
    return launch_status();
}

// the config fields that must agree (book_spill may differ: the window is rebased; book_capacity is compared as the tile the env got)
static void snap_norm_config(cda_config* c) { c->book_spill = 0; c->book_capacity = 0; }

int cda_snapshot_check_header(const cda_env* e, const cda_snapshot_header* h, int64_t blob_bytes) {
    if (!e || !h) return CDA_ERR_INVALID;
    if (h->magic != CDA_SNAP_MAGIC || h->version != CDA_SNAP_VERSION) return CDA_ERR_INVALID;
    if (h->n_markets < 1 || h->header_bytes != snap_table_bytes(h->n_markets) || h->total_bytes > blob_bytes || h->total_bytes < h->header_bytes) return CDA_ERR_INVALID;
    if (h->book_capacity != e->cap || h->record_stride != e->P.lay.stride || h->n_hist != e->P.cfg.n_hist || h->num_agents != e->P.cfg.num_agents) return CDA_ERR_INVALID;
    if (h->em_agent_fields != CDA_EM_AGENT_FIELDS || h->em_env_fields != CDA_EM_ENV_FIELDS || h->section_meta_bytes != (int32_t)sizeof(SnapMeta)) return CDA_ERR_INVALID;
    if ((h->episode_metrics_on != 0) != (e->P.lay.ep_on != 0) || (e->P.lay.ep_on && h->nav_tolerance != e->P.ep_tol)) return CDA_ERR_INVALID;
    cda_config a = h->cfg, b = e->P.cfg;
    snap_norm_config(&a); snap_norm_config(&b);
    if (memcmp(&a, &b, sizeof a) != 0) return CDA_ERR_INVALID;
    return CDA_OK;
}

int cda_snapshot_restore(cda_env* e, int32_t first_market, const void* blob_dev, int64_t blob_bytes, int32_t src_first, int32_t n_markets, float* obs_out, void* stream) {
    if (!e || !blob_dev || !range_ok(e, first_market, n_markets) || src_first < 0 || blob_bytes < 256 || ((uintptr_t)blob_dev & 255) != 0) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    const hipStream_t st = (hipStream_t)stream;
    cda_snapshot_header h;
    HIPCHK(hipMemcpyAsync(&h, blob_dev, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (cda_snapshot_check_header(e, &h, blob_bytes) != CDA_OK) return CDA_ERR_INVALID;
    if ((int64_t)src_first + (int64_t)n_markets > (int64_t)h.n_markets) return CDA_ERR_INVALID;
    if (!e->snap_flag) HIPCHK(hipMalloc((void**)&e->snap_flag, sizeof(uint32_t)));
    HIPCHK(hipMemsetAsync(e->snap_flag, 0, sizeof(uint32_t), st));
    launch_1d(k_snap_check, n_markets, 256, 0, st, (const uint8_t*)blob_dev, (long long)h.total_bytes, (int)src_first,
                       (int)n_markets, e->P, e->cap, e->snap_flag);
    HIPCHK(hipGetLastError());
    uint32_t bad = 1;
    HIPCHK(hipMemcpyAsync(&bad, e->snap_flag, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad) return CDA_ERR_INVALID;                      // nothing of the env has been written
    hipLaunchKernelGGL(k_snap_restore, grid_for(n_markets), dim3(64 * CDA_WPB), 0, st, e->arena, e->P, (int)first_market,
                       (const uint8_t*)blob_dev, (int)src_first, (int)n_markets, (int)(h.spill_cap == e->P.lay.spill_cap), obs_out);
    HIPCHK(hipGetLastError());
    return tape_after_restore(e, first_market, n_markets, st);      // (a blob carries no tape: the restored markets' records from here on are an episode's tail)
}

}  // extern "C"
