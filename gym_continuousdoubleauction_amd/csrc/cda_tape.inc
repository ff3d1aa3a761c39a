// cda_tape.inc - the trade tape's storage and read-out (include/cda.h cda_tape_*), included at the end of cda_hip.hip (the wave toolkit: cda_wave.hpp, ahead of
// every .inc).  The record's layout as the readers see it - tape_load and the tape_* accessors - stands beside TapeSpan below.
//
// The reference's order book keeps OrderBook.tape: one transaction_record per fill (orderbook.py:108-140).  Here a market's tape is a ring of
// `capacity` records (CDA_TAPE_WORDS int32 each, cda_tape_record) in a buffer of its own, beside the arena: neither the market record, nor the state
// dump, nor the snapshot blob know of it.  The WRITERS are the tape instances of the market-wave kernels (cda_kernels.inc k_tstep, k_tape_run,
// k_tape_place_order: match<.., TAPE = true> stores the record at the point of the fill); an env launches them instead of k_step / k_run_random /
// k_place_order while its tape is on, and never otherwise.  Per market, TapeMeta (cda_market.hpp): n_total, n_episode, episode, partial.
//
//   reset (cda_reset*, the auto-reset pass behind a step with info tensors: k_tape_episode behind k_reset, same mask; the in-kernel auto reset:
//   tape_finish)                    n_prev = n_episode, n_episode = 0, episode += 1, partial = 0.  The ring is NOT cleared: the episode that just ended
//                                   stays readable, and n_prev says where it lies (tape_span below).
//   cda_snapshot_restore            n_episode = 0, n_prev = 0, partial = 1 (the blob carries no tape: what follows is an episode's tail).
// The reductions over an episode's records (price / volume bars, agent-to-agent flows) are in cda_tape_bars.inc.
//
// The readers below are one thread per market (counts), one workgroup (the offset scan) or one wave per market (the copies: a record is two 16-byte
// words, lane l moves word l of the market's run - contiguous in the ring up to its wrap, contiguous in the output).

static_assert(sizeof(cda_tape_record) == CDA_TAPE_WORDS * 4 && sizeof(cda_tape_record) == 32, "cda_tape_record layout");

__global__ __launch_bounds__(256) void k_tape_episode(TapeMeta* meta, const uint8_t* mask, int first, int end) {
    const int mi = first + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (mi >= end || (mask && !mask[mi])) return;
    meta[mi].n_prev = meta[mi].n_episode; meta[mi].prev_partial = meta[mi].partial;
    meta[mi].n_episode = 0; meta[mi].episode += 1; meta[mi].partial = 0;
}
__global__ __launch_bounds__(256) void k_tape_partial(TapeMeta* meta, int first, int end) {
    const int mi = first + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (mi >= end) return;
    meta[mi].n_episode = 0; meta[mi].partial = 1; meta[mi].n_prev = 0; meta[mi].prev_partial = 0;
}
__global__ __launch_bounds__(256) void k_tape_counts(const TapeMeta* meta, int n, long long* n_total, int32_t* n_episode, int32_t* episode, int32_t* partial, int32_t* n_prev) {
    const int mi = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (mi >= n) return;
    const TapeMeta h = meta[mi];
    if (n_total) n_total[mi] = h.n_total;
    if (n_episode) n_episode[mi] = h.n_episode;
    if (episode) episode[mi] = h.episode;
    if (partial) partial[mi] = h.partial;
    if (n_prev) n_prev[mi] = h.n_prev;
}

// what market mi still holds of [cursor, n_total): the ring keeps the last `cap` records
struct TapeRun { long long start, count, dropped; };
__device__ __forceinline__ TapeRun tape_run(const TapeMeta* meta, uint32_t cap, int mi, long long cursor) {
    const long long total = meta[mi].n_total;
    if (cursor < 0) cursor = 0;
    if (cursor > total) cursor = total;
    TapeRun r;
    r.count = total - cursor; r.dropped = 0;
    if (r.count > (long long)cap) { r.dropped = r.count - (long long)cap; r.count = (long long)cap; }
    r.start = total - r.count;
    return r;
}
// count + scan: ONE workgroup (the scheme of k_snap_offsets)
constexpr int TAPE_SCAN_THREADS = 1024;
__global__ __launch_bounds__(TAPE_SCAN_THREADS) void k_tape_offsets(const TapeMeta* meta, uint32_t cap, int first, int n, const long long* cursor, long long* off, long long* dropped) {
    __shared__ long long part[TAPE_SCAN_THREADS];
    const int t = (int)threadIdx.x, chunk = (n + TAPE_SCAN_THREADS - 1) / TAPE_SCAN_THREADS;
    const int lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    long long s = 0;
    for (int i = lo; i < hi; i++) s += tape_run(meta, cap, first + i, cursor[i]).count;
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < TAPE_SCAN_THREADS; d <<= 1) {
        const long long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = t > 0 ? part[t - 1] : 0;
    for (int i = lo; i < hi; i++) {
        const TapeRun r = tape_run(meta, cap, first + i, cursor[i]);
        off[i] = run; run += r.count;
        if (dropped) dropped[i] = r.dropped;
    }
    if (t == TAPE_SCAN_THREADS - 1) off[n] = part[t];
}
// `count` records from ring index `start` on (mod cap) -> dst, 16 bytes per lane and pass
__device__ __forceinline__ void tape_copy(uint4* dst, const uint4* ring, uint32_t cap, long long start, long long count, int lane) {
    const uint32_t mask = cap - 1u, s0 = (uint32_t)start & mask;
    for (long long w = lane; w < 2 * count; w += WAVE) {
        const uint32_t slot = (s0 + (uint32_t)(w >> 1)) & mask;
        dst[w] = ring[2 * (size_t)slot + (size_t)(w & 1)];
    }
}
// pack: wave k <- market first + k; a market whose run does not fit below out_records is left alone (its cursor too)
__global__ __launch_bounds__(64 * CDA_WPB) void k_tape_pack(TapeArgs T, int first, int n, long long* cursor, const long long* off, uint4* out, long long out_records) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w;
    const TapeRun r = tape_run(T.meta, T.cap, mi, cursor[w]);
    const long long o = off[w];
    if (o < 0 || o + r.count > out_records || off[w + 1] - o != r.count) return;
    tape_copy(out + 2 * o, T.ring + (size_t)mi * (size_t)T.cap * 2, T.cap, r.start, r.count, lane);
    if (lane == 0) cursor[w] = r.start + r.count;
}
// One of the two episodes a market remembers, in record numbers: the current one is [n_total - n_episode, n_total), the previous one (the episode that ended at
// the market's last reset) the n_prev records before it; `start` / `count`: what the ring still holds of it (the ring keeps [n_total - cap, n_total)), `lost`: the
// records of its head that are already overwritten, `partial`: its head was never recorded (the market had been restored from a snapshot).
struct TapeSpan { long long start, count, lost; int partial; };
__device__ __forceinline__ TapeSpan tape_span(const TapeMeta& h, uint32_t cap, int which) {
    long long hi = h.n_total - (which == CDA_TAPE_PREVIOUS ? (long long)h.n_episode : 0ll);
    long long lo = hi - (long long)(which == CDA_TAPE_PREVIOUS ? h.n_prev : h.n_episode);
    if (lo < 0) lo = 0;
    if (hi < lo) hi = lo;
    long long floor = h.n_total - (long long)cap;
    if (floor < lo) floor = lo;
    if (floor > hi) floor = hi;
    TapeSpan s;
    s.start = floor; s.count = hi - floor; s.lost = floor - lo; s.partial = which == CDA_TAPE_PREVIOUS ? h.prev_partial : h.partial;
    return s;
}
// THE LAYOUT OF A RECORD, as the readers see it: two 16-byte words r0, r1 of the ring = cda_tape_record (include/cda.h).  The writer is match<.., TAPE = true>
// (cda_book.inc); every reader decodes through the accessors below and nowhere else.  They are MACROS on purpose: an inlined function hands the optimiser facts
// about its result (value ranges, noundef) that the hand-written decoders never had, and six reader kernels then compiled to other code than their parent's;
// as text substitution every reader is instruction for instruction what it was (profiles/readers/identity.txt).  Being macros, they may evaluate an argument
// more than once, and tape_load ASSIGNS to its last two arguments: pass plain variables (r0, r1, a ring element), never an expression with side effects.
static_assert(offsetof(cda_tape_record, price) == 4 && offsetof(cda_tape_record, quantity) == 8 && offsetof(cda_tape_record, counter_id) == 12,
              "r0 = (time, price, quantity, counter_id)");
static_assert(offsetof(cda_tape_record, init_id) == 24 && offsetof(cda_tape_record, sides_step) == 28, "r1 = (counter_order_id, counter_left, init_id, sides_step)");
// Sides: 0 = bid (bought), 1 = ask (sold); counter_id: the resting order's trader (maker), init_id: the incoming order's (taker); a self-trade has both equal.
#define tape_price(r0) ((int32_t)(r0).y)
#define tape_qty(r0) ((int32_t)(r0).z)
#define tape_counter_id(r0) ((r0).w)
#define tape_init_id(r1) ((r1).z)
#define tape_self(r0, r1) ((r0).w == (r1).z)
#define tape_counter_side(r1) ((int)((r1).w & 1u))
#define tape_init_side(r1) ((int)(((r1).w >> 1) & 1u))
#define tape_step(r1) ((r1).w >> 2)
// ... and of the raw sides_step word (r1.w), for a kernel that keeps the word itself (k_tape_signs)
#define tape_stepw(w) ((w) >> 2)
#define tape_init_sells(w) (((w) & 2u) != 0u)
// r0, r1 <- record s0 + idx of the ring (slot masked: the run wraps where the ring does); a lane without a record (`in` false) gets zeros
#define tape_load(ring, mask, s0, idx, in, r0, r1) do { \
        r0 = make_uint4(0u, 0u, 0u, 0u); r1 = r0; \
        if (in) { const uint32_t slot_ = ((s0) + (uint32_t)(idx)) & (mask); r0 = (ring)[2 * (size_t)slot_]; r1 = (ring)[2 * (size_t)slot_ + 1]; } \
    } while (0)
// the last k records of the current (or the previous) episode, oldest first; rows beyond the count are zero
__global__ __launch_bounds__(64 * CDA_WPB) void k_tape_last(TapeArgs T, int first, int n, int which, int kmax, uint4* out, int32_t* counts) {
    READER_WAVE();
    if (w >= n) return;
    const int mi = first + w;
    const TapeMeta h = T.meta[mi];
    const TapeSpan sp = tape_span(h, T.cap, which);
    const long long cnt = sp.count > (long long)kmax ? (long long)kmax : sp.count;
    uint4* dst = out + 2 * (size_t)w * (size_t)kmax;
    tape_copy(dst, T.ring + (size_t)mi * (size_t)T.cap * 2, T.cap, sp.start + sp.count - cnt, cnt, lane);
    for (long long i = 2 * cnt + lane; i < 2 * (long long)kmax; i += WAVE) dst[i] = make_uint4(0u, 0u, 0u, 0u);
    if (counts && lane == 0) counts[w] = (int32_t)cnt;
}

// a reset of [first, first + n) under `mask` (NULL = all) has been queued on `stream`: the tape's counters follow it
static int tape_after_reset(cda_env* e, int32_t first, int32_t n, const uint8_t* mask, hipStream_t stream) {
    if (!e->tape.ring) return CDA_OK;
    launch_1d(k_tape_episode, n, 256, 0, stream, e->tape.meta, mask, (int)first, (int)(first + n));
    return launch_status();
}
static int tape_after_restore(cda_env* e, int32_t first, int32_t n, hipStream_t stream) {
    if (!e->tape.ring) return CDA_OK;
    launch_1d(k_tape_partial, n, 256, 0, stream, e->tape.meta, (int)first, (int)(first + n));
    return launch_status();
}
static void tape_free(cda_env* e) {
    if (e->tape.ring) (void)hipFree(e->tape.ring);
    if (e->tape.meta) (void)hipFree(e->tape.meta);
    memset(&e->tape, 0, sizeof e->tape);
}

extern "C" {

int cda_tape_enable(cda_env* e, int64_t capacity_records) {
    if (!e || capacity_records < 0 || capacity_records > CDA_TAPE_CAP_MAX || (capacity_records & (capacity_records - 1)) != 0) return CDA_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    tape_free(e);
    if (capacity_records == 0) return CDA_OK;
    const size_t n = (size_t)e->P.n_markets;
    DevBuf<uint4> ring; DevBuf<TapeMeta> meta;
    if (ring.alloc(n * (size_t)capacity_records * sizeof(cda_tape_record)) != hipSuccess || meta.alloc(n * sizeof(TapeMeta)) != hipSuccess) { (void)hipGetLastError(); return CDA_ERR_NOMEM; }
    hipError_t he = hipMemset(ring, 0, n * (size_t)capacity_records * sizeof(cda_tape_record));
    if (he == hipSuccess) he = hipMemset(meta, 0, n * sizeof(TapeMeta));
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he != hipSuccess) return hip_fail(he, "cda_tape_enable");
    e->tape.ring = ring.release(); e->tape.meta = meta.release(); e->tape.cap = (uint32_t)capacity_records; e->tape.pad = 0;
    return CDA_OK;
}
int64_t cda_tape_capacity(const cda_env* e) { return e && e->tape.ring ? (int64_t)e->tape.cap : 0; }

int cda_tape_counts_ex(cda_env* e, int64_t* n_total_dev, int32_t* n_episode_dev, int32_t* episode_dev, int32_t* partial_dev, int32_t* n_previous_dev, void* stream) {
    if (!e) return CDA_ERR_INVALID;
    if (!e->tape.ring) return CDA_ERR_UNSUPPORTED;
    HIPCHK(hipSetDevice(e->device));
    launch_1d(k_tape_counts, e->P.n_markets, 256, 0, (hipStream_t)stream, (const TapeMeta*)e->tape.meta, (int)e->P.n_markets,
                       (long long*)n_total_dev, n_episode_dev, episode_dev, partial_dev, n_previous_dev);
    return launch_status();
}
int cda_tape_counts(cda_env* e, int64_t* n_total_dev, int32_t* n_episode_dev, int32_t* episode_dev, int32_t* partial_dev, void* stream) {
    return cda_tape_counts_ex(e, n_total_dev, n_episode_dev, episode_dev, partial_dev, NULL, stream);
}
int cda_tape_offsets(cda_env* e, int32_t first_market, int32_t n_markets, const int64_t* cursor_dev, int64_t* offsets_dev, int64_t* dropped_dev, void* stream) {
    if (!e || !cursor_dev || !offsets_dev || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->tape.ring) return CDA_ERR_UNSUPPORTED;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_tape_offsets, dim3(1), dim3(TAPE_SCAN_THREADS), 0, (hipStream_t)stream, (const TapeMeta*)e->tape.meta, e->tape.cap, (int)first_market, (int)n_markets,
                       (const long long*)cursor_dev, (long long*)offsets_dev, (long long*)dropped_dev);
    return launch_status();
}
int cda_tape_pack(cda_env* e, int32_t first_market, int32_t n_markets, int64_t* cursor_dev, const int64_t* offsets_dev, void* records_out_dev, int64_t capacity_records,
                  void* stream) {
    if (!reader_args_ok(e, cursor_dev, first_market, n_markets) || !offsets_dev || capacity_records < 0 || (capacity_records > 0 && !records_out_dev) ||
        !aligned(records_out_dev, 16) || !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->tape.ring) return CDA_ERR_UNSUPPORTED;
    return reader_launch(e, k_tape_pack, n_markets, CDA_WPB, 0, stream, e->tape, (int)first_market, (int)n_markets, (long long*)cursor_dev, (const long long*)offsets_dev,
                         (uint4*)records_out_dev, (long long)capacity_records);
}
int cda_tape_last_of(cda_env* e, int32_t first_market, int32_t n_markets, int32_t which, int32_t k, void* records_out_dev, int32_t* counts_out_dev, void* stream) {
    if (!reader_args_ok(e, records_out_dev, first_market, n_markets) || k < 1 || !which_ok(which) || !aligned(records_out_dev, 16) ||
        !range_ok(e, first_market, n_markets)) return CDA_ERR_INVALID;
    if (!e->tape.ring) return CDA_ERR_UNSUPPORTED;
    return reader_launch(e, k_tape_last, n_markets, CDA_WPB, 0, stream, e->tape, (int)first_market, (int)n_markets, (int)which, (int)k, (uint4*)records_out_dev, counts_out_dev);
}
int cda_tape_last(cda_env* e, int32_t first_market, int32_t n_markets, int32_t k, void* records_out_dev, int32_t* counts_out_dev, void* stream) {
    return cda_tape_last_of(e, first_market, n_markets, CDA_TAPE_CURRENT, k, records_out_dev, counts_out_dev, stream);
}

}  // extern "C"
