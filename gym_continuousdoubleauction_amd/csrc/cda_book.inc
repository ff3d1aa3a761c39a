// cda_book.inc - everything of a market-wave that depends on the BOOK CAPACITY: the pooled order book and its LDS image,
// matching, the ledger functions (they take the per-wave LDS image), the observation.  Included once per compiled
// capacity by cda_kernels.inc, inside `namespace cda { namespace CDA_CAPNS {` with CDA_CAP defined (256 or 512).
// No include guard on purpose.  Reference citations are relative to /root/reference/gym_continuousDoubleAuction/envs/.
constexpr int CAP = CDA_CAP;
// The two sides share ONE pool of CAP slots per field: bids grow up from slot 0, asks grow down from slot CAP-1
// (logical index i of the ask side lives in physical slot CAP-1-i).  Halves the LDS footprint of a market
// (4 KB), which is what lets more than 4 waves per SIMD be resident; capacity is CAP resting orders per market.
__host__ __device__ constexpr int book_phys(int s, int i) { return s == 0 ? i : CAP - 1 - i; }
struct BookField {
    int32_t v[CAP];
    struct Row { int32_t* base; int s; __device__ __forceinline__ int32_t& operator[](int i) const { return base[book_phys(s, i)]; } };
    struct CRow { const int32_t* base; int s; __device__ __forceinline__ const int32_t& operator[](int i) const { return base[book_phys(s, i)]; } };
    __device__ __forceinline__ Row operator[](int s) { return Row{v, s}; }
    __device__ __forceinline__ CRow operator[](int s) const { return CRow{v, s}; }
};
struct Book {                    // LDS image of the book, queue order per side (best first, FIFO in a level)
    BookField price, qty;
    BookField oo;                // (order_id << 4) | owner   (owner < 16, order_id < 2^27)
    BookField ts;
};
constexpr int BOOK_BYTES = sizeof(Book);   // 4096
// L.tl: [TL_N + s] orders of side s in its HBM ring, [TL_BASE + s] ring slot of the first of them, [TL_PTR_LO/HI] the market's
// spill region, [TL_CAP] ring slots per side (0 = this env has no HBM tier), [TL_ORD ..] one order read back from a ring
enum { TL_N = 0, TL_BASE = 2, TL_PTR_LO = 4, TL_PTR_HI = 5, TL_CAP = 6, TL_ORD = 8, TL_WORDS = 12 };
struct Lds {                     // per-wave LDS image; `acc` is sized for the env's agent count at launch
    Book book;
    int32_t lvl_px[2][CDA_K_ROWS];
    int32_t lvl_sz[2][CDA_K_ROWS];
    int32_t act_tsp[CDA_MAX_AGENTS];   // decoded order of agent a: type | side << 2 | (price + 1) << 4   (price < 2^24)
    int32_t act_size[CDA_MAX_AGENTS];
    int32_t tl[TL_WORDS];        // the market's HBM tier (below): ring counts / bases, where the ring lives, scratch of the cold routines
    Acc acc[CDA_MAX_AGENTS];     // only the first num_agents records are backed by LDS
};
// bytes of LDS one wave needs for `agents` accounts
// (the history ring of the observation, n_hist x 42 floats, is staged behind the accounts: lds_hist())
__host__ __device__ constexpr int lds_bytes_per_wave(int agents, int n_hist) {
    return (int)(sizeof(Book) + 2 * 2 * CDA_K_ROWS * 4 + 2 * CDA_MAX_AGENTS * 4 + TL_WORDS * 4) + agents * (int)sizeof(Acc) + ((n_hist * CDA_SNAPSHOT_DIM * 4 + 15) & ~15);
}

__device__ __forceinline__ float* lds_hist(Lds& L, int agents) { return reinterpret_cast<float*>(&L.acc[agents]); }

// book record in HBM: [field][CAP] int32, pooled like the LDS image; only the live prefix of each side moves.
// Prefetch form: the first 64 entries of every array are requested BEFORE the header (which holds the
// counts) has arrived, so the two HBM round trips of a naive load overlap into one.
struct BookPrefetch { int32_t v[2][BOOK_FIELDS]; };
__device__ __forceinline__ BookPrefetch prefetch_book(const int32_t* bp, int lane) {
    BookPrefetch r;
    #pragma unroll
    for (int s = 0; s < 2; s++) {
        #pragma unroll
        for (int f = 0; f < BOOK_FIELDS; f++) r.v[s][f] = bp[f * CAP + book_phys(s, lane)];
    }
    return r;
}
__device__ __forceinline__ void finish_book_load(const int32_t* bp, const BookPrefetch& pre, Book& bk, const Mkt& m, int lane) {
    #pragma unroll
    for (int s = 0; s < 2; s++) {
        const int ns = mkt_n(m, s);
        if (lane < ns) { bk.price[s][lane] = pre.v[s][0]; bk.qty[s][lane] = pre.v[s][1]; bk.oo[s][lane] = pre.v[s][2]; bk.ts[s][lane] = pre.v[s][3]; }
        for (int i = lane + WAVE; i < ns; i += WAVE) {
            const int ph = book_phys(s, i);
            bk.price[s][i] = bp[0 * CAP + ph]; bk.qty[s][i] = bp[1 * CAP + ph]; bk.oo[s][i] = bp[2 * CAP + ph]; bk.ts[s][i] = bp[3 * CAP + ph];
        }
    }
}
__device__ __forceinline__ void load_book(const int32_t* bp, Book& bk, const Mkt& m, int lane) {
    #pragma unroll
    for (int s = 0; s < 2; s++) {
        for (int i = lane; i < mkt_n(m, s); i += WAVE) {
            const int ph = book_phys(s, i);
            bk.price[s][i] = bp[0 * CAP + ph]; bk.qty[s][i] = bp[1 * CAP + ph]; bk.oo[s][i] = bp[2 * CAP + ph]; bk.ts[s][i] = bp[3 * CAP + ph];
        }
    }
}
__device__ __forceinline__ void store_book(int32_t* bp, const Book& bk, const Mkt& m, int lane) {
    #pragma unroll
    for (int s = 0; s < 2; s++) {
        for (int i = lane; i < mkt_n(m, s); i += WAVE) {
            const int ph = book_phys(s, i);
            __builtin_nontemporal_store(bk.price[s][i], &bp[0 * CAP + ph]); __builtin_nontemporal_store(bk.qty[s][i], &bp[1 * CAP + ph]);
            __builtin_nontemporal_store(bk.oo[s][i], &bp[2 * CAP + ph]); __builtin_nontemporal_store(bk.ts[s][i], &bp[3 * CAP + ph]);
        }
    }
}
// ======================================================================================
// Order book primitives (OrderTree / OrderList, orderbook/ordertree.py, orderlist.py)
// ======================================================================================
// remove `cnt` entries starting at `idx` (shift the tail down)
__device__ __forceinline__ void book_remove(Book& bk, int s, int n, int idx, int cnt, int lane) {
    for (int base = idx - (idx % WAVE); base < n - cnt; base += WAVE) {
        int i = base + lane;
        bool mv = i >= idx && i < n - cnt;
        int p = 0, q = 0, o = 0, t = 0;
        if (mv) { p = bk.price[s][i + cnt]; q = bk.qty[s][i + cnt]; o = bk.oo[s][i + cnt]; t = bk.ts[s][i + cnt]; }
        CDA_WSYNC();
        if (mv) { bk.price[s][i] = p; bk.qty[s][i] = q; bk.oo[s][i] = o; bk.ts[s][i] = t; }
        CDA_WSYNC();
    }
}
// OrderTree.insert_order (ordertree.py:44-58): an order joins the tail of its price level, i.e. it goes behind every resting order
// whose price is better or equal.  tile_upper_bound counts those among the n tile orders of side s.
__device__ __forceinline__ int tile_upper_bound(const Book& bk, int s, int n, int price, int lane) {
    int pos = 0;
    for (int base = 0; base < n; base += WAVE) {
        int i = base + lane;
        bool c = false;
        if (i < n) { int rp = bk.price[s][i]; c = (s == S_BID) ? (rp >= price) : (rp <= price); }
        pos += __popcll(__ballot(c));
    }
    return pos;
}
// open slot `pos` of a tile side holding n orders (the caller knows the pool has room) and put the order there
__device__ __forceinline__ void tile_insert_at(Book& bk, int s, int n, int pos, int price, int qty, int32_t oo, int ts, int lane) {
    for (int base = n - (n % WAVE); base >= 0; base -= WAVE) {
        int i = base + lane;
        bool mv = i > pos && i <= n;
        int p = 0, q = 0, o = 0, t = 0;
        if (mv) { p = bk.price[s][i - 1]; q = bk.qty[s][i - 1]; o = bk.oo[s][i - 1]; t = bk.ts[s][i - 1]; }
        CDA_WSYNC();
        if (mv) { bk.price[s][i] = p; bk.qty[s][i] = q; bk.oo[s][i] = o; bk.ts[s][i] = t; }
        CDA_WSYNC();
    }
    // every lane writes the same values to the same slot (keeps each lane's view coherent)
    bk.price[s][pos] = price; bk.qty[s][pos] = qty; bk.oo[s][pos] = oo; bk.ts[s][pos] = ts;
    CDA_WSYNC();
}
// the hot path's insert: the whole side is in the tile and the pool has room (n + n_other < CAP)
__device__ __forceinline__ void book_insert(Book& bk, int s, int n, int price, int qty, int owner, int oid, int ts, int lane) {
    tile_insert_at(bk, s, n, tile_upper_bound(bk, s, n, price, lane), price, qty, oo_pack(oid, owner), ts, lane);
}
// Trader._get_order_ID (agent/trader.py:254-287): index on the side or -1
// (tile part; `oldest_ts` receives the timestamp of a modify's candidate so that the side's HBM tail, if any, can be asked for
// an older one)
__device__ __forceinline__ int find_own_order(const Book& bk, int s, int n, int tr, int type, int price, int lane, uint32_t& oldest_ts) {
    oldest_ts = 0xffffffffu;
    if (type == T_MODIFY) {                 // oldest own order: minimum timestamp (LOB.time is unique per resting order)
        uint32_t best = 0xffffffffu;
        int at = -1;                                           // where this lane saw its own minimum: no second pass over the book
        for (int i = lane; i < n; i += WAVE) {
            const int32_t oo = bk.oo[s][i];
            const uint32_t ts = (uint32_t)bk.ts[s][i];
            if (oo_owner(oo) == tr && ts < best) { best = ts; at = i; }
        }
        const uint32_t mn = wave_min_u32(best);
        if (mn == 0xffffffffu) return -1;
        oldest_ts = mn;
        const uint64_t mk = __ballot(best == mn);               // exactly one lane: timestamps are unique
        return __builtin_amdgcn_readlane(at, __ffsll((long long)mk) - 1);
    }
    // limit / cancel: first own order at that price in order_map insertion order == first in the
    // level's FIFO, i.e. first hit in queue order (SURVEY A.5)
    for (int base = 0; base < n; base += WAVE) {
        int i = base + lane;
        bool c = i < n && oo_owner(bk.oo[s][i]) == tr && bk.price[s][i] == price;
        uint64_t mk = __ballot(c);
        if (mk) return base + (__ffsll((long long)mk) - 1);
    }
    return -1;
}

// ======================================================================================
// The HBM tier of the book.
//
// The reference's OrderTree is unbounded (ordertree.py:5-58: a SortedDict of price levels plus an order map) and a limit
// order that does not cross ALWAYS rests (orderbook.py:162-194).  Here a side of the book is one logical queue-ordered
// array Q[0 .. n): its first t orders - the top of the book - are the LDS TILE (`Book`, staged from / to the market record
// every step), the other n - t orders, the TAIL, stay in HBM in the market's spill region:
//
//     int32 hdr[16]                          [0],[1] tail orders of the bid / ask side, [2],[3] ring slot of each side's first tail order
//     int32 ring[2 sides][4 fields][R]       R = Params::lay.spill_cap slots (a power of two); Q[t + i] of side s sits in
//                                            slot (base_s + i) mod R of each of the side's four field arrays
//
// A ring, because both ends move: an order evicted from a full tile is PREPENDED to its side's tail (base - 1), a tile that
// runs low is refilled from the tail's head (base + k), and an insertion / removal inside the tail shifts whichever part
// of it is shorter.  Nothing that happens inside a tile touches the tail, so a market whose whole book fits its tile - every
// market of the BASELINE workloads, see profiles/r03/book_census.json - never executes any of this: the hot path tests
// one status bit (mkt_has_tail) or the pool count and moves on.  Everything below is out of line (CDA_COLD) for the same
// reason: it must not cost the step kernel registers.  The routines get the wave's LDS image by its LDS byte address
// (the low half of the generic address) and find the ring through L.tl, which load_tail_meta() filled at the head of the
// launch; tile counts travel packed (bids | asks << 16, bit 31 = the order was dropped: tile and ring both full).
// Wave-uniform control flow throughout; a ring is read and written by the wave that owns the market, and nobody else.
// ======================================================================================
#define CDA_COLD __attribute__((noinline)) __device__
constexpr int TILE_LOW = 32;          // a side with a tail is refilled when its tile holds fewer orders than this
constexpr int TILE_KEEP = CAP / 4 + 32;   // ... if need be at the expense of the other side's tile, which keeps at least this many
constexpr int TILE_EVICT = 32;        // orders a full pool hands to a tail at a time
__device__ __forceinline__ Lds& lds_at(uint32_t lds_addr) { return *reinterpret_cast<Lds*>(cda_smem + lds_addr); }     // cda_smem sits at LDS address 0 (cda_dec.hpp)
__device__ __forceinline__ uint32_t lds_addr_of(const Lds& L) { return (uint32_t)(uintptr_t)&L; }
__device__ __forceinline__ uint32_t pack_counts(int nb, int na) { return (uint32_t)nb | ((uint32_t)na << 16); }
struct Tail {
    int32_t* ring;                // the market's rings: [side][field][cap]
    uint32_t cap;
    __device__ __forceinline__ int32_t* field(int s, int f) const { return ring + (size_t)(s * BOOK_FIELDS + f) * (size_t)cap; }
    __device__ __forceinline__ uint32_t slot(int base, int i) const { return (uint32_t)(base + i) & (cap - 1u); }
};
__device__ __forceinline__ Tail tail_of(const Lds& L) {
    Tail T;
    T.ring = reinterpret_cast<int32_t*>(((uint64_t)(uint32_t)L.tl[TL_PTR_HI] << 32) | (uint64_t)(uint32_t)L.tl[TL_PTR_LO]) + 16;
    T.cap = (uint32_t)L.tl[TL_CAP];
    return T;
}
// A ring written by some lanes is read by other lanes OF THE SAME WAVE later in the same launch (a market belongs to one
// wave; other launches see it through the kernel boundary): the stores must have left the wave before those loads issue,
// nothing more - the CU's write-through L1 serves both.  Workgroup scope says exactly that (s_waitcnt vmcnt(0), no cache
// action).  Agent scope, used in the first version, made every cold order write back and invalidate the XCD's L2
// (buffer_wbl2 sc1 + buffer_inv sc1) - 40 us per order, measured.
__device__ __forceinline__ void tail_fence() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }

// the first k (<= 64) tail orders of side s move to the end of its tile, which holds t orders and has room for k more
__device__ __forceinline__ void tail_pop_to_tile(Lds& L, const Tail& T, int s, int t, int k, int lane) {
    const int base = L.tl[TL_BASE + s], tn = L.tl[TL_N + s];
    if (lane < k) {
        const uint32_t sl = T.slot(base, lane);
        const int32_t p = T.field(s, 0)[sl], q = T.field(s, 1)[sl], o = T.field(s, 2)[sl], ts = T.field(s, 3)[sl];
        L.book.price[s][t + lane] = p; L.book.qty[s][t + lane] = q; L.book.oo[s][t + lane] = o; L.book.ts[s][t + lane] = ts;
    }
    CDA_WSYNC();
    L.tl[TL_BASE + s] = base + k; L.tl[TL_N + s] = tn - k;
    CDA_WSYNC();
}
// the last k (<= 64) of the t tile orders of side s become the head of its tail (the caller checked the ring has room)
__device__ __forceinline__ void tile_push_to_tail(Lds& L, const Tail& T, int s, int t, int k, int lane) {
    const int base = L.tl[TL_BASE + s] - k, tn = L.tl[TL_N + s];
    if (lane < k) {
        const uint32_t sl = T.slot(base, lane);
        const int i = t - k + lane;
        T.field(s, 0)[sl] = L.book.price[s][i]; T.field(s, 1)[sl] = L.book.qty[s][i]; T.field(s, 2)[sl] = L.book.oo[s][i]; T.field(s, 3)[sl] = L.book.ts[s][i];
    }
    CDA_WSYNC();
    L.tl[TL_BASE + s] = base; L.tl[TL_N + s] = tn + k;
    CDA_WSYNC();
}
// number of tail orders of side s whose price is better than (strict) / better than or equal to `price`: a 64-ary search,
// every round one gather of up to 64 prices (two rounds cover 4096 orders)
__device__ __forceinline__ int tail_bound(const Tail& T, int s, int base, int tn, int32_t price, bool strict, int lane) {
    const int32_t* pf = T.field(s, 0);
    int lo = 0, hi = tn;
    while (hi > lo) {
        const int step = (hi - lo + 63) >> 6, idx = lo + (lane + 1) * step - 1;
        bool c = false;
        if (idx < hi) {
            const int32_t rp = pf[T.slot(base, idx)];
            c = s == S_BID ? (strict ? rp > price : rp >= price) : (strict ? rp < price : rp <= price);
        }
        const int cnt = __popcll(__ballot(c));          // the probes that pass are a prefix: the side is sorted
        const int nhi = lo + (cnt + 1) * step - 1;
        lo = lo + cnt * step;
        hi = nhi < hi ? nhi : hi;
    }
    return lo;
}
// open tail position p of side s (shift whichever part of the tail is shorter by one slot) and write the order there
__device__ __forceinline__ void tail_insert_at(Lds& L, const Tail& T, int s, int p, int32_t price, int32_t qty, int32_t oo, int32_t ts, int lane) {
    int base = L.tl[TL_BASE + s];
    const int tn = L.tl[TL_N + s];
    if (p <= tn - p) {                                   // the p orders in front move one slot towards the head
        for (int b = 0; b < p; b += WAVE) {
            const int i = b + lane;
            int32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
            const uint32_t from = T.slot(base, i), to = T.slot(base, i - 1);
            if (i < p) { v0 = T.field(s, 0)[from]; v1 = T.field(s, 1)[from]; v2 = T.field(s, 2)[from]; v3 = T.field(s, 3)[from]; }
            if (i < p) { T.field(s, 0)[to] = v0; T.field(s, 1)[to] = v1; T.field(s, 2)[to] = v2; T.field(s, 3)[to] = v3; }
        }
        base -= 1;
    } else {                                             // the tn - p orders behind it move one slot towards the end, last ones first
        for (int b = 0; b < tn - p; b += WAVE) {
            const int i = tn - 1 - b - lane;
            int32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
            const uint32_t from = T.slot(base, i), to = T.slot(base, i + 1);
            if (i >= p) { v0 = T.field(s, 0)[from]; v1 = T.field(s, 1)[from]; v2 = T.field(s, 2)[from]; v3 = T.field(s, 3)[from]; }
            if (i >= p) { T.field(s, 0)[to] = v0; T.field(s, 1)[to] = v1; T.field(s, 2)[to] = v2; T.field(s, 3)[to] = v3; }
        }
    }
    const uint32_t at = T.slot(base, p);
    if (lane == 0) { T.field(s, 0)[at] = price; T.field(s, 1)[at] = qty; T.field(s, 2)[at] = oo; T.field(s, 3)[at] = ts; }
    L.tl[TL_BASE + s] = base; L.tl[TL_N + s] = tn + 1;
    CDA_WSYNC();
}

// After orders left a tile (a match, a cancel, a modify): a side that continues in HBM gets its tile topped up from the head
// of its tail, so that the top of the book - best price, the levels of the observation, the orders a sweep consumes next -
// is in LDS again.  Returns the tile counts.
CDA_COLD uint32_t cold_rebalance(uint32_t lds_addr, uint32_t counts) {
    Lds& L = lds_at(lds_addr);
    const Tail T = tail_of(L);
    const int lane = lane_id();
    int nb = (int)(counts & 0x7fffu), na = (int)((counts >> 16) & 0x7fffu);
    bool moved = false;
    #pragma unroll
    for (int s = 0; s < 2; s++) {
        for (;;) {
            const int t = s ? na : nb, to = s ? nb : na, tn = L.tl[TL_N + s];
            if (tn <= 0 || t >= TILE_LOW) break;
            const int want = tn < WAVE ? tn : WAVE;
            int room = CAP - t - to;
            if (room < want && to > TILE_KEEP) {         // the other side's tile gives way (its own tail takes what it gives up)
                int e = want - room;
                if (e > to - TILE_KEEP) e = to - TILE_KEEP;
                if (L.tl[TL_N + (s ^ 1)] + e <= (int)T.cap) {
                    tile_push_to_tail(L, T, s ^ 1, to, e, lane);
                    if (s) nb -= e; else na -= e;
                    room += e;
                }
            }
            const int k = want < room ? want : room;
            if (k <= 0) break;
            tail_pop_to_tile(L, T, s, t, k, lane);
            if (s) na += k; else nb += k;
            moved = true;
        }
    }
    if (moved) tail_fence();
    return pack_counts(nb, na);
}

// OrderTree.insert_order (ordertree.py:44-58) when the side continues in HBM or the tile pool is full: the order goes to its
// place in the side's ONE queue order, wherever that is.  Returns the tile counts (bit 31: dropped, tile and ring are full).
CDA_COLD uint32_t cold_insert(uint32_t lds_addr, uint32_t counts, int s, int32_t price, int32_t qty, int32_t oo, int32_t ts) {
    Lds& L = lds_at(lds_addr);
    const Tail T = tail_of(L);
    const int lane = lane_id();
    int t = (int)((s ? counts >> 16 : counts) & 0x7fffu), to = (int)((s ? counts : counts >> 16) & 0x7fffu);
    const int tn = L.tl[TL_N + s];
    uint32_t dropped = 0;
    const int pos = tile_upper_bound(L.book, s, t, price, lane);
    bool in_tile = pos < t || tn == 0;                   // else: every tile order is better or equal and a tail follows
    if (in_tile && t + to >= CAP) {
        if (pos == t) in_tile = false;                   // behind the whole tile of a full pool: the order starts the side's tail
        else {                                           // make room: the larger tile hands its last orders to its tail
            const bool own = t >= to;
            const int e = own ? s : s ^ 1;
            int k = own ? t - pos : to - 1;
            if (k > TILE_EVICT) k = TILE_EVICT;
            if (L.tl[TL_N + e] + k > (int)T.cap) { dropped = 1; in_tile = false; }
            else { tile_push_to_tail(L, T, e, own ? t : to, k, lane); if (own) t -= k; else to -= k; }
        }
    }
    if (!dropped) {
        if (in_tile) { tile_insert_at(L.book, s, t, pos, price, qty, oo, ts, lane); t += 1; }
        else {
            const int tn2 = L.tl[TL_N + s];
            const int p2 = tn2 > 0 ? tail_bound(T, s, L.tl[TL_BASE + s], tn2, price, false, lane) : 0;
            if (p2 == 0 && t + to < CAP) { tile_insert_at(L.book, s, t, t, price, qty, oo, ts, lane); t += 1; }   // the boundary: the tile takes it
            else if (tn2 >= (int)T.cap) dropped = 1;
            else tail_insert_at(L, T, s, p2, price, qty, oo, ts, lane);
        }
    }
    tail_fence();
    return (s ? pack_counts(to, t) : pack_counts(t, to)) | (dropped << 31);
}

// Trader._get_order_ID (trader.py:254-287) continued into the tail of side s, whose tile (t orders) was searched first.
// modify: an own order OLDER than the tile's candidate (`tile_oldest_ts`, 0xffffffff = none); limit / cancel (only asked
// when the tile has no hit): the first own order at `price` in queue order.  Returns the index in the tail or -1.
CDA_COLD int cold_find(uint32_t lds_addr, int s, int t, int tr, int type, int32_t price, uint32_t tile_oldest_ts) {
    Lds& L = lds_at(lds_addr);
    const Tail T = tail_of(L);
    const int lane = lane_id();
    const int base = L.tl[TL_BASE + s], tn = L.tl[TL_N + s];
    if (tn <= 0) return -1;
    if (type == T_MODIFY) {
        uint32_t best = tile_oldest_ts;
        int at = -1;
        for (int b = 0; b < tn; b += 2 * WAVE) {         // two gathers in flight per round
            const int i0 = b + lane, i1 = b + WAVE + lane;
            const uint32_t s0 = T.slot(base, i0), s1 = T.slot(base, i1);
            int32_t o0 = -1, o1 = -1; uint32_t t0 = 0xffffffffu, t1 = 0xffffffffu;
            if (i0 < tn) { o0 = T.field(s, 2)[s0]; t0 = (uint32_t)T.field(s, 3)[s0]; }
            if (i1 < tn) { o1 = T.field(s, 2)[s1]; t1 = (uint32_t)T.field(s, 3)[s1]; }
            if (i0 < tn && oo_owner(o0) == tr && t0 < best) { best = t0; at = i0; }
            if (i1 < tn && oo_owner(o1) == tr && t1 < best) { best = t1; at = i1; }
        }
        const uint32_t mn = wave_min_u32(best);
        if (mn >= tile_oldest_ts) return -1;             // the tile's candidate (or nothing at all) stands
        const uint64_t mk = __ballot(best == mn && at >= 0);
        return __builtin_amdgcn_readlane(at, __ffsll((long long)mk) - 1);
    }
    if (t > 0) {                                         // the tail starts where the tile ends: a quote better than the tile's last order is not in it
        const int32_t lp = L.book.price[s][t - 1];
        if (s == S_BID ? price > lp : price < lp) return -1;
    }
    for (int i = tail_bound(T, s, base, tn, price, true, lane); i < tn; i += WAVE) {      // the level starts behind every strictly better order
        const int j = i + lane;
        bool hit = false, past = false;
        if (j < tn) {
            const uint32_t sl = T.slot(base, j);
            const int32_t rp = T.field(s, 0)[sl], ro = T.field(s, 2)[sl];
            past = rp != price; hit = !past && oo_owner(ro) == tr;
        }
        const uint64_t hm = __ballot(hit), pm = __ballot(past);
        const int fh = hm ? __ffsll((long long)hm) - 1 : 64, fp = pm ? __ffsll((long long)pm) - 1 : 64;
        if (fh < fp) return i + fh;
        if (pm) return -1;
    }
    return -1;
}
// tail order `idx` of side s -> L.tl[TL_ORD ..] = price, qty, (order_id << 4) | owner, timestamp
CDA_COLD void cold_tail_read(uint32_t lds_addr, int s, int idx) {
    Lds& L = lds_at(lds_addr);
    const Tail T = tail_of(L);
    const int lane = lane_id();
    const uint32_t sl = T.slot(L.tl[TL_BASE + s], idx);
    if (lane < BOOK_FIELDS) L.tl[TL_ORD + lane] = T.field(s, lane)[sl];
    CDA_WSYNC();
}
// OrderBook.modify_order in place (orderbook.py:210-266: same price, quantity not larger) on tail order `idx`
CDA_COLD void cold_tail_update(uint32_t lds_addr, int s, int idx, int32_t qty, int32_t ts) {
    Lds& L = lds_at(lds_addr);
    const Tail T = tail_of(L);
    const uint32_t sl = T.slot(L.tl[TL_BASE + s], idx);
    if (lane_id() == 0) { T.field(s, 1)[sl] = qty; T.field(s, 3)[sl] = ts; }
    tail_fence();
}
// OrderTree.remove_order_by_id (ordertree.py:60-77) for tail order `idx`: the shorter part of the tail closes the gap
CDA_COLD void cold_tail_remove(uint32_t lds_addr, int s, int idx) {
    Lds& L = lds_at(lds_addr);
    const Tail T = tail_of(L);
    const int lane = lane_id();
    int base = L.tl[TL_BASE + s];
    const int tn = L.tl[TL_N + s];
    if (idx < tn - 1 - idx) {                            // the idx orders in front move one slot towards the end, last ones first
        for (int b = 0; b < idx; b += WAVE) {
            const int i = idx - 1 - b - lane;
            int32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
            const uint32_t from = T.slot(base, i), to = T.slot(base, i + 1);
            if (i >= 0) { v0 = T.field(s, 0)[from]; v1 = T.field(s, 1)[from]; v2 = T.field(s, 2)[from]; v3 = T.field(s, 3)[from]; }
            if (i >= 0) { T.field(s, 0)[to] = v0; T.field(s, 1)[to] = v1; T.field(s, 2)[to] = v2; T.field(s, 3)[to] = v3; }
        }
        base += 1;
    } else {                                             // the orders behind it move one slot towards the head
        for (int b = idx + 1; b < tn; b += WAVE) {
            const int i = b + lane;
            int32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
            const uint32_t from = T.slot(base, i), to = T.slot(base, i - 1);
            if (i < tn) { v0 = T.field(s, 0)[from]; v1 = T.field(s, 1)[from]; v2 = T.field(s, 2)[from]; v3 = T.field(s, 3)[from]; }
            if (i < tn) { T.field(s, 0)[to] = v0; T.field(s, 1)[to] = v1; T.field(s, 2)[to] = v2; T.field(s, 3)[to] = v3; }
        }
    }
    L.tl[TL_BASE + s] = base; L.tl[TL_N + s] = tn - 1;
    CDA_WSYNC();
    tail_fence();
}
// State_Helper.set_agg_LOB (state_helper.py:113-214) continued into the tail of side s: the tile (t orders) gave `carry`
// price levels so far and fewer than the ten the observation shows are complete
CDA_COLD void cold_aggregate(uint32_t lds_addr, int s, int t, int carry) {
    Lds& L = lds_at(lds_addr);
    const Tail T = tail_of(L);
    const int lane = lane_id();
    const int base = L.tl[TL_BASE + s], tn = L.tl[TL_N + s];
    int32_t prev = t > 0 ? L.book.price[s][t - 1] : -1;
    for (int b = 0; b < tn && carry <= CDA_K_ROWS; b += WAVE) {
        const int i = b + lane;
        const bool valid = i < tn;
        int32_t p = 0, q = 0;
        if (valid) { const uint32_t sl = T.slot(base, i); p = T.field(s, 0)[sl]; q = T.field(s, 1)[sl]; }
        const int32_t up = __shfl(p, (lane + 63) & 63, WAVE);
        const int32_t pp = lane == 0 ? prev : up;
        const bool head = valid && p != pp;
        const uint64_t mk = __ballot(head);
        const uint64_t le = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
        const int lvl = carry + __popcll(mk & le) - 1;
        if (valid && lvl >= 0 && lvl < CDA_K_ROWS) {
            atomicAdd(&L.lvl_sz[s][lvl], q);
            if (head) L.lvl_px[s][lvl] = p;
        }
        carry += __popcll(mk);
        prev = __builtin_amdgcn_readlane(p, 63);
    }
    CDA_WSYNC();
}
// the status bits of the market follow the ring counts
__device__ __forceinline__ void sync_tail_status(const Lds& L, Mkt& m) {
    m.status = (m.status & ~ST_TAIL_ANY) | (L.tl[TL_N] > 0 ? ST_TAIL_BID : 0) | (L.tl[TL_N + 1] > 0 ? ST_TAIL_ASK : 0);
}
__device__ __forceinline__ void set_counts(Mkt& m, uint32_t counts) { m.nb = (int32_t)(counts & 0x7fffu); m.na = (int32_t)((counts >> 16) & 0x7fffu); }
__device__ __forceinline__ int total_orders(const Lds& L, const Mkt& m) { return m.nb + m.na + ((m.status & ST_TAIL_ANY) ? L.tl[TL_N] + L.tl[TL_N + 1] : 0); }
// Memory-to-memory style on purpose: every statement loads its operands from the account record in LDS and
// stores its result back, so that almost nothing is live across the (rare) calls into the rounding helpers.
// Keeping the whole account in registers made this function need 165 VGPRs (callee-saved registers are sparse
// in the AMDGPU calling convention) and capped the kernel at 3-4 waves per SIMD.
#define ACC_UPD(field, expr) do { D _r = (expr); st_dec(a.field, _r, flags); } while (0)
__device__ __forceinline__ void xfer_inc(Acc& a, bool counter, D v, uint32_t& flags) {   // size_increase_cash_transfer (cash_processor.py:31-36)
    cda_dec& fld = counter ? a.hold : a.cash;
    D r = d_sub(ld_dec(fld), v);
    st_dec(fld, r, flags);
}
__device__ __forceinline__ void xfer_dec(Acc& a, bool counter, D v, uint32_t& flags) {   // size_decrease_cash_transfer (cash_processor.py:38-45)
    ACC_UPD(cash, d_add(ld_dec(a.cash), v));
    if (counter) { ACC_UPD(hold, d_sub(ld_dec(a.hold), v)); ACC_UPD(cash, d_add(ld_dec(a.cash), v)); }
}
// position_val = raw + profit with raw = n * VWAP, mkt = n * price (account.py:128-131, :141-143, :155-157)
__device__ __forceinline__ D posval_from(Acc& a, uint32_t n, int32_t price, bool is_long) {
    D raw = d_mul_int(ld_dec(a.vwap), n), mkt = d_price_times(price, n);
    return d_add(raw, cal_profit(is_long, mkt, raw));
}
// One fill (trader.py:303-345 _process_trades / _process_counter_party, account.py:215-231 process_acc): the passive
// party and the initiator settle at the same time, each on its owner lane plus helper lanes (+16, +32).  The ledger
// update of every mode is laid out as the SAME sequence of generic operations so that both parties - whatever their
// modes - run them in one instruction stream:
//   stage 1  one multiplication   owner: VWAP * |pos|  (numerator term of _size_increase/_size_decrease, `raw` of _covered)
//   stage 2  one addition         owner: numerator +- trade value | profit = +-(mkt - raw) | position_val += trade value (_neutral)
//                                 helpers: the cash / cash_on_hold transfers that do not depend on the owner's chain
//   stage 3  owner only           VWAP = numerator / n   or the rest of _covered / _covered_side_chg
// Operations on ONE field keep the reference's order; different fields of an account are independent.
//
// LAZY_POSVAL: inside k_step every fill is followed, before anything can read it, by Calculate.mark_to_mkt (it runs
// whenever the tape is non-empty), which recomputes position_val from (net_position, VWAP, price) alone.  The value
// _size_increase/_size_decrease store is therefore dead there and its four decimal operations are skipped; the paths
// that READ position_val (_neutral, _covered) are untouched.  The one-order test hook keeps the full semantics.
template <bool LAZY_POSVAL>
__device__ __forceinline__ void settle_fill(Lds& L, int tr, int counter, int32_t q, int32_t price, int init_side, uint32_t& flags, int lane CDA_TF_PARAM) {
    uint32_t f = 0;
    TF_BEGIN();
    const int al = lane_acc(lane), g = lane_grp(lane);
    if (counter != tr) {
        if ((al == tr || al == counter) && g < 3) {
            Acc& a = L.acc[al];
            const bool is_counter = al == counter;
            const int own_side = is_counter ? init_side ^ 1 : init_side;
            // net_position, num_trades, num_trades_step, num_passive_fills_step are one aligned 16-byte group: read here in one
            // request (with the VWAP: one LDS round trip for both), written back in one at the end of stage 3
            int4 cnt = *reinterpret_cast<const int4*>(&a.net_position);
            const D vwap0 = ld_dec(a.vwap);
            const int32_t pos = cnt.x;
            const uint32_t ap = (uint32_t)(pos < 0 ? -pos : pos);
            const bool is_long = pos > 0;
            int mode;                                       // 0 _neutral, 1 _size_increase, 2 _size_decrease, 3 _covered, 4 _covered_side_chg
            if (pos == 0) mode = 0;
            else if (is_long == (own_side == S_BID)) mode = 1;
            else mode = ap > (uint32_t)q ? 2 : (ap == (uint32_t)q ? 3 : 4);
            const D tv = d_price_times(price, (uint32_t)q);                     // trade value
            D X = d_zero(), mkt = d_zero();
            TF_END(14);
            if (g == 0 && mode != 0) X = d_mul_int(vwap0, ap);                  // stage 1
            TF_END(15);
            D x2 = d_zero(), y2 = d_zero();
            cda_dec* dst = nullptr;
            bool s2 = false;
            if (g == 0) {
                s2 = true;
                if (mode == 0) { x2 = ld_dec(a.posval); y2 = tv; dst = &a.posval; }                 // account.py:173-176
                else if (mode <= 2) { x2 = X; y2 = tv; y2.sign = mode == 2 ? 1 : 0; }               // account.py:124-133, :151-161
                else { mkt = d_price_times(price, ap); x2 = is_long ? mkt : X; y2 = d_neg(is_long ? X : mkt); }   // calculate.py cal_profit
            } else if (mode <= 2) {
                if (g == 1) {                               // first statement of size_increase / size_decrease_cash_transfer (cash_processor.py:31-45)
                    s2 = true;
                    dst = (mode != 2 && is_counter) ? &a.hold : &a.cash;
                    x2 = ld_dec(*dst); y2 = tv; y2.sign = mode != 2 ? 1 : 0;
                } else if (mode == 2 && is_counter) {       // the passive party's escrow release
                    s2 = true;
                    dst = &a.hold; x2 = ld_dec(a.hold); y2 = d_neg(tv);
                }
            }
            D Y = d_zero();
            TF_END(16);
            if (s2) { Y = d_add(x2, y2); if (dst) st_dec(*dst, Y, f); }        // stage 2
            TF_END(17);
            if (g == 0) {                                    // stage 3
                cnt.y += 1; cnt.z += 1; cnt.w += is_counter ? 1 : 0;
                if (mode == 0) st_dec(a.vwap, d_price(price), f);
                else if (mode <= 2) {
                    const uint32_t n = mode == 1 ? ap + (uint32_t)q : ap - (uint32_t)q;
                    ACC_UPD(vwap, d_div_u32(Y, n));
                    if (!LAZY_POSVAL) ACC_UPD(posval, posval_from(a, n, price, is_long));
                    if (mode == 2 && is_counter) ACC_UPD(cash, d_add(ld_dec(a.cash), tv));       // third statement of size_decrease_cash_transfer
                } else {                                     // _covered (account.py:135-149)
                    D pv = d_add(X, Y);
                    ACC_UPD(cash, d_add(ld_dec(a.cash), d_sub(pv, mkt)));                        // size_zero_cash_transfer (cash_processor.py:47-53)
                    st_dec(a.posval, d_zero(), f); st_dec(a.vwap, d_zero(), f);
                    if (mode == 3) xfer_dec(a, is_counter, tv, f);
                    else {                                   // _covered_side_chg (account.py:163-171)
                        xfer_dec(a, is_counter, mkt, f);
                        D npv = d_price_times(price, (uint32_t)q - ap);
                        st_dec(a.posval, npv, f); st_dec(a.vwap, d_price(price), f);
                        xfer_inc(a, is_counter, npv, f);
                    }
                }
                int64_t np = (int64_t)pos + (own_side == S_BID ? (int64_t)q : -(int64_t)q);
                if (np > 2147483647LL || np < -2147483647LL) f |= CDA_FLAG_INT_OVERFLOW << 8;
                cnt.x = (int32_t)np;
                *reinterpret_cast<int4*>(&a.net_position) = cnt;
            }
            if (mode >= 3) { TF_END(22); TF_COUNT(21); } else if (g == 0 && mode == 0) { TF_END(23); TF_COUNT(12); } else TF_END(18);
            TF_COUNT(20);
        }
        CDA_WSYNC();
        TF_WAVE(tr, counter);
        TF_RESYNC();
    } else if (lane == tr) {                             // init_is_counter_cash_transfer (cash_processor.py:55-62)
        Acc& a = L.acc[lane];
        D tv = d_price_times(price, (uint32_t)q);
        D hold = d_sub(ld_dec(a.hold), tv), cash = d_add(ld_dec(a.cash), tv);
        st_dec(a.hold, hold, f); st_dec(a.cash, cash, f);
    }
    if (__ballot((f & 0xffu) != 0)) flags |= CDA_FLAG_DEC_DOMAIN;
    if (__ballot((f >> 8) != 0)) flags |= CDA_FLAG_INT_OVERFLOW;
    TF_END(19);
    TF_WAVE_END();
}

// matching loops of OrderBook.process_order_list / process_market_order / process_limit_order
// (orderbook.py:61-194).  limit < 0 = market order.  Returns the unfilled quantity.
// TAILS: the general build (a side may continue in the HBM tier, "The HBM tier of the book" above).  The hot kernels are
// compiled with TAILS = false - exactly the tile-only code - and hand a market whose book may outgrow its tile during the step
// to the general build BEFORE they touch it (cda_kernels.inc, market_is_cold).
// TAPE: the tape-writing instances (include/cda.h cda_tape_enable) append one record per fill to the market's ring, here, where price,
// quantity, both parties, the resting order's id and what is left of it are at hand - self-trades included: the reference appends its
// transaction_record before _process_trades looks at the parties (orderbook.py:108-140).  One lane, two 16-byte vector stores.
// (The record's layout is stated once, for every reader, by the accessors beside TapeSpan in cda_tape.inc: tape_load, tape_price .. tape_step.)
template <bool TAILS, bool LAZY_POSVAL, bool TAPE = false>
__device__ __forceinline__ int32_t match(Lds& L, Mkt& m, int tr, int own_side, int32_t qty, int32_t limit, int lane) {
    int opp = own_side ^ 1;
    Book& bk = L.book;
    for (;;) {
        int h = 0;
        const int nopp = mkt_n(m, opp);
        while (qty > 0 && h < nopp) {
            int32_t p = bk.price[opp][h];
            if (limit >= 0) { if (own_side == S_BID ? !(limit >= p) : !(limit <= p)) break; }
            int32_t rq = bk.qty[opp][h], c = oo_owner(bk.oo[opp][h]), f;
            if constexpr (TAPE) {
                if (lane == 0) {
                    uint4* rec = m.tape_ring + 2 * (size_t)(m.tape_pos & m.tape_mask);
                    const int32_t fq = qty < rq ? qty : rq;
                    rec[0] = make_uint4((uint32_t)m.lob_time, (uint32_t)p, (uint32_t)fq, (uint32_t)c);
                    rec[1] = make_uint4((uint32_t)bk.oo[opp][h] >> 4, (uint32_t)(qty < rq ? rq - qty : -1), (uint32_t)tr,
                                        ((uint32_t)m.t_step << 2) | ((uint32_t)own_side << 1) | (uint32_t)opp);
                }
                m.tape_pos += 1; m.tape_new += 1;
            }
            if (qty < rq) { f = qty; bk.qty[opp][h] = rq - qty; qty = 0; CDA_WSYNC(); }    // all lanes store the same value
            else { f = rq; qty -= rq; h++; }
            m.has_trade = 1; m.last_trade_price = p;
            TACC_COUNT(m, 5, 1);
            // The launch ends with its slowest market-wave, and the slow ones are those that settle many fills: from the first
            // fill on, this wave asks its SIMD for instruction-issue priority over the (lighter) waves it shares the SIMD with.
            m.fills += 1;
            if (m.fills == 1) __builtin_amdgcn_s_setprio(1);
            else if (m.fills == 2) __builtin_amdgcn_s_setprio(2);
            else if (m.fills == 3) __builtin_amdgcn_s_setprio(3);
            if (!CDA_MKT_DBG(m, 0x1000)) settle_fill<LAZY_POSVAL>(L, tr, c, f, p, own_side, m.flags, lane CDA_TF_ARG(m));
        }
        if (h) { book_remove(bk, opp, nopp, 0, h, lane); mkt_set_n(m, opp, nopp - h); }
        if constexpr (TAILS) {
            if (!mkt_has_tail(m, opp)) break;
            // the side continues in HBM: top the tile up, and go on if the sweep consumed all of it and wants more
            const bool ran_out = qty > 0 && h == nopp;
            set_counts(m, cold_rebalance(lds_addr_of(L), pack_counts(m.nb, m.na)));
            sync_tail_status(L, m);
            if (!ran_out || mkt_n(m, opp) == 0) break;
        } else break;
    }
    return qty;
}

// cash -+= v and hold +-= v of account `tr` (cash_processor.py:15-29 order_in_book_passive_party with dir = -1: escrow a
// resting order; :85-97 cancel_cash_transfer with dir = +1: release it).  Group 0 updates cash, group 1 cash_on_hold.
__device__ __forceinline__ void cash_hold_transfer(Lds& L, int tr, int32_t price, int32_t qty, int cash_dir, uint32_t& flags, int lane) {
    const int g = lane_grp(lane);
    if (lane_acc(lane) == tr && g < 2) {
        Acc& a = L.acc[tr];
        D v = d_price_times(price, (uint32_t)qty);
        cda_dec& fld = g == 0 ? a.cash : a.hold;
        v.sign = (g == 0) == (cash_dir > 0) ? 0 : 1;
        const D cur = ld_dec(fld);
        D r = d_add_order_value(cur, v);
        if (r.exp == D_NOT_HANDLED) r = d_add(cur, v);
        st_dec(fld, r, flags);
    }
    CDA_WSYNC();
}

// Trader._order_approved (agent/trader.py:108-151), evaluated by lane `tr`, result broadcast
__device__ __forceinline__ bool order_approved(Lds& L, const Mkt& m, int tr, int side, int32_t size, int32_t price, int lane) {
    int ok = 0;
    if (lane == tr) {
        const Acc& a = L.acc[lane];
        // every LDS operand is requested up front (one round trip instead of four dependent ones)
        const D nav = ld_dec(a.nav), cash = ld_dec(a.cash);
        const int32_t pos32 = a.net_position;
        const int32_t opp_best = L.book.price[side ^ 1][0];              // read even if that side is empty (slot 0 / CAP-1 exists)
        if (d_sgn(nav) > 0) {
            int64_t pos = pos32, opening;
            int64_t apos = pos < 0 ? -pos : pos;
            if ((side == S_BID && pos >= 0) || (side == S_ASK && pos <= 0)) opening = size;
            else { opening = (int64_t)size - apos; if (opening < 0) opening = 0; }
            if (opening <= 0) ok = 1;
            else {
                D est;
                if (price < 0) {
                    int opp = side ^ 1;
                    if (mkt_n(m, opp) > 0) est = d_price(opp_best);
                    else if (m.has_trade) est = d_price(m.last_trade_price);
                    else est = d_from_u32(1);
                } else est = d_price(price);
                // order_val = opening * est = ov * 10^-1 with ov < 2^63 (est is a tick price or 1: coefficient < 2^28).  When the
                // bit lengths alone prove cash > order_val the exact decimal compare is skipped (cash of 1e6 vs orders of 1e2..1e5).
                uint64_t ov = (uint64_t)((uint32_t)est.w0) * (uint64_t)opening;          // exact: est.w1 == est.w2 == 0
                int kdig = est.exp - cash.exp;                                            // cash coefficient is compared with ov * 10^kdig
                int bc = bits128(d_c128(cash)), bo = 64 - __clzll(ov | 1ull);
                if (!cash.sign && kdig >= 0 && kdig <= 30 && opening < (1LL << 31) && bc - 1 >= bo + ((kdig * 3402) >> 10) + 1) ok = 1;
                else ok = d_cmp(cash, d_mul_u32(est, (uint32_t)opening, 0)) >= 0;
            }
        }
    }
    return __ballot(ok != 0) != 0;                       // only lane `tr` can have set it
}

// Trader.place_order (agent/trader.py:49-106) with Trader._place_limit_order / _modify_limit_order /
// __modify_limit_order / _cancel_limit_order (:189-252) and OrderBook.process_order / modify_order /
// cancel_order (orderbook/orderbook.py:33-59, :196-266).  Structured so that the matching loop has ONE
// call site: the type-specific part only decides what (if anything) is matched and what may rest.
template <bool TAILS, bool LAZY_POSVAL, bool TAPE = false>
__device__ __forceinline__ void place_order(Lds& L, Mkt& m, int tr, int type, int side, int32_t size, int32_t price, int lane) {
    if (side == S_NONE) return;
    TACC_BEGIN();
    bool approved_ = CDA_MKT_DBG(m, 0x100) ? true : order_approved(L, m, tr, side, size, type == T_MARKET ? -1 : price, lane);
    TACC_END(m, 0);
    if (!approved_) {
        if (lane == tr) L.acc[lane].num_rejected_step += 1;
        return;
    }
    if ((type == T_MARKET || type == T_LIMIT) && lane == tr) L.acc[lane].order_step_placed = 1;
    Book& bk = L.book;
    int32_t rest_price = 0, rest_qty = 0;
    bool do_match = false, can_rest = false;
    int32_t m_limit = -1, rest_oid = 0;
    uint32_t f = 0;
    if (type == T_MARKET) {
        m.lob_time += 1; m.next_oid += 1;                     // orderbook.py:39-44
        do_match = true;
    } else {
        const int nside = mkt_n(m, side);
        uint32_t tile_ts;
        int idx = CDA_MKT_DBG(m, 0x400) ? -1 : find_own_order(bk, side, nside, tr, type, price, lane, tile_ts);
        int tidx = -1;                                        // >= 0: the order lives in the side's HBM tail, at this index
        if constexpr (TAILS) {
            if (mkt_has_tail(m, side) && (type == T_MODIFY || idx < 0)) {
                tidx = cold_find(lds_addr_of(L), side, nside, tr, type, price, tile_ts);
                if (tidx >= 0) idx = -1;
            }
        }
        TACC_END(m, 1);
        if (type == T_LIMIT && idx < 0 && tidx < 0) {         // a new order
            m.lob_time += 1; m.next_oid += 1;
            do_match = true; can_rest = true; m_limit = price; rest_oid = m.next_oid;
        } else if (idx >= 0 || tidx >= 0) {
            int32_t op, oq, ooid;
            if (tidx < 0) { op = bk.price[side][idx]; oq = bk.qty[side][idx]; ooid = (int32_t)((uint32_t)bk.oo[side][idx] >> 4); }
            else { cold_tail_read(lds_addr_of(L), side, tidx); op = L.tl[TL_ORD]; oq = L.tl[TL_ORD + 1]; ooid = (int32_t)((uint32_t)L.tl[TL_ORD + 2] >> 4); }
            m.lob_time += 1;
            TACC_END(m, 4);
            if (type == T_CANCEL) {                           // trader.py:237-252: cancel, then release the escrow
                if (tidx < 0) { book_remove(bk, side, nside, idx, 1, lane); mkt_set_n(m, side, nside - 1); }
                else { cold_tail_remove(lds_addr_of(L), side, tidx); sync_tail_status(L, m); }
                TACC_END(m, 6);
                if (!CDA_MKT_DBG(m, 0x200)) cash_hold_transfer(L, tr, op, oq, +1, f, lane);
                TACC_END(m, 7);
            } else {                                          // upsert / modify: release, then modify_order
                if (!CDA_MKT_DBG(m, 0x200)) cash_hold_transfer(L, tr, op, oq, +1, f, lane);
                TACC_END(m, 7);
                TACC_COUNT(m, 10, 1);
                if (price == op && size <= oq) {              // in place: priority kept, timestamp := now
                    if (tidx < 0) { bk.qty[side][idx] = size; bk.ts[side][idx] = m.lob_time; CDA_WSYNC(); }
                    else cold_tail_update(lds_addr_of(L), side, tidx, size, m.lob_time);
                    rest_price = price; rest_qty = size;
                } else {                                      // remove and re-process with the same order id
                    if (tidx < 0) { book_remove(bk, side, nside, idx, 1, lane); mkt_set_n(m, side, nside - 1); }
                    else { cold_tail_remove(lds_addr_of(L), side, tidx); sync_tail_status(L, m); }
                    do_match = true; can_rest = true; m_limit = price; rest_oid = ooid;
                }
                TACC_END(m, 6);
            }
        }
    }
    if (m.next_oid >= (1 << 27)) m.flags |= CDA_FLAG_INT_OVERFLOW;
    TACC_END(m, 4);
    if (do_match) {
        int32_t left = match<TAILS, LAZY_POSVAL, TAPE>(L, m, tr, side, size, m_limit, lane);
        TACC_END(m, 2);
        if (left > 0 && can_rest) {
            const int nown = mkt_n(m, side);
            bool rested = true;
            if ((!TAILS || !mkt_has_tail(m, side)) && nown + mkt_n(m, side ^ 1) < CAP) {       // the side is its tile and the pool has room
                book_insert(bk, side, nown, price, left, tr, rest_oid, m.lob_time, lane);
                mkt_set_n(m, side, nown + 1);
            } else if (TAILS && L.tl[TL_CAP] != 0) {          // the HBM tier takes what the tile cannot (ordertree.py:5-58 is unbounded)
                const uint32_t c = cold_insert(lds_addr_of(L), pack_counts(m.nb, m.na), side, price, left, oo_pack(rest_oid, tr), m.lob_time);
                set_counts(m, c);
                sync_tail_status(L, m);
                rested = (c >> 31) == 0;
            } else rested = false;                            // an env built without the HBM tier (book_spill = -1): the pool is the book
            if (rested) { rest_price = price; rest_qty = left; m.peak_orders = max(m.peak_orders, TAILS ? total_orders(L, m) : m.nb + m.na); }
            else m.flags |= CDA_FLAG_BOOK_OVERFLOW;
        }
        TACC_END(m, 3);
    }
    TACC_END(m, 4);
    if (rest_qty > 0 && !CDA_MKT_DBG(m, 0x200)) { cash_hold_transfer(L, tr, rest_price, rest_qty, -1, f, lane); TACC_COUNT(m, 11, 1); }
    TACC_END(m, 8);
    if (__ballot(f != 0)) m.flags |= CDA_FLAG_DEC_DOMAIN;
    if constexpr (TAILS) {
        if (m.status & ST_TAIL_ANY) {                         // a cancel / modify may have emptied a tile whose side continues in HBM
            set_counts(m, cold_rebalance(lds_addr_of(L), pack_counts(m.nb, m.na)));
            sync_tail_status(L, m);
        }
    }
}

// Exchg_Helper.mark_to_mkt + Calculate.mark_to_mkt (exchg_helper.py:56-66, calculate.py:35-55)
__device__ __forceinline__ void mark_to_mkt(Lds& L, Mkt& m, int A, int lane) {
    if (!m.has_trade) return;
    m.last_price = m.last_trade_price;
    uint32_t f = 0;
    // Three independent chains per account run on the owner lane and its two helpers in the same instruction stream:
    //   group 0: diff = +-(p - VWAP), profit = diff * |pos|      group 1: raw = VWAP * |pos|      group 2: cash + cash_on_hold
    // then the owner finishes position_val = raw + profit, nav = (cash + hold) + position_val: 4 dependent operations, not 6.
    const int g = lane_grp(lane), al = lane_acc(lane);
    const bool act = al < A && g < 3;
    // stage 1 (g0): diff = +-(p - VWAP); stage 2 (g0, g1): profit = diff * |pos|, raw = VWAP * |pos|; stage 3, ONE addition site
    // for two lanes: g0 position_val = raw + profit, g2 cash + cash_on_hold; stage 4 (g0): nav = (cash + hold) + position_val.
    D r1 = d_zero(), r2 = d_zero();
    uint32_t ap = 0;
    if (act && g != 2) {
        const Acc& a = L.acc[al];
        int32_t pos = a.net_position;
        ap = (uint32_t)(pos < 0 ? -pos : pos);
        D vwap = ld_dec(a.vwap);
        if (g == 0) {
            D p = d_price(m.last_trade_price);
            r1 = d_add(pos >= 0 ? p : vwap, d_neg(pos >= 0 ? vwap : p));
        }
        r2 = d_mul_int(g == 0 ? r1 : vwap, ap);
    }
    D raw = d_shfl(r2, (lane + 16) & 63);
    D s3 = d_zero();
    if (act && g != 1) {
        const Acc& a = L.acc[al];
        const D x = g == 0 ? raw : ld_dec(a.cash), y = g == 0 ? r2 : ld_dec(a.hold);
        s3 = d_add(x, y);
    }
    D ssum = d_shfl(s3, (lane + 32) & 63);
    if (act && g == 0) {
        Acc& a = L.acc[al];
        D nav = d_add(ssum, s3);
        a.prev_nav = a.nav;
        st_dec(a.posval, s3, f); st_dec(a.nav, nav, f);
        if (d_cmp(nav, ld_dec(a.max_nav)) > 0) st_dec(a.max_nav, nav, f);
    }
    CDA_WSYNC();
    if (__ballot(f != 0)) m.flags |= CDA_FLAG_DEC_DOMAIN;
}

// ======================================================================================
// Observation (State_Helper.set_agg_LOB, exchg/state_helper.py:113-214)
// ======================================================================================
// top-K aggregation per side -> L.lvl_px / L.lvl_sz (integers; 0 = empty level)
template <bool TAILS>
__device__ __forceinline__ void aggregate_levels(Lds& L, const Mkt& m, int lane) {
    if (lane < 2 * CDA_K_ROWS) { (&L.lvl_px[0][0])[lane] = 0; (&L.lvl_sz[0][0])[lane] = 0; }
    CDA_WSYNC();
    #pragma unroll
    for (int s = 0; s < 2; s++) {
        int carry = 0, n = mkt_n(m, s);
        for (int base = 0; base < n && carry <= CDA_K_ROWS; base += WAVE) {
            int i = base + lane;
            bool valid = i < n;
            int p = valid ? L.book.price[s][i] : 0;
            int pp = (valid && i > 0) ? L.book.price[s][i - 1] : -1;
            const int q = valid ? L.book.qty[s][i] : 0;                  // requested with the prices: one LDS round trip
            bool head = valid && (i == 0 || p != pp);
            uint64_t mk = __ballot(head);
            uint64_t le = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
            int lvl = carry + __popcll(mk & le) - 1;
            if (valid && lvl < CDA_K_ROWS) {
                atomicAdd(&L.lvl_sz[s][lvl], q);
                if (head) L.lvl_px[s][lvl] = p;
            }
            carry += __popcll(mk);
        }
        if constexpr (TAILS) { if (carry <= CDA_K_ROWS && mkt_has_tail(m, s)) cold_aggregate(lds_addr_of(L), s, n, carry); }     // the levels continue in HBM
    }
    CDA_WSYNC();
}
// raw f32[40] = agg_LOB_raw (state_helper.py:159-160); empty ask levels stay +0.0
__device__ __forceinline__ float raw_value(const Lds& L, int j) {
    int row = j / CDA_K_ROWS, k = j % CDA_K_ROWS;
    int v = row == 0 ? L.lvl_px[0][k] : row == 1 ? L.lvl_sz[0][k] : row == 2 ? L.lvl_px[1][k] : L.lvl_sz[1][k];
    float f = (float)v;
    return (row >= 2 && v != 0) ? -f : f;
}
// one normalised snapshot value for lane j in [0,42)
__device__ __forceinline__ float snapshot_value(const Lds& L, const Mkt& m, int tick, int j) {
    double l1_bid = (double)L.lvl_px[0][0], l1_ask = (double)L.lvl_px[1][0], M;
    bool two = l1_bid > 0 && l1_ask > 0;
    if (two) M = (l1_bid + l1_ask) / 2.0;
    else if (l1_bid > 0) M = l1_bid;
    else if (l1_ask > 0) M = l1_ask;
    else { M = (double)m.last_price; if (M <= 0) M = 100.0; }
    double out;
    if (j < 40) {
        // rows 0 / 2 (bid / ask price distance) share one division, rows 1 / 3 (sizes) one square root: the 20 + 20 lanes of
        // a row pair run ONE instruction sequence instead of two
        const int row = j / CDA_K_ROWS, k = j % CDA_K_ROWS, side = row >> 1;
        const double raw = (double)((row & 1) ? L.lvl_sz[side][k] : L.lvl_px[side][k]);
        if (raw == 0.0) out = 0.0;                                     // empty level (raw values are never negative)
        else if (row & 1) { const double r = sqrt(raw); out = side ? -r : r; }
        else { const double q = (side ? raw - M : M - raw) / M; out = side ? -q : q; }
    } else {
        // lanes 40 (log M) and 41 (log1p of the spread in ticks) share ONE evaluation: M is a half-integer, M - 1 is exact, and
        // float32(log1p(M - 1)) == float32(numpy.log(M)) == float32(libm log(M)) for EVERY M = k/2 with k <= 2^25, i.e. for every
        // mid of two prices below 2^24 ticks (the price clamp of step_market) - swept exhaustively by tools/sweep_libm.py, so
        // there is no separate log().  log1p(+0) = +0 covers the one-sided book.
        double arg = 0.0;
        if (j == 40) arg = M - 1.0;
        else if (two) { double st = (l1_ask - l1_bid) / (double)tick; arg = st > 0.0 ? st : 0.0; }
        out = glibc_log1p(arg);
    }
    return (float)out;
}

