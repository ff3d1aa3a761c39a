/*
 * cda.h - C-ABI of the MI355X-native vectorised continuous-double-auction environment.
 *
 * This is the drop-in boundary for ONE hot path of ChuaCheowHuan/gym-continuousDoubleAuction:
 * reset()/step() of the multi-agent limit-order-book env, batched over N independent markets.
 * The reference has no FFI; its boundary is the Python class
 *   gym_continuousDoubleAuction/envs/continuousDoubleAuction_env.py:21  (continuousDoubleAuctionEnv)
 * bound at gym_continuousDoubleAuction/train/train.py:441-443 (tune.register_env) and
 * gym_continuousDoubleAuction/__init__.py:18-21 (gymnasium.register).  Each entry point below
 * names the reference method it replaces.  A maintainer binds it with ctypes;
 * the in-tree Python host side (gym_continuousdoubleauction_amd/vec_env.py, env.py) is that binding.
 *
 * Conventions
 *  - every function returns CDA_OK (0) or a negative cda_status; nothing throws or exits;
 *  - array arguments are caller-owned DEVICE pointers (e.g. torch tensors' data_ptr()) unless the
 *    name ends in _host; the library owns only the opaque cda_env arena;
 *  - kernels are enqueued on the caller's HIP stream (`stream` is a hipStream_t, NULL = default
 *    stream) and are asynchronous; calls on one cda_env are not re-entrant;
 *  - there is NO CPU fallback: cda_create fails with CDA_ERR_NO_DEVICE when no gfx950 GPU is present.
 */
#ifndef CDA_H
#define CDA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Observation layout: config/tunable_constants.json:8-10 (k_rows 10, book_rows 4, extra_dim 2). */
#define CDA_K_ROWS        10
#define CDA_BOOK_ROWS     4
#define CDA_EXTRA_DIM     2
#define CDA_SNAPSHOT_DIM  42            /* book_rows*k_rows + extra_dim */
#define CDA_RAW_DIM       40            /* agg_LOB_raw: state_helper.py:159-160 */
#define CDA_MAX_HIST      16            /* n_hist upper bound of this build (reference default 4) */
#define CDA_TICK_MAX      65536         /* tick_size upper bound: prices live below 2^24, a ladder of ten levels of the largest tick still fits */
#define CDA_MAX_AGENTS    16            /* agents per market upper bound of this build */
#define CDA_BOOK_CAP      256           /* default LDS book tile: the top of a market's book, both sides together (cda_config.book_capacity) */
#define CDA_BOOK_CAP_MAX  512           /* the larger compiled tile; also sizes the arrays of the fixed-size parity dump (cda_market_state) */
#define CDA_SPILL_MIN     64            /* smallest / largest HBM spill ring per side (cda_config.book_spill, a power of two) */
#define CDA_SPILL_MAX     (1 << 20)
#define CDA_NUM_REWARD_TERMS 5          /* reward_helper.py:75-81 */
#define CDA_MAX_GROUPS    16            /* cda_step_groups: concurrent market groups per env */

typedef enum cda_status {
    CDA_OK = 0,
    CDA_ERR_INVALID = -1,       /* bad argument / config outside the supported domain */
    CDA_ERR_NO_DEVICE = -2,     /* no HIP device (the product path has no CPU fallback) */
    CDA_ERR_HIP = -3,           /* a HIP runtime call failed; see cda_strerror */
    CDA_ERR_UNSUPPORTED = -4,   /* a tick_size outside 1 .. CDA_TICK_MAX (the config carries integer ticks only: SURVEY App. A.10); a launch this env does not qualify for */
    CDA_ERR_NOMEM = -5
} cda_status;

/* Per-market sticky flag bits reported by cda_last_flags. */
#define CDA_FLAG_BOOK_OVERFLOW   0x1u   /* a rest was dropped: the market's book (LDS tile + HBM spill ring) was full */
#define CDA_FLAG_INT_OVERFLOW    0x2u   /* a size/position/price left the int32 / 2^24 domain */
#define CDA_FLAG_DEC_DOMAIN      0x4u   /* a ledger value left the 28-digit / exponent domain */
#define CDA_FLAG_NAV_CONSERVATION 0x8u  /* episode metrics (cda_episode_metrics_enable): an episode of this market ended with sum(NAV) != num_agents * init_cash
                                           beyond the tolerance; unlike the others it survives the device-side auto reset */

/*
 * Env config: the 17 keys of continuousDoubleAuction_env.py:27-55 with the defaults of
 * config/env_defaults.json:8-27 (is_render and tape_display_length do not reach the numeric path).
 */
typedef struct cda_config {
    int32_t num_agents;          /* num_of_agents        (5)       */
    int32_t max_step;            /* max_step             (64)      */
    int32_t n_hist;              /* n_hist               (4)       */
    int32_t tick_size;           /* tick_size            (1) - an INTEGER tick, 1 .. CDA_TICK_MAX: the price ladder's step (action_helper.py:341-397) and the unit of the
                                    observation's spread (state_helper.py:202-206); off the integer grid the reference's float price arithmetic is platform dependent */
    int64_t init_cash;           /* init_cash            (1000000) - integer, > -2^62 */
    int32_t initial_price_min;   /* initial_price_min    (10)      */
    int32_t initial_price_max;   /* initial_price_max    (100)     */
    int32_t min_size;            /* min_size             (1) - at least 1: a decoded size is rint(|sample|) + min_size, and the reference has no behaviour for an order
                                    of quantity 0 (its process_order exits); with the two below: min_size <= mkt_max_size, limit_size_multiple >= 1 and
                                    mkt_max_size * limit_size_multiple + min_size <= 2^30 / CDA_BOOK_CAP_MAX = 2^21 */
    int32_t mkt_max_size;        /* mkt_max_size         (100)     */
    int32_t limit_size_multiple; /* limit_size_multiple  (10)      */
    int32_t auto_reset;          /* extension, 0 = off (the reference has no such key; parity runs leave it 0). 1: a market whose
                                    step ended its episode (terminated or truncated) is reset in place right after that step, with
                                    reset(seed=None) semantics (the RNG stream continues, continuousDoubleAuction_env.py:186-188);
                                    its obs row then holds the NEW episode's first observation, reward / flags / info are the
                                    finished step's */
    int32_t book_capacity;       /* extension: size of the LDS-staged book TILE, the top of a market's book, both sides together:
                                    256 or 512 resting orders (two compiled builds of the market kernels); 0 = by agent count: 256 up
                                    to 8 agents, 512 above.  What does not fit the tile lives in the HBM spill ring below */
    int32_t book_spill;          /* extension: resting orders PER SIDE a market can hold in HBM behind its tile (the reference's
                                    OrderTree is unbounded, ordertree.py:5-58).  0 = automatic: num_agents * max_step rounded up to a
                                    power of two (at least 1024) - a side cannot grow faster than one order per agent and step, so
                                    no order is ever dropped inside an episode (halved, down to CDA_SPILL_MIN, while the rings of all markets would take more than a
                                    quarter of the free device memory: compare cda_book_spill / cda_book_spill_wanted); n > 0: rounded up to a power of two in
                                    [CDA_SPILL_MIN, CDA_SPILL_MAX]; -1: no HBM tier (the round-1/2 behaviour: the tile is the whole
                                    book).  A rest that fits neither is dropped and flagged (CDA_FLAG_BOOK_OVERFLOW), never silently */
    double  order_penalty;       /* 0.1  */
    double  trade_penalty;       /* 0.05 */
    double  drawdown_penalty;    /* 0.2  */
    double  passive_bonus;       /* 0.1  */
    double  loss_multiplier;     /* 1.5  */
} cda_config;

/*
 * A ledger value: Python `Decimal` (prec 28, ROUND_HALF_EVEN) as sign / coefficient / exponent.
 * value = (-1)^sign * (w[0] + w[1]*2^32 + w[2]*2^64) * 10^exp, coefficient < 10^28.
 * `str(Decimal)` is reproduced on the host from this triple (info["NAV"], info_helper.py:54).
 */
typedef struct cda_dec {
    uint32_t w[3];
    int16_t  exp;
    uint8_t  sign;
    uint8_t  pad;
} cda_dec;

/* Optional SoA outputs mirroring Info_Helper.set_info (info_helper.py:30-116). Any pointer may be NULL. */
typedef struct cda_info_ptrs {
    cda_dec* nav;                    /* [N,A]  exact NAV (info["NAV"] = str of this)        */
    int32_t* num_trades;             /* [N,A]                                                */
    int32_t* net_position;           /* [N,A]                                                */
    double*  vwap;                   /* [N,A]  float(acc.VWAP)                               */
    double*  cash;                   /* [N,A]                                                */
    double*  cash_on_hold;           /* [N,A]                                                */
    double*  position_val;           /* [N,A]                                                */
    double*  drawdown;               /* [N,A]                                                */
    double*  max_nav;                /* [N,A]                                                */
    int32_t* num_trades_step;        /* [N,A]  read before zeroing (exchg_helper.py:116-120)  */
    int32_t* num_passive_fills_step; /* [N,A]                                                */
    int32_t* order_step_placed;      /* [N,A]                                                */
    int32_t* num_rejected_step;      /* [N,A]                                                */
    uint8_t* is_pass_action;         /* [N,A]                                                */
    double*  reward_terms;           /* [N,A,5] nav_term, order, trade, drawdown, passive    */
    double*  last_price;             /* [N]                                                  */
    double*  best_bid;               /* [N]  NaN encodes None                                */
    double*  best_ask;               /* [N]  NaN encodes None                                */
    double*  spread;                 /* [N]  NaN encodes None                                */
    int32_t* lob_actions;            /* [N,A,4] env.LOB_actions (continuousDoubleAuction_env.py:284-285): agent a's decoded order
                                        {side 0 bid / 1 ask, type 0 market / 1 limit / 2 modify / 3 cancel, size, price in ticks or
                                        -1 for a market order}; side = -1 (row all -1) when the agent passed or was absent  */
} cda_info_ptrs;

/* ---- parity dump of one market (host struct) ------------------------------------------- */
typedef struct cda_order {
    int32_t price;      /* integer ticks (the book's Decimal('<price>.0')) */
    int32_t qty;
    int32_t owner;      /* trader index = Order.trade_id (order.py:17)      */
    int32_t order_id;
    int32_t timestamp;
} cda_order;

typedef struct cda_account_state {
    cda_dec cash, cash_on_hold, position_val, vwap, nav, prev_nav, max_nav;
    int32_t net_position, num_trades;
    int32_t num_trades_step, num_passive_fills_step, order_step_placed, num_rejected_step;
} cda_account_state;

/* The dump holds the first CDA_BOOK_CAP_MAX orders of each side; n_bids / n_asks are the TRUE counts and MAY EXCEED the arrays (since round 3:
 * the book is unbounded; cda_get_book reads a side of any length).  A C caller walking the arrays must stop at
 * min(n_bids, CDA_BOOK_CAP_MAX) / min(n_asks, CDA_BOOK_CAP_MAX).  cda_set_state with a count above CDA_BOOK_CAP_MAX means "keep the book as it is"
 * (the counts must equal the market's current ones) and restores everything else of the dump. */
typedef struct cda_market_state {
    uint64_t rng_state_hi, rng_state_lo, rng_inc_hi, rng_inc_lo;  /* numpy PCG64 */
    uint32_t rng_has_uint32, rng_uinteger;
    int32_t  t_step, lob_time, next_order_id;
    int32_t  last_price;          /* env.last_price (integer valued at tick_size 1) */
    int32_t  has_trade;           /* len(LOB.tape) > 0 */
    int32_t  last_trade_price;    /* LOB.tape[-1]['price'] */
    uint32_t done_mask;           /* env.done_set as a bit mask */
    uint32_t flags;
    int32_t  n_bids, n_asks;
    cda_order bids[CDA_BOOK_CAP_MAX]; /* queue order: best price first, FIFO inside a level */
    cda_order asks[CDA_BOOK_CAP_MAX];
    cda_account_state acc[CDA_MAX_AGENTS];
    float    hist[CDA_MAX_HIST * CDA_SNAPSHOT_DIM];  /* oldest frame first */
} cda_market_state;

typedef struct cda_env cda_env;

/* Fill `cfg` with config/env_defaults.json:8-27. */
int cda_default_config(cda_config* cfg);

/* Replaces continuousDoubleAuctionEnv.__init__ (continuousDoubleAuction_env.py:27-119) for
 * n_markets independent envs on HIP device `device`. */
int cda_create(const cda_config* cfg, int32_t n_markets, int32_t device, cda_env** out);
int cda_destroy(cda_env* env);

/* Replaces reset(seed=...) (continuousDoubleAuction_env.py:175-231).
 *  seeds : u64[N] device, or NULL = seed=None (every selected market keeps its RNG stream;
 *          a market that was never seeded is seeded with its index);
 *  mask  : u8[N] device, or NULL = all markets;   obs_out : f32[N, n_hist*42] (rows of unselected
 *          markets are left untouched). */
int cda_reset(cda_env* env, const uint64_t* seeds, const uint8_t* mask, float* obs_out, void* stream);

/* Replaces step(action_dict) (continuousDoubleAuction_env.py:265-309).
 *  category i32[N,A], size_mean f32[N,A], size_sigma f32[N,A], price i32[N,A], price_offset i32[N,A]:
 *  the Dict action of action_helper.py:126-138; `present` u8[N,A] or NULL (= every agent acts)
 *  encodes an action dict holding a subset of the agents, iterated in ascending agent order.
 *  Out: obs f32[N,n_hist*42] (one shared vector per market, state_helper.py:76,109),
 *  reward f64[N,A], terminated u8[N] / truncated u8[N] (the "__all__" flags, done_helper.py:20-54),
 *  info (nullable). */
int cda_step(cda_env* env,
             const int32_t* category, const float* size_mean, const float* size_sigma,
             const int32_t* price, const int32_t* price_offset, const uint8_t* present,
             float* obs_out, double* reward_out, uint8_t* terminated_out, uint8_t* truncated_out,
             const cda_info_ptrs* info_out, void* stream);

/* The same step for the markets [first_market, first_market + n_markets) only.  Every array argument is still the
 * FULL [N, ...] array (the kernel indexes it by global market); only the launch covers fewer markets.  Markets never
 * interact, so disjoint sub-ranges of one env may be stepped CONCURRENTLY on different streams: the reference's step()
 * has no cross-env barrier either (one env object per market, continuousDoubleAuction_env.py:86,197), the batch-wide
 * barrier of cda_step is an artefact of launching all markets as one grid. */
int cda_step_range(cda_env* env, int32_t first_market, int32_t n_markets,
                   const int32_t* category, const float* size_mean, const float* size_sigma,
                   const int32_t* price, const int32_t* price_offset, const uint8_t* present,
                   float* obs_out, double* reward_out, uint8_t* terminated_out, uint8_t* truncated_out,
                   const cda_info_ptrs* info_out, void* stream);
int cda_reset_range(cda_env* env, int32_t first_market, int32_t n_markets, const uint64_t* seeds, const uint8_t* mask,
                    float* obs_out, void* stream);
/* cda_step_range with EPISODE-END CAPTURE (auto_reset envs only; fin_index_out NULL = plain cda_step_range).  The device-side auto reset overwrites the
 * finished episode's last observation in obs_out with the new episode's first one; the reference's consumers still need the old one - RLlib bootstraps a
 * time-limit truncation with V(last observation) (the env's `truncateds`, continuousDoubleAuction_env.py:303), its episode record stores it with the
 * last step (train/episode_record.py:431-470).  A market whose episode ended with this step therefore appends that observation to a compact list first:
 * slot = atomicAdd(fin_count, 1); if slot < fin_cap: fin_obs[slot][n_hist * 42] = the observation, fin_index_out[market] = slot.  fin_index_out i32[N]
 * is pre-set to -1 and fin_count i32[1] zeroed by the caller.  Cold paths only: the step's hot code is unchanged. */
int cda_step_range_capture(cda_env* env, int32_t first_market, int32_t n_markets,
                           const int32_t* category, const float* size_mean, const float* size_sigma,
                           const int32_t* price, const int32_t* price_offset, const uint8_t* present,
                           float* obs_out, double* reward_out, uint8_t* terminated_out, uint8_t* truncated_out,
                           const cda_info_ptrs* info_out, float* fin_obs, int32_t fin_cap, int32_t* fin_count, int32_t* fin_index_out, void* stream);
/* The rollout's POLICY INSIDE THE STEP KERNEL (one launch per chain and step instead of a policy launch and a step launch): for the markets of the range, the
 * policy / value network of include/cda_mlp.h (wb, theta: cda_mlp_pack's images for the env's history depth) is evaluated on obs_in f32 [N][42 n_hist] by the step kernel's own
 * workgroups (sixteen market-waves each: bf16 MFMA on their sixteen rows), every agent's action is sampled exactly as cda_mlp_policy_step samples it (same key:
 * seed, *counter_dev, draw = the step's number; bit for bit the same actions, log-probabilities, values, records), WRITTEN to the five action arrays / a_cont /
 * logp / value / rec (may be NULL) / dist (may be NULL), and the markets are stepped with them exactly as cda_step_range_capture steps them (same outputs, same
 * auto reset and episode-end capture).  What the reference does between two env.step calls - RLlib's policy forward + action sampling, train/train.py:453-541 -
 * moved into the step itself.  cda_policy_step_supported: 1 when this env qualifies (256-order book tile, n_hist 1 / 2 / 4 / 8 - the depths the network is
 * compiled for -, <= 8 agents, no hand-back records);
 * otherwise cda_policy_step_range returns CDA_ERR_UNSUPPORTED and the caller launches the two kernels (cda_mlp_rollout_chain does). */
int cda_policy_step_supported(const cda_env* env);
int cda_policy_step_advised(const cda_env* env);      /* supported AND the env's markets fit the device in one round of sixteen-market workgroups (N <= 16 x CUs): where the one launch wins */
int cda_policy_step_range(cda_env* env, int32_t first_market, int32_t n_markets, const void* wb, const float* theta, const float* obs_in,
                          uint64_t seed, const int64_t* counter_dev, int64_t draw,
                          int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset,
                          float* a_cont, float* logp, float* value, float* rec, float* dist,
                          float* obs_out, double* reward_out, uint8_t* terminated_out, uint8_t* truncated_out,
                          float* fin_obs, int32_t fin_cap, int32_t* fin_count, int32_t* fin_index_out, void* stream);
/* The same ONE launch for every other network of include/cda_mlp.h: activation = the hidden activation's code (0 tanh, 1 relu, 2 elu, 3 linear: CDA_MLP_ACT of the
 * network objects), vf_share_layers = 1 for the shared trunk (the _vfs objects; wb / theta are that network's images).  cda_policy_step_range is the tanh network with
 * its own value network, fixed at compile time (k_policy_step); these entry points launch k_net_step, one kernel per history depth that reads the two choices from
 * its arguments - the activation in the two hidden layers' epilogues, the trunk by idling the value half's waves - and is otherwise the same code: bit for bit the
 * actions, log-probabilities, values, records and step outputs of that network's cda_mlp_policy_step followed by cda_step_range_capture.  (0, 0) forwards to
 * cda_policy_step_range.  An activation outside 0 .. 3 or vf_share_layers outside 0 / 1: CDA_ERR_INVALID from all three, before anything is launched.
 * cda_net_step_supported: cda_policy_step_supported's conditions on the env - they do not depend on the network; cda_net_step_advised: cda_policy_step_advised's
 * rule, N <= 16 x CUs, for every network (profiles/net_step/cost.txt).  cda_net_step_range's arguments behind the two codes are cda_policy_step_range's. */
int cda_net_step_supported(const cda_env* env, int32_t activation, int32_t vf_share_layers);
int cda_net_step_advised(const cda_env* env, int32_t activation, int32_t vf_share_layers);
int cda_net_step_range(cda_env* env, int32_t activation, int32_t vf_share_layers,
                       int32_t first_market, int32_t n_markets, const void* wb, const float* theta, const float* obs_in,
                       uint64_t seed, const int64_t* counter_dev, int64_t draw,
                       int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset,
                       float* a_cont, float* logp, float* value, float* rec, float* dist,
                       float* obs_out, double* reward_out, uint8_t* terminated_out, uint8_t* truncated_out,
                       float* fin_obs, int32_t fin_cap, int32_t* fin_count, int32_t* fin_index_out, void* stream);
/* One-launch steps (cda_policy_step_range / cda_net_step_range launches) enqueued on this env since cda_create: a host-side counter - an enqueue inside a stream
 * capture counts once, replays of the captured graph do not.  Tells a caller (and a test) which path a rollout chain took.  NULL env: 0. */
int64_t cda_policy_step_launch_count(const cda_env* env);
/* cda_step as n_groups (<= CDA_MAX_GROUPS) launches, group g = the markets cda_group_range() names, on streams[g].
 * One host call; each group is an independent chain of launches on its own stream, so one group's slowest market
 * overlaps the other groups' work instead of stalling the whole batch.  The outputs of group g are complete when
 * streams[g] reaches this point; ordering against other streams is the caller's business (events). */
int cda_step_groups(cda_env* env, int32_t n_groups,
                    const int32_t* category, const float* size_mean, const float* size_sigma,
                    const int32_t* price, const int32_t* price_offset, const uint8_t* present,
                    float* obs_out, double* reward_out, uint8_t* terminated_out, uint8_t* truncated_out,
                    const cda_info_ptrs* info_out, void* const* streams);
/* markets of group `group` of `n_groups`: [first, first + count) with first = N*group/n_groups (integer division) */
void cda_group_range(int32_t n_markets, int32_t n_groups, int32_t group, int32_t* first_out, int32_t* count_out);

/* The hand-back to a central learner (north_star: "RCCL all-gather over xGMI only for the observation/reward tensors handed
 * back to the learner"; the reference hands step()'s return value to RLlib in-process, train/train.py:509-518).  Of a market's
 * n_hist x 42 observation only the newest frame is new each step, so what has to travel is ONE compact record per market:
 *
 *     f32 frame[42]   the newest observation frame (state_helper.py:94-111 appends it to the history)
 *     f64 reward[A]
 *     u8  terminated, truncated      the "__all__" flags
 *     u8  restarted                   1: the observation restarts from `frame` (reset / auto-reset: all n_hist frames equal it)
 *     padding to cda_handback_stride(A) bytes (a multiple of 8)
 *
 * cda_set_handback(env, records): from now on every step (and reset) ALSO writes records[market] (device, [N, stride] bytes;
 * NULL switches it off).  The records of a contiguous market range are contiguous, so a group chain hands its own range to
 * the collective where the kernel left it.  cda_handback_unpack is the receiving side, for ANY process (it needs no env):
 * n_segments x seg_records records (an all-gathered buffer: one segment per rank), record k of segment s belonging to row
 * row0 + s * seg_row_stride + k of the learner's full arrays - the observation row is shifted by one frame and the new frame
 * appended (or, restarted, all frames set), reward / flags rows are overwritten.  One launch.  (n_rows_total: see cda_set_handback_geometry.) */
int32_t cda_handback_stride(int32_t num_agents);
int cda_set_handback(cda_env* env, void* records_dev);
int cda_handback_unpack(const void* records_dev, int32_t n_segments, int32_t seg_records, int64_t seg_row_stride, int64_t row0,
                        int32_t num_agents, int32_t n_hist, int64_t n_rows_total,
                        float* obs_full, double* reward_full, uint8_t* terminated_full, uint8_t* truncated_full, void* stream);
/* Uneven shards (n_rows_total not divisible by the rank count): every rank steps and sends the SAME number of records - the largest shard,
 * the smaller ones padded with markets nobody reads - and the receiving side skips the padding: with n_rows_total > 0, segment s owns
 * seg_row_stride rows (the last one n_rows_total - s * seg_row_stride) and record k of it is used only while row0 + k is below that.
 * n_rows_total = 0: every record is used (equal shards).  cda_set_handback_geometry gives the native chains (cda_step_groups_handback,
 * cda_handback_groups) the same two numbers: rows between two ranks' first markets, global row count (0, 0 = equal shards of N). */
int cda_set_handback_geometry(cda_env* env, int64_t shard_row_stride, int64_t n_rows_total);

/* cda_step_groups AND the hand-back of every chain in ONE host call (a Python loop over chains - stream context, collective, unpack -
 * costs ~25 us of host time per chain and step, more than the step itself): on streams[g], for the markets of group g,
 *     k_step  ->  ncclAllGather(this rank's records of group g -> gathered[g], world x count x stride bytes)  ->  cda_handback_unpack
 * into the learner-side arrays (row of global market = rank * shard_rows + local market).  comms[g] is an RCCL communicator
 * (ncclComm_t) the caller created for chain g - one per chain, so that the chains' collectives may be in flight together; the library
 * resolves ncclAllGather from the RCCL already loaded in the process (no link-time dependency).  world == 1: comms may be NULL, the
 * records are unpacked where the kernel left them.  Needs cda_set_handback. */
int cda_step_groups_handback(cda_env* env, int32_t n_groups,
                             const int32_t* category, const float* size_mean, const float* size_sigma,
                             const int32_t* price, const int32_t* price_offset, const uint8_t* present,
                             float* obs_out, double* reward_out, uint8_t* terminated_out, uint8_t* truncated_out,
                             const cda_info_ptrs* info_out, void* const* streams,
                             void* const* comms, int32_t world, void* const* gathered,
                             float* obs_full, double* reward_full, uint8_t* terminated_full, uint8_t* truncated_full);
/* the hand-back alone (after a reset: its records carry `restarted`), same arguments */
int cda_handback_groups(cda_env* env, int32_t n_groups, void* const* streams, void* const* comms, int32_t world, void* const* gathered,
                        float* obs_full, double* reward_full, uint8_t* terminated_full, uint8_t* truncated_full);

/* Replaces CDA_rand.run_random (CDA_rand.py:40-85): every market plays uniform random agents (the law and the
 * counter-based sampler of include/cda_random_agents.h, keyed by action_seed, market_index_base + market, the
 * market's own step counter and the agent) for up to n_steps steps, stopping early at its episode's end
 * (terminated or truncated), ALL INSIDE ONE LAUNCH: a market-wave keeps its state in LDS from step to step and
 * never waits for the slower markets of the batch.  Bit-identical to n_steps calls of cda_step on the same actions.
 *  Out (each nullable): obs f32[N,n_hist*42] after the last step taken, episode_return f64[N,A] = the sum, in step
 *  order, of each agent's rewards over the steps taken, terminated / truncated u8[N] of the last step taken (0 if
 *  none), steps_taken i32[N]. */
int cda_run_random(cda_env* env, int32_t n_steps, uint64_t action_seed, uint64_t market_index_base,
                   float* obs_out, double* episode_return_out, uint8_t* terminated_out, uint8_t* truncated_out,
                   int32_t* steps_taken_out, void* stream);
/* The same sampler on the host (host pointers, [n_markets, num_agents] each): the actions cda_run_random plays at
 * step `step`, for callers and tests that want to replay them through cda_step. */
int cda_random_actions_host(uint64_t action_seed, uint64_t market_index_base, int32_t step, int32_t n_markets,
                            int32_t num_agents, int32_t* category, float* size_mean, float* size_sigma,
                            int32_t* price, int32_t* price_offset);

/* The same sampler on the device: the actions of steps [step0, step0 + n_steps), five [n_steps, n_markets, num_agents]
 * device arrays - the resident synthetic input of bench.py (generator keyed (seed, step, market, agent)). */
int cda_random_actions(uint64_t action_seed, uint64_t market_index_base, int32_t step0, int32_t n_steps, int32_t n_markets,
                       int32_t num_agents, int32_t* category, float* size_mean, float* size_sigma, int32_t* price,
                       int32_t* price_offset, void* stream);

/* The reference's end-of-episode invariant (train/callbk/league_based_self_play_callback.py:679-704) for every market, on
 * the device: total = Decimal(0); total += NAV_a for a = 0..A-1 (the accounts' current NAV, in that order, prec-28
 * arithmetic); error = total - Decimal(init_cash) * A.  abs_error_out f64[N] (device) receives float(abs(error)),
 * violated_out u8[N] (device, nullable) whether it exceeds `tolerance` (the reference's nav_tolerance, 1e-6). */
int cda_nav_conservation(cda_env* env, double tolerance, double* abs_error_out, uint8_t* violated_out, void* stream);

/* ---- every episode checked and summarised on the device --------------------------------------------------------------------
 * What the reference's callback does around an episode (train/callbk/league_based_self_play_callback.py):
 *   on_episode_step (:541-600)   tallies per episode: passes, rejections, per-agent trades / passive fills, sum and sum of squares of the five reward terms;
 *   on_episode_end  (:627-755)   sum of the agents' NAV == num_agents x init_cash in Decimal (nav_tolerance 1e-6), `nav_conservation_violations` += 1 otherwise;
 *                                per-agent NAV / drawdown / |net_position| / num_trades of the last step (_log_episode_account :418-470); pass and rejection
 *                                fractions, reward-term means and variance shares, the most maker-like agent's passive share (_log_activity :295-416);
 *   train.py:1109-1164           the driver stops the run on a violation (strict_nav_check).
 * With auto_reset the finished episode's ledger is wiped by the in-kernel reset before any host code could look at it, so all of it happens on the
 * device.  cda_episode_metrics_enable(env, 1, tolerance): from now on
 *   - every step adds agent a's step counters and reward terms to the running tallies of (market, a) in the market record (fire-and-forget atomics:
 *     nothing is loaded and no register is held across the step);
 *   - a market whose episode ended (all agents done, or max_step reached) is CHECKED AND CREDITED exactly once, in the cold paths that handle an episode
 *     end - the in-kernel auto reset of cda_step / cda_policy_step_range, the auto-reset pass behind a step with info tensors, cda_reset of a market
 *     whose episode is over, the end of cda_run_random: the exact decimal sum of NAV (the arithmetic of cda_nav_conservation) sets the sticky
 *     CDA_FLAG_NAV_CONSERVATION bit (it survives the auto reset) and counts a violation; the tallies and the last step's account figures are added
 *     to per-(market, agent) and per-market accumulators;  a reset of a market whose episode is NOT over discards its running tallies (an episode
 *     the reference's callback never sees end either).
 * An episode IN FLIGHT at the call: cda_episode_metrics_enable (on or off) zeroes every market's running tallies and touches nothing else.  An episode that is
 * under way at an enable is therefore still checked and credited at its end, with the tallies (passes, rejections, placed, trades, passive fills, reward-term sums,
 * return - and the maker ratio formed from them) of the steps AFTER the enable only, while its step count (CDA_EM_AGENT_STEPS, CDA_EM_ENV_STEPS: the episode's
 * t_step) and the end-of-episode account figures (NAV, drawdown, position, num_trades, bankrupt, the conservation check) are the whole episode's.  A disable stops
 * the tallying and the crediting at once - an episode that ends while the metrics are off is never credited; one that is still under way when they are enabled
 * again falls under the rule above - and keeps the accumulators: a collection after it returns what was credited before it.  The setting (on, nav_tolerance) is an argument of every step
 * launch: a captured graph of step launches holds the setting of its capture and must not be replayed under another (mlp.RolloutChains.run refuses).
 * cda_episode_metrics_collect reduces the accumulators over the markets, by module: module_of i32[N,A] (device; NULL = every slot is module 0) names
 * the module that played slot a of market i during the episodes collected (league self-play: the draw of cda_league_assign; values outside
 * [0, n_modules) are skipped) -> agent_out f64[n_modules, CDA_EM_AGENT_FIELDS], env_out f64[CDA_EM_ENV_FIELDS] (device), in a FIXED order (two launches;
 * the same inputs give the same bits).  clear != 0 zeroes the accumulators behind the read.  Call it before slot assignments change.
 * Sums of integers are exact in f64 (< 2^53). */
#define CDA_EM_AGENT_FIELDS 32
enum {                                   /* per module: sums over the (episode, agent) pairs the module played */
    CDA_EM_EPISODES = 0,                 /* (episode, agent) pairs credited */
    CDA_EM_AGENT_STEPS = 1,              /* tally["agent_steps"] */
    CDA_EM_PASSES = 2,                   /* is_pass_action */
    CDA_EM_REJECTIONS = 3,               /* num_rejected_step */
    CDA_EM_PLACED = 4,                   /* order_step_placed */
    CDA_EM_TRADES = 5,                   /* num_trades_step */
    CDA_EM_PASSIVE = 6,                  /* num_passive_fills_step */
    CDA_EM_TERM_SUM = 7,                 /* 7..11: sum of reward term j over the agent-steps */
    CDA_EM_TERM_SQ = 12,                 /* 12..16: sum of its square */
    CDA_EM_RETURN_SUM = 17,              /* sum of episode returns (f64 sum of the step rewards, in step order) */
    CDA_EM_RETURN_SQ = 18,
    CDA_EM_NAV_SUM = 19,                 /* float(NAV) at the episode's last step */
    CDA_EM_NAV_MIN = 20,
    CDA_EM_NAV_MAX = 21,
    CDA_EM_DRAWDOWN_SUM = 22,            /* float(max(0, max_nav - nav)) */
    CDA_EM_ABS_POSITION_SUM = 23,
    CDA_EM_NUM_TRADES_SUM = 24,          /* acc.num_trades (the episode total) */
    CDA_EM_MAKER_RATIO_SUM = 25,         /* passive / trades of the pairs with trades >= 5 (_MIN_TRADES_FOR_MAKER_RATIO) */
    CDA_EM_MAKER_RATIO_N = 26,
    CDA_EM_MAKER_RATIO_MAX = 27,
    CDA_EM_BANKRUPT = 28                 /* pairs that ended in done_set (nav <= 0) */
};
#define CDA_EM_ENV_FIELDS 8
enum {                                   /* per env: sums over the episodes that ended */
    CDA_EM_ENV_EPISODES = 0,
    CDA_EM_ENV_NAV_VIOLATIONS = 1,       /* nav_conservation_violations */
    CDA_EM_ENV_NAV_ERROR_SUM = 2,        /* float(abs(sum(NAV) - A * init_cash)) */
    CDA_EM_ENV_NAV_ERROR_MAX = 3,
    CDA_EM_ENV_MAKER_MAX_SUM = 4,        /* maker_fill_ratio_max: the episode's max over its qualifying agents */
    CDA_EM_ENV_MAKER_MAX_N = 5,          /* episodes with a qualifying agent */
    CDA_EM_ENV_STEPS = 6,                /* env steps of the episodes */
    CDA_EM_ENV_TERMINATED = 7            /* episodes that ended with every agent done (the others were truncated at max_step) */
};
int cda_episode_metrics_enable(cda_env* env, int32_t on, double nav_tolerance);
int cda_episode_metrics_collect(cda_env* env, const int32_t* module_of, int32_t n_modules, double* agent_out, double* env_out, int32_t clear, void* stream);
#define CDA_EM_MAX_MODULES 32

/* Test/diagnostic hook: Trader.place_order (agent/trader.py:49-106) for ONE decoded order on one
 * market, bypassing decode and the RNG. type: 0 market, 1 limit, 2 modify, 3 cancel; side: 0 bid,
 * 1 ask; price in ticks (ignored for market). Synchronous. */
int cda_place_order(cda_env* env, int32_t market, int32_t trader, int32_t type, int32_t side,
                    int32_t size, int32_t price);
/* Test/diagnostic hook: Exchg_Helper.mark_to_mkt (exchg_helper.py:56-66) on one market. Synchronous. */
int cda_mark_to_mkt(cda_env* env, int32_t market);

/* Parity dump / restore of one market (synchronous; host struct). */
int cda_get_state(cda_env* env, int32_t market, cda_market_state* out_host);
int cda_set_state(cda_env* env, int32_t market, const cda_market_state* in_host);

/* One side of one market's book, whole, in queue order (best price first, FIFO inside a level; ordertree.py / orderlist.py):
 * up to max_orders orders -> orders_out_host (host), the side's true length -> n_out_host.  side: 0 bids, 1 asks.  Synchronous. */
int cda_get_book(cda_env* env, int32_t market, int32_t side, cda_order* orders_out_host, int32_t max_orders, int32_t* n_out_host);
/* Orders per side the HBM spill ring of this env holds (0 = no HBM tier) - what cda_create GRANTED - and what was asked for (automatic:
 * num_agents * max_step rounded up to a power of two, the size with which no order is ever dropped inside an episode).  The automatic size is
 * halved while the rings would take more than a quarter of the free device memory; when granted < wanted the book is bounded by tile + ring and
 * a rest beyond it is dropped and flagged (CDA_FLAG_BOOK_OVERFLOW) - a caller can tell at construction. */
int32_t cda_book_spill(const cda_env* env);
int32_t cda_book_spill_wanted(const cda_env* env);

/* Pre-step raw top-10 snapshot agg_LOB_raw f32[N,40] (state_helper.py:159-160) -> device buffer. */
int cda_get_raw_snapshot(cda_env* env, float* raw_out, void* stream);

/* Per-market sticky flags u32[N] -> device buffer. */
int cda_last_flags(cda_env* env, uint32_t* flags_out, void* stream);
/* Book census i32[N] -> device buffer: the most resting orders (both sides together) each market has held since its
 * last reset.  The reference's OrderTree is unbounded (ordertree.py:5-58); this build holds cda_book_capacity(env) in the
 * LDS tile and cda_book_spill(env) per side behind it in HBM. */
int cda_book_peak(cda_env* env, int32_t* peak_out, void* stream);

/* Structural invariants of every market -> u32[N] device buffer of CDA_INV_* bits (0 = all hold): sides sorted best
 * price first (ordertree.py:44-58), book not crossed (orderbook.py:162-194), quantities positive,
 * cash_on_hold == value of the trader's own resting orders, exactly (cash_processor.py:15-29, :85-97), positions net
 * to zero (account.py:196-213).  A size-independent property check for runs too large to replay on the CPU. */
#define CDA_INV_BIDS_SORTED   0x01u
#define CDA_INV_ASKS_SORTED   0x02u
#define CDA_INV_CROSSED       0x04u
#define CDA_INV_QTY           0x08u
#define CDA_INV_ESCROW        0x10u
#define CDA_INV_NET_POSITION  0x20u
#define CDA_INV_OWNER         0x80u
#define CDA_INV_BOOK_COUNT    0x100u
int cda_check_invariants(cda_env* env, uint32_t* violations_out, void* stream);

/* Device self-tests of the ledger arithmetic and the RNG (host pointers; synchronous).
 * op: 0 add, 1 sub, 2 mul, 3 div, 4 cmp (result in out[i].w[0]: 0 lt, 1 eq, 2 gt), 5 to-double
 * (bits in out[i].w[0..1]). For mul/div `b` must be integer valued with coefficient < 2^32.
 * 6 = a + b through the cash / cash_on_hold transfer leaf with the general addition as its fallback
 * (out[i].pad = 1 when the leaf itself produced the result). */
int cda_selftest_dec(int32_t device, int32_t op, int32_t n, const cda_dec* a_host, const cda_dec* b_host,
                     cda_dec* out_host);
/* Draw, on the device, the env's RNG schedule for one seed: one integers(lo,hi+1), then `n_steps`
 * times {n_normals standard normals, one permutation(perm_n)}. Outputs host arrays. */
int cda_selftest_rng(int32_t device, uint64_t seed, int32_t lo, int32_t hi, int32_t n_steps,
                     int32_t n_normals, int32_t perm_n, int32_t* first_int_host,
                     double* normals_host /*[n_steps*n_normals]*/, int32_t* perms_host /*[n_steps*perm_n]*/,
                     uint64_t* final_state_host /*[6]: state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger*/);

/* The restated libm functions numpy's generator calls on the host (csrc/cda_libm.hpp; op 0: log1p, glibc 2.35
 * s_log1p.c; op 1: exp, glibc 2.35 e_exp.c as built with FMA; device only, op 2: the f64 square root the observation
 * uses, which must be the correctly rounded IEEE one) evaluated on the device / by the same source compiled
 * for the host (no GPU needed).  Host pointers; synchronous. */
int cda_selftest_libm(int32_t device, int32_t op, int32_t n, const double* x_host, double* y_host);
int cda_selftest_libm_host(int32_t op, int32_t n, const double* x_host, double* y_host);

/* Learner side of the PPO loop on the batched env (the reference trains through RLlib's PPO, train/train.py:453-541,
 * config/train_config.json `ppo`): clipped-surrogate + value + entropy loss of one minibatch and its gradient with respect to the
 * network outputs in ONE launch (csrc/cda_ppo.hip).  A ROW of network outputs serves `agents_per_row` consecutive samples: every agent
 * of a market is handed the same observation (state_helper.py:76,109), so a shared policy's outputs are the same for all of them and
 * the network runs once per market-step; agents_per_row = 1 is the plain one-row-per-sample op.  With B = rows * agents_per_row:
 * logits f32[rows,24] = category 9 | price 10 | price_offset 3 | two Gaussian means, value f32[rows], log_std f32[2], actions
 * a_cat / a_price / a_off i64[B] and a_cont f32[B,2], logp_old / adv / ret f32[B] (sample r * agents_per_row + a belongs to row r).
 * Out: d_logits f32[rows,24], d_value f32[rows] (gradients of the loss, summed over the row's samples), sums5 f64[5] (scratch), out6
 * f32[6] = mean policy loss, mean value loss, mean entropy, loss, d loss / d log_std[0..1] (means over the B samples).  Device pointers.
 * row_index i64[rows] (optional, NULL = identity): the rows are a shuffled minibatch and the samples of row r live at
 * row_index[r] * agents_per_row + a in the per-sample arrays (which then hold the WHOLE batch, unshuffled) - an epoch's shuffle moves
 * the observations only.
 * out_stride != 0 (a multiple of 4 above 24): `logits` is the network's padded output matrix f32[rows, out_stride] as it stands - logits
 * in columns 0..23, the value in column 24 - and `d_logits` its gradient in the same shape (d value in column 24, zeros behind);
 * `value` / `d_value` are not used (may be NULL).  out_stride == 0: the separate arrays described above. */
int cda_ppo_loss(const float* logits, const float* value, const float* log_std, const int64_t* a_cat, const int64_t* a_price,
                 const int64_t* a_off, const float* a_cont, const float* logp_old, const float* adv, const float* ret,
                 const int64_t* row_index, int64_t rows, int32_t agents_per_row, int32_t out_stride, float clip, float vf_coef, float ent_coef,
                 float* d_logits, float* d_value, double* sums5, float* out6, void* stream);

/* The rollout's policy step (csrc/cda_ppo.hip): sample the Dict action of B = rows * agents_per_row (market, agent) pairs from the
 * network outputs (logits f32[rows, logits_stride]: 24 for the bare logits, or the padded output matrix of cda_ppo_loss's out_stride,
 * whose column 24 is then copied to value_out f32[rows] if that is not NULL; row sharing as in cda_ppo_loss) in ONE launch: a_cat / a_price / a_off i64[B],
 * a_cont f32[B,2] (the raw Gaussian samples), logp f32[B], and the env's five action arrays i32 / f32 [B] (size_mean = tanh,
 * size_sigma = sigmoid of the Gaussian samples: the Box bounds of action_helper.py:126-138).  Randomness is counter based, keyed
 * (seed, *counter_dev, sample); counter_dev (i64[1], device) is incremented on the stream after every call, so a captured HIP graph
 * draws fresh numbers on every replay. */
int cda_policy_sample(const float* logits, int32_t logits_stride, float* value_out, const float* log_std, int64_t rows, int32_t agents_per_row,
                      uint64_t seed, int64_t* counter_dev,
                      int64_t* a_cat, int64_t* a_price, int64_t* a_off, float* a_cont, float* logp,
                      int32_t* env_category, float* env_size_mean, float* env_size_sigma, int32_t* env_price, int32_t* env_price_offset, void* stream);

/* Generalised advantage estimation over a rollout (ppo.gae's recursion, one launch): rew / val / done f32[n_steps, batch] (done = 1 where
 * the episode ended with that step), last_val f32[batch] -> adv, ret f32[n_steps, batch].  Device pointers. */
int cda_gae(const float* rew, const float* val, const float* last_val, const float* done, int32_t n_steps, int64_t batch,
            float gamma, float lam, float* adv, float* ret, void* stream);

/* Rollout buffers in one launch: for k < n_items copy bytes[k] bytes from src[k] to dst_base[k] + *slot_dev * bytes[k] (slot t of a
 * [T, bytes[k]] buffer; the caller keeps *slot_dev below T), then, if bump, *slot_dev += 1 on the stream.  The slot index is read on
 * the device, so a captured HIP graph replays the call unchanged for every step of a rollout.  src / dst_base / bytes are HOST arrays
 * of device pointers / sizes (read at call time); n_items <= CDA_SLOT_ITEMS_MAX. */
#define CDA_SLOT_ITEMS_MAX 12
int cda_store_slots(int32_t n_items, const void* const* src, void* const* dst_base, const int64_t* bytes, int64_t* slot_dev, int32_t bump, void* stream);

/* ---- device snapshot / restore of a market range --------------------------------------------------------------------------------
 * A compact, position-independent image of markets [first, first + n) of an env, built on the device (csrc/cda_snapshot.inc): per market the
 * whole record (header words with the PCG64 state, accounts, history frames, the book tile, the running episode tallies), its done_buf byte,
 * its rows of the episode-metric accumulators and, for a side whose book continues in the HBM ring, the ring's count and base and ONLY the live
 * window of orders.  The blob holds no address.  Layout: cda_snapshot_header (256 B), int64 offsets[n + 1] (byte offset of every market's
 * section from the blob's start; offsets[n] = total bytes) zero padded to a multiple of 256 B, then the sections, each 256-B aligned.
 *
 *   cda_snapshot_offsets  sizes every market's section from its header and status words and scans them into offsets_dev i64[n + 1] (device)
 *                         on `stream`; offsets_dev[n] (one 8-byte read) is the blob size the caller allocates.
 *   cda_snapshot_pack     writes the blob (device, 256-B aligned, blob_bytes >= offsets_dev[n]) on `stream`; the env must not be stepped
 *                         between the two calls (stream order).
 *   cda_snapshot_restore  markets [src_first, src_first + n) of a blob -> markets [first_market, first_market + n) of `env` (this env or any other
 *                         with the same numeric config, tile, history depth, agent count and episode-metrics setting; its n_markets and
 *                         book_spill may differ: a ring window is rebased into the target's ring, at the saved base when the capacities are
 *                         equal).  SYNCHRONOUS in its checks: the header is read back and every section is vetted on the device before any
 *                         byte of the env is written; a blob that does not fit (config, tile, depth, agents, metrics, a live window larger than
 *                         the target's ring, a corrupt header or table) returns CDA_ERR_INVALID and leaves the env as it was.  Then, on
 *                         `stream`, the arena is written in place (captured graphs keep their addresses) and, if obs_out (f32 [N, n_hist*42],
 *                         device) is not NULL, the restored markets' observation rows are re-emitted from their history frames.
 *   cda_snapshot_check_header   the host half of those checks, for a header already on the host (CDA_OK / CDA_ERR_INVALID).
 *   cda_snapshot_table_bytes    bytes of header + offset table for n markets: where the first section starts. */
#define CDA_SNAP_MAGIC   0x53414443u    /* "CDAS" */
#define CDA_SNAP_VERSION 1u
typedef struct cda_snapshot_header {
    uint32_t magic, version;
    int32_t  header_bytes;          /* = cda_snapshot_table_bytes(n_markets) */
    int32_t  n_markets;             /* markets in the blob */
    int64_t  total_bytes;
    int32_t  book_capacity, record_stride, n_hist, num_agents;
    int32_t  spill_cap;             /* ring of the env the blob was taken from */
    int32_t  episode_metrics_on;
    double   nav_tolerance;
    int32_t  first_market;          /* of the env the blob was taken from */
    int32_t  em_agent_fields, em_env_fields, section_meta_bytes;
    cda_config cfg;                 /* the full config of the env the blob was taken from */
    uint8_t  reserved[88];
} cda_snapshot_header;
int64_t cda_snapshot_table_bytes(int32_t n_markets);
int cda_snapshot_offsets(cda_env* env, int32_t first_market, int32_t n_markets, int64_t* offsets_dev, void* stream);
int cda_snapshot_pack(cda_env* env, int32_t first_market, int32_t n_markets, const int64_t* offsets_dev, void* blob_dev, int64_t blob_bytes, void* stream);
int cda_snapshot_check_header(const cda_env* env, const cda_snapshot_header* header_host, int64_t blob_bytes);
int cda_snapshot_restore(cda_env* env, int32_t first_market, const void* blob_dev, int64_t blob_bytes, int32_t src_first, int32_t n_markets,
                         float* obs_out, void* stream);

/* ---- trade tape: every fill recorded on the device ------------------------------------------------------------------------------------
 * The reference's order book keeps OrderBook.tape, one transaction_record per fill, appended in process_order_list (orderbook.py:108-140) -
 * self-trades included - and read by everything that looks at executions rather than accounts (state_helper.py:148-156, tape_dump).
 * cda_tape_enable(env, capacity): from now on the step launches of this env (cda_step*, cda_step_range*, cda_step_groups*, cda_run_random,
 * cda_place_order; the general step that continues into the HBM tier of the book included) append one cda_tape_record per fill to a ring of
 * `capacity` records per market, in memory of its own (capacity a power of two <= CDA_TAPE_CAP_MAX; 0 = off, and the memory is freed).  OFF by
 * default; while it is off no launch runs a tape-writing instance (the instances an env without a tape launches carry no tape code).  While it is on cda_policy_step_supported answers 0
 * (rollout chains take their two-launch path and record through the step kernel).  Synchronous (it waits for the device); do not toggle it
 * between the capture and the replay of a graph that holds step launches.
 * Per market: n_total (fills since enable; the ring slot of record j is j % capacity), n_episode (fills since the market's last reset = the
 * reference's len(LOB.tape)), episode (resets since enable), partial, n_previous.  A reset - cda_reset*, the device-side auto reset - remembers
 * n_episode as n_previous (the fills of the step that ended the episode included), zeroes n_episode, bumps episode and clears partial; it does NOT
 * clear the ring: the episode that just ended stays readable until newer fills overwrite it.  In record numbers the current episode is
 * [n_total - n_episode, n_total) and the previous one [n_total - n_episode - n_previous, n_total - n_episode); the ring holds [n_total - capacity,
 * n_total).  Snapshots do not carry the tape: cda_snapshot_restore zeroes the restored markets' n_episode and n_previous and sets partial = 1
 * (what follows is an episode's tail).
 *   cda_tape_counts    n_total i64[N], n_episode i32[N], episode i32[N], partial i32[N] (device; each may be NULL).
 *   cda_tape_counts_ex the same and n_previous i32[N] (may be NULL too).
 *   cda_tape_offsets   the streaming read, first half: for market first + i everything from cursor_dev[i] (a record number; i64[n], device) to
 *                      n_total that the ring still holds -> offsets_dev i64[n + 1] (exclusive scan of the counts; offsets[n] = records in all),
 *                      dropped_dev i64[n] (may be NULL): records of [cursor, n_total) the ring had already overwritten.
 *   cda_tape_pack      second half: the records, market by market, each market's oldest first, dense into records_out_dev
 *                      [capacity_records][CDA_TAPE_WORDS] i32 (device, 16-B aligned, capacity_records >= offsets[n]); cursor_dev[i] := n_total.  The env
 *                      must not be stepped between the two calls (stream order); a market whose run would not fit is left alone, cursor included.
 *   cda_tape_last      the last k records of each market's CURRENT episode, oldest first -> records_out_dev [n][k][CDA_TAPE_WORDS] i32 (rows beyond
 *                      the count are zero), counts_out_dev i32[n] (may be NULL): what state_helper.py walks with tape_display_length.
 *   cda_tape_last_of   the same of the episode `which` names: CDA_TAPE_CURRENT or CDA_TAPE_PREVIOUS (the episode that ended at the market's last reset).
 * Reductions over the records of one remembered episode, on the device, one launch each, a wave per market (no atomics on global memory: the result
 * does not depend on scheduling).  All take `which` as cda_tape_last_of does and fill info_out_dev i32 [n][4] (may be NULL): {records aggregated,
 * records of that episode the ring had already overwritten, records whose bar index was >= n_bars (not aggregated; 0 for flows), 1 = the episode's
 * head was never recorded (partial)}.
 *   cda_tape_bars      price / volume bars: bar b of market first + i covers the episode's records whose step index (sides_step >> 2) lies in
 *                      [b * bar_steps, (b + 1) * bar_steps) -> bars_out_dev [n][n_bars] cda_tape_bar (device, 16-B aligned).  open / close: the first /
 *                      last such record in tape order; a bar without fills is all zeros (n_trades == 0).  Within an episode the step index never
 *                      decreases, so a bar is one run of records; every row of the output is written exactly once.
 *   cda_tape_flows     who trades with whom: flows_out_dev i64 [n][A][A][3] (A = num_agents), [init_id][counter_id] = {quantity, notional (price x
 *                      quantity), fills}; the diagonal holds the self-trades.
 *   cda_tape_exec      the execution report, per agent: stats_out_dev i64 [n][A][CDA_TAPE_STAT_WORDS] and markouts_out_dev i64 [n][A][n_horizons][2][4]
 *                      (device, 8-B aligned).  A party's side is 0 = bid (it bought, sign +1) or 1 = ask (it sold, sign -1); a self-trade (init_id ==
 *                      counter_id) moves no position and is counted in self_qty / self_fills only; S_last = the step of the last held record.
 *                      stats words, in order: buy_qty, sell_qty, buy_notional, sell_notional (price x quantity; both roles), maker_qty, maker_fills (the
 *                      agent was counter_id), taker_qty, taker_fills (init_id), self_qty, self_fills, final_pos, max_long (largest running position,
 *                      >= 0), max_short (most negative, <= 0), abs_pos_steps (sum over the steps 0 .. S_last of |position at the end of the step|),
 *                      first_step, last_step of the agent's non-self fills (-1 without any).  The running position starts at 0 at the first held record.
 *                      markouts[agent][horizon h][role: 0 maker, 1 taker] = {sum of sign x (mark(s + k_h) - price) x quantity, quantity, fills - over the
 *                      agent's non-self fills in that role with s + k_h <= S_last -, fills with s + k_h > S_last (open: counted, never marked)};
 *                      mark(t) = the price of the last held record whose step is <= t (the last print).  horizons_dev_or_host: n_horizons int32 >= 0,
 *                      1 <= n_horizons <= CDA_TAPE_MAX_HORIZONS; a host array is read during the call, a device array costs a synchronising copy.
 *                      info's third word is 0.
 * bar_steps < 1, n_bars < 1, n_horizons outside 1 .. CDA_TAPE_MAX_HORIZONS, a negative horizon, a misaligned output, a range outside the env or another
 * `which`: CDA_ERR_INVALID.  CDA_ERR_UNSUPPORTED from the readers while the tape is off. */
#define CDA_TAPE_CURRENT  0
#define CDA_TAPE_PREVIOUS 1
#define CDA_TAPE_WORDS   8
#define CDA_TAPE_CAP_MAX (1 << 20)
typedef struct cda_tape_record {       /* transaction_record of orderbook.py:108-140 */
    int32_t time;                      /* 'time' = 'timestamp': LOB.time at the fill */
    int32_t price;                     /* 'price', as the book holds it (ticks x tick_size) */
    int32_t quantity;                  /* 'quantity' */
    int32_t counter_id;                /* counter_party['ID']: the resting order's trader */
    int32_t counter_order_id;          /* counter_party['order_id'] */
    int32_t counter_left;              /* counter_party['new_book_quantity']; -1 where the reference stores None (the resting order was consumed) */
    int32_t init_id;                   /* init_party['ID']: the incoming order's trader (== counter_id in a self-trade) */
    int32_t sides_step;                /* bit 0: counter_party['side'] (0 bid, 1 ask); bit 1: init_party['side']; bits 2..: the env step index t of the episode */
} cda_tape_record;
int cda_tape_enable(cda_env* env, int64_t capacity_records);
int64_t cda_tape_capacity(const cda_env* env);
int cda_tape_counts(cda_env* env, int64_t* n_total_dev, int32_t* n_episode_dev, int32_t* episode_dev, int32_t* partial_dev, void* stream);
int cda_tape_offsets(cda_env* env, int32_t first_market, int32_t n_markets, const int64_t* cursor_dev, int64_t* offsets_dev, int64_t* dropped_dev, void* stream);
int cda_tape_pack(cda_env* env, int32_t first_market, int32_t n_markets, int64_t* cursor_dev, const int64_t* offsets_dev, void* records_out_dev,
                  int64_t capacity_records, void* stream);
int cda_tape_last(cda_env* env, int32_t first_market, int32_t n_markets, int32_t k, void* records_out_dev, int32_t* counts_out_dev, void* stream);
typedef struct cda_tape_bar {          /* 48 bytes = twelve int32 words */
    int32_t open, high, low, close;    /* prices as the records hold them; all 0 where n_trades == 0 */
    int32_t n_trades;                  /* fills in the bar */
    int32_t n_self;                    /* ... of which counter_id == init_id */
    int64_t volume;                    /* sum of quantity */
    int64_t buy_volume;                /* ... over the fills whose initiator side is bid */
    int64_t notional;                  /* sum of price x quantity */
} cda_tape_bar;
int cda_tape_counts_ex(cda_env* env, int64_t* n_total_dev, int32_t* n_episode_dev, int32_t* episode_dev, int32_t* partial_dev, int32_t* n_previous_dev, void* stream);
int cda_tape_last_of(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, int32_t k, void* records_out_dev, int32_t* counts_out_dev, void* stream);
int cda_tape_bars(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, int32_t bar_steps, int32_t n_bars, void* bars_out_dev,
                  int32_t* info_out_dev, void* stream);
int cda_tape_flows(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, int64_t* flows_out_dev, int32_t* info_out_dev, void* stream);
#define CDA_TAPE_STAT_WORDS   16
#define CDA_TAPE_MAX_HORIZONS 8
int cda_tape_exec(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* horizons_dev_or_host, int32_t n_horizons,
                  int64_t* stats_out_dev, int64_t* markouts_out_dev, int32_t* info_out_dev, void* stream);

/* ---- quote tape: the top of the book per step, recorded on the device -----------------------------------------------------------------
 * The trade tape keeps the prints; this keeps the other half of a market-data feed, the quotes over time.  cda_quotes_enable(env, capacity_steps):
 * from now on every step launch of this env (cda_step*, cda_step_range*, cda_step_groups*, the rollout, evaluation and league chains - everything
 * that steps) first records, for every market of its range whose episode is not over, one cda_quote_record into the market's ring of
 * `capacity_steps` records (1 .. CDA_QUOTE_CAP_MAX, any value; memory of its own beside the arena): the recorder's launch runs behind the attached
 * order schedule's and ahead of the step kernel, so the quote of step t is the book that step t's agent orders meet.  The step kernels are the ones
 * of an env without quotes; the market record, cda_market_state, state dumps and snapshot blobs do not change.  OFF by default.  While it is on
 * cda_policy_step_supported answers 0 (rollout chains take their two-launch path) and cda_run_random returns CDA_ERR_UNSUPPORTED (it steps inside
 * one launch).  Enable / disable are synchronous; do not toggle between the capture and the replay of a graph that holds step launches.
 * A record: the step index t, flags, and per side the best price, the summed quantity of that price level - followed into the HBM tier of the book
 * where the level is deeper than the tile - and the number of its orders.  An absent side stores zeros; a volume or count beyond INT32_MAX stores
 * INT32_MAX and sets CDA_QUOTE_SATURATED.
 * Episodes.  Per market a meta row of eight int32 words: n_total (64 bits, words 0 - 1: records since enable; record j lies in slot j % capacity),
 * n_episode (records of the current episode), n_prev, first / prev_first (the step of each episode's first record), gap, flags (bit 0: the current
 * episode's head was never recorded - partial -, bit 1: the previous one's).  Recorder and readers apply ONE rule, a pure function of the row and
 * the market's current t_step: t_step == first + n_episode - nothing changes; t_step == 0 with n_episode > 0 - the market was reset: the held
 * episode becomes the previous one, the current one starts empty; anything else - a snapshot restore moved the clock: the current episode restarts
 * at t_step, empty and partial (unless t_step is 0), what it held stays in the ring as `gap` records between the previous episode and the new
 * current one.  The readers apply the rule lazily: right behind a step whose in-kernel auto reset ended an episode, CDA_TAPE_PREVIOUS already names
 * that episode, as it does on the trade tape.  The ring is never cleared: what it holds of an episode is the episode's intersection with the last
 * `capacity` records; the readers report the rest as lost.
 *   cda_quote_meta     the rolled meta rows -> meta_out_dev i32 [n][8].
 *   cda_quote_series   the held records of the episode `which` (CDA_TAPE_CURRENT / CDA_TAPE_PREVIOUS), oldest first, the last k of them where it
 *                      holds more -> records_out_dev [n][k] cda_quote_record (device, 16-B aligned; rows beyond the count are zero), counts_out_dev
 *                      i32 [n] (may be NULL), info_out_dev i32 [n][4] (may be NULL): {records returned, records of the episode's head the ring had
 *                      overwritten, step of the first returned record, partial}.
 *   cda_quote_stats    stats_out_dev i64 [n][CDA_QUOTE_STAT_WORDS] over the held records (8-B aligned), in order: steps; two-sided, bid-only,
 *                      ask-only and empty steps; over the two-sided steps the sum, sum of squares, minimum and maximum of the spread (ask - bid; 0
 *                      and 0 without any), the sum of m2 = bid + ask (twice the mid, kept integer), the sums of the bid and of the ask best-level
 *                      volume; over consecutive held steps that are both two-sided their number, the number of m2 changes, the sum of |m2' - m2|
 *                      and of (m2' - m2)^2 (the realised variance of the mid, times four).  info_out_dev as cda_quote_series (records aggregated
 *                      first).
 *   cda_tape_spreads   the trade tape joined to the quotes by step; needs both services on.  spreads_out_dev i64 [n][A][n_horizons][2][6] (8-B
 *                      aligned; A = num_agents; role 0 = maker = counter_id, 1 = taker = init_id): over the agent's non-self fills in that role - step s,
 *                      price p, quantity q, side = +1 where the agent bought, -1 where it sold; m2(t) of the quote of step t - {cost_now = sum of
 *                      side (2p - m2(s)) q, cost_later = sum of side (2p - m2(s + k)) q, qty, fills - all four over the fills whose quotes at s and at
 *                      s + k are both held and two-sided -, open = fills with s + k beyond the last held quote step (counted, never extrapolated),
 *                      unquoted = the other fills: a quote at s or s + k that is one-sided or no longer held}.  horizons_host: n_horizons int32 >= 0
 *                      (host memory, read during the call), 1 <= n_horizons <= CDA_TAPE_MAX_HORIZONS.  info_out_dev i32 [n][4] (may be NULL): {tape
 *                      records aggregated, tape records lost to its ring, quote records lost to theirs, partial bits: 1 tape, 2 quotes}.  Both
 *                      episodes are named by `which`; the tape's and the quotes' notion of it agree wherever steps and resets alone moved the clock.
 * One launch each, a wave per market, exact integers, no atomics on global memory.  A NULL pointer, a range outside the env, a misaligned output,
 * capacity_steps or k < 1, another `which`, n_horizons outside its bounds or a negative horizon: CDA_ERR_INVALID, nothing is launched.
 * CDA_ERR_UNSUPPORTED from the readers while a service they need is off. */
#define CDA_QUOTE_WORDS      8
#define CDA_QUOTE_CAP_MAX    (1 << 20)
#define CDA_QUOTE_STAT_WORDS 16
#define CDA_QUOTE_BID        1
#define CDA_QUOTE_ASK        2
#define CDA_QUOTE_SATURATED  4
typedef struct cda_quote_record {
    int32_t step;                      /* the env step index t of the episode: the book as step t's orders meet it */
    int32_t flags;                     /* CDA_QUOTE_BID | CDA_QUOTE_ASK: the side has a best level; CDA_QUOTE_SATURATED */
    int32_t bid_price;                 /* best prices, as the book holds them; 0 on an absent side */
    int32_t ask_price;
    int32_t bid_volume;                /* summed quantity of the best level */
    int32_t ask_volume;
    int32_t bid_orders;                /* orders on the best level */
    int32_t ask_orders;
} cda_quote_record;
int cda_quotes_enable(cda_env* env, int64_t capacity_steps);
int cda_quotes_disable(cda_env* env);
int64_t cda_quotes_capacity(const cda_env* env);
int cda_quote_meta(cda_env* env, int32_t first_market, int32_t n_markets, int32_t* meta_out_dev, void* stream);
int cda_quote_series(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, int32_t k, void* records_out_dev, int32_t* counts_out_dev,
                     int32_t* info_out_dev, void* stream);
int cda_quote_stats(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, int64_t* stats_out_dev, int32_t* info_out_dev, void* stream);
int cda_tape_spreads(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* horizons_host, int32_t n_horizons,
                     int64_t* spreads_out_dev, int32_t* info_out_dev, void* stream);

/* ---- the stylised-facts report: return and order-flow statistics of one remembered episode, on the device -----------------------------
 * The time-series structure of the market the agents produce - what an agent-based market is validated against: are mid-price returns
 * uncorrelated while their magnitudes cluster, how fat are the return tails, how persistent is the sign of order flow, how much does signed
 * volume move the price.  Three reductions, each over the episode `which` names (CDA_TAPE_CURRENT / CDA_TAPE_PREVIOUS) of the markets
 * [first_market, first_market + n_markets), one launch on `stream`, a wave per market, no atomics on global memory; stylised.py states every
 * word in numpy.  EVERY output word is an additive int64 sum (two's-complement wrap, as cda_quote_stats' dm2_sq): a fold over markets, episodes
 * or ranks is a plain sum; there are no min / max words.  The sums are exact while bid + ask < 2^31, a bar's signed volume |Q_b| < 2^31 (it is
 * kept as an int32 word) and no sum leaves int64: a market has at most CDA_STYL_MAX_BARS = 2^12 bars, so |r| < 2^25 and |Q_b| < 2^25 always
 * suffice (2^12 products below 2^50), and a tape holds at most 2^20 fills, so quantities below 2^21 always suffice for cda_tape_signs' qq.
 * Definitions.  m2(s) = bid_price + ask_price of the quote record of episode step s, defined iff the record is held and two-sided.  The bar points
 * are the steps s with s % bar_steps == 0 on the episode's absolute step grid (a lost head does not shift it); point p is step p x bar_steps.  The
 * return at point p is r_p = m2((p + 1) bar_steps) - m2(p bar_steps), defined iff both are (half price units, as dm2).  The sign of a fill is +1
 * where the initiator bought (its side bit is 0), -1 where it sold; self-trades are fills like any other and are counted separately.
 * lags_host: n_lags int32 (host memory, read during the call), 1 <= n_lags <= CDA_STYL_MAX_LAGS, each lag in 1 .. CDA_STYL_MAX_LAG (0 allowed
 * for cda_tape_flow_returns); a lag that runs past the end of the episode yields zeros.  The bar points of the longest episode of the range,
 * ceil(largest max_step of its rows / bar_steps), must be at most CDA_STYL_MAX_BARS (a wave keeps a whole episode's points in LDS): checked on
 * the host, before the launch.
 *   cda_quote_returns      needs the quote tape.  base_out_dev i64 [n][8]: bars (the points held), returns (the returns that are defined), missing
 *                          (adjacent held point pairs with an endpoint that is not two-sided), sum_r, sum_abs, sum_r2, up, down (returns > 0, < 0).
 *                          lagged_out_dev i64 [n][n_lags][4], per lag l over the points where r_p and r_(p + l) are both defined: n, rr = sum r r',
 *                          aa = sum |r| |r'| (volatility clustering), ra = sum r |r'| (the leverage term).  hist_out_dev i64 [n][2 hist_half + 1]:
 *                          bin clamp(r / tick, -hist_half, hist_half) + hist_half, tick = the tick_size of the market's own row (prices are multiples
 *                          of it: the division is exact); the end bins hold the clipped mass.  1 <= hist_half <= CDA_STYL_MAX_HIST_HALF.
 *                          info_out_dev i32 [n][4] (may be NULL) as cda_quote_stats fills it.  At bar_steps 1: returns == cda_quote_stats' pairs,
 *                          sum_r2 == dm2_sq, sum_abs == abs_dm2.
 *   cda_tape_signs         needs the trade tape; over the held fills in tape order.  base_out_dev i64 [n][8]: fills, buys, sells, buy_qty, sell_qty,
 *                          self_fills, runs (maximal runs of equal sign), steps_with_fills.  lagged_out_dev i64 [n][n_lags][4], lags in TRADE time,
 *                          over the fills i and i + l: n, ss = sum s s', qq = sum (s q)(s' q'), same_step (pairs whose two fills carry the same env
 *                          step: one sweep prints many same-sign fills in one step).  info_out_dev as cda_tape_flows fills it.
 *   cda_tape_flow_returns  needs both.  Bar b covers the steps [b bar_steps, (b + 1) bar_steps); Q_b = sum of sign x quantity over its held fills (a
 *                          bar without fills has Q_b = 0 and counts).  Where the tape ring has lost the episode's head every bar up to and including
 *                          the bar of the first held fill is excluded (no fill held at all: every bar) and counted in bars_excluded.
 *                          lagged_out_dev i64 [n][n_lags][6], per lag l >= 0 over the kept bars b whose r_(b + l) is defined: n, q = sum Q_b, r = sum
 *                          r_(b + l), qr, qq, rr - lag 0: the contemporaneous impact regression (Kyle's lambda = cov / var, and its R^2); lags >= 1:
 *                          does flow predict returns.  base_out_dev i64 [n][4]: the kept bars' fills, the kept bars that have fills, bars_excluded,
 *                          the kept bars' quantity.  info_out_dev i32 [n][4] (may be NULL) as cda_tape_spreads fills it.
 *   cda_stylised_check_host  the argument check the three make, on the host alone (no env, no device): kind = CDA_STYL_RETURNS / CDA_STYL_SIGNS /
 *                          CDA_STYL_FLOW_RETURNS, max_step = the largest max_step of the range; CDA_OK or CDA_ERR_INVALID.  bar_steps, hist_half and
 *                          max_step are read only by the kinds that take them.
 * A NULL or misaligned output (8 B; info 4 B), a range outside the env, another `which`, n_lags outside 1 .. CDA_STYL_MAX_LAGS, a lag outside its
 * bounds, bar_steps < 1, hist_half outside 1 .. CDA_STYL_MAX_HIST_HALF or too many bar points: CDA_ERR_INVALID, nothing is launched.
 * CDA_ERR_UNSUPPORTED while a service the reduction needs is off. */
#define CDA_STYL_MAX_BARS      4096
#define CDA_STYL_MAX_LAGS      8
#define CDA_STYL_MAX_LAG       (1 << 20)
#define CDA_STYL_MAX_HIST_HALF 64
#define CDA_STYL_RETURNS       0
#define CDA_STYL_SIGNS         1
#define CDA_STYL_FLOW_RETURNS  2
int cda_quote_returns(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* lags_host, int32_t n_lags, int32_t bar_steps,
                      int32_t hist_half, int64_t* base_out_dev, int64_t* lagged_out_dev, int64_t* hist_out_dev, int32_t* info_out_dev, void* stream);
int cda_tape_signs(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* lags_host, int32_t n_lags, int64_t* base_out_dev,
                   int64_t* lagged_out_dev, int32_t* info_out_dev, void* stream);
int cda_tape_flow_returns(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* lags_host, int32_t n_lags, int32_t bar_steps,
                          int64_t* lagged_out_dev, int64_t* base_out_dev, int32_t* info_out_dev, void* stream);
int cda_stylised_check_host(int32_t kind, const int32_t* lags_host, int32_t n_lags, int32_t bar_steps, int32_t hist_half, int32_t max_step);

/* ---- depth tape: the Level-2 ladder per step, recorded on the device, and the book-shape reports -----------------------------------------
 * The quote tape keeps one level per side over time, cda_book_levels the whole ladder at one instant; this keeps the ladder over time.
 * cda_depth_enable(env, capacity_steps, levels): from now on every step launch of this env first records, for every market of its range whose
 * episode is not over, the best `levels` price levels of both sides (1 .. CDA_DEPTH_MAX_LEVELS) into the market's ring of `capacity_steps`
 * records (1 .. CDA_QUOTE_CAP_MAX; n_markets x capacity x (1 + levels) x 16 bytes of its own beside the arena; CDA_ERR_NOMEM leaves the env as
 * it was).  The recorder's launch runs behind the order schedule's and the quote recorder's and ahead of the step kernel.  OFF by default;
 * enable / disable are synchronous, as cda_quotes_enable is, and everything said there of graphs, cda_policy_step_supported (0 while on),
 * cda_run_random (CDA_ERR_UNSUPPORTED while on), snapshots and state dumps (unchanged) holds.  The service needs neither other tape.
 * A record is 1 + levels 16-byte words.  Word 0 = (step, flags, bid_levels, ask_levels): the counts are the levels recorded of the side, at most
 * `levels`; flags CDA_DEPTH_BID / CDA_DEPTH_ASK: the side has a level; CDA_DEPTH_SATURATED: a volume above INT32_MAX was stored as INT32_MAX;
 * CDA_DEPTH_BID_MORE / CDA_DEPTH_ASK_MORE: the side has more than `levels` levels.  Word 1 + l = cda_depth_level l = (bid_price, bid_volume,
 * ask_price, ask_volume), best first, prices as the book holds them; rows at or beyond a side's count are zero.
 * Episodes: the quote tape's meta row and its ONE rule (above), over rows and rings of this service's own.
 *   cda_depth_meta       the rolled meta rows -> meta_out_dev i32 [n][8].
 *   cda_depth_series     the last k held records of the episode `which`, oldest first -> records_out_dev i32 [n][k][(1 + levels) x 4] (16-B aligned;
 *                        rows beyond the count are zero), counts_out_dev i32 [n] and info_out_dev i32 [n][4] (either may be NULL) as cda_quote_series.
 * Three reductions, one launch each, a wave per market, exact int64, every output word additive (two's-complement wrap): a fold over markets,
 * episodes or ranks is a plain sum; depth.py states every word in numpy.  m2(s) = bid_price[0] + ask_price[0] of the held record of step s, defined
 * iff that record is two-sided; tick = the tick_size of the market's own row (prices are multiples of it); a level at or beyond a side's count is
 * absent.  info_out_dev i32 [n][4] (may be NULL): {records aggregated, records lost to the ring, step of the first held record, partial}.
 *   cda_depth_profile    1 <= max_dist <= CDA_DEPTH_MAX_DIST.  base_out_dev i64 [n][8]: held steps, two-sided steps, bid-more steps, ask-more steps,
 *                        saturated steps, sum of bid_levels, sum of ask_levels, 0.  levels_out_dev i64 [n][2][levels][3], per side and level index over
 *                        the held records where that level exists: steps, sum of volume, sum of |price_l - price_0| / tick.  shape_out_dev i64
 *                        [n][2][max_dist + 1]: volume by distance d = |price_l - price_0| / tick from the same side's best, in bin min(d, max_dist).
 *   cda_depth_imbalance  1 <= k <= levels, 1 <= half <= CDA_STYL_MAX_HIST_HALF, lags in 1 .. CDA_STYL_MAX_LAG.  B, A = the bid / ask volume of the first k
 *                        levels; bin = floor(2 B half / (B + A)) over the two-sided records (0 .. 2 half - 1).  resp_out_dev i64 [n][n_lags][2 half][5],
 *                        per lag l over the steps s whose record is two-sided and whose r = m2(s + l) - m2(s) is defined: n, sum r, sum r^2, up, down.
 *                        base_out_dev i64 [n][4]: held steps, two-sided steps, sum of B - A, sum of B + A over the two-sided steps.
 *   cda_depth_ofi        multi-level order-flow imbalance against returns, bar by bar.  For consecutive held records s - 1 (primed) and s and level m:
 *                        e_m(s) = [Pb >= Pb'] qb - [Pb <= Pb'] qb' - [Pa <= Pa'] qa + [Pa >= Pa'] qa'; an absent bid level reads as (0, 0), an absent
 *                        ask level as (INT32_MAX, 0).  OFI_K(s) = sum of e_m(s) over m < K, K = depths_host[j] in 1 .. levels, 1 <= n_depths <=
 *                        CDA_DEPTH_MAX_DEPTHS.  Bars, points and returns as cda_tape_flow_returns / cda_quote_returns define them, from this tape's m2;
 *                        OFI_b = the sum over the pairs whose step s lies in bar b (an episode's first step has no pair).  Where the episode's head is
 *                        not held (lost to the ring, or partial) every bar up to and including the bar of the first held step is excluded and counted
 *                        (no record held: every word is zero).
 *                        lagged_out_dev i64 [n][n_depths][n_lags][6], per lag l >= 0 over the kept bars b whose r_(b + l) is defined: n, q = sum OFI_b,
 *                        r, qr, qq, rr.  base_out_dev i64 [n][4]: pairs used (in the kept bars that are complete: all their steps held), those bars,
 *                        bars excluded, saturated records held.  Exact while bid + ask < 2^31, |OFI_b| < 2^31 (a bar's word is int32 and wraps, in
 *                        the specification alike) and no sum leaves int64: at most 2^12 bars, so |r| < 2^25 and |OFI_b| < 2^25 always suffice.
 *   cda_depth_check_host the argument check the three make, on the host alone: kind = CDA_DEPTH_PROFILE / _IMBALANCE / _OFI; levels = the service's;
 *                        a = max_dist / k / bar_steps, b = unused / half / max_step (the largest of the range); CDA_OK or CDA_ERR_INVALID.
 * A NULL pointer, a misaligned output (records 16 B, int64 8 B, int32 4 B), a range outside the env, another `which` or a parameter out of bounds:
 * CDA_ERR_INVALID; depth off: CDA_ERR_UNSUPPORTED from the readers.  Nothing is launched behind a refusal. */
#define CDA_DEPTH_MAX_LEVELS 16
#define CDA_DEPTH_MAX_DIST   256
#define CDA_DEPTH_MAX_DEPTHS 4
#define CDA_DEPTH_BID        1
#define CDA_DEPTH_ASK        2
#define CDA_DEPTH_SATURATED  4
#define CDA_DEPTH_BID_MORE   8
#define CDA_DEPTH_ASK_MORE   16
#define CDA_DEPTH_PROFILE    0
#define CDA_DEPTH_IMBALANCE  1
#define CDA_DEPTH_OFI        2
typedef struct cda_depth_head {        /* word 0 of a record */
    int32_t step;                      /* the env step index t of the episode: the book as step t's orders meet it */
    int32_t flags;                     /* CDA_DEPTH_* */
    int32_t bid_levels;                /* levels recorded of the side: min(the side's levels, `levels`) */
    int32_t ask_levels;
} cda_depth_head;
typedef struct cda_depth_level {       /* word 1 + l of a record */
    int32_t bid_price;
    int32_t bid_volume;
    int32_t ask_price;
    int32_t ask_volume;
} cda_depth_level;
int cda_depth_enable(cda_env* env, int64_t capacity_steps, int32_t levels);
int cda_depth_disable(cda_env* env);
int64_t cda_depth_capacity(const cda_env* env);
int32_t cda_depth_levels(const cda_env* env);
int cda_depth_meta(cda_env* env, int32_t first_market, int32_t n_markets, int32_t* meta_out_dev, void* stream);
int cda_depth_series(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, int32_t k, void* records_out_dev, int32_t* counts_out_dev,
                     int32_t* info_out_dev, void* stream);
int cda_depth_profile(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, int32_t max_dist, int64_t* base_out_dev, int64_t* levels_out_dev,
                      int64_t* shape_out_dev, int32_t* info_out_dev, void* stream);
int cda_depth_imbalance(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* lags_host, int32_t n_lags, int32_t k, int32_t half,
                        int64_t* resp_out_dev, int64_t* base_out_dev, int32_t* info_out_dev, void* stream);
int cda_depth_ofi(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, const int32_t* lags_host, int32_t n_lags, int32_t bar_steps,
                  const int32_t* depths_host, int32_t n_depths, int64_t* lagged_out_dev, int64_t* base_out_dev, int32_t* info_out_dev, void* stream);
int cda_depth_check_host(int32_t kind, int32_t levels, const int32_t* lags_host, int32_t n_lags, int32_t a, int32_t b, const int32_t* depths_host, int32_t n_depths);

/* ---- order tape: every decoded order of a step and its execution rank, recorded on the device, and two order-flow reports -----------------
 * The trade tape holds what a step's orders did, the quote and depth tapes the book they met; this holds the orders themselves: what every agent
 * sent - type, side, size, price as the step decodes them (the `lob_actions` info words) - and where the step's shuffle put it in the execution
 * order.  cda_order_tape_enable(env, capacity_steps): from now on every step launch of this env first records, for every market of its range
 * whose episode is not over, one record of 1 + num_agents 16-byte words into the market's ring of `capacity_steps` records (a power of two in
 * 1 .. CDA_QUOTE_CAP_MAX; n_markets x capacity x (1 + num_agents) x 16 bytes of its own beside the arena; CDA_ERR_NOMEM leaves the env as it was).
 * The recorder's launch runs behind the order schedule's, the quote recorder's and the depth recorder's and ahead of the step kernel; it decodes
 * the step's actions and shuffles them on a COPY of the market's generator state: it consumes no draw and writes nothing into the market record.
 * OFF by default; enable / disable are synchronous, as cda_quotes_enable is, and everything said there of graphs, cda_policy_step_supported and
 * cda_net_step_supported (0 while on), cda_run_random (CDA_ERR_UNSUPPORTED while on), snapshots and state dumps (unchanged) holds.
 * Word 0 = cda_order_head.  Word 1 + a = cda_order_slot of agent a:
 *   code    -1: the agent was not present in this step (size, price = -1, action = 0).  Otherwise bits 0-1 = type (0 market, 1 limit, 2 modify,
 *           3 cancel), bits 2-3 = side (0 bid, 1 ask, 2 passed), bits 4-7 = execution rank (0 = executed first; 0 for a pass), bit 8
 *           (CDA_ORDER_CLAMPED) = the decode clamped size or price (the step flags CDA_FLAG_INT_OVERFLOW).
 *   size, price   the `lob_actions` words: price in ticks, -1 for a market order; both -1 for a pass.
 *   action  the clamped raw action: category | level << 4 | offset << 8 (category 0 .. 8, level 0 .. 9, offset 0 .. 2).
 * Episodes: the quote tape's meta row and its ONE rule (above), over rows and rings of this service's own; a record is indexed by its step.
 *   cda_order_tape_meta    the rolled meta rows -> meta_out_dev i32 [n][8].
 *   cda_order_tape_series  the last k held records of the episode `which`, oldest first -> records_out_dev i32 [n][k][(1 + num_agents) x 4] (16-B
 *                          aligned; rows beyond the count are zero), counts_out_dev i32 [n] and info_out_dev i32 [n][4] (either may be NULL) as
 *                          cda_quote_series.
 * Two reductions, one launch each, a wave per market, exact int64, every output word additive; order_tape.py states every word in numpy.
 *   cda_order_flow   flow_out_dev i64 [n][num_agents][CDA_ORDER_FLOW_WORDS] over the held records of the episode: steps present, passes, steps
 *                    absent; per type x side (index type x 2 + side) orders and submitted quantity; for LIMIT orders against the record's own touch:
 *                    crossing (bid price >= best_ask with the ask side non-empty, ask price <= best_bid with the bid side non-empty), else with
 *                    the own side empty no_reference, else inside (improves the own best), at_touch, behind and behind_ticks (the summed distance
 *                    to the own best / the market's tick_size); zeros up to 32 words.  info_out_dev i32 [n][4] as cda_quote_stats.
 *   cda_order_fills  fills_out_dev i64 [n][num_agents][CDA_ORDER_FILL_WORDS]: the trade tape of the episode joined to the order records on the
 *                    fill's step.  Per order type (4): orders, submitted quantity (over the held order records), orders with at least one fill as
 *                    initiator in their own step, quantity so filled - a held fill with init_id == a at step s belongs to agent a's order of step
 *                    s.  Then maker_fills, maker_qty (counter_id == a), self_fills, self_qty (both ids == a), unmatched_fills, unmatched_qty
 *                    (init_id == a and no order record of the step is held, or a sent no order in it: hook, stream or scheduled flow), zeros up to
 *                    24 words.  A fill with an id outside the env's agents is skipped.  Needs both tapes: CDA_ERR_UNSUPPORTED while either is
 *                    off.  info_out_dev i32 [n][8] (may be NULL): {order records held, lost, step of the first, partial, fills held, lost, step of
 *                    the first held fill (-1: none), partial}.
 *   cda_order_tape_check_host  the argument check of the entry points, on the host alone: kind = CDA_ORDER_CHECK_ENABLE (a = capacity_steps) /
 *                    _SERIES (a = which, b = k) / _REPORT (a = which); num_agents = the env's; CDA_OK or CDA_ERR_INVALID.
 * A NULL pointer, a misaligned output (records 16 B, int64 8 B, int32 4 B), a range outside the env, another `which`: CDA_ERR_INVALID; the tape
 * off: CDA_ERR_UNSUPPORTED from the readers.  Nothing is launched behind a refusal. */
#define CDA_ORDER_FLOW_WORDS   32
#define CDA_ORDER_FILL_WORDS   24
#define CDA_ORDER_CLAMPED      256
#define CDA_ORDER_CHECK_ENABLE 0
#define CDA_ORDER_CHECK_SERIES 1
#define CDA_ORDER_CHECK_REPORT 2
typedef struct cda_order_head {        /* word 0 of a record */
    int32_t step;                      /* the env step index t of the episode */
    int32_t flags;                     /* bits 0 / 1 = CDA_QUOTE_BID / CDA_QUOTE_ASK: the side is non-empty ahead of the step; bits 8..15: orders; bits 16..23: passes */
    int32_t best_bid;                  /* ahead of the step, in ticks; 0 where the side is empty */
    int32_t best_ask;
} cda_order_head;
typedef struct cda_order_slot {        /* word 1 + a of a record */
    int32_t code;
    int32_t size;
    int32_t price;
    int32_t action;
} cda_order_slot;
int cda_order_tape_enable(cda_env* env, int64_t capacity_steps);
int cda_order_tape_disable(cda_env* env);
int64_t cda_order_tape_capacity(const cda_env* env);
int cda_order_tape_meta(cda_env* env, int32_t first_market, int32_t n_markets, int32_t* meta_out_dev, void* stream);
int cda_order_tape_series(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, int32_t k, void* records_out_dev, int32_t* counts_out_dev,
                          int32_t* info_out_dev, void* stream);
int cda_order_flow(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, int64_t* flow_out_dev, int32_t* info_out_dev, void* stream);
int cda_order_fills(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, int64_t* fills_out_dev, int32_t* info_out_dev, void* stream);
int cda_order_tape_check_host(int32_t kind, int32_t num_agents, int64_t a, int32_t b);

/* ---- the P&L report: every agent's mark-to-mid equity curve over one remembered episode, on the device -----------------------------------
 * What did each agent's P&L do over the episode: the trade tape joined to the quote tape on the bar points, one launch on `stream`, a wave per
 * market, no atomics on global memory; pnl.py states every word in numpy.  The conventions of the stylised-facts report hold: m2(s) = bid_price
 * + ask_price of the held, two-sided quote record of step s; point p is step p x bar_steps on the episode's absolute grid and is HELD iff its
 * quote record is.  The MARK m(p) is m2 of the latest held point p' <= p whose quote is two-sided - carried forward over points, not over the
 * steps between them; a held point is MARKED if there is such a p' (the held points before the first two-sided one are unmarked) and STALE if it
 * is marked and its own quote is not two-sided.  An agent's fills are the non-self fills (counter_id != init_id) it is a party of, signed sq =
 * +quantity where it bought (its side bit is 0), -quantity where it sold; a fill of step s is INSIDE point p iff s < p x bar_steps (the quote of
 * a step is taken ahead of the step's orders).  pos(p) = the sum of sq, C(p) = the sum of -sq x price over the held fills inside p, and the
 * equity, in half price units, is E(p) = 2 C(p) + pos(p) m(p) at the marked points.  For adjacent marked points the increment d_p = E(p + 1) -
 * E(p) = inv_p + trd_p exactly, inv_p = pos(p) (m(p + 1) - m(p)) the carried inventory times the mid's move, trd_p = the sum over the agent's
 * fills of bar p of sq (m(p + 1) - 2 price).  Nothing is extrapolated: where the tape ring has lost the episode's head pos and C start from the
 * first held fill, where the quote ring has, the points start at the first held quote; info says what was lost.  Fills at steps >= (the last
 * marked point) x bar_steps - all fills, where no point is marked - are in no equity point: OPEN, counted, never marked.
 *   stats_out_dev     i64 [n][A][CDA_PNL_WORDS]: points (marked), stale, unmarked, bars (increments), equity_first, equity_last, inventory (sum
 *                     inv_p), trading (sum trd_p), sum_d2 (sum d_p^2), up, down (bars with d_p > 0 / < 0), under_water (marked points with E below
 *                     its running maximum, which starts at equity_first), max_drawdown (max of running maximum - E, >= 0), equity_max, equity_min
 *                     (over the marked points; 0 where there is none), open_fills.  Products are int64 and sums wrap in two's complement; a bar's
 *                     signed quantity is kept as an int32 word, as cda_tape_flow_returns' Q_b.  All words are additive except max_drawdown and
 *                     equity_max, which fold by max, and equity_min, which folds by min - over the rows with points > 0.
 *   equity_out_dev    i64 [n][A][n_points] or NULL: E(p) on the absolute grid, 0 where p is not marked.
 *   position_out_dev  i32 [n][A][n_points] or NULL: pos(p), 0 where p is not held.
 *   marks_out_dev     i32 [n][n_points] or NULL: m(p), 0 where p is not marked.
 *   info_out_dev      i32 [n][4] or NULL, as cda_tape_spreads fills it.
 * Needs both tapes on, else CDA_ERR_UNSUPPORTED.  The bar points of the range's longest episode, ceil(largest max_step / bar_steps), must be <=
 * CDA_STYL_MAX_BARS and, with any series output, <= n_points: checked on the host before the launch - cda_tape_pnl_check_host is that check alone
 * (no env, no device; want_series != 0: a series output is asked for; max_step = the largest max_step of the range).  A NULL stats, a misaligned
 * output (8 B; the int32 outputs 4 B), a range outside the env, another `which`, bar_steps < 1 or too many points: CDA_ERR_INVALID, nothing is
 * launched.  Every word of every requested output is written exactly once - rows and columns of unheld points are zeros: no memset needed. */
#define CDA_PNL_WORDS 16
int cda_tape_pnl(cda_env* env, int32_t first_market, int32_t n_markets, int32_t which, int32_t bar_steps, int64_t* stats_out_dev, int64_t* equity_out_dev,
                 int32_t* position_out_dev, int32_t* marks_out_dev, int32_t n_points, int32_t* info_out_dev, void* stream);
int cda_tape_pnl_check_host(int32_t bar_steps, int32_t n_points, int32_t want_series, int32_t max_step);

/* ---- the book report: reductions over the STANDING book, on the device ------------------------------------------------------------------
 * The resting orders of markets [first_market, first_market + n_markets), read where they lie - the record's tile and, behind it, the HBM spill
 * ring - by one wave per (market, side), one launch each, on `stream`; no call synchronises the host and none writes the arena.  A side is walked
 * in queue order: best price first, FIFO inside a level (the order of cda_get_book).  Side 0 = bids, 1 = asks.  All sums are 64-bit integers:
 * the results are exact and do not depend on scheduling.  A = num_agents.
 *   cda_book_counts    counts_out_dev i32 [n][2][2] = (resting orders, distinct price levels) per side.
 *   cda_book_levels    the Level-2 ladder over the WHOLE side, ring included: levels_out_dev i64 [n][2][max_levels][3] = (price, volume, orders) per
 *                      level, best first; rows past the side's level count are zero.  1 <= max_levels <= CDA_BOOK_MAX_LEVELS.
 *   cda_book_impact    what a market order of sizes_host[k] units would pay now: impact_out_dev i64 [n][2][n_sizes][3] = (filled, notional,
 *                      last_price) for an order that consumes this side by price-time priority - side 0: the bids, hit by a sell; side 1: the asks,
 *                      lifted by a buy; the taker's own resting orders are part of the side, as they are for the matching loop.  filled =
 *                      min(size, the side's quantity); notional = sum of price x quantity over what is consumed, the last order partially;
 *                      last_price = the price of the last order touched, 0 on an empty side.  sizes_host: n_sizes int64 >= 1, read during the
 *                      call, 1 <= n_sizes <= CDA_BOOK_MAX_SIZES (they travel in the kernel arguments).
 *   cda_book_agents    agents_out_dev i64 [n][2][A][6] = (orders, quantity, notional = sum of price x quantity, best_price, worst_price, ahead_qty)
 *                      per agent and side; best_price / worst_price = the prices of the agent's first / last own order in queue order, ahead_qty =
 *                      the quantity resting strictly before the agent's first own order in queue order; all six are 0 for an agent with nothing on
 *                      that side.  An agent's bid + ask notional is its cash_on_hold.
 *   cda_book_offsets   the Level-3 dump of all markets in two launches, first half: offsets_dev i64 [2 n + 1], the exclusive scan of the sides'
 *                      order counts (offsets[2 n] = orders in all).
 *   cda_book_pack      second half: orders_out_dev i32 [capacity_orders][5], rows of (price, qty, owner, order_id, timestamp) - cda_order, the rows
 *                      of cda_get_book; side s of market first + i lies at rows offsets[2 i + s] .. offsets[2 i + s + 1].  total_orders = the
 *                      offsets[2 n] the caller read (its one 8-byte read); capacity_orders >= total_orders.  The env must not be stepped between
 *                      the two calls (stream order); a side whose count no longer matches its offsets is left alone.
 * NULL env or output, a range outside the env, max_levels or n_sizes outside their bounds, a size < 1, a misaligned output, capacity_orders <
 * total_orders: CDA_ERR_INVALID, nothing is launched. */
#define CDA_BOOK_MAX_LEVELS 4096
#define CDA_BOOK_MAX_SIZES  16
int cda_book_counts(cda_env* env, int32_t first_market, int32_t n_markets, int32_t* counts_out_dev, void* stream);
int cda_book_levels(cda_env* env, int32_t first_market, int32_t n_markets, int32_t max_levels, int64_t* levels_out_dev, void* stream);
int cda_book_impact(cda_env* env, int32_t first_market, int32_t n_markets, const int64_t* sizes_host, int32_t n_sizes, int64_t* impact_out_dev, void* stream);
int cda_book_agents(cda_env* env, int32_t first_market, int32_t n_markets, int64_t* agents_out_dev, void* stream);
int cda_book_offsets(cda_env* env, int32_t first_market, int32_t n_markets, int64_t* offsets_dev, void* stream);
int cda_book_pack(cda_env* env, int32_t first_market, int32_t n_markets, const int64_t* offsets_dev, int64_t total_orders, void* orders_out_dev,
                  int64_t capacity_orders, void* stream);

/* ---- scripted opponents: rule-based agents on the device ---------------------------------------------------------------------------------
 * The laws (pass, noise taker, market maker, order-imbalance trader), their 64-byte cda_script_profile and the integer cda_script_view they read are stated
 * once, in include/cda_scripted_agents.h (cda_scripted_decide); the reference has no such opponent.  The pointers below named profiles / views are arrays of
 * those structs.
 *   cda_scripted_attach   slot_script_dev i32 [N][A] (device): 0 = the slot is not scripted, 1 + k = it plays profiles_dev[k]; profiles_dev: n_profiles
 *                         (1 .. 16) profiles (device, 8-B aligned).  Both tables are read back and vetted first: an invalid profile or a slot value outside
 *                         0 .. n_profiles returns CDA_ERR_INVALID and changes nothing (synchronous).  The env KEEPS the two pointers - the caller's resident
 *                         tensors, the scheme of cda_league.slot_net - so a captured graph stays valid while their contents change; `seed` keys the taker's
 *                         draws, market_index_base + market is the market's global index in them (the shards of a multi-GPU run draw as the whole would).
 *   cda_scripted_detach   forgets them.  Every attach and detach moves cda_scripted_epoch (a graph captured under another epoch holds stale launches);
 *                         while scripts are attached cda_policy_step_supported answers 0, as it does for the tape.
 *   cda_scripted_actions  ONE launch on `stream`, a wave per market of the range: every scripted slot's action of the market's state NOW, into the five
 *                         FULL [N][A] action arrays (indexed by global market, as cda_step_range reads them), and - where given - a_cont f32 [N][A][2] = 0, 0,
 *                         logp f32 [N][A] = 0 and the 32-byte sample record f32 [N][A][8] as the league's random module writes it (category, price,
 *                         price_offset, 0 | 0, 0; words 6, 7 untouched; 16-B aligned).  Slots that are not scripted keep their bytes; the arena is only
 *                         read.  The taker's draw is keyed (seed, *counter_dev or 0 when NULL, global market, draw, agent).  Nothing attached: CDA_OK, no launch.
 *                         cda_mlp_rollout_chain and its league / eval siblings call it between the policy launch and the step.
 *   cda_scripted_decide_host   the same function on host arrays, no device: item i plays profiles_host[profile_index_host[i]] on views_host[i] with the key
 *                         (seed, counter, market_host[i], draw_host[i], agent_host[i]).  cda_scripted_profile_check_host: CDA_OK iff every profile is valid. */
int cda_scripted_attach(cda_env* env, const int32_t* slot_script_dev, const void* profiles_dev, int32_t n_profiles, uint64_t seed, uint64_t market_index_base);
int cda_scripted_detach(cda_env* env);
int64_t cda_scripted_epoch(const cda_env* env);
int cda_scripted_attached(const cda_env* env);
int cda_scripted_actions(cda_env* env, int32_t first_market, int32_t n_markets, const int64_t* counter_dev, int64_t draw,
                         int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset,
                         float* a_cont, float* logp, float* record, void* stream);
int cda_scripted_decide_host(const void* profiles_host, int32_t n_profiles, const int32_t* profile_index_host, const void* views_host, int64_t n,
                             uint64_t seed, uint64_t counter, const uint64_t* market_host, const uint32_t* draw_host, const uint32_t* agent_host,
                             int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset);
int cda_scripted_profile_check_host(const void* profiles_host, int32_t n_profiles);

/* ---- the label tap: a law's answer for slots it does not play (DAgger) -------------------------------------------------------------------
 * Behaviour cloning records what the scripted slots did in THEIR situation.  The tap asks a law about any slot - the learner's, with the learner's position and
 * resting orders - at every step of a rollout chain, keeps the answer beside the rollout's buffers and, for DAgger's beta-mixture, lets it replace the slot's
 * action with a given probability.  One kernel (csrc/cda_scripted_label.inc k_script_label) serves the attached scripts and the label table in one walk of the book.
 *   cda_label_tap_attach  slot_label_dev i32 [N][A] (device): 0 = not labelled, 1 + k = labelled by profiles_dev[k] (n_profiles 1 .. 16, device, 8-B aligned), with
 *                         `seed` and market_index_base of its own.  mix_q32_dev: ONE u64 in device memory, 0 .. 2^32, read by the kernel at every launch - the host
 *                         may rewrite it between replays of a captured graph.  rows: the rows of the six label buffers, each [rows][N][A] (category, price,
 *                         price_offset, played i32; size_mean, size_sigma f32; 4-B aligned).  Both tables and the mix word are read back and vetted first: an invalid
 *                         profile, a slot value outside 0 .. n_profiles, a mix word above 2^32, a bad alignment or rows < 1 returns CDA_ERR_INVALID and changes
 *                         nothing (synchronous).  The env KEEPS every pointer: the caller's resident memory, as with cda_scripted_attach.
 *   cda_label_tap_detach  forgets them.  Every attach and detach moves cda_label_tap_epoch; while a tap is attached cda_policy_step_supported answers 0.
 *   cda_scripted_step_actions   what a rollout chain calls between the policy launch and step t (cda_mlp_rollout_chain and its siblings).  No tap: it IS
 *                         cda_scripted_actions with draw = t - the same kernel and launch, or none.  Tap attached: ONE k_script_label launch.  An attached slot gets
 *                         exactly what cda_scripted_actions writes.  A labelled slot's five words go to row t of the label buffers, and `played` gets 0 or 1:
 *                         for a labelled slot that is NOT attached, w = cda_script_mix_draw(label seed, *counter_dev or 0, market_index_base + market, t, agent)
 *                         (include/cda_scripted_agents.h), and if (w & 0xffffffff) < *mix_q32_dev the label also overwrites the slot's env action - a_cont, logp and
 *                         the record as a scripted slot's - and played = 1.  A slot both attached and labelled plays its attached law and is never mixed.  A slot
 *                         named in neither table keeps all its bytes.  t >= rows: CDA_ERR_INVALID before any launch.
 *   cda_label_actions     the labels of the state NOW, one launch, no tap needed: the given table's answers into five [N][A] arrays (global market index), written only
 *                         where the table names a profile (a value outside 1 .. n_profiles names none); no mixing, the env's actions are not touched.  Asynchronous:
 *                         the tables are not read back.
 *   cda_label_mix_host    the mix decision on host arrays: played_out[i] = (cda_script_mix_draw(seed, counter, market[i], draw[i], agent[i]) & 0xffffffff) < mix_q32.
 * Not covered: the league chains' UPDATE (a mixed-in action is no policy sample), checkpoints and snapshots (a tap is not saved), the dict facades, data-parallel runs. */
int cda_label_tap_attach(cda_env* env, const int32_t* slot_label_dev, const void* profiles_dev, int32_t n_profiles, uint64_t seed, uint64_t market_index_base,
                         const uint64_t* mix_q32_dev, int32_t rows, int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset,
                         int32_t* played);
int cda_label_tap_detach(cda_env* env);
int cda_label_tap_attached(const cda_env* env);
int64_t cda_label_tap_epoch(const cda_env* env);
int cda_scripted_step_actions(cda_env* env, int32_t first_market, int32_t n_markets, const int64_t* counter_dev, int32_t t,
                              int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset,
                              float* a_cont, float* logp, float* record, void* stream);
int cda_label_actions(cda_env* env, int32_t first_market, int32_t n_markets, const int32_t* slot_label_dev, const void* profiles_dev, int32_t n_profiles, uint64_t seed,
                      uint64_t market_index_base, const int64_t* counter_dev, int64_t draw, int32_t* category, float* size_mean, float* size_sigma, int32_t* price,
                      int32_t* price_offset, void* stream);
int cda_label_mix_host(uint64_t seed, uint64_t counter, const uint64_t* market_host, const uint32_t* draw_host, const uint32_t* agent_host, int64_t n, uint64_t mix_q32,
                       int32_t* played_out);

/* ---- scripted opponents with memory: trend, value and execution laws on per-slot state -----------------------------------------------------
 * A sibling family of the scripted opponents above: the laws, their 64-byte cda_stateful_profile, the per-slot state (CDA_STATEFUL_WORDS = 4 int64, word 0 the
 * header: last t_step | tag) and the one update rule are stated once, in include/cda_stateful_agents.h (cda_stateful_advance, cda_stateful_decide).  The view is
 * cda_script_view as it is.  The stateless family's entry points, kernels and profile are untouched; with nothing stateful attached an env launches what it launched.
 *   cda_stateful_attach   slot_dev i32 [N][A] (device): 0 = the slot is not stateful, 1 + k = it plays profiles_dev[k]; profiles_dev: n_profiles (1 .. 16) profiles
 *                         (device, 8-B aligned); state_dev i64 [N][A][4] (device, 32-B aligned: CDA_ERR_INVALID otherwise), zeroed by the caller for a fresh start.
 *                         Both tables are read back and vetted first: an invalid profile or a slot value outside 0 .. n_profiles returns CDA_ERR_INVALID and changes
 *                         nothing (synchronous).  The env KEEPS the three pointers - the caller's resident tensors - so a captured graph stays valid while their
 *                         contents change; `seed` keys the value law's draws, market_index_base + market is the market's global index in them.
 *   cda_stateful_detach   forgets them.  Every attach and detach moves cda_stateful_epoch; while a table is attached cda_policy_step_supported and
 *                         cda_net_step_supported answer 0, as for scripts.
 *   cda_stateful_actions  ONE launch on `stream` (csrc/cda_stateful.inc k_stateful_actions), a wave per market of the range: every stateful slot's state advanced on
 *                         the market's state NOW and its action written, into the five FULL [N][A] action arrays and - where given - a_cont, logp and the sample
 *                         record exactly as cda_scripted_actions writes them for a scripted slot.  Slots that are not stateful keep their bytes, actions and state;
 *                         the arena is only read.  A second call at the same t_step changes no state and writes the same action.  The value law's draw is keyed
 *                         (seed, *counter_dev or 0 when NULL, global market, draw, agent).  Nothing attached: CDA_OK, no launch.
 *                         cda_scripted_step_actions - the one call every rollout chain makes between the policy launch and the step - issues this launch, with
 *                         draw = t, BEHIND what it issues for the stateless family: a slot both tables name plays its stateful law.
 *   cda_stateful_advance_host   the same two functions on host arrays, no device: item i plays profiles_host[profile_index_host[i]] (its tag: 1 + that index) on
 *                         views_host[i] and the four words state_inout[4 i ..], advanced in place, with the key (seed, counter, market_host[i], draw_host[i],
 *                         agent_host[i]).  cda_stateful_profile_check_host: CDA_OK iff every profile is valid.
 * Not covered: training loops that attach stateful opponents themselves (a resumable run would have to carry the state tensor), the label tap with stateful experts,
 * data-parallel runs, the dict facades, the state inside cda_snapshot_* blobs (the caller clones and restores its own tensor). */
int cda_stateful_attach(cda_env* env, const int32_t* slot_dev, const void* profiles_dev, int32_t n_profiles, int64_t* state_dev, uint64_t seed, uint64_t market_index_base);
int cda_stateful_detach(cda_env* env);
int64_t cda_stateful_epoch(const cda_env* env);
int cda_stateful_attached(const cda_env* env);
int cda_stateful_actions(cda_env* env, int32_t first_market, int32_t n_markets, const int64_t* counter_dev, int64_t draw,
                         int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset,
                         float* a_cont, float* logp, float* record, void* stream);
int cda_stateful_advance_host(const void* profiles_host, int32_t n_profiles, const int32_t* profile_index_host, const void* views_host, int64_t n,
                              uint64_t seed, uint64_t counter, const uint64_t* market_host, const uint32_t* draw_host, const uint32_t* agent_host, int64_t* state_inout,
                              int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset);
int cda_stateful_profile_check_host(const void* profiles_host, int32_t n_profiles);

/* ---- order streams: explicit orders into every market of a range, in one launch ------------------------------------------------------------
 * cda_submit_orders plays, for every market of [first_market, first_market + n_markets), the messages msgs_dev[offsets_dev[i] .. offsets_dev[i + 1])
 * (i counts from the range's first market) in order: ONE asynchronous launch on `stream`, a wave per market, the market's record loaded once and
 * stored once.  For every market the stream is equivalent, bit for bit in the market's record (header, tile, HBM ring, accounts, sticky flags,
 * peak_orders, lob_time, order ids), to calling cda_place_order / cda_mark_to_mkt once per valid message, in order - the same instance of the
 * matching code (general book, full position-value semantics), the cached level aggregation invalidated as the hook does, no observation frame
 * pushed, t_step not moved, the episode-metric tallies not touched.  On a tape-enabled env the tape-writing sibling runs: the tape then holds what
 * the hook would have written call by call.
 *   validity     a message outside the hook's accepted domain - trader outside 0 .. num_agents-1, type outside 0 .. 4, side outside 0 / 1, size < 1,
 *                price < 1 for types 1 .. 3 - is SKIPPED: status CDA_ORD_INVALID, zero deltas, counted in the summary; the rest of the stream runs.  A
 *                CDA_OP_MARK message carries nothing but its type: its other fields are not looked at.  The device validates (the streams live in device
 *                memory); cda_order_msgs_check_host applies the same rule to host data: *first_bad_out = index of the first invalid message, -1 = none.
 *                (env NULL: trader is checked against CDA_MAX_AGENTS; cda_order_msgs_check_agents_host takes the agent count itself - neither needs a device.)
 *   empty        a market whose stream is empty is neither loaded nor stored: its record stays byte-identical.  So does a market none of whose messages
 *                was valid.
 *   offsets      non-decreasing.  A negative or decreasing pair makes that market's stream empty and sets its summary's `invalid` to -1.
 *   results_dev  one cda_order_result per message, indexed like msgs_dev (16-B aligned), or NULL.  summary_dev: int32 [n_markets][4] = messages done,
 *                rejected, invalid, and fills (16-B aligned), or NULL.
 *   flags        CDA_ORDERS_CLEAR_STEP_COUNTERS: after a market's stream every account's step counters are cleared (exchg_helper.py:116-120), so that
 *                seeded or exogenous flow does not reach the next step's reward terms - the one difference from the hook sequence.
 *   cda_submit_orders_window   the same for the messages [skip, skip + limit) of every market's stream, n_msgs = messages behind msgs_dev (a market whose
 *                offsets reach beyond them is treated like a decreasing pair; -1 = not known): successive windows give the state of one launch, so a caller
 *                can bound what a single launch runs.
 * NULL env / offsets / msgs, a range outside the env, a misaligned pointer, unknown flag bits, skip < 0, limit < 1: CDA_ERR_INVALID, nothing is launched. */
typedef struct cda_order_msg {       /* one message, 16 bytes, device memory */
    int32_t price;    /* ticks; ignored for a market order and for CDA_OP_MARK */
    int32_t size;
    int16_t trader;   /* 0 .. num_agents-1 */
    int8_t  type;     /* 0 market, 1 limit, 2 modify, 3 cancel (cda_place_order's), 4 = CDA_OP_MARK: Exchg_Helper.mark_to_mkt, no trader */
    int8_t  side;     /* 0 bid, 1 ask */
    int32_t tag;      /* caller's, copied nowhere: for the caller's own bookkeeping */
} cda_order_msg;
typedef struct cda_order_result {    /* one result per message, 16 bytes */
    int32_t status;          /* CDA_ORD_INVALID: not executed; CDA_ORD_REJECTED: Trader._order_approved said no; CDA_ORD_DONE */
    int32_t n_fills;         /* fills this message caused (self-trades included: one tape record each) */
    int32_t position_delta;  /* trader's net_position after - before */
    int32_t resting_delta;   /* resting orders of the market, both sides, tile + HBM ring, after - before */
} cda_order_result;
#define CDA_OP_MARK 4
#define CDA_ORD_INVALID  0
#define CDA_ORD_REJECTED 1
#define CDA_ORD_DONE     2
#define CDA_ORDERS_CLEAR_STEP_COUNTERS 1u
int cda_submit_orders(cda_env* env, int32_t first_market, int32_t n_markets, const int64_t* offsets_dev, const cda_order_msg* msgs_dev,
                      cda_order_result* results_dev, int32_t* summary_dev, uint32_t flags, void* stream);
int cda_submit_orders_window(cda_env* env, int32_t first_market, int32_t n_markets, const int64_t* offsets_dev, const cda_order_msg* msgs_dev, int64_t n_msgs,
                             int64_t skip, int64_t limit, cda_order_result* results_dev, int32_t* summary_dev, uint32_t flags, void* stream);
int cda_order_msgs_check_host(const cda_env* env, const cda_order_msg* msgs_host, int64_t n, int64_t* first_bad_out);
int cda_order_msgs_check_agents_host(int32_t num_agents, const cda_order_msg* msgs_host, int64_t n, int64_t* first_bad_out);

/* ---- order schedules: per-step order flow played inside steps and rollouts --------------------------------------------------------------------
 * An order schedule is attached to the env.  It holds n_sched rows of n_steps windows each: step_offsets_dev, int64 [n_sched][n_steps + 1], indexes one
 * array of cda_order_msg - row r owns, for step t of an episode, the messages msgs_dev[off[r][t] .. off[r][t + 1]); sched_of_dev, int32 [n_markets], names
 * every market's row (-1 = none; many markets may share a row).  All three live in caller-owned device memory that must stay valid, and unchanged, while
 * attached.  Every step entry point (cda_step, cda_step_range, cda_step_range_capture, cda_step_groups, cda_step_groups_handback - hence the rollout,
 * evaluation and league chains of include/cda_mlp.h, which step through them) first plays, on the same stream, the window of each market's current t_step,
 * then runs the step: window 0 is the seed book of every episode - the in-kernel auto reset included -, windows 1 .. are background flow that arrives
 * before the step's own orders execute (the agents decided on the state at the end of the previous step).
 *   which window   for market i of the range nothing plays when no schedule is attached, sched_of[i] < 0, or the market's episode is over (all agents
 *                  done, or t_step >= its max_step).  Otherwise t = t_step[i]; with CDA_SCHEDULE_LOOP t %= n_steps, without it t >= n_steps plays nothing.
 *   the play       the window's messages run in order under exactly the contract of cda_submit_orders above: each valid message equals one
 *                  cda_place_order / cda_mark_to_mkt call, invalid ones are skipped and counted, no observation frame is pushed, t_step does not move,
 *                  the episode-metric tallies are not touched, the cached level aggregation is invalidated when an order was placed, and a market whose
 *                  window is empty or holds nothing valid is neither loaded nor stored - its record stays byte-identical.  On a tape-enabled env the
 *                  tape-writing sibling runs.  The trader of a message is an ordinary agent slot (NAV conservation stays exact).
 *   flags          CDA_SCHEDULE_LOOP (above); CDA_SCHEDULE_CLEAR_STEP_COUNTERS = CDA_ORDERS_CLEAR_STEP_COUNTERS behind every played window - off, a
 *                  scheduled fill reaches the step's reward terms like any fill inside the step.
 *   cda_schedule_attach   reads both index tables back and vets them before the env changes (cda_schedule_check_host's rule; pointers aligned 4 / 8 /
 *                  16; no unknown flag bits): one fault returns CDA_ERR_INVALID and changes nothing.  It waits for the device to be idle, zeroes the
 *                  counters and moves cda_schedule_epoch; so does cda_schedule_detach (a graph captured under another epoch holds stale launches).
 *   cda_schedule_counts   the env-owned cumulative table, int64 [n_markets][4] = messages done, rejected, invalid, fills since the attach, rows
 *                  [first, first + n) copied to out_dev on `stream` (a market that never played a window: zeros).
 *   cda_schedule_play     the launch the step entry points issue first, on its own: a no-op while nothing is attached.  For tests and custom loops - a
 *                  caller who ALSO steps through the entry points plays the window twice.
 *   cda_schedule_check_host   the attach rule on host data, no device: CDA_OK, CDA_ERR_INVALID for a NULL / non-positive argument, or which table is
 *                  wrong - CDA_SCHEDULE_BAD_SCHED_OF (a value outside -1 .. n_sched-1), _BAD_START (a row starts below 0), _BAD_ROW (a row decreases),
 *                  _BAD_END (a row ends beyond n_msgs).
 * While a schedule is attached cda_policy_step_supported answers 0 (the chains take the two launches, as with scripted opponents) and cda_run_random
 * returns CDA_ERR_UNSUPPORTED.  Snapshot blobs carry no schedule: restoring keeps the target env's attachment, and t_step - in the blob - puts a restored
 * market at the right window. */
#define CDA_SCHEDULE_LOOP 1u
#define CDA_SCHEDULE_CLEAR_STEP_COUNTERS 2u
#define CDA_SCHEDULE_BAD_SCHED_OF 1
#define CDA_SCHEDULE_BAD_START    2
#define CDA_SCHEDULE_BAD_ROW      3
#define CDA_SCHEDULE_BAD_END      4
int cda_schedule_attach(cda_env* env, const int32_t* sched_of_dev, const int64_t* step_offsets_dev, int32_t n_sched, int32_t n_steps,
                        const cda_order_msg* msgs_dev, int64_t n_msgs, uint32_t flags);
int cda_schedule_detach(cda_env* env);
int cda_schedule_attached(const cda_env* env);
int64_t cda_schedule_epoch(const cda_env* env);
int cda_schedule_counts(cda_env* env, int32_t first_market, int32_t n_markets, int64_t* out_dev, void* stream);
int cda_schedule_play(cda_env* env, int32_t first_market, int32_t n_markets, void* stream);
int cda_schedule_check_host(int32_t num_agents, int32_t n_markets, const int32_t* sched_of, const int64_t* step_offsets, int32_t n_sched, int32_t n_steps,
                            int64_t n_msgs);

/* ---- per-market parameters: many configurations in one env ----------------------------------------------------------------------------
 * Every market reads the fields below from a row of its own (a device table every env has; cda_create fills each row from the config).  The
 * config's other fields - num_agents, n_hist, book_capacity, book_spill, auto_reset - set shapes, memory and kernel choice and hold for the
 * whole env.
 *   cda_market_params_from_config   the row a config implies (host only).
 *   cda_check_market_params         validates rows against an env config without a device: a row is valid when the config with the row merged
 *                                   in passes cda_create's checks and row.max_step <= config.max_step (the automatic spill ring is sized from
 *                                   the config's horizon); CDA_ERR_UNSUPPORTED for a tick outside 1 .. CDA_TICK_MAX, CDA_ERR_INVALID otherwise.
 *   cda_set_market_params           rows_host[i] -> market first_market + i.  Every row is validated first (the checks above, and a size scale
 *                                   that fits the env's spill ring); one bad row returns the error and changes nothing.  Synchronous: it waits
 *                                   for the device to be idle, then writes the table.
 *   cda_get_market_params           the rows last written (the config's row for a market never set).
 * Contract: a kernel uses the row that is in the table when it runs.  The markets are NOT reset: a changed init_cash, price range or horizon
 * acts on a running episode from its next step on (sum(NAV) is then checked against the new init_cash) - resetting the changed markets is the
 * caller's business (the Python env does it).  A snapshot blob carries no rows: restoring one keeps the target markets' rows. */
typedef struct cda_market_params {
    int32_t max_step;
    int32_t tick_size;
    int64_t init_cash;
    int32_t initial_price_min, initial_price_max;
    int32_t min_size, mkt_max_size, limit_size_multiple;
    int32_t reserved;               /* 0 */
    double  order_penalty, trade_penalty, drawdown_penalty, passive_bonus, loss_multiplier;
} cda_market_params;
int cda_market_params_from_config(const cda_config* cfg, cda_market_params* out_host);
int cda_check_market_params(const cda_config* env_cfg, int32_t n, const cda_market_params* rows_host);
int cda_set_market_params(cda_env* env, int32_t first_market, int32_t n_markets, const cda_market_params* rows_host);
int cda_get_market_params(const cda_env* env, int32_t first_market, int32_t n_markets, cda_market_params* rows_host_out);

const char* cda_strerror(int status);
int32_t cda_num_markets(const cda_env* env);
int32_t cda_num_agents(const cda_env* env);
int32_t cda_book_capacity(const cda_env* env);   /* 256 or 512: the LDS tile this env was built with */
int32_t cda_obs_dim(const cda_env* env);
/* Bytes the arena keeps per market in HBM. */
int64_t cda_state_bytes_per_market(const cda_env* env);

#ifdef __cplusplus
}
#endif
#endif /* CDA_H */
