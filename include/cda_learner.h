/*
 * cda_learner.h - C-ABI of the learner-side kernels that do not depend on the network's shape: the epoch's keyed permutation, the two unfused PPO loss
 * kernels, generalised advantage estimation into the sample records, the returns of completed episodes and the league's per-episode slot assignment
 * (csrc/cda_learner.hip).
 *
 * Unlike the entry points of cda_mlp.h these exist ONCE in the library, under the names below: none of them reads the history depth, the hidden activation or
 * vf_share_layers, so they carry no [_h<H>][_<act>][_vfs] suffix (csrc/cda_mlp_variant.h) and serve every compiled network variant.  They see a network only
 * through its 32-float output rows (24 policy outputs | value | padding: the layout at the top of cda_mlp.h, the same at every depth) and the sample records.
 *
 * cda_mlp.h includes this header, so a consumer of the network's C-ABI has these declarations too.  Conventions as in cda.h: device pointers, caller-owned,
 * plain sizes; CDA_OK or a negative cda_status; kernels are enqueued on `stream`.  No CPU fallback.
 */
#ifndef CDA_LEARNER_H
#define CDA_LEARNER_H

#include <stdint.h>
#include "cda.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The policy heads' columns of a network output row: CDA_HEAD_CATEGORY + CDA_HEAD_PRICE + CDA_HEAD_OFFSET categorical logits, then the two Gaussian means =
 * CDA_HEAD_LOGITS columns; column CDA_HEAD_LOGITS is the value. */
#define CDA_HEAD_CATEGORY 9
#define CDA_HEAD_PRICE    10
#define CDA_HEAD_OFFSET   3
#define CDA_HEAD_LOGITS   24

/* An epoch's shuffle: perm i64[n] = a pseudo-random PERMUTATION of 0 .. n-1 determined by `key` (a keyed bijective mixer + cycle walking, one
 * launch; the sort behind torch.randperm is ~10 launches). */
int cda_mlp_permutation(uint64_t key, int64_t n, int64_t* perm, void* stream);

/* cda_ppo_loss (cda.h) for int32 action arrays - the env's own action tensors as the rollout kernel wrote them.  norm_rows > 0:
 * the means (and the gradient's 1/B) are over norm_rows * agents_per_row samples instead of rows * agents_per_row (a minibatch
 * processed in several sub-batches); sums5 is then NOT cleared and out6 not written unless finish != 0. */
int cda_ppo_loss32(const float* outputs, const float* log_std, const int32_t* a_cat, const int32_t* a_price, const int32_t* a_off,
                   const float* a_cont, const float* logp_old, const float* adv, const float* ret, const int64_t* row_index,
                   int64_t rows, int32_t agents_per_row, int32_t out_stride, float clip, float vf_coef, float ent_coef,
                   float* d_outputs, double* sums5, float* out6, int64_t norm_rows, int32_t clear, int32_t finish, void* stream);

/* Sample records: what the update's loss reads of a sample, as ONE 32-byte record - a row's A samples are then one contiguous piece (the seven
 * separate per-sample arrays cost seven scattered gathers per row).  Words: */
#define CDA_REC_CATEGORY  0   /* i32 */
#define CDA_REC_PRICE     1   /* i32 */
#define CDA_REC_OFFSET    2   /* i32 */
#define CDA_REC_CONT0     3   /* f32: the raw Gaussian samples */
#define CDA_REC_CONT1     4
#define CDA_REC_LOGP      5   /* f32: log-probability under the rollout's policy */
#define CDA_REC_ADV       6   /* f32: advantage (unnormalised) */
#define CDA_REC_RET       7   /* f32: return */
/* Generalised advantage estimation of a whole rollout, straight from its buffers into the records (ppo.gae's recursion, one launch): reward f64
 * [T][N][A] (scaled by reward_scale here), value f32 [T+1][N] (slot T = the bootstrap value), terminated / truncated u8 [T][N] -> words ADV, RET
 * of rec [T][N][A][8]; stats2 f64[2] receives the sum of the advantages and of their squares. */
int cda_gae_records(const double* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int64_t n_markets,
                    int32_t num_agents, float reward_scale, float gamma, float lam, float* rec, double* stats2, void* stream);
/* The same with the time-limit bootstrap RLlib applies (a TRUNCATED, not terminated, step's target continues with V(last observation of the cut episode) instead of 0;
 * the device-side auto reset overwrites that observation, so the rollout captures it: cda_rollout_bufs.fin_*): fin_index i32 [T][N], fin_value f32
 * [max(n_trainable, 1)][fin_value_stride] = cda_mlp_values on the captured list.  n_trainable = 0: one shared policy; > 0: the league layout below. */
int cda_gae_records_bootstrap(const double* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int64_t n_markets,
                              int32_t num_agents, int32_t n_trainable, float reward_scale, float gamma, float lam,
                              const int32_t* fin_index, const float* fin_value, int64_t fin_value_stride, float* rec, double* stats, void* stream);
/* Training against scripted opponents (include/cda.h cda_scripted_attach): ONE shared policy plays and trains slots 0 .. n_slots - 1 of every market, the slots behind
 * them are scripted - their records hold no policy sample and must reach no loss.  cda_gae_records_bootstrap(n_trainable = 0)'s recursion, thread for thread, over the
 * slots < n_slots only: words ADV, RET of those slots' records are bit-equal to what it writes there, the other slots' words ADV, RET are NOT written, and stats2 f64[2]
 * sums the T * N * n_slots trained samples (that product is the count the update normalises with).  value f32 [T+1][N]; fin_index (NULL = no time-limit bootstrap) i32
 * [T][N], fin_value f32 [capacity].  The update then reads the leading slots through the record stride: cda_mlp_forward_backward(agents_per_row = n_slots,
 * cda_ppo_extra.rec_stride = 8 * num_agents).  1 <= n_slots <= num_agents. */
int cda_gae_records_slots(const double* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int64_t n_markets,
                          int32_t num_agents, int32_t n_slots, float reward_scale, float gamma, float lam,
                          const int32_t* fin_index, const float* fin_value, float* rec, double* stats2, void* stream);

/* cda_gae_records for a league: value f32 [n_trainable][T+1][N]; slot p < n_trainable gets advantage / return from net p's values, the other slots' records are left
 * alone; stats2k f64 [n_trainable][2]: per net, the sums its update normalises the advantages with. */
int cda_gae_records_league(const double* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int64_t n_markets,
                           int32_t num_agents, int32_t n_trainable, float reward_scale, float gamma, float lam, float* rec, double* stats2k, void* stream);

/* Returns of COMPLETED episodes out of a rollout's buffers (what a learning curve is drawn from when the horizon is shorter than an episode): running f64 [N][A]
 * carries each (market, agent)'s return so far from rollout to rollout; a step that ends the market's episode adds the total to done_sum f64 [A] and 1 to
 * done_count f64 [A] (both accumulate: the caller clears them) and restarts it.  per_slot: what a league needs to credit returns to the MODULE that played a slot. */
int cda_episode_returns(const double* reward, const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int64_t n_markets, int32_t num_agents,
                        double* running, double* done_sum, double* done_count, double* per_slot /* f64 [N][A][2] or NULL: this rollout's (sum, number) per (market, agent) */, void* stream);
/* cda_ppo_loss32 reading sample records (rec = [all rows][A][8]; row_index as there).  adv_stats2 (may be NULL) + adv_count: the advantages are
 * normalised on the fly, (adv - mean) / (std + 1e-8) with the unbiased std over the adv_count samples the sums were taken over. */
int cda_ppo_loss_records(const float* outputs, const float* log_std, const float* rec, const double* adv_stats2, int64_t adv_count, const int64_t* row_index,
                         int64_t rows, int32_t agents_per_row, int32_t out_stride, float clip, float vf_coef, float ent_coef,
                         float* d_outputs, double* sums5, float* out6, int64_t norm_rows, int32_t clear, int32_t finish, void* stream);

/* The reference's agent-to-module mapping fn (league_based_self_play_callback.py:1286-1344) for all markets at once, on the device: slot s < n_trainable -> net s;
 * every other slot draws np.random.RandomState((episode_crc[market] + s) mod 2^32).choice(pool, p = probs) - bit for bit: one freshly seeded MT19937's first
 * random_sample(), searchsorted(cumsum(probs) / cumsum(probs)[-1], u, side = "right") - and receives pool_net[draw] (a bank row or CDA_LEAGUE_RANDOM).
 * episode_crc u32 [N] = zlib.crc32(str(episode id)) (host), pool_cdf f64 [pool_size] the normalised cumulative weights, slot_pool (may be NULL) i32 [N][A]: the draw
 * itself (index into the pool; -1 for the trainable slots) - what names the module in an episode record. */
int cda_league_assign(const uint32_t* episode_crc, int32_t n_markets, int32_t num_agents, int32_t n_trainable, const double* pool_cdf, const int32_t* pool_net,
                      int32_t pool_size, int32_t* slot_net, int32_t* slot_pool, void* stream);
/* ... with scripted modules (include/cda.h cda_scripted_attach) in the pool: cda_league_assign's draw bit for bit - the same generator, the same searchsorted on the
 * (longer) cdf - and one more table and output: pool_script i32 [pool_size], 0 or 1 + the index of the profile a scripted pool entry plays (its pool_net entry is
 * CDA_LEAGUE_RANDOM: the scripted launch overwrites the random module's action), and slot_script i32 [N][A] <- pool_script[draw], 0 in the trainable slots and where
 * a network or the random module plays.  slot_script is the table the env was attached with (resident: rewritten in place per episode, no re-attach, captured rollout
 * graphs stay valid).  With an all-zero pool_script the other outputs equal cda_league_assign's. */
int cda_league_assign_scripted(const uint32_t* episode_crc, int32_t n_markets, int32_t num_agents, int32_t n_trainable, const double* pool_cdf, const int32_t* pool_net,
                               const int32_t* pool_script, int32_t pool_size, int32_t* slot_net, int32_t* slot_script, int32_t* slot_pool, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CDA_LEARNER_H */
