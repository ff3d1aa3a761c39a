/*
 * cda_imitate.h - C-ABI of behaviour cloning on the fused network: demonstrations packed into sample records, and the negative log-likelihood of those records
 * under the policy's Dict-action distribution (csrc/cda_learner.hip, next to the PPO loss kernels whose row body they share the pieces of).
 *
 * Like the entry points of cda_learner.h these exist ONCE in the library, under the names below: they see a network only through its 32-float output rows and
 * the sample records, so they carry no [_h<H>][_<act>][_vfs] suffix and serve every compiled network variant.  The loss kernel honours the contract of the two PPO
 * loss kernels - d_outputs f32 [rows][out_stride] and five f64 sums - so cda_mlp_backward, cda_mlp_wgrad and cda_mlp_adam (cda_mlp.h) train a network on it unchanged.
 *
 * Conventions as in cda.h: device pointers, caller-owned, plain sizes; CDA_OK or a negative cda_status; kernels are enqueued on `stream`.  No CPU fallback.
 */
#ifndef CDA_IMITATE_H
#define CDA_IMITATE_H

#include <stdint.h>
#include "cda_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

/* slot_src: where the demonstration of a (market, slot) comes from */
#define CDA_BC_SRC_NONE   0   /* the slot's samples do not count: weight 0 (the label and target words are still written, as for CDA_BC_SRC_ENV) */
#define CDA_BC_SRC_ENV    1   /* an env action (a scripted opponent's, a recorded run's): the Gaussian targets are the inverse of the policy's squash */
#define CDA_BC_SRC_POLICY 2   /* a policy sample: the raw Gaussian samples are copied from a_cont */
/* The env's Box actions are size_mean = tanh(x0), size_sigma = sigmoid(x1) of the raw Gaussian samples (ppo.to_env_actions).  The inverse is taken of the action
 * clamped to [-M, M] and [1 - M, M], M = 1 - 2^-10: a scripted pass (size_mean 0, size_sigma 0) and the Box bounds themselves have finite targets. */
#define CDA_BC_SQUASH_BOUND 0.9990234375f

/* Demonstrations -> sample records, one launch, one thread per (step, market, agent).  category, price, price_offset i32 and size_mean, size_sigma f32, all
 * [n_steps][n_markets][num_agents] (a rollout's action buffers: the scripted slots' actions are recorded there like the policy's); a_cont f32 [..][2] (may be NULL
 * when no slot is CDA_BC_SRC_POLICY: such a slot then falls back to the inverse squash); slot_src i32 and slot_weight f32 [n_markets][num_agents].
 * rec f32 [n_steps][n_markets][num_agents][8] (CDA_REC_*, 16-byte aligned): words CATEGORY, PRICE, OFFSET <- the three labels, CONT0, CONT1 <- the raw Gaussian
 * targets, word CDA_REC_LOGP <- the sample's WEIGHT (slot_weight, 0 where slot_src is CDA_BC_SRC_NONE or unknown); words ADV, RET are not written (a caller may have
 * run cda_gae_records into them).  stats2 f64[2] accumulates the sum of the written weights and the number of samples with weight > 0: the caller clears it. */
int cda_bc_records(const int32_t* category, const int32_t* price, const int32_t* price_offset, const float* size_mean, const float* size_sigma, const float* a_cont,
                   const int32_t* slot_src, const float* slot_weight, int32_t n_steps, int64_t n_markets, int32_t num_agents, float* rec, double* stats2, void* stream);

/* The behaviour-cloning loss of cda_bc_records' records, in cda_ppo_loss_records' position (outputs, log_std, rec, row_index, rows, agents_per_row, out_stride,
 * d_outputs, sums5, out6, norm_rows, clear, finish as there; rec 16-byte aligned).  With B = norm_rows * agents_per_row (rows * agents_per_row when norm_rows == 0),
 * k = loss_scale / B, a row's three softmax heads lp_*, means l[22], l[23], value l[24], the two log_std ls_i, and a sample's labels (c, p, o), targets x_i,
 * weight w (word CDA_REC_LOGP) and return ret (word CDA_REC_RET):
 *     z_i  = (x_i - l[22 + i]) * exp(-ls_i)
 *     logp = lp_cat[c] + lp_price[p] + lp_off[o] - z0^2 / 2 - ls0 - z1^2 / 2 - ls1 - log(2 pi)
 *     L    = k * sum of w * (-logp + vf_coef * (l[24] - ret)^2 - ent_coef * H)          H: the row's entropy, as the PPO loss kernels compute it
 * A label outside its head's range is clamped (below 0 -> 0, above the last -> the last), in logp and in the gradient alike.
 * d_outputs <- dL / d outputs (column 24 the value's; the columns behind it zeros).  sums5 words 3, 4 accumulate dL / d log_std (cda_mlp_adam applies them as they
 * are); words 0..2 accumulate loss_scale * sum of w * (-logp), w * (l[24] - ret)^2, w * H, which the finishing step - finish != 0 here, or cda_mlp_adam given
 * loss_samples = B - divides by B: out6[0] = k * sum of w * (-logp) is the NLL, out6[1], out6[2] the weighted value error and entropy, out6[3] = L.
 * loss_scale: a minibatch of shuffled rows holds a varying weight; the caller passes 1 / (expected weight per sample), so L is the mean over the counted samples in
 * expectation, without a second pass.
 * logp_out (may be NULL) f32 [rows][agents_per_row]: every sample's UNWEIGHTED logp, by destination row - the demonstration log-likelihood.
 * bc_stats (may be NULL) f64[8], accumulated, cleared by the caller: sum of w | sum of w * [argmax cat == c] | ... [argmax price == p] | ... [argmax off == o] (ties
 * to the lowest index) | sum of w * (x0 - l[22])^2 | sum of w * (x1 - l[23])^2 | number of samples with w > 0 | 0. */
int cda_bc_loss_records(const float* outputs, const float* log_std, const float* rec, const int64_t* row_index, int64_t rows, int32_t agents_per_row, int32_t out_stride,
                        float vf_coef, float ent_coef, float loss_scale, float* d_outputs, double* sums5, float* out6, int64_t norm_rows, int32_t clear, int32_t finish,
                        float* logp_out, double* bc_stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CDA_IMITATE_H */
