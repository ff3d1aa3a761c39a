// cda_learner.hip - the learner-side kernels that do not depend on the network's shape (include/cda_learner.h): the epoch's keyed permutation, the unfused PPO
// loss on int32 action arrays and on sample records, GAE straight into the records, the returns of completed episodes, the league's slot assignment; and behaviour
// cloning (include/cda_imitate.h): demonstrations packed into sample records and their negative log-likelihood, on the PPO loss's own head_probs / pick / RecordSamples.
// csrc/cda_mlp.hip is compiled once per (history depth, activation, vf_share_layers) with every entry point renamed (csrc/cda_mlp_variant.h); nothing here reads
// any of the three, so this file is compiled ONCE and its entry points keep their names for every variant.  Nothing in cda_mlp.hip calls into this file.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cda_learner.h"
#include "../../include/cda_imitate.h"

// The library is built with -ffp-contract=off (the env kernels' f64 sums must match CPython's).  These kernels came out of csrc/cda_mlp.hip, which switches
// contraction back on for itself, and they keep it: without the pragma the compiler splits their fused multiply-adds (the v_fma_f64 of the advantage variance in
// k_ppo_loss_rec, the f32 ones of the loss and of GAE) into a multiply and an add, which rounds differently - the numbers of every recorded run would move.
#pragma clang fp contract(fast)

namespace {
constexpr int N_CAT = CDA_HEAD_CATEGORY, N_PRICE = CDA_HEAD_PRICE, N_OFF = CDA_HEAD_OFFSET, N_LOGITS = CDA_HEAD_LOGITS;      // (csrc/cda_mlp_dev.inc's names)

// ---- update: the epoch's shuffle as a keyed bijection (no sort) -----------------------------------------------------------------------
// perm[i] = walk(i): a bijective mixer on [0, 2^bits) (add, odd multiply, xor-shift: each step invertible), iterated until the value falls
// below n (cycle walking: < 2 rounds on average, since 2^bits < 2 n).  torch.randperm is a device sort: ~10 launches, 130 us per epoch.
__device__ __forceinline__ unsigned int perm_mix(unsigned int x, int bits, unsigned long long key) {
    const unsigned int mask = bits >= 32 ? 0xffffffffu : ((1u << bits) - 1u);
    const int s1 = (bits + 1) / 2, s2 = (2 * bits + 2) / 3;
    #pragma unroll
    for (int r = 0; r < 4; r++) {
        x = (x + (unsigned int)(key >> (16 * r))) & mask;
        x = (x * 0x9E3779B1u) & mask;
        x ^= x >> s1;
        x = (x * 0x85EBCA6Bu) & mask;
        x ^= x >> s2;
    }
    return x;
}
__global__ void k_make_perm(unsigned long long key, long long n, int bits, long long* __restrict__ perm) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned int x = (unsigned int)i;
    do { x = perm_mix(x, bits, key); } while ((long long)x >= n);
    perm[i] = (long long)x;
}

// ---- the unfused loss for int32 actions (cda_ppo.hip's k_ppo_loss, same arithmetic): ONE row body, samples from the seven arrays or from the records -----------
template <int N>
__device__ __forceinline__ void head_probs(const float* l, float* p, float* lp, float& ent) {
    float mx = l[0];
    #pragma unroll
    for (int q = 1; q < N; q++) mx = fmaxf(mx, l[q]);
    float s = 0.0f;
    #pragma unroll
    for (int q = 0; q < N; q++) { p[q] = __expf(l[q] - mx); s += p[q]; }
    const float ls = __logf(s), inv = 1.0f / s;
    float hh = 0.0f;
    #pragma unroll
    for (int q = 0; q < N; q++) { p[q] *= inv; lp[q] = l[q] - mx - ls; hh -= p[q] * lp[q]; }
    ent = hh;
}
template <int N>
__device__ __forceinline__ float pick(const float* v, int a) {
    float r = v[0];
    #pragma unroll
    for (int q = 1; q < N; q++) r = (a == q || (q == N - 1 && a > q)) ? v[q] : r;
    return r;
}
// One sample as the loss reads it, and the two places a row's samples come from: a source is positioned on a row (seek) and yields sample a of it (get).
struct Sample { int cat, price, off; float cont0, cont1, logp_old, adv, ret; };
// ... the seven per-sample arrays (the env's own action tensors and the rollout's): seven scattered gathers per row
struct ArraySamples {
    const int* __restrict__ a_cat; const int* __restrict__ a_price; const int* __restrict__ a_off;
    const float* __restrict__ a_cont; const float* __restrict__ logp_old; const float* __restrict__ adv; const float* __restrict__ ret;
    long long first;
    __device__ __forceinline__ void seek(long long src_row, int agents) { first = src_row * agents; }
    __device__ __forceinline__ Sample get(int a) const {
        const long long i = first + a;
        return Sample{a_cat[i], a_price[i], a_off[i], a_cont[2 * i], a_cont[2 * i + 1], logp_old[i], adv[i], ret[i]};
    }
};
// ... the sample records: a row's A samples are ONE contiguous piece of A x 32 bytes (the seven arrays: 1.3 KB fetched per row for 128 B used); with adv_stats (the
// sums of the advantages and of their squares over n_stat samples) the advantages are normalised on the fly, (adv - mean) / (unbiased std + 1e-8)
struct RecordSamples {
    const float* __restrict__ rec;
    float adv_mean, adv_rstd;
    const float4* rp;
    __device__ __forceinline__ RecordSamples(const float* __restrict__ rec_, const double* __restrict__ adv_stats, long long n_stat) : rec(rec_), adv_mean(0.0f), adv_rstd(1.0f), rp(nullptr) {
        if (adv_stats) {
            const double m = adv_stats[0] / (double)n_stat, var = (adv_stats[1] - (double)n_stat * m * m) / (double)(n_stat - 1);
            adv_mean = (float)m; adv_rstd = 1.0f / ((float)sqrt(var > 0.0 ? var : 0.0) + 1e-8f);
        }
    }
    __device__ __forceinline__ void seek(long long src_row, int agents) { rp = reinterpret_cast<const float4*>(rec + src_row * agents * 8); }
    __device__ __forceinline__ Sample get(int a) const {
        const float4 w0 = rp[2 * a], w1 = rp[2 * a + 1];
        return Sample{__float_as_int(w0.x), __float_as_int(w0.y), __float_as_int(w0.z), w0.w, w1.x, w1.y, (w1.z - adv_mean) * adv_rstd, w1.w};
    }
};
// The loss of one output row per thread (256 rows per workgroup): the clipped surrogate, value and entropy terms of the row's `agents` samples, their gradient at the
// row's outputs -> d_out, and the workgroup's five sums (policy loss, squared value error, entropy, d loss / d log_std x 2) -> sums f64[5], one atomic each.
template <class Src>
__device__ __forceinline__ void ppo_loss_rows(Src src, const float* __restrict__ outputs, const float* __restrict__ log_std, const long long* __restrict__ row_index,
                                              long long R, long long Rnorm, int agents, int stride, float clip, float vf_coef, float ent_coef,
                                              float* __restrict__ d_out, double* __restrict__ sums) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const float invB = 1.0f / ((float)Rnorm * (float)agents);
    float pg = 0.0f, vl = 0.0f, en = 0.0f, dls0 = 0.0f, dls1 = 0.0f;
    if (r < R) {
        float l[N_LOGITS], d[N_LOGITS], p[N_CAT + N_PRICE + N_OFF], lp[N_CAT + N_PRICE + N_OFF];
        const float4* lp4 = reinterpret_cast<const float4*>(outputs + r * stride);
        #pragma unroll
        for (int q = 0; q < N_LOGITS / 4; q++) { const float4 v = lp4[q]; l[4 * q] = v.x; l[4 * q + 1] = v.y; l[4 * q + 2] = v.z; l[4 * q + 3] = v.w; }
        const float ls0 = log_std[0], ls1 = log_std[1];
        const float is0 = __expf(-ls0), is1 = __expf(-ls1);
        const float HALF_LOG_2PI = 0.918938533204672742f;
        float h0, h1, h2;
        head_probs<N_CAT>(l, p, lp, h0);
        head_probs<N_PRICE>(l + N_CAT, p + N_CAT, lp + N_CAT, h1);
        head_probs<N_OFF>(l + N_CAT + N_PRICE, p + N_CAT + N_PRICE, lp + N_CAT + N_PRICE, h2);
        const float ent = h0 + h1 + h2 + 1.0f + 2.0f * HALF_LOG_2PI + ls0 + ls1;
        const float es = ent_coef * invB;
        #pragma unroll
        for (int q = 0; q < N_LOGITS; q++) d[q] = 0.0f;
        const float val = outputs[r * stride + N_LOGITS];
        float G = 0.0f, dval = 0.0f;
        src.seek(row_index ? row_index[r] : r, agents);
        for (int a = 0; a < agents; a++) {
            const Sample s = src.get(a);
            const int ac = s.cat, ap = s.price, ao = s.off;
            const float z0 = (s.cont0 - l[22]) * is0, z1 = (s.cont1 - l[23]) * is1;
            const float logp = -0.5f * z0 * z0 - ls0 - HALF_LOG_2PI - 0.5f * z1 * z1 - ls1 - HALF_LOG_2PI +
                               pick<N_CAT>(lp, ac) + pick<N_PRICE>(lp + N_CAT, ap) + pick<N_OFF>(lp + N_CAT + N_PRICE, ao);
            const float Av = s.adv, ratio = __expf(logp - s.logp_old);
            const float un = ratio * Av, cl = fminf(fmaxf(ratio, 1.0f - clip), 1.0f + clip) * Av;
            pg -= fminf(un, cl);
            const float g_logp = (un <= cl) ? -un * invB : 0.0f;
            const float dv = val - s.ret;
            vl += dv * dv;
            dval += 2.0f * vf_coef * dv * invB;
            en += ent;
            G += g_logp;
            #pragma unroll
            for (int q = 0; q < N_CAT; q++) d[q] += (q == ac) ? g_logp : 0.0f;
            #pragma unroll
            for (int q = 0; q < N_PRICE; q++) d[N_CAT + q] += (q == ap) ? g_logp : 0.0f;
            #pragma unroll
            for (int q = 0; q < N_OFF; q++) d[N_CAT + N_PRICE + q] += (q == ao) ? g_logp : 0.0f;
            d[22] += g_logp * z0 * is0;
            d[23] += g_logp * z1 * is1;
            dls0 += g_logp * (z0 * z0 - 1.0f) - es;
            dls1 += g_logp * (z1 * z1 - 1.0f) - es;
        }
        const float esA = es * (float)agents;
        #pragma unroll
        for (int q = 0; q < N_CAT; q++) d[q] += -G * p[q] + esA * p[q] * (lp[q] + h0);
        #pragma unroll
        for (int q = 0; q < N_PRICE; q++) d[N_CAT + q] += -G * p[N_CAT + q] + esA * p[N_CAT + q] * (lp[N_CAT + q] + h1);
        #pragma unroll
        for (int q = 0; q < N_OFF; q++) d[N_CAT + N_PRICE + q] += -G * p[N_CAT + N_PRICE + q] + esA * p[N_CAT + N_PRICE + q] * (lp[N_CAT + N_PRICE + q] + h2);
        float4* dp4 = reinterpret_cast<float4*>(d_out + r * stride);
        #pragma unroll
        for (int q = 0; q < N_LOGITS / 4; q++) dp4[q] = make_float4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
        dp4[N_LOGITS / 4] = make_float4(dval, 0.0f, 0.0f, 0.0f);
        for (int q = N_LOGITS / 4 + 1; q < stride / 4; q++) dp4[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    float v5[5] = {pg, vl, en, dls0, dls1};
    __shared__ float part[5][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    #pragma unroll
    for (int q = 0; q < 5; q++) {
        float x = v5[q];
        #pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if (lane == 0) part[q][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const double t = (double)part[threadIdx.x][0] + (double)part[threadIdx.x][1] + (double)part[threadIdx.x][2] + (double)part[threadIdx.x][3];
        atomicAdd(&sums[threadIdx.x], t);
    }
}
__global__ __launch_bounds__(256) void k_ppo_loss32(const float* __restrict__ outputs, const float* __restrict__ log_std,
                                                    const int* __restrict__ a_cat, const int* __restrict__ a_price, const int* __restrict__ a_off,
                                                    const float* __restrict__ a_cont, const float* __restrict__ logp_old, const float* __restrict__ adv,
                                                    const float* __restrict__ ret, const long long* __restrict__ row_index, long long R, long long Rnorm, int agents,
                                                    int stride, float clip, float vf_coef, float ent_coef, float* __restrict__ d_out, double* __restrict__ sums) {
    ppo_loss_rows(ArraySamples{a_cat, a_price, a_off, a_cont, logp_old, adv, ret, 0}, outputs, log_std, row_index, R, Rnorm, agents, stride, clip, vf_coef, ent_coef, d_out, sums);
}
__global__ __launch_bounds__(256) void k_ppo_loss_rec(const float* __restrict__ outputs, const float* __restrict__ log_std, const float* __restrict__ rec,
                                                      const double* __restrict__ adv_stats, long long n_stat, const long long* __restrict__ row_index,
                                                      long long R, long long Rnorm, int agents, int stride, float clip, float vf_coef, float ent_coef,
                                                      float* __restrict__ d_out, double* __restrict__ sums) {
    ppo_loss_rows(RecordSamples(rec, adv_stats, n_stat), outputs, log_std, row_index, R, Rnorm, agents, stride, clip, vf_coef, ent_coef, d_out, sums);
}
__global__ void k_ppo_finish32(const double* sums, long long B, float vf_coef, float ent_coef, float* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const double pg = sums[0] / (double)B, vl = sums[1] / (double)B, en = sums[2] / (double)B;
        out[0] = (float)pg; out[1] = (float)vl; out[2] = (float)en; out[3] = (float)(pg + (double)vf_coef * vl - (double)ent_coef * en);
        out[4] = (float)sums[3]; out[5] = (float)sums[4];
    }
}

// ---- the rollout's sample records: GAE straight into them, and the loss reading them -----------------------------------------------------
// One thread per (market, agent) column walks its T steps backwards (ppo.gae's recursion) on the rollout's own buffers - reward f64 [T][N][A]
// (scaled here), value f32 [T + 1][N] (slot T = the bootstrap value), terminated / truncated u8 [T][N] - and writes advantage and return into
// words 6, 7 of the step's sample record.  The sums of the advantages and of their squares go to stats f64[2] (cleared by the caller): the
// update normalises on the fly, (adv - mean) / (std + 1e-8) with the unbiased std, as ppo_update does with torch ops.
// n_train > 0 (league self-play): slot p < n_train is played by trainable net p, whose values are value[p][T + 1][N] and whose sums go to stats[2 p ..];
// the other slots' samples feed no update and are skipped.
__global__ __launch_bounds__(256) void k_gae_records(const double* __restrict__ reward, const float* __restrict__ value, const unsigned char* __restrict__ term,
                                                     const unsigned char* __restrict__ trunc, int T, long long N, int Ag, int n_train, float reward_scale, float gamma, float lam,
                                                     const int* __restrict__ fin_index, const float* __restrict__ fin_value, long long fin_value_stride,
                                                     float* __restrict__ rec, double* __restrict__ stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x, B = N * Ag;
    double s1 = 0.0, s2 = 0.0;
    const int slot = (int)(i % Ag);
    if (i < B && (n_train <= 0 || slot < n_train)) {
        const long long n = i / Ag;
        if (n_train > 0) { value += (long long)slot * (T + 1) * N; fin_value += (long long)slot * fin_value_stride; }
        float nxt = value[(long long)T * N + n], run = 0.0f;
        // eight steps' operands requested together, then the recursion over them (one step at a time, every iteration paid a memory round trip:
        // 39 us for 64 steps)
        for (int t0 = T - 1; t0 >= 0; t0 -= 8) {
            float rw[8], vv[8], nd[8], bv[8];
            #pragma unroll
            for (int u = 0; u < 8; u++) {
                const int t = t0 - u >= 0 ? t0 - u : 0;
                const long long k = (long long)t * B + i, kn = (long long)t * N + n;
                const bool tm = term[kn] != 0, tr = trunc[kn] != 0;
                rw[u] = (float)reward[k] * reward_scale; vv[u] = value[kn]; nd[u] = (tm | tr) ? 0.0f : 1.0f;
                // a time-limit truncation (not a termination) whose last observation was captured: the step bootstraps with V(that observation) - the value
                // of the state the episode was cut in - instead of 0; nothing propagates across the episode boundary either way (nd = 0)
                bv[u] = 0.0f;
                if (fin_index && tr && !tm) { const int fi = fin_index[kn]; if (fi >= 0) bv[u] = fin_value[fi]; }
            }
            #pragma unroll
            for (int u = 0; u < 8; u++) {
                const int t = t0 - u;
                if (t >= 0) {
                    const long long k = (long long)t * B + i;
                    const float delta = rw[u] + gamma * (nxt * nd[u] + bv[u]) - vv[u];
                    run = delta + gamma * lam * nd[u] * run;
                    *reinterpret_cast<float2*>(rec + 8 * k + 6) = make_float2(run, run + vv[u]);
                    s1 += (double)run; s2 += (double)run * (double)run;
                    nxt = vv[u];
                }
            }
        }
    }
    if (n_train > 0) {                                                          // per net: a wave reduction and two atomics per (wave, net)
        for (int p = 0; p < n_train; p++) {
            double a1 = slot == p ? s1 : 0.0, a2 = slot == p ? s2 : 0.0;
            #pragma unroll
            for (int o = 32; o > 0; o >>= 1) { a1 += __shfl_down(a1, o, 64); a2 += __shfl_down(a2, o, 64); }
            if ((threadIdx.x & 63) == 0) { atomicAdd(&stats[2 * p], a1); atomicAdd(&stats[2 * p + 1], a2); }
        }
        return;
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_down(s1, o, 64); s2 += __shfl_down(s2, o, 64); }
    __shared__ double part[2][4];
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = s1; part[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x < 2) atomicAdd(&stats[threadIdx.x], (part[threadIdx.x][0] + part[threadIdx.x][1]) + (part[threadIdx.x][2] + part[threadIdx.x][3]));
}
// k_gae_records' recursion for ONE shared policy that plays slots 0 .. n_slots - 1 of every market only (the other slots are scripted opponents: their records are
// no policy samples).  One thread per (market, slot < n_slots): the same operands in the same order as k_gae_records' n_train == 0 thread of that column, so words 6, 7
// are bit-equal to what it writes there; the other slots' records are not touched and stats f64[2] (cleared by the caller) sums the T * N * n_slots trained samples.
// A kernel of its own: k_gae_records stays the code object it was.
__global__ __launch_bounds__(256) void k_gae_records_slots(const double* __restrict__ reward, const float* __restrict__ value, const unsigned char* __restrict__ term,
                                                           const unsigned char* __restrict__ trunc, int T, long long N, int Ag, int n_slots, float reward_scale, float gamma, float lam,
                                                           const int* __restrict__ fin_index, const float* __restrict__ fin_value, float* __restrict__ rec, double* __restrict__ stats) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x, B = N * Ag;
    double s1 = 0.0, s2 = 0.0;
    if (j < N * n_slots) {
        const long long n = j / n_slots;
        const long long i = n * Ag + (j - n * n_slots);                         // the column of rec / reward: (market n, slot j mod n_slots)
        float nxt = value[(long long)T * N + n], run = 0.0f;
        for (int t0 = T - 1; t0 >= 0; t0 -= 8) {                                // eight steps' operands requested together (k_gae_records)
            float rw[8], vv[8], nd[8], bv[8];
            #pragma unroll
            for (int u = 0; u < 8; u++) {
                const int t = t0 - u >= 0 ? t0 - u : 0;
                const long long k = (long long)t * B + i, kn = (long long)t * N + n;
                const bool tm = term[kn] != 0, tr = trunc[kn] != 0;
                rw[u] = (float)reward[k] * reward_scale; vv[u] = value[kn]; nd[u] = (tm | tr) ? 0.0f : 1.0f;
                bv[u] = 0.0f;
                if (fin_index && tr && !tm) { const int fi = fin_index[kn]; if (fi >= 0) bv[u] = fin_value[fi]; }
            }
            #pragma unroll
            for (int u = 0; u < 8; u++) {
                const int t = t0 - u;
                if (t >= 0) {
                    const long long k = (long long)t * B + i;
                    const float delta = rw[u] + gamma * (nxt * nd[u] + bv[u]) - vv[u];
                    run = delta + gamma * lam * nd[u] * run;
                    *reinterpret_cast<float2*>(rec + 8 * k + 6) = make_float2(run, run + vv[u]);
                    s1 += (double)run; s2 += (double)run * (double)run;
                    nxt = vv[u];
                }
            }
        }
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_down(s1, o, 64); s2 += __shfl_down(s2, o, 64); }
    __shared__ double part[2][4];
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = s1; part[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x < 2) atomicAdd(&stats[threadIdx.x], (part[threadIdx.x][0] + part[threadIdx.x][1]) + (part[threadIdx.x][2] + part[threadIdx.x][3]));
}
// Returns of COMPLETED episodes from a rollout's buffers: running f64 [N][A] carries every (market, agent)'s return so far across rollouts; a step that ends
// the market's episode adds the agent's total to done_sum f64 [A] (and 1 to done_count f64 [A]) and restarts it.  One thread per (market, agent), forwards in time.
__global__ __launch_bounds__(256) void k_episode_returns(const double* __restrict__ reward, const unsigned char* __restrict__ term, const unsigned char* __restrict__ trunc,
                                                         int T, long long N, int Ag, double* __restrict__ running, double* __restrict__ done_sum, double* __restrict__ done_count,
                                                         double* __restrict__ per_slot) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x, B = N * Ag;
    if (i >= B) return;
    const long long n = i / Ag; const int a = (int)(i - n * Ag);
    double run = running[i], s = 0.0, c = 0.0;
    for (int t0 = 0; t0 < T; t0 += 8) {                                         // eight steps' operands requested together (one step at a time: a round trip per step, 72 us for 64)
        double rw[8]; bool dn[8];
        #pragma unroll
        for (int u = 0; u < 8; u++) {
            const int t = t0 + u < T ? t0 + u : T - 1;
            rw[u] = reward[(long long)t * B + i]; dn[u] = (term[(long long)t * N + n] | trunc[(long long)t * N + n]) != 0;
        }
        #pragma unroll
        for (int u = 0; u < 8; u++)
            if (t0 + u < T) { run += rw[u]; if (dn[u]) { s += run; c += 1.0; run = 0.0; } }
    }
    running[i] = run;
    if (c > 0.0) { atomicAdd(&done_sum[a], s); atomicAdd(&done_count[a], c); }
    if (per_slot) { per_slot[2 * i] = s; per_slot[2 * i + 1] = c; }              // this rollout's completed episodes of (market, agent): sum of returns, number
}
}  // namespace

extern "C" int cda_mlp_permutation(uint64_t key, int64_t n, int64_t* perm, void* stream) {
    if (!perm || n < 1 || n > ((int64_t)1 << 31)) return CDA_ERR_INVALID;
    int bits = 1;
    while (((int64_t)1 << bits) < n) bits++;
    hipLaunchKernelGGL(k_make_perm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned long long)key, (long long)n, bits, (long long*)perm);
    return hipGetLastError() == hipSuccess ? CDA_OK : CDA_ERR_HIP;
}

extern "C" int cda_ppo_loss32(const float* outputs, const float* log_std, const int32_t* a_cat, const int32_t* a_price, const int32_t* a_off,
                              const float* a_cont, const float* logp_old, const float* adv, const float* ret, const int64_t* row_index,
                              int64_t rows, int32_t agents_per_row, int32_t out_stride, float clip, float vf_coef, float ent_coef,
                              float* d_outputs, double* sums5, float* out6, int64_t norm_rows, int32_t clear, int32_t finish, void* stream) {
    if (!outputs || !log_std || !a_cat || !a_price || !a_off || !a_cont || !logp_old || !adv || !ret || !d_outputs || !sums5 || !out6 || rows < 1 ||
        agents_per_row < 1 || agents_per_row > CDA_MAX_AGENTS || out_stride <= N_LOGITS || (out_stride & 3) || norm_rows < 0) return CDA_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const long long rn = norm_rows > 0 ? norm_rows : rows;
    if (clear && hipMemsetAsync(sums5, 0, 5 * sizeof(double), st) != hipSuccess) return CDA_ERR_HIP;
    hipLaunchKernelGGL(k_ppo_loss32, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, outputs, log_std, a_cat, a_price, a_off, a_cont, logp_old, adv, ret,
                       (const long long*)row_index, (long long)rows, rn, (int)agents_per_row, (int)out_stride, clip, vf_coef, ent_coef, d_outputs, sums5);
    if (finish) hipLaunchKernelGGL(k_ppo_finish32, dim3(1), dim3(64), 0, st, (const double*)sums5, rn * agents_per_row, vf_coef, ent_coef, out6);
    return hipGetLastError() == hipSuccess ? CDA_OK : CDA_ERR_HIP;
}

static int gae_records(const double* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int64_t n_markets,
                       int32_t num_agents, int32_t n_train, float reward_scale, float gamma, float lam, float* rec, double* stats, void* stream,
                       const int32_t* fin_index = NULL, const float* fin_value = NULL, int64_t fin_value_stride = 0) {
    if (!reward || !value || !terminated || !truncated || !rec || !stats || n_steps < 1 || n_markets < 1 || num_agents < 1 || num_agents > CDA_MAX_AGENTS ||
        n_train < 0 || n_train > num_agents || (fin_index && !fin_value)) return CDA_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, 2 * sizeof(double) * (n_train > 0 ? n_train : 1), st) != hipSuccess) return CDA_ERR_HIP;
    const long long B = (long long)n_markets * num_agents;
    hipLaunchKernelGGL(k_gae_records, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, reward, value, (const unsigned char*)terminated, (const unsigned char*)truncated,
                       (int)n_steps, (long long)n_markets, (int)num_agents, (int)n_train, reward_scale, gamma, lam, (const int*)fin_index, fin_value, (long long)fin_value_stride, rec, stats);
    return hipGetLastError() == hipSuccess ? CDA_OK : CDA_ERR_HIP;
}
extern "C" int cda_gae_records(const double* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int64_t n_markets,
                               int32_t num_agents, float reward_scale, float gamma, float lam, float* rec, double* stats2, void* stream) {
    return gae_records(reward, value, terminated, truncated, n_steps, n_markets, num_agents, 0, reward_scale, gamma, lam, rec, stats2, stream);
}
// ... with the time-limit bootstrap: fin_index i32 [T][N] (slot of the step's captured last observation, -1 = none), fin_value f32 [max(n_trainable, 1)][fin_value_stride]
// (cda_mlp_values on the captured list).  n_trainable = 0: one shared policy (cda_gae_records' layout), > 0: the league's (cda_gae_records_league's).
extern "C" int cda_gae_records_bootstrap(const double* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int64_t n_markets,
                                         int32_t num_agents, int32_t n_trainable, float reward_scale, float gamma, float lam,
                                         const int32_t* fin_index, const float* fin_value, int64_t fin_value_stride, float* rec, double* stats, void* stream) {
    return gae_records(reward, value, terminated, truncated, n_steps, n_markets, num_agents, n_trainable, reward_scale, gamma, lam, rec, stats, stream, fin_index, fin_value, fin_value_stride);
}
// ... for one shared policy on slots 0 .. n_slots - 1 of every market (the other slots: scripted opponents): cda_gae_records_bootstrap(n_trainable = 0)'s recursion over
// those slots only (k_gae_records_slots); fin_index / fin_value may be NULL (no time-limit bootstrap), fin_value is the shared policy's one row.
extern "C" int cda_gae_records_slots(const double* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int64_t n_markets,
                                     int32_t num_agents, int32_t n_slots, float reward_scale, float gamma, float lam,
                                     const int32_t* fin_index, const float* fin_value, float* rec, double* stats2, void* stream) {
    if (!reward || !value || !terminated || !truncated || !rec || !stats2 || n_steps < 1 || n_markets < 1 || num_agents < 1 || num_agents > CDA_MAX_AGENTS ||
        n_slots < 1 || n_slots > num_agents || (fin_index && !fin_value) || ((uintptr_t)rec & 7) != 0) return CDA_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(stats2, 0, 2 * sizeof(double), st) != hipSuccess) return CDA_ERR_HIP;
    const long long B = (long long)n_markets * n_slots;
    hipLaunchKernelGGL(k_gae_records_slots, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, reward, value, (const unsigned char*)terminated, (const unsigned char*)truncated,
                       (int)n_steps, (long long)n_markets, (int)num_agents, (int)n_slots, reward_scale, gamma, lam, (const int*)fin_index, fin_value, rec, stats2);
    return hipGetLastError() == hipSuccess ? CDA_OK : CDA_ERR_HIP;
}
extern "C" int cda_gae_records_league(const double* reward,const float* value, const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int64_t n_markets,
                                      int32_t num_agents, int32_t n_trainable, float reward_scale, float gamma, float lam, float* rec, double* stats2k, void* stream) {
    if (n_trainable < 1) return CDA_ERR_INVALID;
    return gae_records(reward, value, terminated, truncated, n_steps, n_markets, num_agents, n_trainable, reward_scale, gamma, lam, rec, stats2k, stream);
}

extern "C" int cda_episode_returns(const double* reward, const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int64_t n_markets, int32_t num_agents,
                                   double* running, double* done_sum, double* done_count, double* per_slot, void* stream) {
    if (!reward || !terminated || !truncated || !running || !done_sum || !done_count || n_steps < 1 || n_markets < 1 || num_agents < 1 || num_agents > CDA_MAX_AGENTS) return CDA_ERR_INVALID;
    const long long B = (long long)n_markets * num_agents;
    hipLaunchKernelGGL(k_episode_returns, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, reward, (const unsigned char*)terminated, (const unsigned char*)truncated,
                       (int)n_steps, (long long)n_markets, (int)num_agents, running, done_sum, done_count, per_slot);
    return hipGetLastError() == hipSuccess ? CDA_OK : CDA_ERR_HIP;
}

extern "C" int cda_ppo_loss_records(const float* outputs, const float* log_std, const float* rec, const double* adv_stats2, int64_t adv_count, const int64_t* row_index,
                                    int64_t rows, int32_t agents_per_row, int32_t out_stride, float clip, float vf_coef, float ent_coef,
                                    float* d_outputs, double* sums5, float* out6, int64_t norm_rows, int32_t clear, int32_t finish, void* stream) {
    if (!outputs || !log_std || !rec || !d_outputs || !sums5 || !out6 || rows < 1 || agents_per_row < 1 || agents_per_row > CDA_MAX_AGENTS ||
        out_stride <= N_LOGITS || (out_stride & 3) || norm_rows < 0 || (adv_stats2 && adv_count < 2)) return CDA_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const long long rn = norm_rows > 0 ? norm_rows : rows;
    if (clear && hipMemsetAsync(sums5, 0, 5 * sizeof(double), st) != hipSuccess) return CDA_ERR_HIP;
    hipLaunchKernelGGL(k_ppo_loss_rec, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, outputs, log_std, rec, adv_stats2, (long long)adv_count,
                       (const long long*)row_index, (long long)rows, rn, (int)agents_per_row, (int)out_stride, clip, vf_coef, ent_coef, d_outputs, sums5);
    if (finish) hipLaunchKernelGGL(k_ppo_finish32, dim3(1), dim3(64), 0, st, (const double*)sums5, rn * agents_per_row, vf_coef, ent_coef, out6);
    return hipGetLastError() == hipSuccess ? CDA_OK : CDA_ERR_HIP;
}

// The reference's agent-to-module mapping (train/callbk/league_based_self_play_callback.py:1286-1344) for every (market, pool slot) at once: slot s >= n_trainable
// of a market draws np.random.RandomState((crc32(str(episode id)) + s) mod 2^32).choice(pool, p) - ONE random_sample() of a freshly seeded MT19937: the
// init_genrand recurrence up to word 398, the twist + tempering of outputs 0 and 1, a 53-bit double, searchsorted(cdf, u, side = "right").  A thread per
// (market, slot): 400 dependent integer steps (the host-side numpy restatement, league.mt19937_first_double, walks the same recurrence over all seeds at
// once: tens of milliseconds at 2048 x 6 - longer than the episode it assigns).
namespace { __global__ __launch_bounds__(256) void k_league_assign(const unsigned int* __restrict__ episode_crc, int N, int Ag, int n_train, const double* __restrict__ cdf,
                                                       const int* __restrict__ pool_net, int P, int* __restrict__ slot_net, int* __restrict__ slot_pool) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= N * Ag) return;
    const int n = i / Ag, s = i - n * Ag;
    if (s < n_train) { slot_net[i] = s; if (slot_pool) slot_pool[i] = -1; return; }
    unsigned int x = episode_crc[n] + (unsigned int)s;                          // (crc + slot) mod 2^32
    unsigned int m0 = x, m1 = 0, m2 = 0, m397 = 0, m398 = 0;
    for (unsigned int k = 1; k <= 398; k++) {
        x = 1812433253u * (x ^ (x >> 30)) + k;
        if (k == 1) m1 = x; else if (k == 2) m2 = x; else if (k == 397) m397 = x; else if (k == 398) m398 = x;
    }
    auto word = [](unsigned int a, unsigned int b, unsigned int c) {             // output k: twist of (mt[k], mt[k + 1], mt[k + 397]), tempered
        const unsigned int y = (a & 0x80000000u) | (b & 0x7fffffffu);
        unsigned int v = c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        v ^= v >> 11; v ^= (v << 7) & 0x9d2c5680u; v ^= (v << 15) & 0xefc60000u; v ^= v >> 18;
        return v;
    };
    const unsigned int w0 = word(m0, m1, m397) >> 5, w1 = word(m1, m2, m398) >> 6;
    const double u = ((double)w0 * 67108864.0 + (double)w1) / 9007199254740992.0;
    int idx = 0;
    for (int q = 0; q < P; q++) idx += cdf[q] <= u ? 1 : 0;                      // searchsorted(..., side = "right")
    if (idx >= P) idx = P - 1;
    slot_net[i] = pool_net[idx];
    if (slot_pool) slot_pool[i] = idx;
} }
extern "C" int cda_league_assign(const uint32_t* episode_crc, int32_t n_markets, int32_t num_agents, int32_t n_trainable, const double* pool_cdf, const int32_t* pool_net,
                                 int32_t pool_size, int32_t* slot_net, int32_t* slot_pool, void* stream) {
    if (!episode_crc || !pool_cdf || !pool_net || !slot_net || n_markets < 1 || num_agents < 1 || num_agents > CDA_MAX_AGENTS || n_trainable < 0 || n_trainable > num_agents ||
        pool_size < 1) return CDA_ERR_INVALID;
    const int n = n_markets * num_agents;
    hipLaunchKernelGGL(k_league_assign, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned int*)episode_crc, (int)n_markets, (int)num_agents,
                       (int)n_trainable, pool_cdf, (const int*)pool_net, (int)pool_size, (int*)slot_net, (int*)slot_pool);
    return hipGetLastError() == hipSuccess ? CDA_OK : CDA_ERR_HIP;
}

// k_league_assign with scripted modules in the pool: the same draw, bit for bit (the same freshly seeded MT19937's first double, the same searchsorted on the - longer -
// cdf), and one more table, pool_script i32 [P]: 0, or 1 + the profile a scripted pool entry plays.  slot_script i32 [N][A] (the env's resident table: k_script_actions
// reads it at the next step) receives pool_script[draw], 0 in the trainable slots; a scripted entry's pool_net is CDA_LEAGUE_RANDOM (validated by the launcher's caller:
// the random module's action is what the scripted launch overwrites).  A kernel of its own: k_league_assign stays the code object it was.
namespace { __global__ __launch_bounds__(256) void k_league_assign_scripted(const unsigned int* __restrict__ episode_crc, int N, int Ag, int n_train, const double* __restrict__ cdf,
                                                                const int* __restrict__ pool_net, const int* __restrict__ pool_script, int P, int* __restrict__ slot_net,
                                                                int* __restrict__ slot_script, int* __restrict__ slot_pool) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= N * Ag) return;
    const int n = i / Ag, s = i - n * Ag;
    if (s < n_train) { slot_net[i] = s; slot_script[i] = 0; if (slot_pool) slot_pool[i] = -1; return; }
    unsigned int x = episode_crc[n] + (unsigned int)s;                          // (crc + slot) mod 2^32
    unsigned int m0 = x, m1 = 0, m2 = 0, m397 = 0, m398 = 0;
    for (unsigned int k = 1; k <= 398; k++) {
        x = 1812433253u * (x ^ (x >> 30)) + k;
        if (k == 1) m1 = x; else if (k == 2) m2 = x; else if (k == 397) m397 = x; else if (k == 398) m398 = x;
    }
    auto word = [](unsigned int a, unsigned int b, unsigned int c) {             // output k: twist of (mt[k], mt[k + 1], mt[k + 397]), tempered
        const unsigned int y = (a & 0x80000000u) | (b & 0x7fffffffu);
        unsigned int v = c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        v ^= v >> 11; v ^= (v << 7) & 0x9d2c5680u; v ^= (v << 15) & 0xefc60000u; v ^= v >> 18;
        return v;
    };
    const unsigned int w0 = word(m0, m1, m397) >> 5, w1 = word(m1, m2, m398) >> 6;
    const double u = ((double)w0 * 67108864.0 + (double)w1) / 9007199254740992.0;
    int idx = 0;
    for (int q = 0; q < P; q++) idx += cdf[q] <= u ? 1 : 0;                      // searchsorted(..., side = "right")
    if (idx >= P) idx = P - 1;
    slot_net[i] = pool_net[idx];
    slot_script[i] = pool_script[idx];
    if (slot_pool) slot_pool[i] = idx;
} }
extern "C" int cda_league_assign_scripted(const uint32_t* episode_crc, int32_t n_markets, int32_t num_agents, int32_t n_trainable, const double* pool_cdf, const int32_t* pool_net,
                                          const int32_t* pool_script, int32_t pool_size, int32_t* slot_net, int32_t* slot_script, int32_t* slot_pool, void* stream) {
    if (!episode_crc || !pool_cdf || !pool_net || !pool_script || !slot_net || !slot_script || n_markets < 1 || num_agents < 1 || num_agents > CDA_MAX_AGENTS ||
        n_trainable < 0 || n_trainable > num_agents || pool_size < 1) return CDA_ERR_INVALID;
    const int n = n_markets * num_agents;
    hipLaunchKernelGGL(k_league_assign_scripted, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned int*)episode_crc, (int)n_markets,
                       (int)num_agents, (int)n_trainable, pool_cdf, (const int*)pool_net, (const int*)pool_script, (int)pool_size, (int*)slot_net, (int*)slot_script, (int*)slot_pool);
    return hipGetLastError() == hipSuccess ? CDA_OK : CDA_ERR_HIP;
}

// ---- behaviour cloning (include/cda_imitate.h): demonstrations -> sample records, and their negative log-likelihood in the PPO loss's position ---------------------
namespace {
// One thread per (step, market, agent): the five env action words of the sample -> words 0..5 of its record, as two vector stores (k_script_actions' shape: a 16-byte
// half, then the 8 bytes in front of ADV | RET, which stay what they were).  The Gaussian targets of an env action invert ppo.to_env_actions' squash on the action
// clamped to the bound; a policy sample's are copied.  Word LOGP carries the weight.  stats f64[2] += (sum of the weights, samples with weight > 0).
__global__ __launch_bounds__(256) void k_bc_records(const int* __restrict__ cat, const int* __restrict__ price, const int* __restrict__ off, const float* __restrict__ size_mean,
                                                    const float* __restrict__ size_sigma, const float* __restrict__ a_cont, const int* __restrict__ slot_src,
                                                    const float* __restrict__ slot_weight, long long total, long long NA, float* __restrict__ rec, double* __restrict__ stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float w = 0.0f;
    if (i < total) {
        const long long col = i % NA;
        const int src = slot_src[col];
        w = (src == CDA_BC_SRC_ENV || src == CDA_BC_SRC_POLICY) ? slot_weight[col] : 0.0f;
        float x0, x1;
        if (src == CDA_BC_SRC_POLICY && a_cont) {
            const float2 x = *reinterpret_cast<const float2*>(a_cont + 2 * i);
            x0 = x.x; x1 = x.y;
        } else {
            const float M = CDA_BC_SQUASH_BOUND;
            const float m = fminf(fmaxf(size_mean[i], -M), M), s = fminf(fmaxf(size_sigma[i], 1.0f - M), M);
            x0 = atanhf(m);
            x1 = logf(s / (1.0f - s));
        }
        *reinterpret_cast<float4*>(rec + 8 * i) = make_float4(__int_as_float(cat[i]), __int_as_float(price[i]), __int_as_float(off[i]), x0);
        *reinterpret_cast<float2*>(rec + 8 * i + 4) = make_float2(x1, w);
    }
    double s1 = (double)w, s2 = w > 0.0f ? 1.0 : 0.0;
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_down(s1, o, 64); s2 += __shfl_down(s2, o, 64); }
    __shared__ double part[2][4];
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = s1; part[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x < 2) atomicAdd(&stats[threadIdx.x], (part[threadIdx.x][0] + part[threadIdx.x][1]) + (part[threadIdx.x][2] + part[threadIdx.x][3]));
}

template <int N>
__device__ __forceinline__ int clamp_label(int a) { return a < 0 ? 0 : (a > N - 1 ? N - 1 : a); }      // what pick<N> reads for label a
template <int N>
__device__ __forceinline__ int argmax_low(const float* v) {                                             // ties to the lowest index
    int b = 0;
    #pragma unroll
    for (int q = 1; q < N; q++) b = v[q] > v[b] ? q : b;
    return b;
}
// ppo_loss_rows' shape - one output row per thread, 256 rows per workgroup, the row's samples out of the records, wave shuffle + an LDS partial per wave + one f64
// atomic per word and workgroup - with the weighted negative log-likelihood in the surrogate's place: dL / dlogp of a sample is -k w whatever the policy thinks of it.
// A sample's word LOGP is its weight (RecordSamples hands it out as logp_old), word RET its return; word ADV is not read.
__global__ __launch_bounds__(256) void k_bc_loss_rec(const float* __restrict__ outputs, const float* __restrict__ log_std, const float* __restrict__ rec,
                                                     const long long* __restrict__ row_index, long long R, long long Rnorm, int agents, int stride, float vf_coef, float ent_coef,
                                                     float loss_scale, float* __restrict__ d_out, double* __restrict__ sums, float* __restrict__ logp_out, double* __restrict__ bc_stats) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const float invB = 1.0f / ((float)Rnorm * (float)agents);
    const float k = loss_scale * invB;
    float nl = 0.0f, vl = 0.0f, en = 0.0f, dls0 = 0.0f, dls1 = 0.0f;
    float bs[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (r < R) {
        RecordSamples src(rec, nullptr, 0);
        float l[N_LOGITS], d[N_LOGITS], p[N_CAT + N_PRICE + N_OFF], lp[N_CAT + N_PRICE + N_OFF];
        const float4* lp4 = reinterpret_cast<const float4*>(outputs + r * stride);
        #pragma unroll
        for (int q = 0; q < N_LOGITS / 4; q++) { const float4 v = lp4[q]; l[4 * q] = v.x; l[4 * q + 1] = v.y; l[4 * q + 2] = v.z; l[4 * q + 3] = v.w; }
        const float ls0 = log_std[0], ls1 = log_std[1];
        const float is0 = __expf(-ls0), is1 = __expf(-ls1);
        const float HALF_LOG_2PI = 0.918938533204672742f;
        float h0, h1, h2;
        head_probs<N_CAT>(l, p, lp, h0);
        head_probs<N_PRICE>(l + N_CAT, p + N_CAT, lp + N_CAT, h1);
        head_probs<N_OFF>(l + N_CAT + N_PRICE, p + N_CAT + N_PRICE, lp + N_CAT + N_PRICE, h2);
        const float ent = h0 + h1 + h2 + 1.0f + 2.0f * HALF_LOG_2PI + ls0 + ls1;
        const float es = ent_coef * k;
        const int best_c = argmax_low<N_CAT>(l), best_p = argmax_low<N_PRICE>(l + N_CAT), best_o = argmax_low<N_OFF>(l + N_CAT + N_PRICE);
        #pragma unroll
        for (int q = 0; q < N_LOGITS; q++) d[q] = 0.0f;
        const float val = outputs[r * stride + N_LOGITS];
        float G = 0.0f, W = 0.0f, dval = 0.0f;
        src.seek(row_index ? row_index[r] : r, agents);
        for (int a = 0; a < agents; a++) {
            const Sample s = src.get(a);
            const int ac = clamp_label<N_CAT>(s.cat), ap = clamp_label<N_PRICE>(s.price), ao = clamp_label<N_OFF>(s.off);
            const float w = s.logp_old;
            const float e0 = s.cont0 - l[22], e1 = s.cont1 - l[23];
            const float z0 = e0 * is0, z1 = e1 * is1;
            const float logp = -0.5f * z0 * z0 - ls0 - HALF_LOG_2PI - 0.5f * z1 * z1 - ls1 - HALF_LOG_2PI +
                               pick<N_CAT>(lp, ac) + pick<N_PRICE>(lp + N_CAT, ap) + pick<N_OFF>(lp + N_CAT + N_PRICE, ao);
            if (logp_out) logp_out[r * agents + a] = logp;
            const float g_logp = -w * k;
            const float dv = val - s.ret;
            nl -= w * logp;
            vl += w * dv * dv;
            dval += 2.0f * vf_coef * dv * w * k;
            en += w * ent;
            G += g_logp;
            W += w;
            #pragma unroll
            for (int q = 0; q < N_CAT; q++) d[q] += (q == ac) ? g_logp : 0.0f;
            #pragma unroll
            for (int q = 0; q < N_PRICE; q++) d[N_CAT + q] += (q == ap) ? g_logp : 0.0f;
            #pragma unroll
            for (int q = 0; q < N_OFF; q++) d[N_CAT + N_PRICE + q] += (q == ao) ? g_logp : 0.0f;
            d[22] += g_logp * z0 * is0;
            d[23] += g_logp * z1 * is1;
            dls0 += g_logp * (z0 * z0 - 1.0f) - es * w;
            dls1 += g_logp * (z1 * z1 - 1.0f) - es * w;
            bs[0] += w; bs[1] += ac == best_c ? w : 0.0f; bs[2] += ap == best_p ? w : 0.0f; bs[3] += ao == best_o ? w : 0.0f;
            bs[4] += w * e0 * e0; bs[5] += w * e1 * e1; bs[6] += w > 0.0f ? 1.0f : 0.0f;
        }
        const float esW = es * W;
        #pragma unroll
        for (int q = 0; q < N_CAT; q++) d[q] += -G * p[q] + esW * p[q] * (lp[q] + h0);
        #pragma unroll
        for (int q = 0; q < N_PRICE; q++) d[N_CAT + q] += -G * p[N_CAT + q] + esW * p[N_CAT + q] * (lp[N_CAT + q] + h1);
        #pragma unroll
        for (int q = 0; q < N_OFF; q++) d[N_CAT + N_PRICE + q] += -G * p[N_CAT + N_PRICE + q] + esW * p[N_CAT + N_PRICE + q] * (lp[N_CAT + N_PRICE + q] + h2);
        float4* dp4 = reinterpret_cast<float4*>(d_out + r * stride);
        #pragma unroll
        for (int q = 0; q < N_LOGITS / 4; q++) dp4[q] = make_float4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
        dp4[N_LOGITS / 4] = make_float4(dval, 0.0f, 0.0f, 0.0f);
        for (int q = N_LOGITS / 4 + 1; q < stride / 4; q++) dp4[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    // words 0..2 carry loss_scale, not k: the finishing step divides them by B (k_ppo_finish32 here, cda_mlp_adam's in the update)
    float v5[5] = {nl * loss_scale, vl * loss_scale, en * loss_scale, dls0, dls1};
    __shared__ float part[5][4];
    __shared__ double bpart[7][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    #pragma unroll
    for (int q = 0; q < 5; q++) {
        float x = v5[q];
        #pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if (lane == 0) part[q][wave] = x;
    }
    if (bc_stats) {                                                             // (uniform: the statistics cost nothing where nobody reads them)
        #pragma unroll
        for (int q = 0; q < 7; q++) {
            double x = (double)bs[q];
            #pragma unroll
            for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
            if (lane == 0) bpart[q][wave] = x;
        }
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const double t = (double)part[threadIdx.x][0] + (double)part[threadIdx.x][1] + (double)part[threadIdx.x][2] + (double)part[threadIdx.x][3];
        atomicAdd(&sums[threadIdx.x], t);
    }
    if (bc_stats && threadIdx.x >= 64 && threadIdx.x < 64 + 7) {
        const int q = threadIdx.x - 64;
        atomicAdd(&bc_stats[q], (bpart[q][0] + bpart[q][1]) + (bpart[q][2] + bpart[q][3]));
    }
}
}  // namespace

extern "C" int cda_bc_records(const int32_t* category, const int32_t* price, const int32_t* price_offset, const float* size_mean, const float* size_sigma, const float* a_cont,
                              const int32_t* slot_src, const float* slot_weight, int32_t n_steps, int64_t n_markets, int32_t num_agents, float* rec, double* stats2, void* stream) {
    if (!category || !price || !price_offset || !size_mean || !size_sigma || !slot_src || !slot_weight || !rec || !stats2 || n_steps < 1 || n_markets < 1 ||
        num_agents < 1 || num_agents > CDA_MAX_AGENTS || ((uintptr_t)rec & 15) != 0 || ((uintptr_t)a_cont & 7) != 0) return CDA_ERR_INVALID;
    const long long NA = (long long)n_markets * num_agents, total = NA * n_steps;
    if (total > ((long long)1 << 31) * 256) return CDA_ERR_INVALID;            // (the grid's x dimension)
    hipLaunchKernelGGL(k_bc_records, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const int*)category, (const int*)price, (const int*)price_offset,
                       size_mean, size_sigma, a_cont, (const int*)slot_src, slot_weight, total, NA, rec, stats2);
    return hipGetLastError() == hipSuccess ? CDA_OK : CDA_ERR_HIP;
}

extern "C" int cda_bc_loss_records(const float* outputs, const float* log_std, const float* rec, const int64_t* row_index, int64_t rows, int32_t agents_per_row,
                                   int32_t out_stride, float vf_coef, float ent_coef, float loss_scale, float* d_outputs, double* sums5, float* out6, int64_t norm_rows,
                                   int32_t clear, int32_t finish, float* logp_out, double* bc_stats, void* stream) {
    if (!outputs || !log_std || !rec || !d_outputs || !sums5 || !out6 || rows < 1 || agents_per_row < 1 || agents_per_row > CDA_MAX_AGENTS ||
        out_stride <= N_LOGITS || (out_stride & 3) || norm_rows < 0 || ((uintptr_t)rec & 15) != 0) return CDA_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const long long rn = norm_rows > 0 ? norm_rows : rows;
    if (clear && hipMemsetAsync(sums5, 0, 5 * sizeof(double), st) != hipSuccess) return CDA_ERR_HIP;
    hipLaunchKernelGGL(k_bc_loss_rec, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, outputs, log_std, rec, (const long long*)row_index, (long long)rows, rn,
                       (int)agents_per_row, (int)out_stride, vf_coef, ent_coef, loss_scale, d_outputs, sums5, logp_out, bc_stats);
    if (finish) hipLaunchKernelGGL(k_ppo_finish32, dim3(1), dim3(64), 0, st, (const double*)sums5, rn * agents_per_row, vf_coef, ent_coef, out6);
    return hipGetLastError() == hipSuccess ? CDA_OK : CDA_ERR_HIP;
}
