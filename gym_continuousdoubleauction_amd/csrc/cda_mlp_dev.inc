// cda_mlp_dev.inc - device helpers of the policy / value network shared by csrc/cda_mlp.hip (the network kernels) and csrc/cda_hip.hip (k_policy_step: the
// rollout's policy evaluated INSIDE the env step kernel).  No include guard and no namespace of its own: each translation unit includes it once, inside the
// namespace it keeps these names in.  The including file has included <hip/hip_runtime.h>, <type_traits> and include/cda_mlp.h (the layout constants).
// Everything here is compiled with floating-point contraction ON - the network has no bit-for-bit constraint of its own, but its two users must round alike:
// the policy evaluated inside the step kernel samples bit for bit what k_mlp_fwd<SAMPLE> samples.  The env kernels are built with -ffp-contract=off; the
// pragma below is file-scoped to this include (cda_hip.hip switches it off again behind the include).
#pragma clang fp contract(fast)
#ifndef CDA_MLP_AD
#define CDA_MLP_AD 2
#endif

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int OBS = CDA_MLP_OBS, KX = CDA_MLP_KX, XT = CDA_MLP_XTILES, HID = CDA_MLP_HID, NOUT = CDA_MLP_NOUT;
constexpr int XS_LD = KX + 8;        // LDS row of the observation tile: 184 bf16 = 368 B = 16 x 23 (odd: ds_read_b128 conflict free) at n_hist = 4; 16 x (2 k + 1) for every depth
// An observation row is 42 H floats = 168 H bytes: 16-byte aligned for even history depths only - rows are requested VW floats at a time
constexpr int VW = (OBS % 4 == 0) ? 4 : 2;
typedef std::conditional<VW == 4, float4, float2>::type obsvec;
template <typename V> __device__ __forceinline__ V vec_zero();
template <> __device__ __forceinline__ float4 vec_zero<float4>() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
template <> __device__ __forceinline__ float2 vec_zero<float2>() { return make_float2(0.0f, 0.0f); }
__device__ __forceinline__ obsvec obs_zero() { return vec_zero<obsvec>(); }
// VW values -> the bf16 LDS image / an f32 LDS row (member access only: an address taken of a register vector sends it through scratch)
__device__ __forceinline__ void obs_to_bf16(__bf16* dst, const float4& v, bool zero) {
    bf16x4 b; b[0] = (__bf16)(zero ? 0.0f : v.x); b[1] = (__bf16)(zero ? 0.0f : v.y); b[2] = (__bf16)(zero ? 0.0f : v.z); b[3] = (__bf16)(zero ? 0.0f : v.w);
    *reinterpret_cast<bf16x4*>(dst) = b;
}
__device__ __forceinline__ void obs_to_bf16(__bf16* dst, const float2& v, bool zero) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    bf16x2_t b; b[0] = (__bf16)(zero ? 0.0f : v.x); b[1] = (__bf16)(zero ? 0.0f : v.y);
    *reinterpret_cast<bf16x2_t*>(dst) = b;
}
__device__ __forceinline__ void obs_spread(float* dst, const float4& v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w; }
__device__ __forceinline__ void obs_spread(float* dst, const float2& v) { dst[0] = v.x; dst[1] = v.y; }
constexpr int ACT_LD = HID + 8;      // LDS row of an activation tile: 264 bf16 = 528 B = 16 x 33
constexpr int DO_LD = NOUT + 8;      // LDS row of the d_out tile: 40 bf16 = 80 B = 16 x 5
constexpr int OUTS_LD = NOUT + 1;    // f32 row of the output tile kept in LDS for the sampling epilogue
constexpr int N_CAT = CDA_HEAD_CATEGORY, N_PRICE = CDA_HEAD_PRICE, N_OFF = CDA_HEAD_OFFSET, N_LOGITS = CDA_HEAD_LOGITS;      // 9, 10, 3, 24 (include/cda_learner.h)
constexpr int LPS_LD = N_CAT + N_PRICE + N_OFF + 1;   // 23 floats: odd, conflict free

__device__ __forceinline__ int rowmap(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
constexpr float TWO_LOG2E = 2.885390081777926814f;
__device__ __forceinline__ float tanh_biased(float a, float bias_scaled) {
    // tanh(a + b) = 1 - 2 / (2^((a + b) 2 log2 e) + 1), b 2 log2 e folded by the caller: fma, v_exp_f32, add, v_rcp_f32, fma.  2^t overflows to
    // +inf for large t (-> 1) and underflows to 0 (-> -1): no clamp needed
    const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(a, TWO_LOG2E, bias_scaled));
    return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}
// ---- the hidden layers' activation: RLlib's fcnet_activation, one per object file (CDA_MLP_ACT: 0 tanh, the default and the reference's; 1 relu; 2 elu, alpha = 1;
// 3 linear).  BIAS_SCALE is folded into the bias where it is loaded; apply(acc, bias_scaled) = act(acc + bias); grad_from_out(h) = act'(z) from the STORED
// output h = act(z) - the backward never sees z.  Every act(0) = 0 (the dead units of a narrow network stay dead).  SiLU / swish has no such derivative (h does not
// determine z), hence no trait.
#ifndef CDA_MLP_ACT
#define CDA_MLP_ACT 0
#endif
template <int ACT> struct ActT;
template <> struct ActT<0> {
    static constexpr float BIAS_SCALE = TWO_LOG2E;
    static __device__ __forceinline__ float apply(float a, float bias_scaled) { return tanh_biased(a, bias_scaled); }
    static __device__ __forceinline__ float grad_from_out(float h) { return 1.0f - h * h; }
};
template <> struct ActT<1> {
    static constexpr float BIAS_SCALE = 1.0f;
    static __device__ __forceinline__ float apply(float a, float b) { return fmaxf(a + b, 0.0f); }
    static __device__ __forceinline__ float grad_from_out(float h) { return h > 0.0f ? 1.0f : 0.0f; }          // (torch: relu'(0) = 0)
};
template <> struct ActT<2> {
    static constexpr float BIAS_SCALE = 1.0f;
    static __device__ __forceinline__ float apply(float a, float b) {
        // z < 0: e^z - 1.  2^(z log2 e) - 1 cancels as z -> 0- (all relative accuracy is gone by |z| ~ 1e-7), so -1/4 < z < 0 takes the Taylor series of
        // expm1 to z^5 (truncation < z^6 / 720: relative 1.4e-6 at -1/4) and only z <= -1/4 (|e^z - 1| >= 0.22) the exponential
        const float z = a + b;
        const float p = z * __builtin_fmaf(z, __builtin_fmaf(z, __builtin_fmaf(z, __builtin_fmaf(z, 1.0f / 120.0f, 1.0f / 24.0f), 1.0f / 6.0f), 0.5f), 1.0f);
        const float e = __builtin_amdgcn_exp2f(z * 1.442695040888963407f) - 1.0f;
        return z > 0.0f ? z : (z > -0.25f ? p : e);
    }
    static __device__ __forceinline__ float grad_from_out(float h) { return h > 0.0f ? 1.0f : h + 1.0f; }     // (e^z = h + 1: exact for alpha = 1)
};
template <> struct ActT<3> {
    static constexpr float BIAS_SCALE = 1.0f;
    static __device__ __forceinline__ float apply(float a, float b) { return a + b; }
    // (h - h) + 1 = 1 for every finite h.  A bare constant leaves the update kernel's stored-h registers dead, and k_mlp_fb's allocation then spills 81 SGPRs
    static __device__ __forceinline__ float grad_from_out(float h) { return (h - h) + 1.0f; }
};
typedef ActT<CDA_MLP_ACT> Act;
__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 zero16() { f32x16 z; for (int r = 0; r < 16; r++) z[r] = 0.0f; return z; }

// The B operand (weights) of a layer goes through a register ring of RING k-steps, statically indexed (the loops are unrolled): a layer is
// PRIMED - its first RING steps requested - before the previous layer's epilogue and barrier, and while step ks multiplies, step ks + RING
// is requested.  hipcc on its own looks ONE step ahead and sinks every other request to just before its use, which leaves a wave with
// 2 .. 8 MFMAs per step waiting ~600 cycles for L2 each time: hence the sched_barriers.
// The weights live in HBM in OPERAND ORDER (cda_mlp_pack / k_adam write them so): for a wave's group of 32 JT output features, column tile jt and
// k-step ks, the 64 lanes' 16-byte pieces are 1 KB of CONTIGUOUS memory - a wave request is eight whole cache lines.  (Read from nn.Linear's
// row-major [out][in] instead, a request touched 32 rows 512 B apart and used 32 B of every 128-B line; four waves' working set does not fit
// the 32-KB L1, so every k-step re-fetched four times its bytes from L2: ~400 cycles per k-step however many MFMAs it held.)
// PAIRED (two column tiles): tile jt, lane j holds weight row 2 j + jt of the group - a lane then holds two NEIGHBOURING output features of the
// same rows, which is one dword of the row-major LDS image of the activations (no cross-lane exchange) - see feature_of() and pack_one().
template <int JT, int KSTEPS, int PF, bool PAIRED = false>
struct WRing {
    static constexpr int RING = PF < KSTEPS ? PF : KSTEPS;
    bf16x8 b[RING][JT];
    const __bf16* base;                                                          // the group's image + this lane's 16 bytes
    __device__ __forceinline__ const bf16x8* piece(int jt, int ks) const { return reinterpret_cast<const bf16x8*>(base + (size_t)(jt * KSTEPS + ks) * 512); }
    __device__ __forceinline__ void prime(const __bf16* __restrict__ group, int /*ld*/, int lane) {
        base = group + lane * 8;
        #pragma unroll
        for (int ks = 0; ks < RING; ks++)
            #pragma unroll
            for (int jt = 0; jt < JT; jt++) b[ks][jt] = *piece(jt, ks);
        __builtin_amdgcn_sched_barrier(0);
    }
};

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// k = the top 24 bits of one 32-bit half -> (k + 0.5) / 2^24 in float32, inside (0, 1): exact below 0.5; above, k + 0.5 is not representable and rounds to even
// (u takes the even 24-bit values), and k = 2^24 - 1 would round to 1.0 - clamped to the largest float32 below 1.  At u == 1 an inverse CDF finds no class
// (t = u * s reaches the running sum's last value) and falls through to the LAST one whatever its probability.
__device__ __forceinline__ float u01(unsigned long long w, int half) {
    const unsigned int x = half ? (unsigned int)(w >> 32) : (unsigned int)w;
    return fminf(((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
}
template <int N>
__device__ __forceinline__ int sample_head(const float* l, float u, float& logp) {
    float mx = l[0];
    #pragma unroll
    for (int j = 1; j < N; j++) mx = fmaxf(mx, l[j]);
    float e[N], s = 0.0f;
    #pragma unroll
    for (int j = 0; j < N; j++) { e[j] = __expf(l[j] - mx); s += e[j]; }
    const float t = u * s;
    float c = 0.0f, la = l[N - 1];
    int a = N - 1;
    bool found = false;
    #pragma unroll
    for (int j = 0; j < N; j++) { c += e[j]; if (!found && t < c) { a = j; la = l[j]; found = true; } }
    logp += la - mx - __logf(s);
    return a;
}

// softmax of one head: p[q], c = max + log(sum) (log p[q] = l[q] - c), entropy
template <int N> __device__ __forceinline__ void head_probs_c(const float* l, float* p, float& c, float& ent) {
    float mx = l[0];
    #pragma unroll
    for (int q = 1; q < N; q++) mx = fmaxf(mx, l[q]);
    float s = 0.0f;
    #pragma unroll
    for (int q = 0; q < N; q++) { p[q] = __expf(l[q] - mx); s += p[q]; }
    const float ls = __logf(s), inv = 1.0f / s;
    float hh = 0.0f;
    #pragma unroll
    for (int q = 0; q < N; q++) { p[q] *= inv; hh -= p[q] * (l[q] - mx - ls); }
    c = mx + ls; ent = hh;
}

// ---- the rollout's policy step, shared arithmetic ---------------------------------------------------------------------------------
// One (row, agent) sample from a row's 24 policy outputs l (9 | 10 | 3 logits, 2 means): three categorical heads by inverse CDF, two Gaussian heads by
// Box-Muller, the action's log-probability, and the env's action words (size_mean = tanh, size_sigma = sigmoid: the Box bounds of action_helper.py:126-138).
// key = the rollout's key (seed, rollout counter, step), i = global sample index (market * agents + agent).
struct SampledAction { int cat, price, off; float x0, x1, logp, size_mean, size_sigma; };
__device__ __forceinline__ SampledAction sample_action(const float (&l)[N_LOGITS], unsigned long long key, long long i, float ls0, float ls1) {
    const float HALF_LOG_2PI = 0.918938533204672742f;
    const unsigned long long w0 = mix64(key + (unsigned long long)i), w1 = mix64(w0), w2 = mix64(w1);
    SampledAction s;
    float lp = 0.0f;
    s.cat = sample_head<N_CAT>(l, u01(w0, 0), lp);
    s.price = sample_head<N_PRICE>(l + N_CAT, u01(w0, 1), lp);
    s.off = sample_head<N_OFF>(l + N_CAT + N_PRICE, u01(w1, 0), lp);
    const float rr = sqrtf(-2.0f * __logf(u01(w1, 1))), th = 6.283185307179586f * u01(w2, 0);
    const float n0 = rr * __cosf(th), n1 = rr * __sinf(th);
    // (explicit fused multiply-adds: left to the contraction pragma, the compiler fused these in one of this function's two inlined copies and not in the other)
    s.x0 = __builtin_fmaf(__expf(ls0), n0, l[22]); s.x1 = __builtin_fmaf(__expf(ls1), n1, l[23]);
    lp += -0.5f * n0 * n0 - ls0 - HALF_LOG_2PI - 0.5f * n1 * n1 - ls1 - HALF_LOG_2PI;
    s.logp = lp;
    s.size_mean = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(__expf(2.0f * s.x0) + 1.0f), 1.0f);      // tanh(x0): 1 - 2 / (e^(2 x0) + 1); libm's tanhf is a call of ~100 instructions
    s.size_sigma = 1.0f / (1.0f + __expf(-s.x1));
    return s;
}
// The MODE of the same distribution (RLlib's to_deterministic(), explore=False): each categorical head takes its largest logit (strict > from index 0: the lowest
// index wins a tie, torch.argmax), the Gaussian heads their means.  logp = the mode's log-probability - sample_action's formula with n0 = n1 = 0; the env words
// are sample_action's expressions of the means.  No randomness.
template <int N>
__device__ __forceinline__ int mode_head(const float* l, float& logp) {
    float mx = l[0];
    int a = 0;
    #pragma unroll
    for (int j = 1; j < N; j++) if (l[j] > mx) { mx = l[j]; a = j; }
    float s = 0.0f;
    #pragma unroll
    for (int j = 0; j < N; j++) s += __expf(l[j] - mx);
    logp -= __logf(s);                                 // l[a] - max - log(sum): l[a] IS the max (a dynamic l[a] keeps every compare mask of the scan live: SGPR spills)
    return a;
}
__device__ __forceinline__ SampledAction mode_action(const float (&l)[N_LOGITS], float ls0, float ls1) {
    const float HALF_LOG_2PI = 0.918938533204672742f;
    SampledAction s;
    float lp = 0.0f;
    s.cat = mode_head<N_CAT>(l, lp);
    s.price = mode_head<N_PRICE>(l + N_CAT, lp);
    s.off = mode_head<N_OFF>(l + N_CAT + N_PRICE, lp);
    s.x0 = l[22]; s.x1 = l[23];
    lp += -ls0 - HALF_LOG_2PI - ls1 - HALF_LOG_2PI;
    s.logp = lp;
    s.size_mean = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(__expf(2.0f * s.x0) + 1.0f), 1.0f);
    s.size_sigma = 1.0f / (1.0f + __expf(-s.x1));
    return s;
}
__device__ __forceinline__ unsigned long long rollout_key(unsigned long long seed, long long counter, long long draw) {
    return mix64(seed + (unsigned long long)counter * 0xd1342543de82ef95ull + (unsigned long long)draw * 0x2545f4914f6cdd1dull);
}
// a row's distribution as the update's KL term wants it: 22 normalised log-probabilities | 2 means
__device__ __forceinline__ void dist_row(const float (&l)[N_LOGITS], float (&o24)[N_LOGITS]) {
    float p[N_CAT + N_PRICE + N_OFF], c0, c1, c2, e0;
    head_probs_c<N_CAT>(l, p, c0, e0); head_probs_c<N_PRICE>(l + N_CAT, p + N_CAT, c1, e0); head_probs_c<N_OFF>(l + N_CAT + N_PRICE, p + N_CAT + N_PRICE, c2, e0);
    #pragma unroll
    for (int q = 0; q < N_LOGITS; q++) o24[q] = q < N_CAT ? l[q] - c0 : (q < N_CAT + N_PRICE ? l[q] - c1 : (q < N_CAT + N_PRICE + N_OFF ? l[q] - c2 : l[q]));
}

// ---- the forward pass of SIXTEEN rows by a workgroup of sixteen waves (k_policy_step: one market per wave) -----------------------------
// Wave w owns ONE 32-feature tile of each hidden layer: network half w / 8, feature group (w / 2) % 4, tile w % 2 of the group's pair - lane (q, h) holds feature
// 256 half + 64 group + 2 q + tile (the packed weight images' order, see WRing) of rows rowmap(r, h); rows 16 .. 31 of the MFMA tile repeat rows 0 .. 15 (the A
// operand is read at row & 15) and are dropped.  Per output element this is the SAME instruction sequence as k_mlp_fwd's - same MFMA, same k order, same
// epilogue arithmetic - so the outputs are bit for bit its outputs (tests/test_hip_policy_step.py).
// LDS: xs bf16 [16][XS_LD] (the observation rows, columns OBS .. KX - 1 zero), h1 / h2 bf16 [2][16][ACT_LD], outs f32 [16][OUTS_LD] (columns 0 .. 23 policy, 24 value).
constexpr int F16_ROWS = 16;
constexpr int F16_XS_BYTES = F16_ROWS * XS_LD * 2, F16_H_BYTES = 2 * F16_ROWS * ACT_LD * 2, F16_OUTS_BYTES = ((F16_ROWS * OUTS_LD * 4 + 15) / 16) * 16;
constexpr int F16_LDS_BYTES = ((F16_XS_BYTES + 15) / 16) * 16 + 2 * F16_H_BYTES + F16_OUTS_BYTES;
struct Fwd16Lds { __bf16* xs; __bf16* h1; __bf16* h2; float* outs; };
__device__ __forceinline__ Fwd16Lds fwd16_lds(unsigned char* base) {
    Fwd16Lds T;
    T.xs = reinterpret_cast<__bf16*>(base);
    T.h1 = reinterpret_cast<__bf16*>(base + ((F16_XS_BYTES + 15) / 16) * 16);
    T.h2 = T.h1 + 2 * F16_ROWS * ACT_LD;
    T.outs = reinterpret_cast<float*>(T.h2 + 2 * F16_ROWS * ACT_LD);
    return T;
}
template <int KSTEPS, int PF>
__device__ __forceinline__ void layer_mma16(const __bf16* a_lds, int a_ld, WRing<1, KSTEPS, PF, false>& W, int lane, f32x16& acc) {
    constexpr int RING = WRing<1, KSTEPS, PF, false>::RING;
    const __bf16* a_base = a_lds + (lane & 15) * a_ld + 8 * (lane >> 5);
    constexpr int AD = CDA_MLP_AD, AR = AD + 1;
    bf16x8 a[AR];
    #pragma unroll
    for (int s0 = 0; s0 < AD && s0 < KSTEPS; s0++) a[s0] = *reinterpret_cast<const bf16x8*>(a_base + 16 * s0);
    #pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++) {
        if (ks + AD < KSTEPS) a[(ks + AD) % AR] = *reinterpret_cast<const bf16x8*>(a_base + 16 * (ks + AD));
        acc = mfma(a[ks % AR], W.b[ks % RING][0], acc);
        if (ks + RING < KSTEPS) W.b[ks % RING][0] = *W.piece(0, ks + RING);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// Call with the observation rows staged in T.xs behind a __syncthreads(); returns behind one (T.outs complete).  Every wave of the workgroup takes part.
template <int PF>
__device__ __forceinline__ void forward16(const __bf16* __restrict__ wb, const float* __restrict__ theta, const Fwd16Lds& T, int w, int lane,
                                          WRing<1, KX / 16, PF, false>& R1) {
    const int q = lane & 31, h = lane >> 5;
    const int half = w >> 3, grp = (w >> 1) & 3, jt = w & 1;
    const int f = 256 * half + 64 * grp + 2 * q + jt;                            // this lane's feature (of 512) in both hidden layers
    const float b1 = theta[CDA_MLP_OFF_B1 + f] * Act::BIAS_SCALE, b2 = theta[CDA_MLP_OFF_B2 + f] * Act::BIAS_SCALE, bo = theta[CDA_MLP_OFF_BO + q];
    const bool heads = (w & 7) == 0;                                             // waves 0 and 8: the policy / value output tile of their half
    WRing<1, HID / 16, PF, false> R2, RO;
    f32x16 acc = zero16();
    layer_mma16(T.xs, XS_LD, R1, lane, acc);                                     // layer 1
    R2.prime(wb + CDA_MLP_WB_W2 + ((size_t)half * HID + 64 * grp) * HID + (size_t)jt * (HID / 16) * 512, HID, lane);
    {
        __bf16* dst = T.h1 + (half * F16_ROWS) * ACT_LD + 64 * grp + 2 * q + jt;
        #pragma unroll
        for (int r = 0; r < 8; r++) dst[rowmap(r, h) * ACT_LD] = (__bf16)Act::apply(acc[r], b1);
    }
    __syncthreads();
    acc = zero16();
    layer_mma16(T.h1 + (half * F16_ROWS) * ACT_LD, ACT_LD, R2, lane, acc);       // layer 2
    if (heads) RO.prime(wb + CDA_MLP_WB_WO + (size_t)half * NOUT * HID, HID, lane);
    {
        __bf16* dst = T.h2 + (half * F16_ROWS) * ACT_LD + 64 * grp + 2 * q + jt;
        #pragma unroll
        for (int r = 0; r < 8; r++) dst[rowmap(r, h) * ACT_LD] = (__bf16)Act::apply(acc[r], b2);
    }
    __syncthreads();
    if (heads) {
        acc = zero16();
        layer_mma16(T.h2 + (half * F16_ROWS) * ACT_LD, ACT_LD, RO, lane, acc);   // heads
        if (half == 0 ? q != N_LOGITS : q == N_LOGITS) {
            #pragma unroll
            for (int r = 0; r < 8; r++) T.outs[rowmap(r, h) * OUTS_LD + q] = acc[r] + bo;
        }
    }
    __syncthreads();
}
// forward16 with the network chosen at RUN time (k_net_step: one kernel instance per history depth for every activation and both trunks): `act` = the ActT<> code
// 0 .. 3 and `shared` = the shared trunk (CDA_MLP_VFS's network), both uniform over the workgroup.  The choice is made in the two hidden-layer epilogues only - the
// MFMA layers are the same code for every network, per output element ActT<act>::apply's own expression on the same accumulator: bit for bit forward16's (and so
// k_mlp_fwd's) outputs of the object compiled with that activation.  Shared trunk: only half 0 exists (Wo row 24 is packed into half 0) - waves 8 .. 15 skip the
// three MFMA phases and only meet the barriers (the k loops are NOT re-split over them: the summation order is k_mlp_fwd's), and wave 0's head tile owns every
// output column, the value's 24 included.  R1 of a wave that skips (shared && w >= 8) is never read: its caller need not prime it.
template <int ACT>
__device__ __forceinline__ void act_store16(__bf16* dst, const f32x16& acc, float bias_scaled, int h) {
    #pragma unroll
    for (int r = 0; r < 8; r++) dst[rowmap(r, h) * ACT_LD] = (__bf16)ActT<ACT>::apply(acc[r], bias_scaled);
}
__device__ __forceinline__ void act_store16_by_code(int act, __bf16* dst, const f32x16& acc, float bias_scaled, int h) {
    switch (act) {                                                               // (uniform: a scalar branch)
        case 0: act_store16<0>(dst, acc, bias_scaled, h); break;
        case 1: act_store16<1>(dst, acc, bias_scaled, h); break;
        case 2: act_store16<2>(dst, acc, bias_scaled, h); break;
        default: act_store16<3>(dst, acc, bias_scaled, h); break;
    }
}
template <int PF>
__device__ __forceinline__ void forward16_net(const __bf16* __restrict__ wb, const float* __restrict__ theta, const Fwd16Lds& T, int w, int lane,
                                              WRing<1, KX / 16, PF, false>& R1, int act, bool shared) {
    const int q = lane & 31, h = lane >> 5;
    const int half = w >> 3, grp = (w >> 1) & 3, jt = w & 1;
    const int f = 256 * half + 64 * grp + 2 * q + jt;
    const float bias_scale = act == 0 ? ActT<0>::BIAS_SCALE : 1.0f;              // ActT<1 .. 3>::BIAS_SCALE (x * 1 = x: the other objects' bias bit for bit)
    static_assert(ActT<1>::BIAS_SCALE == 1.0f && ActT<2>::BIAS_SCALE == 1.0f && ActT<3>::BIAS_SCALE == 1.0f, "BIAS_SCALE follows the activation");
    const float b1 = theta[CDA_MLP_OFF_B1 + f] * bias_scale, b2 = theta[CDA_MLP_OFF_B2 + f] * bias_scale, bo = theta[CDA_MLP_OFF_BO + q];
    const bool work = !(shared && half);                                         // the value half of a shared trunk does not exist
    const bool heads = (w & 7) == 0 && work;
    WRing<1, HID / 16, PF, false> R2, RO;
    f32x16 acc = zero16();
    if (work) {
        layer_mma16(T.xs, XS_LD, R1, lane, acc);                                 // layer 1
        R2.prime(wb + CDA_MLP_WB_W2 + ((size_t)half * HID + 64 * grp) * HID + (size_t)jt * (HID / 16) * 512, HID, lane);
        act_store16_by_code(act, T.h1 + (half * F16_ROWS) * ACT_LD + 64 * grp + 2 * q + jt, acc, b1, h);
    }
    __syncthreads();
    if (work) {
        acc = zero16();
        layer_mma16(T.h1 + (half * F16_ROWS) * ACT_LD, ACT_LD, R2, lane, acc);   // layer 2
        if (heads) RO.prime(wb + CDA_MLP_WB_WO + (size_t)half * NOUT * HID, HID, lane);
        act_store16_by_code(act, T.h2 + (half * F16_ROWS) * ACT_LD + 64 * grp + 2 * q + jt, acc, b2, h);
    }
    __syncthreads();
    if (heads) {
        acc = zero16();
        layer_mma16(T.h2 + (half * F16_ROWS) * ACT_LD, ACT_LD, RO, lane, acc);   // heads
        if (shared || (half == 0 ? q != N_LOGITS : q == N_LOGITS)) {
            #pragma unroll
            for (int r = 0; r < 8; r++) T.outs[rowmap(r, h) * OUTS_LD + q] = acc[r] + bo;
        }
    }
    __syncthreads();
}
