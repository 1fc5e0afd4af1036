// resco_ppo_train.h -- the PPO update of the S stacked actor-critics on the device: loss, backward, per-signal gradient clipping
// and Adam (rs_ppo_create / rs_ppo_grad / rs_ppo_step / rs_ppo_fit of include/resco_sim.h).
//
// What it replaces (resco_amd/agents/ippo.py: BatchedPPOLearner.loss, .clip_grad_per_signal, torch.optim.Adam inside ._fit): per
// Adam step ~200 small launches of the batched PyTorch learner, which pads every signal to lmax lanes.  Here every signal runs at
// its own lane count L_s (hs = L_s - 1 rows of conv output) and action count A_s; all arithmetic is fp32.
//
// The network of one signal (BatchedIPPO's layouts, all fp32, updated in place):
//     obs f16 [L][5] -> conv 2x2, 64 channels, ReLU -> feat[k], k = c * (H * 4) + h * 4 + w  (H = lmax - 1; only h < hs is real)
//     z1 = b1 + feat W1 [K][64], ReLU;  z2 = b2 + a1 W2 [64][64], ReLU;  logits = b3 + a2 W3 [64][amax];  value = bv + a2 Wv [64][1]
//
// Launches of one minibatch gradient (rs_ppo_grad), rows gathered through idx inside the kernels (row = idx[i]):
//   1. ppo_fwd_bwd_kernel, one workgroup per (64-row tile, signal): fc1 forward on v_mfma_f32_32x32x2_f32 with the conv features
//      formed in registers as the A operand; fc2, heads, the per-row loss gradient (ppo_row_loss_grad), backward to dz1 (written
//      to the workspace, zero for the rows a short last tile pads) and the tile's partial sums of the small layers' gradients.
//   2. ppo_fc1_bwd_kernel, one workgroup per (signal, 128-feature block = conv row h x half the channels, chunk of PPT_CH rows):
//      recomputes the features, dW1 = feat^T dz1 and dfeat = W1 dz1^T on the same MFMA, the conv gradients from dfeat.
//   3. ppo_reduce_kernel: partials -> gradients, chunks / tiles in ascending order.
// and of one optimiser step (rs_ppo_step): ppo_norm_kernel (squared norm per (signal, part)), ppo_adam_kernel (clip scale + Adam).
//
// Every sum has ONE order, fixed by the shapes alone: an MFMA accumulator is a k-ordered fmaf chain; rows are summed in ascending
// order inside a tile / chunk, then tiles / chunks in ascending order; the norm as PPT_T strided partial sums and a halving tree
// (of fp32 pairs, ppo_pair_add).
// No floating-point atomics: two runs from the same state give the same bits.
//
// The scalar pieces (per-row loss gradient, clip scale, Adam element update) are RS_PPO_HD functions in plain C++ that a host
// compiler builds as well (tests/ppo_train_host).
#pragma once
#include "resco_ppo.h"

#define PPT_NT 10           // tensors of a BatchedIPPO, in rs_ppo_tensors order
enum { PT_CONV_W = 0, PT_CONV_B, PT_FC1_W, PT_FC1_B, PT_FC2_W, PT_FC2_B, PT_FC3_W, PT_FC3_B, PT_V_W, PT_V_B };
#define PPT_AMAX 8          // actions per signal at most (POL_QMAX)
#define PPT_TM 64           // rows of a forward / backward tile
#define PPT_CH 512          // rows of a chunk of the fc1 backward (a multiple of PPT_TM)
#define PPT_T 256           // threads of every workgroup here
// per-tile partial sums of the small layers, floats from the tile's base
#define PPT_P_W2 0          // [64 k][64 j]
#define PPT_P_B2 4096       // [64]
#define PPT_P_W3 4160       // [64 k][9]: policy columns 0 .. A_s - 1, value head in column 8
#define PPT_P_B3 4736       // [9] (+ 7 unused)
#define PPT_P_B1 4752       // [64]
#define PPT_P_LOSS 4816     // pg, vf, ent as (hi, lo) pairs: three hi, three lo (+ 10 unused)
#define PPT_P_SIZE 4832
#define PPT_N_SMALL (PPT_P_SIZE + 320)      // outputs of the reduction beyond fc1_w: the tile partials, then conv [64 c][5]

// what the gradient kernels read of rs_ppo_config (the optimiser's constants: PpoStepConsts below)
struct PpoHyper { float clip_eps, entropy_coef, value_coef; };
struct PpoTensors { float *p[PPT_NT]; };

// ---------------------------------------------------------------------------------------------------------------- scalar pieces
// One sample of one signal: d(loss)/d(logits[0 .. A)), d(loss)/d(value) of
//     loss = inv_b * ( -min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv) + value_coef (value - ret)^2 - entropy_coef H )
// with lp = log_softmax(logits)[action], ratio = exp(lp - logp_old), H = -sum p lp over the signal's own A actions, and the three
// terms (-min(..), (value - ret)^2, H) un-scaled.  A == 1: lp = 0, p = 1 and the policy gradient is exactly zero.
RS_PPO_HD void ppo_row_loss_grad(const float *logits, int A, float value, int action, float logp_old, float adv, float ret, float inv_b,
                                 float clip_eps, float entropy_coef, float value_coef, float *dlogits, float *dvalue, float *terms) {
    float mx = logits[0];
    for (int a = 1; a < A; ++a) mx = logits[a] > mx ? logits[a] : mx;
    float se = 0.0f;
    for (int a = 0; a < A; ++a) se += expf(logits[a] - mx);
    const float lse = mx + logf(se);
    float lp[PPT_AMAX], pr[PPT_AMAX], ent = 0.0f;
    for (int a = 0; a < A; ++a) { lp[a] = logits[a] - lse; pr[a] = expf(lp[a]); ent -= pr[a] * lp[a]; }
    const float ratio = expf(lp[action] - logp_old);
    const float lo = 1.0f - clip_eps, hi = 1.0f + clip_eps;
    const float rc = ratio < lo ? lo : (ratio > hi ? hi : ratio);
    const float s1 = ratio * adv, s2 = rc * adv;
    const bool inside = ratio >= lo && ratio <= hi;
    // d(-min(s1, s2)) / d(lp): the unclipped branch (and the clamp's own pass-through inside the interval) gives -adv ratio
    const float dlp = (inside || s1 < s2) ? -(adv * ratio) * inv_b : 0.0f;
    const float ce = entropy_coef * inv_b;
    for (int a = 0; a < A; ++a) {
        const float onehot = a == action ? 1.0f : 0.0f;
        dlogits[a] = dlp * (onehot - pr[a]) + ce * (pr[a] * (lp[a] + ent));       // -entropy_coef dH/dz, dH/dz = -p (lp + H)
    }
    const float dv = value - ret;
    *dvalue = value_coef * 2.0f * dv * inv_b;
    terms[0] = -(s1 < s2 ? s1 : s2);
    terms[1] = dv * dv;
    terms[2] = ent;
}

// Sums that decide more than their own rounding (the squared gradient norm, whose clip scale multiplies every gradient; the loss
// terms, means of O(1) values): fp32 pairs (hi, lo) with the rounding error of every addition kept (Knuth's two-sum), so that the
// result does not depend on how many terms came before.  Plain fp32 operations; exact only without contraction and fast-math.
RS_PPO_HD void ppo_pair_add(float *hi, float *lo, float x, float x_lo) {
    const float s = *hi + x, bb = s - *hi;
    const float e = (*hi - (s - bb)) + (x - bb);
    *hi = s;
    *lo += e + x_lo;
}

// The same idea for the few operations between the squared norm and the Adam moments.  The clip scale multiplies every gradient
// of a signal, and a moment of the first steps is a short product of it: rounded to fp32 at every operation the moments are 2 - 3
// ulp off, which is as much as torch's own float32 learner is off, but not within a small multiple of what it happens to be off on
// a tensor of a handful of elements (v_b has one per signal).  So scale, clipped gradient and the two moment updates are formed as
// fp32 pairs (fmaf for the exact product error) and rounded ONCE when the moment is stored; the constants come as pairs of the
// caller's doubles.  The parameter step then uses the stored fp32 moments as torch does.
struct PpoPair { float hi, lo; };
RS_PPO_HD PpoPair ppo_pair_norm(float a, float b) { const float s = a + b; return PpoPair{s, b - (s - a)}; }      // |a| >= |b|
RS_PPO_HD PpoPair ppo_pair_sum(PpoPair a, PpoPair b) {
    float hi = a.hi, lo = a.lo;
    ppo_pair_add(&hi, &lo, b.hi, b.lo);
    return ppo_pair_norm(hi, lo);
}
RS_PPO_HD PpoPair ppo_pair_mul(PpoPair a, PpoPair b) {
    const float p = a.hi * b.hi;
    return ppo_pair_norm(p, fmaf(a.hi, b.hi, -p) + (a.hi * b.lo + a.lo * b.hi));
}
RS_PPO_HD PpoPair ppo_pair_div(PpoPair a, PpoPair b) {
    const float q = a.hi / b.hi;
    const PpoPair qb = ppo_pair_mul(b, PpoPair{q, 0.0f});
    const PpoPair r = ppo_pair_sum(a, PpoPair{-qb.hi, -qb.lo});
    return ppo_pair_norm(q, r.hi / b.hi);
}
RS_PPO_HD PpoPair ppo_pair_sqrt(PpoPair a) {
    if (!(a.hi > 0.0f)) return PpoPair{0.0f, 0.0f};
    const float r = sqrtf(a.hi), p = r * r;
    const float rem = ((a.hi - p) - fmaf(r, r, -p)) + a.lo;
    return ppo_pair_norm(r, rem / (r + r));
}

// the constants of a step as pairs of the caller's doubles (host side: ppo_step_consts)
struct PpoStepConsts { PpoPair om_beta1, beta2, om_beta2, max_grad_norm, norm_eps; float adam_eps, step_size, bc2_sqrt; };
static inline PpoPair ppo_pair_of(double d) { const float hi = (float)d; return PpoPair{hi, (float)(d - (double)hi)}; }
// torch.optim.Adam forms step_size = lr / (1 - beta1^t), sqrt(1 - beta2^t), 1 - beta1, 1 - beta2 in double and rounds them where
// they meet the tensors; clip_grad_per_signal's constants are max_grad_norm and 1e-6
static inline PpoStepConsts ppo_step_consts(double lr, double adam_eps, double beta1, double beta2, double max_grad_norm, long long t) {
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    return PpoStepConsts{ppo_pair_of(1.0 - beta1), ppo_pair_of(beta2), ppo_pair_of(1.0 - beta2), ppo_pair_of(max_grad_norm), ppo_pair_of(1e-6),
                         (float)adam_eps, (float)(lr / bc1), (float)sqrt(bc2)};
}

// torch.nn.utils.clip_grad_norm_ per signal, as BatchedPPOLearner.clip_grad_per_signal: min(1, max_norm / (norm + 1e-6))
RS_PPO_HD PpoPair ppo_clip_scale(PpoPair sq_norm, const PpoStepConsts &K) {
    const PpoPair s = ppo_pair_div(K.max_grad_norm, ppo_pair_sum(ppo_pair_sqrt(sq_norm), K.norm_eps));
    return s.hi < 1.0f ? s : PpoPair{1.0f, 0.0f};
}

// torch.optim.Adam's element update (no weight decay, no amsgrad) of the gradient g clipped by `scale`:
//     m += (g scale - m) (1 - beta1);   v = v beta2 + (1 - beta2) (g scale)^2;   p -= step_size m / (sqrt(v) / bc2_sqrt + eps)
RS_PPO_HD void ppo_adam_element(float *p, float *m, float *v, float g, PpoPair scale, const PpoStepConsts &K) {
    const PpoPair gc = ppo_pair_mul(scale, PpoPair{g, 0.0f});
    const PpoPair dm = ppo_pair_mul(ppo_pair_sum(gc, PpoPair{-*m, 0.0f}), K.om_beta1);
    const float m1 = ppo_pair_sum(PpoPair{*m, 0.0f}, dm).hi;                                   // exp_avg.lerp_(grad, 1 - beta1)
    const float v1 = ppo_pair_sum(ppo_pair_mul(K.beta2, PpoPair{*v, 0.0f}), ppo_pair_mul(ppo_pair_mul(gc, gc), K.om_beta2)).hi;
    const float denom = sqrtf(v1) / K.bc2_sqrt + K.adam_eps;
    *m = m1;
    *v = v1;
    *p = *p - K.step_size * (m1 / denom);
}

#ifdef __HIPCC__
typedef float ppt_f16 __attribute__((ext_vector_type(16)));

struct PpoTrainTab {
    int32_t S, lmax, amax, H;               // H = lmax - 1
    const int32_t *lanes, *n_actions;       // device [S]
    PpoTensors par, grad, m, v;
    PpoHyper hp;
    int32_t bpad_max;                       // rows of the dz1 workspace per signal (max_minibatch rounded up to PPT_TM)
    int32_t tiles_max, chunks_max;
    float *dz1;                             // [S][bpad_max][64]
    float *part;                            // [S][tiles_max][PPT_P_SIZE]
    float *pw1;                             // [chunks_max][S][H * 256][64]
    float *pconv;                           // [chunks_max][S][H][64][5]
    float *sqpart;                          // [S][H + 1][hi, lo]
};

struct PpoBatch {
    const __half *obs;                      // [n][S][lmax][5]
    const int32_t *act;                     // [n][S]
    const float *logp, *adv, *ret;          // [n][S]
    const int32_t *idx;                     // [B]
    int32_t B;
    __device__ const __half *row(int i, int s, int S, int ow) const { return obs + ((size_t)idx[i] * S + s) * ow; }
};

__device__ static inline ppt_f16 ppt_zero16() { ppt_f16 z; for (int i = 0; i < 16; ++i) z[i] = 0.0f; return z; }
__device__ static inline float ppt_conv(float b, float w0, float w1, float w2, float w3, float o00, float o01, float o10, float o11) {
    return fmaf(w3, o11, fmaf(w2, o10, fmaf(w1, o01, fmaf(w0, o00, b))));
}

// ------------------------------------------------------------------------------------- 1. forward, loss, backward to dz1, per tile
__global__ void __launch_bounds__(PPT_T) ppo_fwd_bwd_kernel(PpoTrainTab T, PpoBatch D) {
    constexpr int OS = 85, ZS = 65;
    __shared__ float bufA[PPT_TM * OS];             // observations, later dz2, later dz1 (both with stride ZS)
    __shared__ float a1_s[PPT_TM * ZS], a2_s[PPT_TM * ZS];
    __shared__ float cw_s[64 * 8];                  // conv weights [c][w00 w01 w10 w11 b . . .]
    __shared__ float lg_s[PPT_TM * 9], dl_s[PPT_TM * 9], lt_s[PPT_TM * 3];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x, s = blockIdx.y, S = T.S, lmax = T.lmax;
    const int hs = T.lanes[s] - 1, A = T.n_actions[s], amax = T.amax;
    const int r0 = tile * PPT_TM, nrows = min(PPT_TM, D.B - r0), ow = lmax * 5;
    const int H4 = T.H * 4;

    for (int e = tid; e < PPT_TM * ow; e += PPT_T) {
        const int r = e / ow, q = e - r * ow;
        float x = 0.0f;
        if (r < nrows) x = __half2float(D.obs[((size_t)D.idx[r0 + r] * S + s) * ow + q]);
        bufA[r * OS + q] = x;
    }
    for (int e = tid; e < 64 * 8; e += PPT_T) {
        const int c = e >> 3, q = e & 7;
        cw_s[e] = q < 4 ? T.par.p[PT_CONV_W][((size_t)s * 64 + c) * 4 + q] : (q == 4 ? T.par.p[PT_CONV_B][s * 64 + c] : 0.0f);
    }
    __syncthreads();

    // ---- fc1 forward: wave wv owns rows (wv & 1) * 32 .. + 31 and outputs (wv >> 1) * 32 .. + 31; k order h, w, c; one accumulator per w
    {
        const int i = lane & 31, g = lane >> 5, mt = wv & 1, nt = wv >> 1, row = mt * 32 + i;
        const float *w1 = T.par.p[PT_FC1_W] + (size_t)s * H4 * 64 * 64 + nt * 32 + i;
        ppt_f16 acc[4];
        for (int w = 0; w < 4; ++w) acc[w] = ppt_zero16();
        for (int h = 0; h < hs; ++h) {
            float o[2][5];
            for (int q = 0; q < 5; ++q) { o[0][q] = bufA[row * OS + h * 5 + q]; o[1][q] = bufA[row * OS + h * 5 + 5 + q]; }
#pragma unroll 4
            for (int c = 0; c < 64; c += 2) {
                const int cc = c + g;
                const float4 cw = *(const float4 *)&cw_s[cc * 8];
                const float cb = cw_s[cc * 8 + 4];
                const float *wk = w1 + ((size_t)cc * H4 + h * 4) * 64;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const float f = fmaxf(ppt_conv(cb, cw.x, cw.y, cw.z, cw.w, o[0][w], o[0][w + 1], o[1][w], o[1][w + 1]), 0.0f);
                    acc[w] = __builtin_amdgcn_mfma_f32_32x32x2f32(f, wk[w * 64], acc[w], 0, 0, 0);
                }
            }
        }
        const float b1 = T.par.p[PT_FC1_B][s * 64 + nt * 32 + i];
        for (int r = 0; r < 16; ++r) {
            const int rr = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
            const float z = ((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r])) + b1;
            a1_s[rr * ZS + nt * 32 + i] = fmaxf(z, 0.0f);
        }
    }
    __syncthreads();

    const int row = lane, kg = wv * 16;             // the small layers: a thread owns one row and 16 wave-uniform columns
    // ---- fc2 forward
    {
        const float *w2 = T.par.p[PT_FC2_W] + (size_t)s * 4096 + kg;
        float z[16];
        for (int j = 0; j < 16; ++j) z[j] = T.par.p[PT_FC2_B][s * 64 + kg + j];
        for (int k = 0; k < 64; ++k) {
            const float a = a1_s[row * ZS + k];
            for (int j = 0; j < 16; ++j) z[j] = fmaf(a, w2[k * 64 + j], z[j]);
        }
        for (int j = 0; j < 16; ++j) a2_s[row * ZS + kg + j] = fmaxf(z[j], 0.0f);
    }
    __syncthreads();
    // ---- heads: wave wv computes columns wv, wv + 4 and (wave 0) the value as column 8
    for (int a = wv; a < 9; a += 4) {
        if (a < 8 && a >= A) continue;
        const float *wc = a < 8 ? T.par.p[PT_FC3_W] + (size_t)s * 64 * amax + a : T.par.p[PT_V_W] + (size_t)s * 64;
        const int st = a < 8 ? amax : 1;
        float z = a < 8 ? T.par.p[PT_FC3_B][s * amax + a] : T.par.p[PT_V_B][s];
        for (int k = 0; k < 64; ++k) z = fmaf(a2_s[row * ZS + k], wc[k * st], z);
        lg_s[row * 9 + a] = z;
    }
    __syncthreads();
    // ---- the loss gradient of every row; rows past the minibatch contribute nothing
    if (tid < PPT_TM) {
        float dl[PPT_AMAX], dv = 0.0f, tm[3] = {0.0f, 0.0f, 0.0f};
        for (int a = 0; a < PPT_AMAX; ++a) dl[a] = 0.0f;
        if (tid < nrows) {
            const size_t smp = (size_t)D.idx[r0 + tid] * S + s;
            float lg[PPT_AMAX];
            for (int a = 0; a < PPT_AMAX; ++a) lg[a] = a < A ? lg_s[tid * 9 + a] : 0.0f;
            int act = D.act[smp];
            act = act < 0 ? 0 : (act >= A ? A - 1 : act);
            ppo_row_loss_grad(lg, A, lg_s[tid * 9 + 8], act, D.logp[smp], D.adv[smp], D.ret[smp], 1.0f / (float)D.B, T.hp.clip_eps,
                              T.hp.entropy_coef, T.hp.value_coef, dl, &dv, tm);
        }
        for (int a = 0; a < PPT_AMAX; ++a) dl_s[tid * 9 + a] = a < A ? dl[a] : 0.0f;
        dl_s[tid * 9 + 8] = dv;
        for (int q = 0; q < 3; ++q) lt_s[tid * 3 + q] = tm[q];
    }
    __syncthreads();
    // ---- dz2 = (z2 > 0) (dlogits W3^T + dvalue Wv^T) -> bufA (the observations are no longer needed)
    {
        float d[16];
        const float dv = dl_s[row * 9 + 8];
        const float *wvv = T.par.p[PT_V_W] + (size_t)s * 64 + kg;
        for (int j = 0; j < 16; ++j) d[j] = dv * wvv[j];
        const float *w3 = T.par.p[PT_FC3_W] + ((size_t)s * 64 + kg) * amax;
        for (int a = 0; a < A; ++a) {
            const float x = dl_s[row * 9 + a];
            for (int j = 0; j < 16; ++j) d[j] = fmaf(x, w3[j * amax + a], d[j]);
        }
        for (int j = 0; j < 16; ++j) bufA[row * ZS + kg + j] = a2_s[row * ZS + kg + j] > 0.0f ? d[j] : 0.0f;
    }
    __syncthreads();
    float *P = T.part + ((size_t)s * T.tiles_max + tile) * PPT_P_SIZE;
    // ---- partial sums over the tile's rows that need dz2: dW2 = a1^T dz2, db2, dW3 / dWv = a2^T dlogits, db3 / dbv, the loss terms
    {
        float g2[16];
        for (int j = 0; j < 16; ++j) g2[j] = 0.0f;
        for (int r = 0; r < PPT_TM; ++r) {
            const float dz = bufA[r * ZS + lane];
            for (int j = 0; j < 16; ++j) g2[j] = fmaf(a1_s[r * ZS + kg + j], dz, g2[j]);
        }
        for (int j = 0; j < 16; ++j) P[PPT_P_W2 + (kg + j) * 64 + lane] = g2[j];
        for (int o = tid; o < 64 * 9; o += PPT_T) {
            const int k = o / 9, a = o - k * 9;
            float acc = 0.0f;
            for (int r = 0; r < PPT_TM; ++r) acc = fmaf(a2_s[r * ZS + k], dl_s[r * 9 + a], acc);
            P[PPT_P_W3 + o] = acc;
        }
        if (tid < 64) {
            float acc = 0.0f;
            for (int r = 0; r < PPT_TM; ++r) acc += bufA[r * ZS + tid];
            P[PPT_P_B2 + tid] = acc;
        } else if (tid < 64 + 9) {
            float acc = 0.0f;
            for (int r = 0; r < PPT_TM; ++r) acc += dl_s[r * 9 + (tid - 64)];
            P[PPT_P_B3 + tid - 64] = acc;
        } else if (tid >= 128 && tid < 131) {
            float hi = 0.0f, lo = 0.0f;
            for (int r = 0; r < PPT_TM; ++r) ppo_pair_add(&hi, &lo, lt_s[r * 3 + (tid - 128)], 0.0f);
            P[PPT_P_LOSS + tid - 128] = hi;
            P[PPT_P_LOSS + 3 + tid - 128] = lo;
        }
    }
    // ---- dz1 = (z1 > 0) dz2 W2^T: into registers, then (every wave has read its rows' dz2) over dz2 in bufA
    float d1[16];
    {
        const float *w2 = T.par.p[PT_FC2_W] + (size_t)s * 4096 + (size_t)kg * 64;
        for (int j = 0; j < 16; ++j) d1[j] = 0.0f;
        for (int q = 0; q < 64; ++q) {
            const float dz = bufA[row * ZS + q];
            for (int j = 0; j < 16; ++j) d1[j] = fmaf(dz, w2[j * 64 + q], d1[j]);
        }
        for (int j = 0; j < 16; ++j) d1[j] = a1_s[row * ZS + kg + j] > 0.0f ? d1[j] : 0.0f;
    }
    __syncthreads();
    for (int j = 0; j < 16; ++j) bufA[row * ZS + kg + j] = d1[j];
    __syncthreads();
    {
        float *dz = T.dz1 + ((size_t)s * T.bpad_max + r0) * 64;
        for (int e = tid; e < PPT_TM * 64; e += PPT_T) dz[e] = bufA[(e >> 6) * ZS + (e & 63)];
        if (tid < 64) {
            float acc = 0.0f;
            for (int r = 0; r < PPT_TM; ++r) acc += bufA[r * ZS + tid];
            P[PPT_P_B1 + tid] = acc;
        }
    }
}

// ------------------------------------------------------------- 2. fc1 backward: dW1, dfeat and the conv gradients, per feature block
// block (h, cb): conv row h, channels cb * 32 .. + 31 = 128 features m = (c - cb * 32) * 4 + w; wave wv owns features wv * 32 .. + 31
// The body is shared with the DQN update (resco_dqn_train.h): Tab = the table of either learner, Batch = its minibatch, which says
// where row i of signal s has its observation (Batch::row) and how many rows there are (Batch::B).
template <class Tab, class Batch> __device__ __forceinline__ void ppt_fc1_bwd_body(const Tab &T, const Batch &D) {
    constexpr int ZS = 65, OS = 11;
    __shared__ float dz_s[32 * ZS], ob_s[32 * OS];
    __shared__ float red_s[4 * 64 * 20];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.x >> 1, cb = blockIdx.x & 1, chunk = blockIdx.y, s = blockIdx.z;
    const int S = T.S, lmax = T.lmax, hs = T.lanes[s] - 1, ow = lmax * 5, H4 = T.H * 4;
    if (h >= hs) return;
    const int i = lane & 31, g = lane >> 5;
    const int bpad = (D.B + PPT_TM - 1) / PPT_TM * PPT_TM;
    const int rbeg = chunk * PPT_CH, rend = min(bpad, rbeg + PPT_CH);
    const float *cwp = T.par.p[PT_CONV_W] + (size_t)s * 256, *cbp = T.par.p[PT_CONV_B] + (size_t)s * 64;
    const float *w1 = T.par.p[PT_FC1_W] + (size_t)s * H4 * 64 * 64;

    // A-operand role: feature m = wv * 32 + i -> channel cA, column wA, fc1 row kA
    const int cA = cb * 32 + wv * 8 + (i >> 2), wA = i & 3;
    const size_t kA = (size_t)cA * H4 + h * 4 + wA;
    const float a_w0 = cwp[cA * 4], a_w1 = cwp[cA * 4 + 1], a_w2 = cwp[cA * 4 + 2], a_w3 = cwp[cA * 4 + 3], a_b = cbp[cA];
    float wf[32];                                   // W1[kA][2 jj + g]: the A operand of dfeat = W1 dz1^T, the same for every row
    for (int jj = 0; jj < 32; ++jj) wf[jj] = w1[kA * 64 + 2 * jj + g];
    // C-layout role of the dfeat tile: lane = row, register r = feature (r & 3) + 8 (r >> 2) + 4 g -> column r & 3, channel cC(r >> 2)
    float c_w[4][5], dconv[4][5];
    for (int q = 0; q < 4; ++q) {
        const int cC = cb * 32 + wv * 8 + 2 * q + g;
        for (int e = 0; e < 4; ++e) c_w[q][e] = cwp[cC * 4 + e];
        c_w[q][4] = cbp[cC];
        for (int e = 0; e < 5; ++e) dconv[q][e] = 0.0f;
    }
    ppt_f16 accw0 = ppt_zero16(), accw1 = ppt_zero16();

    for (int rb = rbeg; rb < rend; rb += 32) {
        __syncthreads();
        {
            const int r = tid >> 3, j0 = (tid & 7) * 8;
            const float4 *src = (const float4 *)(T.dz1 + ((size_t)s * T.bpad_max + rb + r) * 64 + j0);
            const float4 x0 = src[0], x1 = src[1];
            float *dst = &dz_s[r * ZS + j0];
            dst[0] = x0.x; dst[1] = x0.y; dst[2] = x0.z; dst[3] = x0.w; dst[4] = x1.x; dst[5] = x1.y; dst[6] = x1.z; dst[7] = x1.w;
        }
        for (int e = tid; e < 32 * 10; e += PPT_T) {
            const int r = e / 10, q = e - r * 10;
            float x = 0.0f;
            if (rb + r < D.B) x = __half2float(D.row(rb + r, s, S, ow)[h * 5 + q]);
            ob_s[r * OS + q] = x;
        }
        __syncthreads();
        // dW1 += feat^T dz1 over the 32 rows, two per MFMA
#pragma unroll 4
        for (int kk = 0; kk < 16; ++kk) {
            const int rr = 2 * kk + g;
            const float *o = &ob_s[rr * OS + wA];
            const float f = fmaxf(ppt_conv(a_b, a_w0, a_w1, a_w2, a_w3, o[0], o[1], o[5], o[6]), 0.0f);
            accw0 = __builtin_amdgcn_mfma_f32_32x32x2f32(f, dz_s[rr * ZS + i], accw0, 0, 0, 0);
            accw1 = __builtin_amdgcn_mfma_f32_32x32x2f32(f, dz_s[rr * ZS + 32 + i], accw1, 0, 0, 0);
        }
        // dfeat[feature][row] = sum_j W1[feature][j] dz1[row][j]
        ppt_f16 accf = ppt_zero16();
#pragma unroll
        for (int jj = 0; jj < 32; ++jj) accf = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[jj], dz_s[i * ZS + 2 * jj + g], accf, 0, 0, 0);
        // conv gradients of row i: through the ReLU of the recomputed pre-activation
        float o[10];
        for (int q = 0; q < 10; ++q) o[q] = ob_s[i * OS + q];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float pre = ppt_conv(c_w[q][4], c_w[q][0], c_w[q][1], c_w[q][2], c_w[q][3], o[w], o[w + 1], o[5 + w], o[6 + w]);
                const float d = pre > 0.0f ? accf[q * 4 + w] : 0.0f;
                dconv[q][0] = fmaf(d, o[w], dconv[q][0]);
                dconv[q][1] = fmaf(d, o[w + 1], dconv[q][1]);
                dconv[q][2] = fmaf(d, o[5 + w], dconv[q][2]);
                dconv[q][3] = fmaf(d, o[6 + w], dconv[q][3]);
                dconv[q][4] += d;
            }
    }
    // the chunk's dW1 partial: C layout, column = output j, register r = feature (r & 3) + 8 (r >> 2) + 4 g
    {
        float *pw = T.pw1 + ((size_t)chunk * S + s) * H4 * 64 * 64;
        for (int r = 0; r < 16; ++r) {
            const int cC = cb * 32 + wv * 8 + 2 * (r >> 2) + g;
            float *dst = pw + ((size_t)cC * H4 + h * 4 + (r & 3)) * 64 + i;
            dst[0] = accw0[r];
            dst[32] = accw1[r];
        }
    }
    // the conv partial: lanes (rows) summed in ascending order
    for (int q = 0; q < 4; ++q)
        for (int e = 0; e < 5; ++e) red_s[(wv * 64 + lane) * 20 + q * 5 + e] = dconv[q][e];
    __syncthreads();
    if (tid < 4 * 2 * 20) {                         // (wave, half g, q * 5 + e)
        const int w_ = tid / 40, rem = tid - w_ * 40, g_ = rem / 20, qe = rem - g_ * 20;
        float acc = 0.0f;
        for (int l = 0; l < 32; ++l) acc += red_s[(w_ * 64 + g_ * 32 + l) * 20 + qe];
        const int cC = cb * 32 + w_ * 8 + 2 * (qe / 5) + g_;
        T.pconv[((((size_t)chunk * S + s) * T.H + h) * 64 + cC) * 5 + qe % 5] = acc;
    }
}
__global__ void __launch_bounds__(PPT_T) ppo_fc1_bwd_kernel(PpoTrainTab T, PpoBatch D) { ppt_fc1_bwd_body(T, D); }

// --------------------------------------------------------------------------------------------- 3. partials -> gradients, fixed order
// grid (S, H + ceil(PPT_N_SMALL / PPT_T)): part p < H = the fc1_w rows of conv row p, the others 256 small outputs each
__global__ void __launch_bounds__(PPT_T) ppo_reduce_kernel(PpoTrainTab T, int B, float *loss_out) {
    const int s = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const int hs = T.lanes[s] - 1, A = T.n_actions[s], amax = T.amax, H4 = T.H * 4, S = T.S;
    const int tiles = (B + PPT_TM - 1) / PPT_TM, chunks = (tiles * PPT_TM + PPT_CH - 1) / PPT_CH;
    if (p < T.H) {
        if (p >= hs) return;
        const size_t per = (size_t)H4 * 64 * 64;
        for (int e = tid; e < 64 * 4 * 64; e += PPT_T) {
            const int j = e & 63, w = (e >> 6) & 3, c = e >> 8;
            const size_t o = (size_t)s * per + ((size_t)c * H4 + p * 4 + w) * 64 + j;
            float acc = 0.0f;
            for (int ch = 0; ch < chunks; ++ch) acc += T.pw1[(size_t)ch * S * per + o];
            T.grad.p[PT_FC1_W][o] = acc;
        }
        return;
    }
    const int o = (p - T.H) * PPT_T + tid;
    if (o >= PPT_N_SMALL) return;
    if (o < PPT_P_SIZE) {
        float *dst = nullptr;
        if (o < PPT_P_B2) dst = T.grad.p[PT_FC2_W] + (size_t)s * 4096 + o;
        else if (o < PPT_P_W3) dst = T.grad.p[PT_FC2_B] + s * 64 + (o - PPT_P_B2);
        else if (o < PPT_P_B3) {
            const int k = (o - PPT_P_W3) / 9, a = (o - PPT_P_W3) - k * 9;
            if (a == 8) dst = T.grad.p[PT_V_W] + s * 64 + k;
            else if (a < A) dst = T.grad.p[PT_FC3_W] + ((size_t)s * 64 + k) * amax + a;
        } else if (o < PPT_P_B1) {
            const int a = o - PPT_P_B3;
            if (a == 8) dst = T.grad.p[PT_V_B] + s;
            else if (a < A) dst = T.grad.p[PT_FC3_B] + s * amax + a;
        } else if (o < PPT_P_LOSS) dst = T.grad.p[PT_FC1_B] + s * 64 + (o - PPT_P_B1);
        else if (o < PPT_P_LOSS + 3 && loss_out) dst = loss_out + s * 3 + (o - PPT_P_LOSS);
        if (!dst) return;
        const float *src = T.part + (size_t)s * T.tiles_max * PPT_P_SIZE + o;
        if (o >= PPT_P_LOSS) {
            float hi = 0.0f, lo = 0.0f;
            for (int t = 0; t < tiles; ++t) ppo_pair_add(&hi, &lo, src[(size_t)t * PPT_P_SIZE], src[(size_t)t * PPT_P_SIZE + 3]);
            *dst = (hi + lo) / (float)B;
            return;
        }
        float acc = 0.0f;
        for (int t = 0; t < tiles; ++t) acc += src[(size_t)t * PPT_P_SIZE];
        *dst = acc;
        return;
    }
    const int e = o - PPT_P_SIZE, c = e / 5, q = e - c * 5;
    float acc = 0.0f;
    for (int ch = 0; ch < chunks; ++ch)
        for (int h = 0; h < hs; ++h) acc += T.pconv[((((size_t)ch * S + s) * T.H + h) * 64 + c) * 5 + q];
    if (q < 4) T.grad.p[PT_CONV_W][((size_t)s * 64 + c) * 4 + q] = acc;
    else T.grad.p[PT_CONV_B][s * 64 + c] = acc;
}

// ------------------------------------------------------------------------------------------------------- 4. clip scale and Adam
// The elements of signal s in parts: p < H the fc1_w rows of conv row p (none when p >= hs), p == H every other tensor.  f(tensor,
// offset) is called for thread tid's elements tid, tid + PPT_T, .. of the part in ascending order; padded fc1 rows and fc3 columns
// are never visited.
template <class F> __device__ static inline void ppo_visit_part(const PpoTrainTab &T, int s, int p, int tid, F f) {
    const int hs = T.lanes[s] - 1, A = T.n_actions[s], amax = T.amax, H4 = T.H * 4;
    if (p < T.H) {
        if (p >= hs) return;
        for (int e = tid; e < 64 * 4 * 64; e += PPT_T)
            f(PT_FC1_W, (size_t)s * H4 * 4096 + ((size_t)(e >> 8) * H4 + p * 4 + ((e >> 6) & 3)) * 64 + (e & 63));
        return;
    }
    for (int e = tid; e < 256; e += PPT_T) f(PT_CONV_W, (size_t)s * 256 + e);
    for (int e = tid; e < 64; e += PPT_T) f(PT_CONV_B, (size_t)s * 64 + e);
    for (int e = tid; e < 64; e += PPT_T) f(PT_FC1_B, (size_t)s * 64 + e);
    for (int e = tid; e < 4096; e += PPT_T) f(PT_FC2_W, (size_t)s * 4096 + e);
    for (int e = tid; e < 64; e += PPT_T) f(PT_FC2_B, (size_t)s * 64 + e);
    for (int e = tid; e < 64 * A; e += PPT_T) f(PT_FC3_W, ((size_t)s * 64 + e / A) * amax + e % A);
    for (int e = tid; e < A; e += PPT_T) f(PT_FC3_B, (size_t)s * amax + e);
    for (int e = tid; e < 64; e += PPT_T) f(PT_V_W, (size_t)s * 64 + e);
    for (int e = tid; e < 1; e += PPT_T) f(PT_V_B, (size_t)s + e);
}

__global__ void __launch_bounds__(PPT_T) ppo_norm_kernel(PpoTrainTab T) {
    __shared__ float ph[PPT_T], pl[PPT_T];
    const int s = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    float hi = 0.0f, lo = 0.0f;
    ppo_visit_part(T, s, p, tid, [&](int t, size_t o) {
        const float g = T.grad.p[t][o], sq = g * g;
        ppo_pair_add(&hi, &lo, sq, fmaf(g, g, -sq));        // the product's own rounding error, exactly
    });
    ph[tid] = hi; pl[tid] = lo;
    __syncthreads();
    for (int off = PPT_T / 2; off > 0; off >>= 1) {
        if (tid < off) ppo_pair_add(&ph[tid], &pl[tid], ph[tid + off], pl[tid + off]);
        __syncthreads();
    }
    if (tid == 0) { T.sqpart[(s * (T.H + 1) + p) * 2] = ph[0]; T.sqpart[(s * (T.H + 1) + p) * 2 + 1] = pl[0]; }
}

__global__ void __launch_bounds__(PPT_T) ppo_adam_kernel(PpoTrainTab T, PpoStepConsts K) {
    const int s = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    float hi = 0.0f, lo = 0.0f;
    for (int q = 0; q <= T.H; ++q) ppo_pair_add(&hi, &lo, T.sqpart[(s * (T.H + 1) + q) * 2], T.sqpart[(s * (T.H + 1) + q) * 2 + 1]);
    const PpoPair scale = ppo_clip_scale(ppo_pair_norm(hi, lo), K);
    ppo_visit_part(T, s, p, tid, [&](int t, size_t o) {
        ppo_adam_element(&T.par.p[t][o], &T.m.p[t][o], &T.v.p[t][o], T.grad.p[t][o], scale, K);
    });
}
#endif
