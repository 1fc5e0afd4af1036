// resco_ppo_train.h -- the PPO update of the S stacked actor-critics on the device: loss, backward, per-signal gradient clipping
// and Adam (rs_ppo_create / rs_ppo_grad / rs_ppo_step / rs_ppo_fit of include/resco_sim.h).
//
// What it replaces (resco_amd/agents/ippo.py: BatchedPPOLearner.loss, .clip_grad_per_signal, torch.optim.Adam inside ._fit): per
// Adam step ~200 small launches of the batched PyTorch learner, which pads every signal to lmax lanes.  Here every signal runs at
// its own lane count and action count; all arithmetic is fp32.
//
// The network, its forward and backward, the reduction and the Adam body are resco_train.h's, with NH = 9 head columns (8 policy
// columns and the value in column 8) and NL = 3 loss terms.  This file adds the per-row loss gradient (ppo_row_loss_grad, an
// RS_PPO_HD function that tests/ppo_train_host builds for the host as well), the minibatch (rows gathered through idx: row i is
// dataset row idx[i]) and the kernels: of one minibatch gradient (rs_ppo_grad) ppo_fwd_bwd_kernel, ppo_fc1_bwd_kernel and
// ppo_reduce_kernel; of one optimiser step (rs_ppo_step) ppo_norm_kernel (the squared gradient norm per (signal, part): PPT_T strided
// partial sums and a halving tree, of fp32 pairs) and ppo_adam_kernel (clip scale + Adam).
#pragma once
#include "resco_train.h"

#define PPO_NH (PPT_AMAX + 1)   // head columns of a tile: the policy's, then the value
#define PPO_NL 3                // loss terms of a row: pg, vf, ent

// what the gradient kernels read of rs_ppo_config (the optimiser's constants: PpoStepConsts of resco_train.h)
struct PpoHyper { float clip_eps, entropy_coef, value_coef; };

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

#ifdef __HIPCC__
struct PpoTrainTab : PptTab {
    PpoHyper hp;
    float *sqpart;                          // [S][H + 1][hi, lo]
};

struct PpoBatch {
    const __half *obs;                      // [n][S][lmax][5]
    const int32_t *act;                     // [n][S]
    const float *logp, *adv, *ret;          // [n][S]
    const int32_t *idx;                     // [B]
    int32_t B;
    __device__ long long src(int i, int, int) const { return idx[i]; }
};

// ------------------------------------------------------------------------------------- 1. forward, loss, backward to dz1, per tile
__global__ void __launch_bounds__(PPT_T) ppo_fwd_bwd_kernel(PpoTrainTab T, PpoBatch D) {
    __shared__ PptTileLds<PPO_NH> L;
    __shared__ float dl_s[PPT_TM * PPO_NH], lt_s[PPT_TM * PPO_NL];
    const PptTile X = ppt_tile(T, D.B);
    const int tid = X.tid, S = T.S, s = X.s, A = X.A;
    if (tid < PPT_TM) L.src[tid] = tid < X.nrows ? D.src(X.r0 + tid, s, S) : -1;
    __syncthreads();
    ppt_tile_load(T.par, T, X, D.obs, L);
    __syncthreads();
    ppt_tile_forward(T.par, T, X, L);
    // ---- the loss gradient of every row; rows past the minibatch contribute nothing
    if (tid < PPT_TM) {
        float dl[PPT_AMAX], dv = 0.0f, tm[PPO_NL] = {0.0f, 0.0f, 0.0f};
        for (int a = 0; a < PPT_AMAX; ++a) dl[a] = 0.0f;
        if (tid < X.nrows) {
            const size_t smp = (size_t)L.src[tid] * S + s;
            float lg[PPT_AMAX];
            for (int a = 0; a < PPT_AMAX; ++a) lg[a] = a < A ? L.lg[tid * PPO_NH + a] : 0.0f;
            int act = D.act[smp];
            act = act < 0 ? 0 : (act >= A ? A - 1 : act);
            ppo_row_loss_grad(lg, A, L.lg[tid * PPO_NH + PPT_AMAX], act, D.logp[smp], D.adv[smp], D.ret[smp], 1.0f / (float)D.B, T.hp.clip_eps,
                              T.hp.entropy_coef, T.hp.value_coef, dl, &dv, tm);
        }
        for (int a = 0; a < PPT_AMAX; ++a) dl_s[tid * PPO_NH + a] = a < A ? dl[a] : 0.0f;
        dl_s[tid * PPO_NH + PPT_AMAX] = dv;
        for (int q = 0; q < PPO_NL; ++q) lt_s[tid * PPO_NL + q] = tm[q];
    }
    __syncthreads();
    ppt_tile_backward<PPO_NH, PPO_NL>(T, X, L, dl_s, lt_s);
}

__global__ void __launch_bounds__(PPT_T) ppo_fc1_bwd_kernel(PpoTrainTab T, PpoBatch D) { ppt_fc1_bwd_body(T, D); }
__global__ void __launch_bounds__(PPT_T) ppo_reduce_kernel(PpoTrainTab T, int B, float *loss_out) { ppt_reduce_body<PPO_NH, PPO_NL>(T, B, loss_out); }

// ------------------------------------------------------------------------------------------------------- 2. clip scale and Adam
__global__ void __launch_bounds__(PPT_T) ppo_norm_kernel(PpoTrainTab T) {
    __shared__ float ph[PPT_T], pl[PPT_T];
    const int s = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    float hi = 0.0f, lo = 0.0f;
    ppt_visit_part<PPO_NH>(T, s, p, tid, [&](int t, size_t o) {
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
    const int s = blockIdx.x;
    float hi = 0.0f, lo = 0.0f;
    for (int q = 0; q <= T.H; ++q) ppo_pair_add(&hi, &lo, T.sqpart[(s * (T.H + 1) + q) * 2], T.sqpart[(s * (T.H + 1) + q) * 2 + 1]);
    ppt_adam_body<PPO_NH>(T, K, ppo_clip_scale(ppo_pair_norm(hi, lo), K));
}
#endif
