// resco_fma2c_train.h -- the A2C update of FMA2C on the device for all K agents and N lock-step environments: returns and advantages,
// the re-run of the segment, the loss, BPTT through both LSTM nets, the per-agent global-norm clip and TF1's RMSProp
// (rs_fma2c_learn_* of include/resco_sim.h).  fp32 throughout; the squared norm in fp32 pairs, the optimiser's element step in double.
//
// What it replaces (resco_amd/agents/fma2c.py: A2CLearner.returns, .loss, torch.autograd.grad, .clip_scales, .rmsprop_step): a BPTT over
// up to 120 steps in eager PyTorch.  The arithmetic is A2CLearner's and tests/fma2c_ref.py: agent_loss_grads', which stay the
// specification; the forward of a step is the acting kernel's (resco_fma2c.h), phase for phase, on the same MFMA.
//
// Kernels of one rs_fma2c_learn_grad, in stream order:
//   ft_returns_kernel    one thread per (environment, agent) walks t backwards: r = clip(reward / norm), R_t = r_t + gamma R_{t+1}
//                        (1 - done_{t+1}), Adv = R - v
//   ft_transpose_kernel  wx^T and wh^T of every (agent, net), so that the backward's B operands are read along rows
//   per group of agents (as many as the workspace holds; blockIdx.y counts from k0):
//     ft_segment_kernel  grid (tiles of 32 environments) x (agents of the group) x (2 nets), 256 threads.  A workgroup owns its 32
//                        sequences for the whole segment: forward t = 0 .. T-1 (rows read, fc layers, z, gates, head, the row's loss
//                        gradient), then backward t = T-1 .. 0 (dh, the gates' backward, dz wx^T with the relu masks, dz wh^T).  What
//                        the weight gradients need goes to a workspace slot private to (agent, net, t, environment):
//                          hc 224 | da 224 (the fc layers' pre-activation gradients) | gates i f o u 256, overwritten by dz |
//                          c_in 64 | h 64 | h_in 64 | dout 8                                                        = FT_SLOT floats
//                        hc stays beside da (g_wx = hc^T dz reads it after the backward), so a slot is 3.6 KB, not 2.4 KB.
//     ft_wgrad_kernel    the weight gradients are sums over the T N rows: one wave per 32 x 32 tile of a gradient tensor and per split
//                        of the row range (a partition fixed by T N alone), the MFMA's operands read straight from the slots and the
//                        rows; bias gradients are the same product with a row of ones.  Each split writes its own partial tensor.
//   ft_reduce_kernel     sums the partials in split order into the gradient vector (the layout of Fma2cOff); ft_loss_kernel the losses
// No floating-point atomics anywhere: two runs, and any grouping of the agents, give the same bits.  A tile of a gradient that lies
// wholly in an agent's padding is written as zero without being multiplied; a partly padded tile multiplies masked (zero) operands.
//
// rs_fma2c_learn_step: ft_norm_kernel (the squared norm of an agent's gradients per (agent, tensor) in fp32 pairs) and
// ft_rmsprop_kernel (clip scale, ms, weights, in place on the packed vector the acting kernel reads).
#pragma once
#include "resco_fma2c.h"

#define FT_HC 0             // offsets in a workspace slot
#define FT_DA 224
#define FT_G 448
#define FT_CIN 704
#define FT_H 768
#define FT_HIN 832
#define FT_DO 896
#define FT_SLOT 904
#define FT_NT 11            // tensors of the packed vector
#define FT_PMAX 16          // most splits of the reduction length T N
#define FT_DS 65            // LDS row stride of dh_next

// ---------------------------------------------------------------------------------------------------------------- scalar pieces
// MA2CImplementation.add_transition (ma2c.py:220-225): r / reward_norm clipped to +-reward_clip (0: none of either)
RS_HD inline float ft_clip_reward(float r, float norm, float clip) {
    if (norm != 0.0f) r = r / norm;
    if (clip != 0.0f) r = r < -clip ? -clip : (r > clip ? clip : r);
    return r;
}
// OnPolicyBuffer._add_R_Adv (ma2c.py:586-598), one step: R_t = r_t + gamma R_{t+1} (1 - done_{t+1})
RS_HD inline float ft_return(float r, float R_next, float gamma, int done_next) { return r + gamma * R_next * (done_next ? 0.0f : 1.0f); }

// One row of one agent's policy net: d(loss)/d(logits) of -inv_nt log(clamp(pi, 1e-10, 1))[act] adv - entropy_coef inv_nt H, and the
// un-scaled terms -log(..)[act] adv and H.  The softmax is the acting kernel's.  Where pi < 1e-10 the clamp passes no gradient (m = 0).
RS_HD inline void ft_pi_row_grad(const float *logit, int n_a, int act, float adv, float inv_nt, float entropy_coef, float dlogit[FM_AMAX],
                                 float *term_pg, float *term_ent) {
    float pi[FM_AMAX], lp[FM_AMAX], m[FM_AMAX];
    float mx = logit[0];
    for (int a = 1; a < n_a; ++a) mx = logit[a] > mx ? logit[a] : mx;
    float s = 0.0f;
    for (int a = 0; a < n_a; ++a) { pi[a] = expf(logit[a] - mx); s += pi[a]; }
    float ent = 0.0f, sm = 0.0f;
    bool all = true;
    for (int a = 0; a < n_a; ++a) {
        pi[a] = pi[a] / s;
        m[a] = pi[a] < 1e-10f ? 0.0f : 1.0f;
        all = all && m[a] != 0.0f;
        lp[a] = logf(pi[a] < 1e-10f ? 1e-10f : (pi[a] > 1.0f ? 1.0f : pi[a]));
        ent -= pi[a] * lp[a];
        sm += pi[a] * m[a];
    }
    const float ca = adv * inv_nt * m[act], ce = entropy_coef * inv_nt;
    for (int a = 0; a < FM_AMAX; ++a) {
        if (a >= n_a) { dlogit[a] = 0.0f; continue; }
        const float onehot = a == act ? 1.0f : 0.0f;
        const float mt = all ? 0.0f : m[a] - sm;
        dlogit[a] = -ca * (onehot - pi[a]) + ce * pi[a] * ((lp[a] + ent) + mt);
    }
    *term_pg = -(lp[act] * adv);
    *term_ent = ent;
}
// ... and of its value net: d(0.5 value_coef inv_nt (R - v)^2)/dv and the un-scaled (R - v)^2
RS_HD inline void ft_v_row_grad(float v, float ret, float inv_nt, float value_coef, float *dv, float *term_vf) {
    const float d = v - ret;
    *dv = value_coef * d * inv_nt;
    *term_vf = d * d;
}
// the agent's loss from the sums of the three terms over its T N rows (the sums are carried in double: T N float32 terms)
RS_HD inline float ft_loss(double sum_pg, double sum_vf, double sum_ent, double nt, float value_coef, float entropy_coef) {
    return (float)(sum_pg / nt + 0.5 * (double)value_coef * (sum_vf / nt) - (double)entropy_coef * (sum_ent / nt));
}

// the gates of one unit with what the backward needs: g = sig(zi), sig(zf), sig(zo), tanh(zu); the expressions of fm_lstm_gate
RS_HD inline void ft_gate_fwd(float zi, float zf, float zo, float zu, float c_in, float g[4], float *c, float *h) {
    g[0] = fm_sigmoid(zi); g[1] = fm_sigmoid(zf); g[2] = fm_sigmoid(zo); g[3] = tanhf(zu);
    const float cn = g[1] * c_in + g[0] * g[3];
    *c = cn;
    *h = g[2] * tanhf(cn);
}
// ... and their backward (fma2c_ref.agent_loss_grads): dh = the head's and the next step's, dc_next the next step's; dz in gate order
// i f o u, dc_prev = dc f keep.  c is recomputed from the gates as the forward formed it, tanh(c) from that.
RS_HD inline void ft_gate_bwd(float dh, float dc_next, const float g[4], float c_in, float keep, float dz[4], float *dc_prev) {
    const float c = g[1] * c_in + g[0] * g[3], tc = tanhf(c);
    const float d_o = dh * tc;
    const float dc = dc_next + dh * g[2] * (1.0f - tc * tc);
    dz[0] = dc * g[3] * g[0] * (1.0f - g[0]);
    dz[1] = dc * c_in * g[1] * (1.0f - g[1]);
    dz[2] = d_o * g[2] * (1.0f - g[2]);
    dz[3] = dc * g[0] * (1.0f - g[3] * g[3]);
    *dc_prev = dc * g[1] * keep;
}

// TF1's RMSPropOptimizer without momentum on one element, formed in double and rounded once: ms <- alpha ms + (1 - alpha) g^2;
// w <- w - lr g / sqrt(ms + eps) (eps inside the root); g = the gradient times the clip scale
RS_HD inline void ft_rmsprop_element(float *w, float *ms, float g, float scale, double lr, double alpha, double eps) {
    const double gs = (double)g * (double)scale;
    const double m = alpha * (double)*ms + (1.0 - alpha) * gs * gs;
    *ms = (float)m;
    *w = (float)((double)*w - lr * gs / sqrt(m + eps));
}

// sizes of the eleven tensors per (agent, net), in the packed order
struct FtSizes {
    size_t sz, off;         // of tensor p (a chain of selects, not an indexed array: no scratch)
    RS_HD FtSizes(int K, int NS, int NW, int NF, int p) {
        const Fma2cOff o(K, NS, NW, NF);
        sz = p == 0 ? (size_t)NS * FM_FW : p == 1 ? FM_FW : p == 2 ? (size_t)NF * FM_FP : p == 3 ? FM_FP : p == 4 ? (size_t)NW * FM_FT : p == 5 ? FM_FT :
             p == 6 ? (size_t)FM_HID * 4 * FM_L : p == 7 ? (size_t)FM_L * 4 * FM_L : p == 8 ? 4 * FM_L : p == 9 ? FM_L * FM_AMAX : FM_AMAX;
        off = p == 0 ? o.fcw_w : p == 1 ? o.fcw_b : p == 2 ? o.fcf_w : p == 3 ? o.fcf_b : p == 4 ? o.fct_w : p == 5 ? o.fct_b : p == 6 ? o.wx : p == 7 ? o.wh :
              p == 8 ? o.lb : p == 9 ? o.head_w : o.head_b;
    }
};
// the fixed partition of the T N rows of a weight gradient: P splits of `per` rows (even: an MFMA step takes two rows)
RS_HD inline int ft_splits(long long R, int *per) {
    long long P = (R + 127) / 128;
    P = P < 1 ? 1 : (P > FT_PMAX ? FT_PMAX : P);
    long long q = (R + P - 1) / P;
    q = (q + 1) & ~1LL;
    *per = (int)q;
    return (int)((R + q - 1) / q);
}
// the 32 x 32 tiles of one (agent, net)'s gradients; the same list for every agent of a map
RS_HD inline int ft_jobs(int NS, int NW, int NF) {
    return 56 + 16 + 8 + ((NS + 31) / 32) * 4 + 4 + ((NF + 31) / 32) * 2 + 2 + ((NW + 31) / 32) + 1 + 2 + 1;
}

#if defined(__HIPCC__)
struct FtRun {              // one rs_fma2c_learn_grad
    const float *w;         // the learner's packed weights
    float *wT;              // [K][2]: wx^T [256][224], then [K][2]: wh^T [256][64]
    float *ws;              // [Kg][2][T N][FT_SLOT]
    float *part;            // [P][n] the partial gradients
    float *grad;            // [n]
    double *lossp;          // [tiles][K][2][3]
    const float *rows;      // [T][N][K][W]
    const int32_t *acts;    // [T][N][K]
    const float *rewards, *values, *R_boot;
    const int32_t *dones;   // [T + 1]
    const float *state0;    // [N][K][4][64]
    float *ret, *adv;       // [T][N][K]
    float gamma, reward_norm, reward_clip, value_coef, entropy_coef;
    int32_t T, N, k0, Kg, P, per;
    size_t n;               // floats of the packed vector
};

__global__ void ft_returns_kernel(Fma2cTab A, FtRun S) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, NK = S.N * A.K;
    if (idx >= NK) return;
    float R = S.R_boot[idx];
    for (int t = S.T - 1; t >= 0; --t) {
        const size_t q = (size_t)t * NK + idx;
        R = ft_return(ft_clip_reward(S.rewards[q], S.reward_norm, S.reward_clip), R, S.gamma, S.dones[t + 1]);
        S.ret[q] = R;
        S.adv[q] = R - S.values[q];
    }
}

__global__ void ft_transpose_kernel(Fma2cTab A, FtRun S) {
    const Fma2cOff o(A.K, A.NS, A.NW, A.NF);
    const size_t k2 = (size_t)A.K * 2, nx = k2 * FM_HID * 4 * FM_L, nh = k2 * FM_L * 4 * FM_L;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < nx) {
        const size_t kn = idx / (FM_HID * 4 * FM_L), q = idx - kn * (FM_HID * 4 * FM_L), c = q / FM_HID, r = q - c * FM_HID;
        S.wT[idx] = S.w[o.wx + kn * FM_HID * 4 * FM_L + r * 4 * FM_L + c];
    } else if (idx < nx + nh) {
        const size_t j = idx - nx, kn = j / (FM_L * 4 * FM_L), q = j - kn * (FM_L * 4 * FM_L), c = q / FM_L, r = q - c * FM_L;
        S.wT[idx] = S.w[o.wh + kn * FM_L * 4 * FM_L + r * 4 * FM_L + c];
    }
}

// ------------------------------------------------------------------------------------- the segment: forward, loss gradient, backward
__global__ void __launch_bounds__(256) ft_segment_kernel(Fma2cTab A, FtRun S) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 31, g = lane >> 5;
    const int kg = blockIdx.y, k = S.k0 + kg, net = blockIdx.z, e0 = blockIdx.x * FM_TM;
    const int N = S.N, T = S.T, K = A.K;
    const int rows = N - e0 < FM_TM ? N - e0 : FM_TM;
    const int n_a = A.n_a[k], n_s = A.n_s[k], n_w = A.n_w[k], n_f = A.n_f[k], W = n_s + n_w + n_f;
    const int n_in = n_w > 0 ? FM_HID : FM_FW + FM_FP, n_out = net == 0 ? n_a : 1;
    const int XS = A.W + 1;
    float *xs = (float *)RS_SMEM;                   // [32][XS] the input rows
    float *hc = xs + FM_TM * XS;                    // [32][FM_HS] fc outputs (224) | h (64)
    float *zz = hc + FM_TM * FM_HS;                 // [32][FM_ZS] LSTM pre-activations; the backward's dz
    float *lg = zz + FM_TM * FM_ZS;                 // [32][8] logits / the value in column 0
    float *dhn = lg + FM_TM * FM_AMAX;              // [32][FT_DS] dh_next
    const Fma2cOff o(K, A.NS, A.NW, A.NF);
    const size_t kn = (size_t)k * 2 + net, R = (size_t)T * N;
    float *slots = S.ws + ((size_t)kg * 2 + net) * R * FT_SLOT;
    const float *hw = S.w + o.head_w + kn * FM_L * FM_AMAX, *hb = S.w + o.head_b + kn * FM_AMAX;
    const float inv_nt = 1.0f / (float)((long long)T * N);
    const int u = tid & 63, rb = tid >> 6;          // the (row rb + 4 j, unit u) elements this thread owns for the whole segment

    float cr[8];                                    // c, then the backward's dc_next, of those elements
    for (int j = 0; j < 8; ++j) {
        const int r = rb + 4 * j;
        const float *st = S.state0 + (((size_t)(e0 + (r < rows ? r : 0)) * K + k) * 4 + 2 * net) * FM_L;
        cr[j] = r < rows ? st[u] : 0.0f;
        hc[r * FM_HS + FM_HID + u] = r < rows ? st[FM_L + u] : 0.0f;
    }
    double l0 = 0.0, l1 = 0.0;                      // thread r < rows: the sums of the row's loss terms over t
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const float keep = S.dones[t] ? 0.0f : 1.0f;
        // ---- 1. the input rows; the state times 1 - done_t
        for (int idx = tid; idx < FM_TM * A.W; idx += 256) {
            const int r = idx / A.W, j = idx - r * A.W;
            xs[r * XS + j] = (r < rows && j < W) ? S.rows[(((size_t)t * N + e0 + r) * K + k) * A.W + j] : 0.0f;
        }
        for (int j = 0; j < 8; ++j) {
            const int r = rb + 4 * j;
            cr[j] = cr[j] * keep;
            const float h = hc[r * FM_HS + FM_HID + u] * keep;
            hc[r * FM_HS + FM_HID + u] = h;
            if (r < rows) {
                float *sl = slots + ((size_t)t * N + e0 + r) * FT_SLOT;
                sl[FT_CIN + u] = cr[j];
                sl[FT_HIN + u] = h;
            }
        }
        __syncthreads();
        // ---- 2. the three fc layers (rs_fma2c_kernel, phase 2)
        for (int tl = wv; tl < 7; tl += 4) {
            if (tl == 6 && n_w == 0) continue;
            const int xoff = tl < 4 ? 0 : (tl < 6 ? n_s + n_w : n_s), nk = tl < 4 ? n_s : (tl < 6 ? n_f : n_w);
            const int ncols = tl < 4 ? FM_FW : (tl < 6 ? FM_FP : FM_FT), col = (tl < 4 ? tl : (tl < 6 ? tl - 4 : 0)) * 32 + i;
            const float *w = S.w + (tl < 4 ? o.fcw_w + kn * A.NS * FM_FW : (tl < 6 ? o.fcf_w + kn * A.NF * FM_FP : o.fct_w + kn * A.NW * FM_FT));
            const float b = S.w[(tl < 4 ? o.fcw_b + kn * FM_FW : (tl < 6 ? o.fcf_b + kn * FM_FP : o.fct_b + kn * FM_FT)) + col];
            fm_f16 acc;
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            for (int kk = 0; kk < nk; kk += 2) {
                const int kq = kk + g;
                const bool in = kq < nk;
                const float a = in ? xs[i * XS + xoff + kq] : 0.0f;
                const float bb = in ? w[(size_t)kq * ncols + col] : 0.0f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
            }
            for (int r = 0; r < 16; ++r) {
                const int rr = (r & 3) + 8 * (r >> 2) + 4 * g;
                const float v = fm_relu(acc[r] + b);
                hc[rr * FM_HS + tl * 32 + i] = v;
                if (rr < rows) slots[((size_t)t * N + e0 + rr) * FT_SLOT + FT_HC + tl * 32 + i] = v;
            }
        }
        __syncthreads();
        // ---- 3. z = hc wx + h wh + b (phase 3)
        {
            const float *wx = S.w + o.wx + kn * FM_HID * 4 * FM_L, *wh = S.w + o.wh + kn * FM_L * 4 * FM_L;
            const int c0 = wv * 32 + i, c1 = (wv + 4) * 32 + i;
            fm_f16 acc0, acc1;
            for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
            for (int kk = 0; kk < n_in; kk += 2) {
                const int kq = kk + g;
                const float a = hc[i * FM_HS + kq];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wx[(size_t)kq * 4 * FM_L + c0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wx[(size_t)kq * 4 * FM_L + c1], acc1, 0, 0, 0);
            }
#pragma unroll 4
            for (int kk = 0; kk < FM_L; kk += 2) {
                const int kq = kk + g;
                const float a = hc[i * FM_HS + FM_HID + kq];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wh[(size_t)kq * 4 * FM_L + c0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wh[(size_t)kq * 4 * FM_L + c1], acc1, 0, 0, 0);
            }
            const float b0 = S.w[o.lb + kn * 4 * FM_L + c0], b1 = S.w[o.lb + kn * 4 * FM_L + c1];
            for (int r = 0; r < 16; ++r) {
                const int rr = (r & 3) + 8 * (r >> 2) + 4 * g;
                zz[rr * FM_ZS + c0] = acc0[r] + b0;
                zz[rr * FM_ZS + c1] = acc1[r] + b1;
            }
        }
        __syncthreads();
        // ---- 4. the gates; the activated gates and the new h go to the slot
        for (int j = 0; j < 8; ++j) {
            const int r = rb + 4 * j;
            const float *z = zz + r * FM_ZS;
            float gt[4], c, h;
            ft_gate_fwd(z[u], z[FM_L + u], z[2 * FM_L + u], z[3 * FM_L + u], cr[j], gt, &c, &h);
            cr[j] = c;
            hc[r * FM_HS + FM_HID + u] = h;
            if (r < rows) {
                float *sl = slots + ((size_t)t * N + e0 + r) * FT_SLOT;
                for (int q = 0; q < 4; ++q) sl[FT_G + q * FM_L + u] = gt[q];
                sl[FT_H + u] = h;
            }
        }
        __syncthreads();
        // ---- 5. the head: thread (row, column)
        {
            const int r = tid >> 3, a = tid & 7;
            if (a < n_out) lg[r * FM_AMAX + a] = fm_head(hc + r * FM_HS + FM_HID, hw, a, hb[a]);
        }
        __syncthreads();
        // ---- 6. the row's loss gradient: one thread per row
        if (tid < rows) {
            const size_t q = ((size_t)t * N + e0 + tid) * K + k;
            float *sl = slots + ((size_t)t * N + e0 + tid) * FT_SLOT + FT_DO;
            if (net == 0) {
                float lgt[FM_AMAX], dl[FM_AMAX], tp, te;
                for (int a = 0; a < FM_AMAX; ++a) lgt[a] = a < n_a ? lg[tid * FM_AMAX + a] : 0.0f;
                int act = S.acts[q];
                act = act < 0 ? 0 : (act >= n_a ? n_a - 1 : act);
                ft_pi_row_grad(lgt, n_a, act, S.adv[q], inv_nt, S.entropy_coef, dl, &tp, &te);
                for (int a = 0; a < FM_AMAX; ++a) sl[a] = dl[a];
                l0 += tp; l1 += te;
            } else {
                float dv, tv;
                ft_v_row_grad(lg[tid * FM_AMAX], S.ret[q], inv_nt, S.value_coef, &dv, &tv);
                sl[0] = dv;
                for (int a = 1; a < FM_AMAX; ++a) sl[a] = 0.0f;
                l0 += tv;
            }
        }
        // the next step writes xs and this thread's own h; lg is written again three barriers from here
    }
    __syncthreads();
    // ---- the tile's loss terms (net 0: policy term, entropy; net 1: squared value error), rows in order
    double *ls = (double *)zz;
    if (tid < FM_TM) { ls[tid * 2] = tid < rows ? l0 : 0.0; ls[tid * 2 + 1] = tid < rows ? l1 : 0.0; }
    __syncthreads();
    if (tid < 2) {
        double a = 0.0;
        for (int r = 0; r < FM_TM; ++r) a += ls[r * 2 + tid];
        S.lossp[(((size_t)blockIdx.x * K + k) * 2 + net) * 3 + tid] = a;
    }
    __syncthreads();

    // ---- backward
    for (int j = 0; j < 8; ++j) { cr[j] = 0.0f; dhn[(rb + 4 * j) * FT_DS + u] = 0.0f; }
    const float *wxT = S.wT + kn * FM_HID * 4 * FM_L, *whT = S.wT + (size_t)K * 2 * FM_HID * 4 * FM_L + kn * FM_L * 4 * FM_L;
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        const float keep = S.dones[t] ? 0.0f : 1.0f;
        // ---- a. dh = dout head_w^T + dh_next, the gates' backward; dz over the slot's gates and into LDS
        for (int j = 0; j < 8; ++j) {
            const int r = rb + 4 * j;
            float dz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (r < rows) {
                float *sl = slots + ((size_t)t * N + e0 + r) * FT_SLOT;
                float dh = 0.0f;
                for (int a = 0; a < n_out; ++a) dh += sl[FT_DO + a] * hw[u * FM_AMAX + a];
                dh += dhn[r * FT_DS + u];
                float gt[4];
                for (int q = 0; q < 4; ++q) gt[q] = sl[FT_G + q * FM_L + u];
                float dcp;
                ft_gate_bwd(dh, cr[j], gt, sl[FT_CIN + u], keep, dz, &dcp);
                cr[j] = dcp;
                for (int q = 0; q < 4; ++q) sl[FT_G + q * FM_L + u] = dz[q];
            }
            for (int q = 0; q < 4; ++q) zz[r * FM_ZS + q * FM_L + u] = dz[q];
        }
        __syncthreads();
        // ---- b. dhc = dz wx^T with the relu masks (7 column tiles; a manager: 6), dh_next = (dz wh^T) keep (2 tiles)
        for (int tl = wv; tl < 9; tl += 4) {
            if (tl == 6 && n_w == 0) continue;
            const float *bt = tl < 7 ? wxT + tl * 32 + i : whT + (tl - 7) * 32 + i;
            const int ld = tl < 7 ? FM_HID : FM_L;
            fm_f16 acc;
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll 4
            for (int kk = 0; kk < 4 * FM_L; kk += 2) {
                const int kq = kk + g;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(zz[i * FM_ZS + kq], bt[(size_t)kq * ld], acc, 0, 0, 0);
            }
            for (int r = 0; r < 16; ++r) {
                const int rr = (r & 3) + 8 * (r >> 2) + 4 * g;
                if (tl >= 7) dhn[rr * FT_DS + (tl - 7) * 32 + i] = acc[r] * keep;
                else if (rr < rows) {
                    float *sl = slots + ((size_t)t * N + e0 + rr) * FT_SLOT;
                    sl[FT_DA + tl * 32 + i] = sl[FT_HC + tl * 32 + i] > 0.0f ? acc[r] : 0.0f;
                }
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------ the weight gradients
// One wave per (32 x 32 tile of a gradient tensor, split of the rows): G[a][b] = sum over the rows of A[row][a] B[row][b].
struct FtJob {
    int a_kind;             // 0: a slot column, 1: an input column, 2: ones in row 0 (a bias)
    int a_off, a_n;         // first column and how many of the 32 are the agent's
    int b_off, b_n;         // the slot column of B and how many of the 32 are live
    size_t out;             // offset of the tile's element (0, 0) in the packed vector
    int ld, m_n, n_n;       // the tensor's row length, and the tile's rows and columns that lie inside the PADDED tensor
};

__device__ inline FtJob ft_job(const Fma2cTab &A, const Fma2cOff &o, int k, int net, int job) {
    const int n_a = A.n_a[k], n_s = A.n_s[k], n_w = A.n_w[k], n_f = A.n_f[k];
    const size_t kn = (size_t)k * 2 + net;
    const int TS = (A.NS + 31) / 32, TF = (A.NF + 31) / 32, TW = (A.NW + 31) / 32;
    const int n_in = n_w > 0 ? FM_HID : FM_FW + FM_FP, n_out = net == 0 ? n_a : 1;
    auto lim = [](int n, int at) { const int v = n - at * 32; return v < 0 ? 0 : (v > 32 ? 32 : v); };
    FtJob J{};
    int j = job;
    if (j < 56) {           // wx [224][256]
        const int at = j >> 3, bt = j & 7;
        J = FtJob{0, FT_HC + at * 32, lim(n_in, at), FT_G + bt * 32, 32, o.wx + kn * FM_HID * 4 * FM_L + (size_t)at * 32 * 4 * FM_L + bt * 32, 4 * FM_L, 32, 32};
        return J;
    }
    j -= 56;
    if (j < 16) {           // wh [64][256]
        const int at = j >> 3, bt = j & 7;
        return FtJob{0, FT_HIN + at * 32, 32, FT_G + bt * 32, 32, o.wh + kn * FM_L * 4 * FM_L + (size_t)at * 32 * 4 * FM_L + bt * 32, 4 * FM_L, 32, 32};
    }
    j -= 16;
    if (j < 8) return FtJob{2, 0, 1, FT_G + j * 32, 32, o.lb + kn * 4 * FM_L + j * 32, 4 * FM_L, 1, 32};
    j -= 8;
    if (j < TS * 4) {       // fcw_w [NS][128]
        const int at = j >> 2, bt = j & 3;
        return FtJob{1, at * 32, lim(n_s, at), FT_DA + bt * 32, 32, o.fcw_w + kn * A.NS * FM_FW + (size_t)at * 32 * FM_FW + bt * 32, FM_FW, lim(A.NS, at), 32};
    }
    j -= TS * 4;
    if (j < 4) return FtJob{2, 0, 1, FT_DA + j * 32, 32, o.fcw_b + kn * FM_FW + j * 32, FM_FW, 1, 32};
    j -= 4;
    if (j < TF * 2) {       // fcf_w [NF][64]
        const int at = j >> 1, bt = j & 1;
        return FtJob{1, n_s + n_w + at * 32, lim(n_f, at), FT_DA + FM_FW + bt * 32, 32, o.fcf_w + kn * A.NF * FM_FP + (size_t)at * 32 * FM_FP + bt * 32, FM_FP, lim(A.NF, at), 32};
    }
    j -= TF * 2;
    if (j < 2) return FtJob{2, 0, 1, FT_DA + FM_FW + j * 32, 32, o.fcf_b + kn * FM_FP + j * 32, FM_FP, 1, 32};
    j -= 2;
    if (j < TW)             // fct_w [NW][32]
        return FtJob{1, n_s + j * 32, lim(n_w, j), FT_DA + FM_FW + FM_FP, 32, o.fct_w + kn * A.NW * FM_FT + (size_t)j * 32 * FM_FT, FM_FT, lim(A.NW, j), 32};
    j -= TW;
    if (j < 1) return FtJob{2, 0, n_w > 0 ? 1 : 0, FT_DA + FM_FW + FM_FP, 32, o.fct_b + kn * FM_FT, FM_FT, 1, 32};
    j -= 1;
    if (j < 2) return FtJob{0, FT_H + j * 32, 32, FT_DO, n_out, o.head_w + kn * FM_L * FM_AMAX + (size_t)j * 32 * FM_AMAX, FM_AMAX, 32, FM_AMAX};
    return FtJob{2, 0, 1, FT_DO, n_out, o.head_b + kn * FM_AMAX, FM_AMAX, 1, FM_AMAX};
}

__global__ void __launch_bounds__(256) ft_wgrad_kernel(Fma2cTab A, FtRun S) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 31, g = lane >> 5;
    const int job = blockIdx.x * 4 + wv;
    if (job >= ft_jobs(A.NS, A.NW, A.NF)) return;
    const int kg = blockIdx.y >> 1, net = blockIdx.y & 1, k = S.k0 + kg, p = blockIdx.z;
    const Fma2cOff o(A.K, A.NS, A.NW, A.NF);
    const FtJob J = ft_job(A, o, k, net, job);
    const long long R = (long long)S.T * S.N;
    const long long r0 = (long long)p * S.per, r1 = r0 + S.per < R ? r0 + S.per : R;
    const float *slots = S.ws + ((size_t)kg * 2 + net) * (size_t)R * FT_SLOT;
    fm_f16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    if (J.a_n > 0 && J.b_n > 0) {
        const bool a_in = i < J.a_n, b_in = i < J.b_n;
        for (long long r = r0; r < r1; r += 2) {
            const long long rr = r + g;
            const bool in = rr < r1;
            const float *sl = slots + (size_t)(in ? rr : r) * FT_SLOT;
            float a = 0.0f, b = 0.0f;
            if (in && a_in) a = J.a_kind == 0 ? sl[J.a_off + i] : (J.a_kind == 1 ? S.rows[((size_t)rr * A.K + k) * A.W + J.a_off + i] : 1.0f);
            if (in && b_in) b = sl[J.b_off + i];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    float *out = S.part + (size_t)p * S.n + J.out;
    if (i < J.n_n)
        for (int r = 0; r < 16; ++r) {
            const int m = (r & 3) + 8 * (r >> 2) + 4 * g;
            if (m < J.m_n) out[(size_t)m * J.ld + i] = acc[r];
        }
}

__global__ void ft_reduce_kernel(FtRun S) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= S.n) return;
    float acc = 0.0f;
    for (int p = 0; p < S.P; ++p) acc += S.part[(size_t)p * S.n + idx];
    S.grad[idx] = acc;
}

__global__ void ft_loss_kernel(Fma2cTab A, FtRun S, float *loss_out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.K) return;
    const int tiles = (S.N + FM_TM - 1) / FM_TM;
    double pg = 0.0, ent = 0.0, vf = 0.0;
    for (int t = 0; t < tiles; ++t) {
        const double *lp = S.lossp + ((size_t)t * A.K + k) * 6;
        pg += lp[0]; ent += lp[1]; vf += lp[3];
    }
    loss_out[k] = ft_loss(pg, vf, ent, (double)((long long)S.T * S.N), S.value_coef, S.entropy_coef);
}

// ------------------------------------------------------------------------------------------------------- norm, clip scale, RMSProp
struct FtStep {
    float *w, *ms, *sqpart, *norms, *scales;    // sqpart [K][FT_NT][hi, lo]; norms, scales [K]
    const float *grad;
    double lr, alpha, eps, max_grad_norm;
};

__global__ void __launch_bounds__(256) ft_norm_kernel(Fma2cTab A, FtStep Q) {
    __shared__ float ph[256], pl[256];
    const int k = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const FtSizes z(A.K, A.NS, A.NW, A.NF, p);
    const float *gq = Q.grad + z.off + (size_t)k * 2 * z.sz;
    float hi = 0.0f, lo = 0.0f;
    for (size_t q = tid; q < 2 * z.sz; q += 256) {
        const float v = gq[q], sq = v * v;
        ppo_pair_add(&hi, &lo, sq, fmaf(v, v, -sq));        // the product's own rounding error, exactly
    }
    ph[tid] = hi; pl[tid] = lo;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) ppo_pair_add(&ph[tid], &pl[tid], ph[tid + off], pl[tid + off]);
        __syncthreads();
    }
    if (tid == 0) { Q.sqpart[(k * FT_NT + p) * 2] = ph[0]; Q.sqpart[(k * FT_NT + p) * 2 + 1] = pl[0]; }
}

__global__ void __launch_bounds__(256) ft_rmsprop_kernel(Fma2cTab A, FtStep Q) {
    const int k = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    float hi = 0.0f, lo = 0.0f;
    for (int q = 0; q < FT_NT; ++q) ppo_pair_add(&hi, &lo, Q.sqpart[(k * FT_NT + q) * 2], Q.sqpart[(k * FT_NT + q) * 2 + 1]);
    const double norm = sqrt((double)hi + (double)lo);
    const float scale = Q.max_grad_norm > 0.0 ? (float)(Q.max_grad_norm / (norm > Q.max_grad_norm ? norm : Q.max_grad_norm)) : 1.0f;
    if (p == 0 && blockIdx.z == 0 && tid == 0) { Q.norms[k] = (float)norm; Q.scales[k] = scale; }
    const FtSizes z(A.K, A.NS, A.NW, A.NF, p);
    const size_t base = z.off + (size_t)k * 2 * z.sz;
    for (size_t q = (size_t)blockIdx.z * 256 + tid; q < 2 * z.sz; q += (size_t)gridDim.z * 256)
        ft_rmsprop_element(Q.w + base + q, Q.ms + base + q, Q.grad[base + q], scale, Q.lr, Q.alpha, Q.eps);
}
#endif
