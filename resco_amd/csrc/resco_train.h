// resco_train.h -- what the fused learner updates share: the trunk of the S stacked per-signal networks, forward and backward, the
// fixed-order reduction of its gradients and Adam.  resco_ppo_train.h (actor-critic: 8 policy columns + the value column) and
// resco_dqn_train.h (Q-network: 8 Q columns) add their loss, their minibatch and thin __global__ wrappers around the bodies here.
//
// The network of one signal (BatchedIPPO's / BatchedIDQN's layouts, all fp32, updated in place), at its own lane count L_s
// (hs = L_s - 1 rows of conv output) and action count A_s:
//     obs f16 [L][5] -> conv 2x2, 64 channels, ReLU -> feat[k], k = c * (H * 4) + h * 4 + w  (H = lmax - 1; only h < hs is real)
//     z1 = b1 + feat W1 [K][64], ReLU;  z2 = b2 + a1 W2 [64][64], ReLU;  heads = b3 + a2 W3 [64][amax]  (+ value = bv + a2 Wv [64][1])
// NH = the head columns of a tile: PPT_AMAX, + 1 with a value head (then column PPT_AMAX); NL = the loss terms a row reports.
//
// The stages of one minibatch gradient, rows gathered inside the kernels (a Batch says where row i of signal s lies: Batch::src):
//   1. per (64-row tile, signal), ppt_tile_load / ppt_tile_forward / the learner's per-row loss gradient / ppt_tile_backward: fc1
//      forward on v_mfma_f32_32x32x2_f32 with the conv features formed in registers as the A operand; fc2, heads; backward to dz1
//      (written to the workspace, zero for the rows a short last tile pads) and the tile's partial sums of the small layers' gradients.
//   2. per (signal, 128-feature block = conv row h x half the channels, chunk of PPT_CH rows), ppt_fc1_bwd_body: recomputes the
//      features, dW1 = feat^T dz1 and dfeat = W1 dz1^T on the same MFMA, the conv gradients from dfeat.
//   3. ppt_reduce_body: partials -> gradients, chunks / tiles in ascending order.
// and of one optimiser step: ppt_adam_body (the clip scale of the caller, then ppo_adam_element) over ppt_visit_part.
//
// Every sum has ONE order, fixed by the shapes alone: an MFMA accumulator is a k-ordered fmaf chain; rows are summed in ascending
// order inside a tile / chunk, then tiles / chunks in ascending order.  No floating-point atomics: two runs from the same state give
// the same bits.  Padded fc1_w rows and fc3 columns are never read or written.
//
// The scalar pieces (fp32 pairs, clip scale, Adam element update) are RS_PPO_HD functions in plain C++ that a host compiler builds
// as well (tests/ppo_train_host, tests/dqn_train_host).
#pragma once
#include "resco_ppo.h"

#define PPT_NT 10           // tensors of a BatchedIPPO, in rs_ppo_tensors order; a BatchedIDQN has the first eight (rs_dqn_tensors)
enum { PT_CONV_W = 0, PT_CONV_B, PT_FC1_W, PT_FC1_B, PT_FC2_W, PT_FC2_B, PT_FC3_W, PT_FC3_B, PT_V_W, PT_V_B };
#define PPT_AMAX 8          // actions per signal at most (POL_QMAX)
#define PPT_TM 64           // rows of a forward / backward tile
#define PPT_CH 512          // rows of a chunk of the fc1 backward (a multiple of PPT_TM)
#define PPT_T 256           // threads of every workgroup here

struct PptTensors { float *p[PPT_NT]; };        // PT_V_W, PT_V_B: NULL in a network without the value head

// per-tile partial sums of the small layers, floats from the tile's base
constexpr int PPT_P_W2 = 0;                                     // [64 k][64 j]
constexpr int PPT_P_B2 = 4096;                                  // [64]
constexpr int PPT_P_W3 = 4160;                                  // [64 k][NH]: columns 0 .. A_s - 1, the value head in column PPT_AMAX
constexpr int ppt_p_b3(int NH) { return PPT_P_W3 + 64 * NH; }   // [NH] (up to 16)
constexpr int ppt_p_b1(int NH) { return ppt_p_b3(NH) + 16; }    // [64]
constexpr int ppt_p_loss(int NH) { return ppt_p_b1(NH) + 64; }  // the NL loss terms as (hi, lo) pairs: NL hi, NL lo (up to 16)
constexpr int ppt_p_size(int NH) { return ppt_p_loss(NH) + 16; }
constexpr int ppt_n_small(int NH) { return ppt_p_size(NH) + 320; }      // outputs of the reduction beyond fc1_w: the tile partials, then conv [64 c][5]

// ---------------------------------------------------------------------------------------------------------------- scalar pieces
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

// what the table of either learner starts with (PpoTrainTab, DqnTrainTab derive from it)
struct PptTab {
    int32_t S, lmax, amax, H;               // H = lmax - 1
    const int32_t *lanes, *n_actions;       // device [S]
    PptTensors par, grad, m, v;
    int32_t bpad_max;                       // rows of the dz1 workspace per signal (the largest minibatch rounded up to PPT_TM)
    int32_t tiles_max, chunks_max;
    float *dz1;                             // [S][bpad_max][64]
    float *part;                            // [S][tiles_max][ppt_p_size(NH)]
    float *pw1;                             // [chunks_max][S][H * 256][64]
    float *pconv;                           // [chunks_max][S][H][64][5]
};

// A minibatch type (PpoBatch, DqnBatch) has obs (f16 rows of [S][lmax][5]), B and src(i, s, S): the row of obs that holds row i of
// signal s.

constexpr int PPT_OS = 85, PPT_ZS = 65;     // LDS strides of an observation row and of a row of 64 activations
// the LDS of a tile workgroup's forward
template <int NH> struct PptTileLds {
    float buf[PPT_TM * PPT_OS];             // observations, later dz2, later dz1 (both with stride PPT_ZS)
    float a1[PPT_TM * PPT_ZS], a2[PPT_TM * PPT_ZS];     // relu(z1), relu(z2)
    alignas(16) float cw[64 * 8];           // conv weights [c][w00 w01 w10 w11 b . . .]
    float lg[PPT_TM * NH];                  // the heads [row][NH]
    long long src[PPT_TM];                  // the row of obs that tile row r reads, < 0 = none (zeros)
};
// where a tile workgroup stands: grid (tiles, S)
struct PptTile { int tid, lane, wv, tile, s, hs, A, r0, nrows; };
__device__ __forceinline__ PptTile ppt_tile(const PptTab &T, int B) {
    const int tid = threadIdx.x, tile = blockIdx.x, s = blockIdx.y, r0 = tile * PPT_TM;
    return PptTile{tid, tid & 63, __builtin_amdgcn_readfirstlane(tid >> 6), tile, s, T.lanes[s] - 1, T.n_actions[s], r0, min(PPT_TM, B - r0)};
}

__device__ static inline ppt_f16 ppt_zero16() { ppt_f16 z; for (int i = 0; i < 16; ++i) z[i] = 0.0f; return z; }
__device__ static inline float ppt_conv(float b, float w0, float w1, float w2, float w3, float o00, float o01, float o10, float o11) {
    return fmaf(w3, o11, fmaf(w2, o10, fmaf(w1, o01, fmaf(w0, o00, b))));
}

// ------------------------------------------------------------------------------------------------- 1. a 64-row tile of one signal
// the rows L.src names and the conv weights of `par` into LDS; the caller puts a barrier before (L.src) and after
template <int NH> __device__ __forceinline__ void ppt_tile_load(const PptTensors &par, const PptTab &T, const PptTile &X, const __half *obs, PptTileLds<NH> &L) {
    const int ow = T.lmax * 5, s = X.s;
    for (int e = X.tid; e < PPT_TM * ow; e += PPT_T) {
        const int r = e / ow, q = e - r * ow;
        const long long src = L.src[r];
        L.buf[r * PPT_OS + q] = src < 0 ? 0.0f : __half2float(obs[((size_t)src * T.S + s) * ow + q]);
    }
    for (int e = X.tid; e < 64 * 8; e += PPT_T) {
        const int c = e >> 3, q = e & 7;
        L.cw[e] = q < 4 ? par.p[PT_CONV_W][((size_t)s * 64 + c) * 4 + q] : (q == 4 ? par.p[PT_CONV_B][s * 64 + c] : 0.0f);
    }
}

// the forward of the network `par` on the loaded tile: leaves relu(z1) in L.a1, relu(z2) in L.a2, the signal's own A head columns in
// L.lg[row * NH + a] and, with a value head, the value in column PPT_AMAX.  Ends with a barrier.
template <int NH> __device__ __forceinline__ void ppt_tile_forward(const PptTensors &par, const PptTab &T, const PptTile &X, PptTileLds<NH> &L) {
    constexpr int OS = PPT_OS, ZS = PPT_ZS;
    const int lane = X.lane, wv = X.wv, s = X.s, amax = T.amax, H4 = T.H * 4;
    // ---- fc1: wave wv owns rows (wv & 1) * 32 .. + 31 and outputs (wv >> 1) * 32 .. + 31; k order h, w, c; one accumulator per w
    {
        const int i = lane & 31, g = lane >> 5, mt = wv & 1, nt = wv >> 1, row = mt * 32 + i;
        const float *w1 = par.p[PT_FC1_W] + (size_t)s * H4 * 64 * 64 + nt * 32 + i;
        ppt_f16 acc[4];
        for (int w = 0; w < 4; ++w) acc[w] = ppt_zero16();
        for (int h = 0; h < X.hs; ++h) {
            float o[2][5];
            for (int q = 0; q < 5; ++q) { o[0][q] = L.buf[row * OS + h * 5 + q]; o[1][q] = L.buf[row * OS + h * 5 + 5 + q]; }
#pragma unroll 4
            for (int c = 0; c < 64; c += 2) {
                const int cc = c + g;
                const float4 cw = *(const float4 *)&L.cw[cc * 8];
                const float cb = L.cw[cc * 8 + 4];
                const float *wk = w1 + ((size_t)cc * H4 + h * 4) * 64;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const float f = fmaxf(ppt_conv(cb, cw.x, cw.y, cw.z, cw.w, o[0][w], o[0][w + 1], o[1][w], o[1][w + 1]), 0.0f);
                    acc[w] = __builtin_amdgcn_mfma_f32_32x32x2f32(f, wk[w * 64], acc[w], 0, 0, 0);
                }
            }
        }
        const float b1 = par.p[PT_FC1_B][s * 64 + nt * 32 + i];
        for (int r = 0; r < 16; ++r) {
            const int rr = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
            const float z = ((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r])) + b1;
            L.a1[rr * ZS + nt * 32 + i] = fmaxf(z, 0.0f);
        }
    }
    __syncthreads();
    const int row = lane, kg = wv * 16;             // the small layers: a thread owns one row and 16 wave-uniform columns
    // ---- fc2
    {
        const float *w2 = par.p[PT_FC2_W] + (size_t)s * 4096 + kg;
        float z[16];
        for (int j = 0; j < 16; ++j) z[j] = par.p[PT_FC2_B][s * 64 + kg + j];
        for (int k = 0; k < 64; ++k) {
            const float a = L.a1[row * ZS + k];
            for (int j = 0; j < 16; ++j) z[j] = fmaf(a, w2[k * 64 + j], z[j]);
        }
        for (int j = 0; j < 16; ++j) L.a2[row * ZS + kg + j] = fmaxf(z[j], 0.0f);
    }
    __syncthreads();
    // ---- heads: wave wv computes columns wv, wv + 4 of the signal's own A and (wave 0) the value
    for (int a = wv; a < X.A; a += 4) {
        const float *wc = par.p[PT_FC3_W] + (size_t)s * 64 * amax + a;
        float z = par.p[PT_FC3_B][s * amax + a];
        for (int k = 0; k < 64; ++k) z = fmaf(L.a2[row * ZS + k], wc[k * amax], z);
        L.lg[row * NH + a] = z;
    }
    if constexpr (NH > PPT_AMAX) {
        if (wv == 0) {
            const float *wc = par.p[PT_V_W] + (size_t)s * 64;
            float z = par.p[PT_V_B][s];
            for (int k = 0; k < 64; ++k) z = fmaf(L.a2[row * ZS + k], wc[k], z);
            L.lg[row * NH + PPT_AMAX] = z;
        }
    }
    __syncthreads();
}

// the backward of the tile from the rows' head gradients dl_s [row][NH] (zero for padded actions and for rows past the minibatch;
// with a value head d(loss)/d(value) in column PPT_AMAX) and loss terms lt_s [row][NL]: dz1 to the workspace and the tile's partial
// sums.  The caller puts a barrier between writing dl_s / lt_s and this.
template <int NH, int NL> __device__ __forceinline__ void ppt_tile_backward(const PptTab &T, const PptTile &X, PptTileLds<NH> &L, const float *dl_s,
                                                                            const float *lt_s) {
    static_assert(NH <= 16 && 2 * NL <= 16, "the tile partials leave 16 floats for b3 and 16 for the loss pairs");
    constexpr int ZS = PPT_ZS, P_B3 = ppt_p_b3(NH), P_B1 = ppt_p_b1(NH), P_LOSS = ppt_p_loss(NH);
    const int tid = X.tid, lane = X.lane, s = X.s, A = X.A, amax = T.amax;
    const int row = lane, kg = X.wv * 16;
    float *bufA = L.buf;
    // ---- dz2 = (z2 > 0) (dheads W3^T + dvalue Wv^T) -> bufA (the observations are no longer needed).  The value term SEEDS the sum
    // (a product, not an fmaf onto +0: the sign of a zero differs), so it is a branch of its own and not one more column.
    {
        float d[16];
        if constexpr (NH > PPT_AMAX) {
            const float dv = dl_s[row * NH + PPT_AMAX];
            const float *wvv = T.par.p[PT_V_W] + (size_t)s * 64 + kg;
            for (int j = 0; j < 16; ++j) d[j] = dv * wvv[j];
        } else {
            for (int j = 0; j < 16; ++j) d[j] = 0.0f;
        }
        const float *w3 = T.par.p[PT_FC3_W] + ((size_t)s * 64 + kg) * amax;
        for (int a = 0; a < A; ++a) {
            const float x = dl_s[row * NH + a];
            for (int j = 0; j < 16; ++j) d[j] = fmaf(x, w3[j * amax + a], d[j]);
        }
        for (int j = 0; j < 16; ++j) bufA[row * ZS + kg + j] = L.a2[row * ZS + kg + j] > 0.0f ? d[j] : 0.0f;
    }
    __syncthreads();
    float *P = T.part + ((size_t)s * T.tiles_max + X.tile) * ppt_p_size(NH);
    // ---- partial sums over the tile's rows that need dz2: dW2 = a1^T dz2, db2, dW3 / dWv = a2^T dheads, db3 / dbv, the loss terms
    {
        float g2[16];
        for (int j = 0; j < 16; ++j) g2[j] = 0.0f;
        for (int r = 0; r < PPT_TM; ++r) {
            const float dz = bufA[r * ZS + lane];
            for (int j = 0; j < 16; ++j) g2[j] = fmaf(L.a1[r * ZS + kg + j], dz, g2[j]);
        }
        for (int j = 0; j < 16; ++j) P[PPT_P_W2 + (kg + j) * 64 + lane] = g2[j];
        for (int o = tid; o < 64 * NH; o += PPT_T) {
            const int k = o / NH, a = o - k * NH;
            float acc = 0.0f;
            for (int r = 0; r < PPT_TM; ++r) acc = fmaf(L.a2[r * ZS + k], dl_s[r * NH + a], acc);
            P[PPT_P_W3 + o] = acc;
        }
        if (tid < 64) {
            float acc = 0.0f;
            for (int r = 0; r < PPT_TM; ++r) acc += bufA[r * ZS + tid];
            P[PPT_P_B2 + tid] = acc;
        } else if (tid < 64 + NH) {
            float acc = 0.0f;
            for (int r = 0; r < PPT_TM; ++r) acc += dl_s[r * NH + (tid - 64)];
            P[P_B3 + tid - 64] = acc;
        } else if (tid >= 128 && tid < 128 + NL) {
            float hi = 0.0f, lo = 0.0f;
            for (int r = 0; r < PPT_TM; ++r) ppo_pair_add(&hi, &lo, lt_s[r * NL + (tid - 128)], 0.0f);
            P[P_LOSS + tid - 128] = hi;
            P[P_LOSS + NL + tid - 128] = lo;
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
        for (int j = 0; j < 16; ++j) d1[j] = L.a1[row * ZS + kg + j] > 0.0f ? d1[j] : 0.0f;
    }
    __syncthreads();
    for (int j = 0; j < 16; ++j) bufA[row * ZS + kg + j] = d1[j];
    __syncthreads();
    {
        float *dz = T.dz1 + ((size_t)s * T.bpad_max + X.r0) * 64;
        for (int e = tid; e < PPT_TM * 64; e += PPT_T) dz[e] = bufA[(e >> 6) * ZS + (e & 63)];
        if (tid < 64) {
            float acc = 0.0f;
            for (int r = 0; r < PPT_TM; ++r) acc += bufA[r * ZS + tid];
            P[P_B1 + tid] = acc;
        }
    }
}

// ------------------------------------------------------------- 2. fc1 backward: dW1, dfeat and the conv gradients, per feature block
// grid (H * 2, chunks, S).  block (h, cb): conv row h, channels cb * 32 .. + 31 = 128 features m = (c - cb * 32) * 4 + w; wave wv owns
// features wv * 32 .. + 31
template <class Batch> __device__ __forceinline__ void ppt_fc1_bwd_body(const PptTab &T, const Batch &D) {
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
            if (rb + r < D.B) x = __half2float(D.obs[((size_t)D.src(rb + r, s, S) * S + s) * ow + h * 5 + q]);
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

// --------------------------------------------------------------------------------------------- 3. partials -> gradients, fixed order
// grid (S, H + ceil(ppt_n_small(NH) / PPT_T)): part p < H = the fc1_w rows of conv row p, the others 256 small outputs each.
// loss_out: NULL or [S][NL], the means over the B rows of the loss terms
template <int NH, int NL> __device__ __forceinline__ void ppt_reduce_body(const PptTab &T, int B, float *loss_out) {
    constexpr int P_B3 = ppt_p_b3(NH), P_B1 = ppt_p_b1(NH), P_LOSS = ppt_p_loss(NH), P_SIZE = ppt_p_size(NH);
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
    if (o >= ppt_n_small(NH)) return;
    if (o < P_SIZE) {
        float *dst = nullptr;
        if (o < PPT_P_B2) dst = T.grad.p[PT_FC2_W] + (size_t)s * 4096 + o;
        else if (o < PPT_P_W3) dst = T.grad.p[PT_FC2_B] + s * 64 + (o - PPT_P_B2);
        else if (o < P_B3) {
            const int k = (o - PPT_P_W3) / NH, a = (o - PPT_P_W3) - k * NH;
            if (NH > PPT_AMAX && a == PPT_AMAX) dst = T.grad.p[PT_V_W] + s * 64 + k;
            else if (a < A) dst = T.grad.p[PT_FC3_W] + ((size_t)s * 64 + k) * amax + a;
        } else if (o < P_B1) {
            const int a = o - P_B3;
            if (NH > PPT_AMAX && a == PPT_AMAX) dst = T.grad.p[PT_V_B] + s;
            else if (a < A) dst = T.grad.p[PT_FC3_B] + s * amax + a;
        } else if (o < P_LOSS) dst = T.grad.p[PT_FC1_B] + s * 64 + (o - P_B1);
        else if (o < P_LOSS + NL && loss_out) dst = loss_out + s * NL + (o - P_LOSS);
        if (!dst) return;
        const float *src = T.part + (size_t)s * T.tiles_max * P_SIZE + o;
        if (o >= P_LOSS) {
            float hi = 0.0f, lo = 0.0f;
            for (int t = 0; t < tiles; ++t) ppo_pair_add(&hi, &lo, src[(size_t)t * P_SIZE], src[(size_t)t * P_SIZE + NL]);
            *dst = (hi + lo) / (float)B;
            return;
        }
        float acc = 0.0f;
        for (int t = 0; t < tiles; ++t) acc += src[(size_t)t * P_SIZE];
        *dst = acc;
        return;
    }
    const int e = o - P_SIZE, c = e / 5, q = e - c * 5;
    float acc = 0.0f;
    for (int ch = 0; ch < chunks; ++ch)
        for (int h = 0; h < hs; ++h) acc += T.pconv[((((size_t)ch * S + s) * T.H + h) * 64 + c) * 5 + q];
    if (q < 4) T.grad.p[PT_CONV_W][((size_t)s * 64 + c) * 4 + q] = acc;
    else T.grad.p[PT_CONV_B][s * 64 + c] = acc;
}

// --------------------------------------------------------------------------------------------------------------------- 4. Adam
// The elements of signal s in parts, grid (S, H + 1): p < H the fc1_w rows of conv row p (none when p >= hs), p == H every other
// tensor (the value head's where NH says the network has one).  f(tensor, offset) is called for thread tid's elements tid, tid + PPT_T, ..
// of the part in ascending order; padded fc1 rows and fc3 columns are never visited.
template <int NH, class F> __device__ static inline void ppt_visit_part(const PptTab &T, int s, int p, int tid, F f) {
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
    if constexpr (NH > PPT_AMAX) {
        for (int e = tid; e < 64; e += PPT_T) f(PT_V_W, (size_t)s * 64 + e);
        for (int e = tid; e < 1; e += PPT_T) f(PT_V_B, (size_t)s + e);
    }
}

// one Adam step of the part (blockIdx.x, blockIdx.y) on the gradients times `scale` ({1, 0}: no clipping)
template <int NH> __device__ __forceinline__ void ppt_adam_body(const PptTab &T, const PpoStepConsts &K, PpoPair scale) {
    ppt_visit_part<NH>(T, blockIdx.x, blockIdx.y, threadIdx.x, [&](int t, size_t o) {
        ppo_adam_element(&T.par.p[t][o], &T.m.p[t][o], &T.v.p[t][o], T.grad.p[t][o], scale, K);
    });
}
#endif
