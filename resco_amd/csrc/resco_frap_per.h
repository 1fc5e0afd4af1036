// resco_frap_per.h -- prioritised experience replay for the fused shared-DQN update of MPLight (resco_frap_train.h;
// rs_mplight_dqn_set_priorities / rs_mplight_dqn_per_rebuild / _per_fill / _per_commit of include/resco_sim.h).  Off by default: without
// rs_mplight_dqn_set_priorities nothing in this file is launched.
//
// MPLight draws from ONE pooled population of rows (t, e, s), so the sums run over all three axes.  The state is the caller's and sits
// beside the ring: prio f32 [T][N][S] (the layout of rew), a leaf q = (|delta| + eps)^alpha >= 0; esum f32 [T][N], the total of the S
// leaves of (t, e); ssum f32 [T], the total of the N values esum[t][.]; pmax f32 [1], the largest q ever written.  Three levels: a draw
// picks a slot by ssum, an environment by the slot's esum, a signal by the leaves of (t, e), each with a random number of its own.
// (Two levels over the N S contiguous leaves of a slot would make every wave walk N S / 64 chunks: 336 on ingolstadt21 x 1024.  With
// three a draw walks ceil(T / 64) + ceil(N / 64) + ceil(S / 64) chunks.)
//
// "THE sum" is per_wave_total of resco_dqn_per.h, whoever takes it: chunks of 64, the inclusive Hillis-Steele scan inside a chunk,
// carry = the cumulative value of lane 63.  esum is ALWAYS THE sum of its leaves as they stand and ssum THE sum of its esum values as
// they stand: rebuild, fill and commit re-sum, they never adjust by a difference, so the three agree bit for bit.  No float atomics:
// pmax is raised by an integer max on the bit pattern.  The pick rule is per_wave_pick's (dqn_per_pick_seq its sequential form).
//
// Launches.  rs_mplight_dqn_sample: frap_per_z_kernel (Z, THE sum of the valid slots' ssum, one wave), frap_per_sample_kernel (one wave
// per draw).  rs_mplight_dqn_grad: frap_per_z_kernel, frap_per_weight_kernel (one workgroup: the rows' importance weights over their
// maximum), then frap_per_tile_kernel or frap_per_tile_opt_kernel<DOUBLE_Q> in the place of the tile kernel the target's options
// select, then the reduction as without.  rs_mplight_dqn_per_commit: frap_per_leaf_kernel (q of every row, pmax), frap_per_esum_kernel
// (one wave per row re-sums its (t, e)), frap_per_ssum_kernel (one wave per row re-sums its slot) -- three launches because an esum
// must see every leaf the minibatch wrote under it, and an ssum every esum.  rs_mplight_dqn_per_rebuild: the last two over every
// (t, e) and every t.  rs_mplight_dqn_per_fill: frap_per_fill_kernel.
// Needs resco_frap_train.h and resco_dqn_per.h before it.
#pragma once
#include "resco_dqn_per.h"
#include "resco_frap_train.h"

// uniform j (0: the slot, 1: the environment, 2: the signal) of draw i of update u: 24 bits, exact in fp32, in [0, 1).  The fourth
// hash argument is 1: the uniform draw (frap_dqn_sample_index) uses (.., 0, 0 .. 2) and the multi-map draw (.., 0, 3 .. 4)
RS_FPT_DEV float frap_per_uniform(uint32_t seed, uint32_t u, uint32_t i, uint32_t j) {
    return (float)(d_hash(seed ^ FRAP_TRAIN_SALT, u, i, 1u, j) >> 8) * 5.9604644775390625e-8f;
}

// fpt_row_loss with the row's importance weight: the Huber term and dy are multiplied by (double) w, and |y - tgt|, evaluated in
// double and rounded ONCE to fp32, is left in *ad for the commit (rows outside the minibatch write nothing)
template <int TAG>
RS_HD inline void fpt_row_loss_per(FrapStage &L, int P, int batch, int r, const float *w, float *ad) {
    L.dy[r] = 0.0; L.term[r] = 0.0;
    if (!L.ok[r]) return;
    const int g = L.g[r];
    fpt_t y = 0.0;
    for (int j = 0; j < P; ++j)
        if (j != g) y += L.y[r][j];
    const fpt_t delta = y - L.tgt[r], a = fabs(delta), wi = (fpt_t)w[r];
    L.dy[r] = wi * ((delta < -1.0 ? -1.0 : (delta > 1.0 ? 1.0 : delta)) / (fpt_t)batch);
    L.term[r] = wi * (a < 1.0 ? 0.5 * delta * delta : a - 0.5);
    ad[r] = (float)a;
}

#ifdef __HIPCC__
struct FrapPer {
    float *prio, *esum, *ssum, *pmax;       // the caller's: [T][N][S], [T][N], [T], [1]
    float *z, *w, *ad;                      // the handle's: Z [1]; the rows' weights and |delta| [max_batch]
    int32_t T, N, S;
    float alpha, eps, beta;
};
// row i of a minibatch, held inside the ring whatever idx says (as the tile kernels hold it)
__device__ __forceinline__ void frap_per_row(const FrapPer &P, const int32_t *idx, int i, int *t, int *e, int *s) {
    const int32_t *p = idx + (size_t)i * 3;
    *t = min(max(p[0], 0), P.T - 1); *e = min(max(p[1], 0), P.N - 1); *s = min(max(p[2], 0), P.S - 1);
}

// Z: grid 1, wave 0
__global__ void __launch_bounds__(PPT_T) frap_per_z_kernel(FrapPer P, int head, int count) {
    const int lane = threadIdx.x & 63;
    if (per_unit() != 0) return;
    const float z = per_wave_total(count - 1, lane, [&](int k) { return P.ssum[per_slot(k, P.T, head, count)]; });
    if (lane == 0) P.z[0] = z;
}

// the draws: grid ceil(B / DQN_PER_WAVES); idx [B][3]
__global__ void __launch_bounds__(PPT_T) frap_per_sample_kernel(FrapPer P, uint32_t seed, uint32_t u, int head, int count, int B, int32_t *idx) {
    const int i = per_unit(), lane = threadIdx.x & 63;
    if (i >= B) return;
    const float r0 = frap_per_uniform(seed, u, (uint32_t)i, 0u), r1 = frap_per_uniform(seed, u, (uint32_t)i, 1u), r2 = frap_per_uniform(seed, u, (uint32_t)i, 2u);
    const int k = per_wave_pick(count - 1, lane, r0 * P.z[0], [&](int q) { return P.ssum[per_slot(q, P.T, head, count)]; });
    const int t = per_slot(k, P.T, head, count);
    const float *es = P.esum + (size_t)t * P.N;
    const int e = per_wave_pick(P.N, lane, r1 * P.ssum[t], [&](int q) { return es[q]; });
    const float *leaf = P.prio + ((size_t)t * P.N + e) * P.S;
    const int s = per_wave_pick(P.S, lane, r2 * es[e], [&](int q) { return leaf[q]; });
    if (lane == 0) { idx[(size_t)i * 3] = t; idx[(size_t)i * 3 + 1] = e; idx[(size_t)i * 3 + 2] = s; }
}

// the rows' weights w_i = raw_i / max_j raw_j: grid 1.  The maximum is a max, so its order does not matter.
__global__ void __launch_bounds__(PPT_T) frap_per_weight_kernel(FrapPer P, const int32_t *idx, int B, int count) {
    __shared__ float mx_s[PPT_T];
    const int tid = threadIdx.x;
    const float Z = P.z[0], M = (float)((long long)(count - 1) * P.N * P.S);
    float mx = 0.0f;
    for (int i = tid; i < B; i += PPT_T) {
        int t, e, s;
        frap_per_row(P, idx, i, &t, &e, &s);
        const float raw = dqn_per_row_weight(P.prio[((size_t)t * P.N + e) * P.S + s], Z, M, P.beta);
        P.w[i] = raw;
        mx = fmaxf(mx, raw);
    }
    mx_s[tid] = mx;
    __syncthreads();
    for (int d = PPT_T / 2; d > 0; d >>= 1) {
        if (tid < d) mx_s[tid] = fmaxf(mx_s[tid], mx_s[tid + d]);
        __syncthreads();
    }
    mx = mx_s[0];
    for (int i = tid; i < B; i += PPT_T) P.w[i] = mx > 0.0f ? P.w[i] / mx : 0.0f;       // (a thread divides what it wrote itself)
}

// frap_dqn_tile_kernel (launch 1 of a gradient, the target's options off) with the rows' weights: a kernel of its own that restates
// the plain one's lines around the shared phases, with its own instantiations of them (FPP_TAG), so that the plain kernel stays as it is
#define FPP_TAG 8
__global__ void __launch_bounds__(FPT_T) frap_per_tile_kernel(FrapTrainTab T, FrapBatch D, const float *wrow, float *ad) {
    constexpr int TAG = FPP_TAG;
    __shared__ FrapStage L;
    const int tid = threadIdx.x, r = tid / FPT_G, j = tid % FPT_G, row = blockIdx.x * FPT_TM + r;
    const int P = T.P, Dm = T.D;
    const float *w = T.par, *wt = T.tgt;
    for (int k = tid; k < 144; k += FPT_T) fpt_prep<TAG>(L, T.par, T.tgt, Dm, k);
    {
        const bool ok = row < D.B;
        int t = 0, e = 0, s = 0;
        if (ok) {
            const int32_t *p = D.idx + (size_t)row * 3;
            t = min(max(p[0], 0), D.T - 1); e = min(max(p[1], 0), D.N - 1); s = min(max(p[2], 0), D.S - 1);
        }
        const bool boot = ok && !D.done[t];
        const size_t cur = ((size_t)t * D.N + e) * D.S + s, nxt = ((size_t)(t + 1 == D.T ? 0 : t + 1) * D.N + e) * D.S + s;
        for (int q = j; q < FPT_W; q += FPT_G) {
            L.obs[r][q] = ok && q < D.W ? D.obs[cur * D.W + q] : 0.0f;
            L.nxt[r][q] = boot && q < D.W ? D.obs[nxt * D.W + q] : 0.0f;
        }
        if (j == 0) {
            const int a = ok ? (int)D.act[cur] : 0;
            L.ok[r] = ok; L.boot[r] = boot;
            L.g[r] = a < 0 ? 0 : (a >= P ? P - 1 : a);
            L.rew[r] = ok ? D.rew[cur] : 0.0f;
        }
    }
    __syncthreads();
    fpt_target_ab<TAG>(L, wt, Dm, P, T.pairs, r, j);
    __syncthreads();
    fpt_target_q<TAG>(L, wt, Dm, P, T.pairs, r, j);
    __syncthreads();
    if (j == 0) fpt_target_value<TAG>(L, P, T.gamma, r);
    if (j < FRAP_MV) fpt_mv_forward<TAG>(L, w, Dm, P, T.pairs, r, j);
    __syncthreads();
    fpt_pair_forward<TAG>(L, w, Dm, P, T.pairs, r, j);
    __syncthreads();
    fpt_item_forward<TAG>(L, w, Dm, P, T.pairs, r, j);
    __syncthreads();
    if (j == 0) fpt_row_loss_per<TAG>(L, P, D.B, r, wrow + (size_t)blockIdx.x * FPT_TM, ad + (size_t)blockIdx.x * FPT_TM);
    __syncthreads();
    fpt_item_backward<TAG>(L, w, Dm, P, r, j);
    __syncthreads();
    if (j == L.g[r]) fpt_row_backward<TAG>(L, w, Dm, P, r);
    __syncthreads();
    if (j < FRAP_MV) fpt_mv_backward<TAG>(L, w, Dm, P, T.pairs, r, j);
    __syncthreads();
    fpt_t *part = T.part + (size_t)blockIdx.x * FG_N;
    for (int e = tid; e < FG_N; e += FPT_T) part[e] = frap_tile_entry<TAG>(L, P, Dm, e);
}

// frap_dqn_tile_opt_kernel<DOUBLE_Q> with the rows' weights: frap_opt_tile_body's phases restated (instantiations FPP_TAG + 1 + DOUBLE_Q)
template <bool DOUBLE_Q>
__global__ void __launch_bounds__(FPT_T) frap_per_tile_opt_kernel(FrapTrainTab T, FrapBatch D, int n_step, const float *wrow, float *ad) {
    constexpr int TAG = FPP_TAG + 1 + (DOUBLE_Q ? 1 : 0);
    __shared__ FrapStage L;
    __shared__ FrapOptRows O;
    const int tid = threadIdx.x, r = tid / FPT_G, j = tid % FPT_G, row = blockIdx.x * FPT_TM + r;
    const int P = T.P, Dm = T.D;
    const float *w = T.par, *wt = T.tgt;
    for (int k = tid; k < 144; k += FPT_T) fpt_prep<TAG>(L, T.par, T.tgt, Dm, k);
    {
        const bool ok = row < D.B;
        int t = 0, e = 0, s = 0;
        if (ok) {
            const int32_t *p = D.idx + (size_t)row * 3;
            t = min(max(p[0], 0), D.T - 1); e = min(max(p[1], 0), D.N - 1); s = min(max(p[2], 0), D.S - 1);
        }
        fpt_opt_load_row<TAG>(L, O, D.obs, D.act, D.rew, D.done, D.T, D.N, D.S, D.W, P, D.head, ok, t, e, s, n_step, T.gamma, r, j);
    }
    __syncthreads();
    fpt_opt_load_next<TAG>(L, O, D.obs, D.W, r, j);
    __syncthreads();
    if constexpr (DOUBLE_Q) {
        fpt_target_ab<TAG, 0>(L, w, Dm, P, T.pairs, r, j);
        __syncthreads();
        fpt_target_q<TAG, 0>(L, w, Dm, P, T.pairs, r, j);
        __syncthreads();
        if (j == 0) fpt_opt_astar<TAG>(L, O, P, r);
    }
    fpt_target_ab<TAG, 1>(L, wt, Dm, P, T.pairs, r, j);
    __syncthreads();
    fpt_target_q<TAG, 1>(L, wt, Dm, P, T.pairs, r, j);
    __syncthreads();
    if (j == 0) fpt_opt_target_value<TAG, DOUBLE_Q>(L, O, P, r);
    if (j < FRAP_MV) fpt_mv_forward<TAG>(L, w, Dm, P, T.pairs, r, j);
    __syncthreads();
    fpt_pair_forward<TAG>(L, w, Dm, P, T.pairs, r, j);
    __syncthreads();
    fpt_item_forward<TAG>(L, w, Dm, P, T.pairs, r, j);
    __syncthreads();
    if (j == 0) fpt_row_loss_per<TAG>(L, P, D.B, r, wrow + (size_t)blockIdx.x * FPT_TM, ad + (size_t)blockIdx.x * FPT_TM);
    __syncthreads();
    fpt_item_backward<TAG>(L, w, Dm, P, r, j);
    __syncthreads();
    if (j == L.g[r]) fpt_row_backward<TAG>(L, w, Dm, P, r);
    __syncthreads();
    if (j < FRAP_MV) fpt_mv_backward<TAG>(L, w, Dm, P, T.pairs, r, j);
    __syncthreads();
    fpt_t *part = T.part + (size_t)blockIdx.x * FG_N;
    for (int e = tid; e < FG_N; e += FPT_T) part[e] = frap_tile_entry<TAG>(L, P, Dm, e);
}

// the commit's leaves: grid ceil(B / PPT_T).  Two rows of a minibatch that name the same (t, e, s) are the same row of the ring: the
// same observation, action and target through the same arithmetic, whatever tile and tile row they sit in (a lane's arithmetic does
// not depend on its row of the tile), so the same delta and the same bits of q.  Both write them to the same leaf -- a benign race.
__global__ void __launch_bounds__(PPT_T) frap_per_leaf_kernel(FrapPer P, const int32_t *idx, int B) {
    const int i = blockIdx.x * PPT_T + threadIdx.x;
    if (i >= B) return;
    int t, e, s;
    frap_per_row(P, idx, i, &t, &e, &s);
    const float q = dqn_per_priority(P.ad[i], P.eps, P.alpha);
    P.prio[((size_t)t * P.N + e) * P.S + s] = q;
    atomicMax((int *)P.pmax, __float_as_int(q));        // q >= 0: the integer order of the bit patterns is the order of the values
}
// esum re-summed from the leaves: grid ceil(n / DQN_PER_WAVES), one wave per unit.  idx: unit o is row o of the minibatch (the commit;
// rows of one (t, e) write the same total); NULL: unit o is (t, e) = (o / N, o % N), n = T N (the rebuild)
__global__ void __launch_bounds__(PPT_T) frap_per_esum_kernel(FrapPer P, const int32_t *idx, int n) {
    const int o = per_unit(), lane = threadIdx.x & 63;
    if (o >= n) return;
    int t = o / P.N, e = o - t * P.N, s;
    if (idx) frap_per_row(P, idx, o, &t, &e, &s);
    const float *leaf = P.prio + ((size_t)t * P.N + e) * P.S;
    const float z = per_wave_total(P.S, lane, [&](int q) { return leaf[q]; });
    if (lane == 0) P.esum[(size_t)t * P.N + e] = z;
}
// ... and ssum from esum, a launch later: unit o is row o of the minibatch, or (idx NULL) slot o, n = T
__global__ void __launch_bounds__(PPT_T) frap_per_ssum_kernel(FrapPer P, const int32_t *idx, int n) {
    const int o = per_unit(), lane = threadIdx.x & 63;
    if (o >= n) return;
    int t = o, e, s;
    if (idx) frap_per_row(P, idx, o, &t, &e, &s);
    const float *es = P.esum + (size_t)t * P.N;
    const float z = per_wave_total(P.N, lane, [&](int q) { return es[q]; });
    if (lane == 0) P.ssum[t] = z;
}

// a new slot enters at the maximum priority: every leaf <- pmax and the slot's sums, which need no read-back: es = THE sum of S
// copies of pmax (every wave computes it) goes to every esum[slot][e], and wave 0 writes ssum[slot] = THE sum of N copies of es.
// Leaves and esum grid-stride; any grid >= 1
__global__ void __launch_bounds__(PPT_T) frap_per_fill_kernel(FrapPer P, int slot) {
    const int n = P.N * P.S, lane = threadIdx.x & 63;
    const float pm = P.pmax[0];
    float *leaf = P.prio + (size_t)slot * n, *es_out = P.esum + (size_t)slot * P.N;
    for (int o = blockIdx.x * PPT_T + threadIdx.x; o < n; o += gridDim.x * PPT_T) leaf[o] = pm;
    const float es = per_wave_total(P.S, lane, [&](int) { return pm; });
    for (int o = blockIdx.x * PPT_T + threadIdx.x; o < P.N; o += gridDim.x * PPT_T) es_out[o] = es;
    if (per_unit() != 0) return;
    const float z = per_wave_total(P.N, lane, [&](int) { return es; });
    if (lane == 0) P.ssum[slot] = z;
}
#endif
