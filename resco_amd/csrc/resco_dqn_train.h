// resco_dqn_train.h -- the DQN update of the S stacked Q-networks of a BatchedIDQN on the device: minibatch sampling from the replay
// ring, target, loss, backward and Adam (rs_dqn_create / rs_dqn_sample / rs_dqn_grad / rs_dqn_step / rs_dqn_update of
// include/resco_sim.h).
//
// What it replaces (resco_amd/agents/idqn_learn.py: DeviceReplay.sample, BatchedDQNLearner.loss, its backward, torch.optim.Adam):
// ~150 small launches per Adam step of the batched PyTorch learner, which pads every signal to lmax lanes and copies the sampled
// observations twice.  Here the ring is read in place (obs f16 [T][N][S][lmax][5], act int16, rew f32 [T][N][S], done one byte per
// slot), every signal runs at its own lane count and action count, and all arithmetic is fp32.
//
// The network, its forward and backward, the reduction and the Adam body are resco_train.h's, with NH = 8 head columns (no value
// head: the tensor sets leave PT_V_W and PT_V_B NULL) and NL = 1 loss term.  This file adds the draw (dqn_sample_index), the per-row
// loss gradient (dqn_row_loss_grad; both built for the host as well by tests/dqn_train_host), the n-step walk (dqn_nstep_walk; built for
// the host by tests/dqn_nstep_host), the minibatch and the kernels.
//
// Launches of one minibatch gradient (rs_dqn_grad); row i of signal s is ring row idx[i][s] = (slot t, environment e):
//   1. dqn_target_kernel, one workgroup per (64-row tile, signal): the TARGET network forward on the successor row ((t + 1) mod T, e)
//      and tgt = rew + gamma max_{a < A_s} Q_target[a]; where done[t] is set the successor is not read at all and tgt = rew.
//      A launch of its own, not a first pass of the workgroup below: a workgroup is bound by the dependent MFMA chain of its fc1, and
//      a minibatch of 256 rows x 21 signals is 84 workgroups on 256 CUs -- one workgroup running both forwards would take twice as
//      long on the same 84 CUs, two launches cost one launch gap and 1 KB of targets per signal through memory (T.y).
//   2. dqn_fwd_bwd_kernel;  3. dqn_fc1_bwd_kernel;  4. dqn_reduce_kernel
// and of one optimiser step (rs_dqn_step): dqn_adam_kernel (PFRL's DQN does not clip gradients: scale {1, 0}).
// rs_dqn_sample is dqn_sample_kernel.  A target network may hold anything in its padded fc1_w rows and fc3 columns.
//
// The options of rs_dqn_set_target (n-step returns, Double DQN; PFRL's IDQN uses neither).  With either one on, launch 1 is
// dqn_target_opt_kernel<DOUBLE_Q> instead; launches 2 - 4, the draw and the Adam step are the same, and with both off nothing of this
// is launched: dqn_target_kernel stays as it is.
//   n_step: every row lane walks its row forward through the ring (dqn_nstep_walk: at most n_step dependent one-byte loads of done,
//   then as many four-byte loads of rew, small beside the fc1 MFMA chain), keeps R = sum_j gamma^j rew_j and g = gamma^m, and names
//   slot (t + m) mod T as the row the tile loads; tgt = R + g boot, or R alone where an episode end cut the walk (nothing is read
//   behind it).  The walk TRUNCATES at the newest slot: a row less than n_step slots behind it bootstraps from the newest observation
//   after fewer rewards.  PFRL's n-step buffer instead holds a transition back until its n successors exist; here the ring is read in
//   place and a row is a row as soon as it has one successor, so the draw is the same whatever the options.
//   double_q: boot = Q_target[argmax_a Q_online[a]] on the same successor rows, the lowest index among equal maxima; the online network
//   is T.par as it stands at this launch, before the update's Adam step.  A second load and forward in the SAME workgroup, not a
//   launch of its own: the successor rows have just been walked to (a launch of its own would walk them again or pass 64-bit row
//   names through memory), a* stays in LDS, and the argument for two launches above does not apply -- the online forward of the
//   successor rows must finish before the target's max in any case, so a separate launch would put one more launch gap on the
//   same dependent chain and run on the same tiles x S workgroups.
//   The cost is one more tile forward in launch 1, paid only with double_q on.
//
// Prioritised replay (rs_dqn_set_priorities) is resco_dqn_per.h: its own draw, the rows' importance weights, launch 2 with them
// (dqn_fwd_bwd_per_kernel) and the write-back of the priorities.  Off by default, and then nothing of it is launched: every kernel
// of this file stays as it is.
#pragma once
#include "resco_train.h"

#define DQN_NH PPT_AMAX     // head columns of a tile: the Q values
#define DQN_NL 1            // loss terms of a row: the Huber term

#ifdef __HIPCC__
#define RS_DQN_DEV __device__ static inline     // (d_hash of resco_step.h is a device function)
#else
#define RS_DQN_DEV static inline                // the host build of the tests brings a d_hash of its own
#endif

// ---------------------------------------------------------------------------------------------------------------- scalar pieces
// One sample of one signal with A actions: y = Q[action] (action clamped into 0 .. A - 1), delta = y - tgt,
//     dQ[action] = clamp(delta, -1, 1) / batch, every other dQ[a < A] = 0,  *term = 0.5 delta^2 where |delta| < 1, else |delta| - 0.5
// = torch's smooth_l1_loss with beta 1 (BatchedDQNLearner.loss) and its gradient under a mean over `batch` rows.
RS_PPO_HD void dqn_row_loss_grad(const float *q, int A, int action, float tgt, float batch, float *dq, float *term) {
    const int a0 = action < 0 ? 0 : (action >= A ? A - 1 : action);
    const float delta = q[a0] - tgt, ad = fabsf(delta);
    const float c = delta < -1.0f ? -1.0f : (delta > 1.0f ? 1.0f : delta);
    for (int a = 0; a < A; ++a) dq[a] = 0.0f;
    dq[a0] = c / batch;
    *term = ad < 1.0f ? 0.5f * delta * delta : ad - 0.5f;
}

// Draw i of signal s in update u: DeviceReplay.sample's distribution (a slot with a written successor, an environment, both uniform
// and independent) from the project's counter hash.  The oldest valid slot is head - count; slot head - 1 has no successor yet.
// hash % n is not exactly uniform: value v < 2^32 mod n is 2^-32 more likely than the others -- with n below 2^21 (slots, environments)
// a relative bias under 5e-4, accepted.  Needs 2 <= count <= T, 0 <= head < T, 1 <= N.  out: (t, e)
RS_DQN_DEV void dqn_sample_index(uint32_t seed, uint32_t u, uint32_t s, uint32_t i, int T, int N, int head, int count, int32_t *out) {
    const uint32_t k = d_hash(seed, u, s, i, 0u) % (uint32_t)(count - 1);
    const uint32_t e = d_hash(seed, u, s, i, 1u) % (uint32_t)N;
    out[0] = (int32_t)(((uint32_t)(head - count + T) + k) % (uint32_t)T);
    out[1] = (int32_t)e;
}

// The n-step walk of the row at slot t of a ring of T slots whose next slot to write is head: newest = (head - 1) mod T is the one
// written slot without a successor.  u_0 = t; step j takes the reward of u_j = (t + j) mod T and the walk stops after it where
// done[u_j] (*cut = 1: an episode ended, nothing behind it is read), where j + 1 == n_step, or where (u_j + 1) mod T == newest (the
// bootstrap row may be the newest slot, a reward may not).  *m = j + 1 rewards were taken, 1 <= *m <= max(n_step, 1); the bootstrap
// row of a walk that was not cut is (t + *m) mod T.  Reads done[u_0 .. u_{m-1}] only.  A t at `newest` is the caller's mistake: the
// walk then runs its n_step slots round the ring, over wrong data but never outside it.  Needs T >= 1, 0 <= t, head < T.
RS_PPO_HD void dqn_nstep_walk(const uint8_t *done, int T, int head, int t, int n_step, int *m, int *cut) {
    const int newest = head == 0 ? T - 1 : head - 1;
    int u = t, j = 0;
    for (;;) {
        const int nxt = u + 1 == T ? 0 : u + 1;
        const bool d = done[u] != 0;
        ++j;
        if (d || j >= n_step || nxt == newest) { *m = j; *cut = d ? 1 : 0; return; }
        u = nxt;
    }
}

#ifdef __HIPCC__
struct DqnTrainTab : PptTab {
    PptTensors tgt;                         // the target network (borrowed like the parameters, only read)
    float gamma;
    float *y;                               // [S][bpad_max]: the rows' targets
};

struct DqnBatch {
    const __half *obs;                      // the ring: [T][N][S][lmax][5]
    const int16_t *act;                     // [T][N][S]
    const float *rew;                       // [T][N][S]
    const uint8_t *done;                    // [T]
    int32_t T, N;
    const int32_t *idx;                     // [B][S][2]: (t, e)
    int32_t B;
    int32_t head;                           // the ring's next slot to write (the n-step walk stops before the newest slot, head - 1)
    // slot and environment of row i of signal s, held inside the ring whatever idx says
    __device__ void at(int i, int s, int S, int *t, int *e) const {
        const int32_t *p = idx + ((size_t)i * S + s) * 2;
        *t = min(max(p[0], 0), T - 1);
        *e = min(max(p[1], 0), N - 1);
    }
    __device__ long long src(int i, int s, int S) const {
        int t, e;
        at(i, s, S, &t, &e);
        return (long long)t * N + e;
    }
};

__global__ void __launch_bounds__(PPT_T) dqn_sample_kernel(uint32_t seed, uint32_t u, int S, int T, int N, int head, int count, int B, int32_t *idx) {
    const int o = blockIdx.x * PPT_T + threadIdx.x;
    if (o >= B * S) return;
    const int i = o / S, s = o - i * S;
    dqn_sample_index(seed, u, (uint32_t)s, (uint32_t)i, T, N, head, count, idx + (size_t)o * 2);
}

// ------------------------------------------------------------------------------------------- 1. the rows' targets, per tile
__global__ void __launch_bounds__(PPT_T, 2) dqn_target_kernel(DqnTrainTab T, DqnBatch D) {
    __shared__ PptTileLds<DQN_NH> L;
    __shared__ long long cur_s[PPT_TM];
    const PptTile X = ppt_tile(T, D.B);
    const int tid = X.tid, S = T.S, s = X.s;
    if (tid < PPT_TM) {
        long long cur = -1, nxt = -1;
        if (tid < X.nrows) {
            int t, e;
            D.at(X.r0 + tid, s, S, &t, &e);
            cur = (long long)t * D.N + e;
            if (!D.done[t]) nxt = (long long)(t + 1 == D.T ? 0 : t + 1) * D.N + e;      // an episode end cuts the bootstrap: nothing is read
        }
        cur_s[tid] = cur; L.src[tid] = nxt;
    }
    __syncthreads();
    ppt_tile_load(T.tgt, T, X, D.obs, L);
    __syncthreads();
    ppt_tile_forward(T.tgt, T, X, L);
    if (tid < PPT_TM) {
        float y = 0.0f;
        if (tid < X.nrows) {
            y = D.rew[(size_t)cur_s[tid] * S + s];
            if (L.src[tid] >= 0) {
                float mx = L.lg[tid * DQN_NH];
                for (int a = 1; a < X.A; ++a) mx = L.lg[tid * DQN_NH + a] > mx ? L.lg[tid * DQN_NH + a] : mx;
                y = y + T.gamma * mx;
            }
        }
        T.y[(size_t)s * T.bpad_max + X.r0 + tid] = y;
    }
}

// ---------------------------------------------------------------- 1'. the rows' targets with n-step returns and / or Double DQN
// (the file's header has the semantics).  Arithmetic in fp32, this order: R = rew_0, g = gamma; for j = 1 .. m - 1: R = R + g rew_j,
// g = g gamma; tgt = cut ? R : R + g boot -- at n_step 1 what dqn_target_kernel computes.
template <bool DOUBLE_Q> __global__ void __launch_bounds__(PPT_T, 2) dqn_target_opt_kernel(DqnTrainTab T, DqnBatch D, int n_step) {
    __shared__ PptTileLds<DQN_NH> L;
    __shared__ float ret_s[PPT_TM], disc_s[PPT_TM];
    __shared__ int astar_s[PPT_TM];
    const PptTile X = ppt_tile(T, D.B);
    const int tid = X.tid, S = T.S, s = X.s;
    if (tid < PPT_TM) {
        long long nxt = -1;
        float R = 0.0f, g = T.gamma;
        if (tid < X.nrows) {
            int t, e, m, cut;
            D.at(X.r0 + tid, s, S, &t, &e);
            dqn_nstep_walk(D.done, D.T, min(max(D.head, 0), D.T - 1), t, n_step, &m, &cut);
            int u = t;
            R = D.rew[((size_t)u * D.N + e) * S + s];
            for (int j = 1; j < m; ++j) {
                u = u + 1 == D.T ? 0 : u + 1;
                R = R + g * D.rew[((size_t)u * D.N + e) * S + s];
                g = g * T.gamma;
            }
            if (!cut) nxt = (long long)(u + 1 == D.T ? 0 : u + 1) * D.N + e;            // an episode end cuts the bootstrap: nothing is read
        }
        ret_s[tid] = R; disc_s[tid] = g; L.src[tid] = nxt; astar_s[tid] = 0;
    }
    __syncthreads();
    if constexpr (DOUBLE_Q) {           // the online network on the successor rows: a* = its best action, the lowest index among equals
        ppt_tile_load(T.par, T, X, D.obs, L);
        __syncthreads();
        ppt_tile_forward(T.par, T, X, L);
        if (tid < PPT_TM) {
            int best = 0;
            float mx = L.lg[tid * DQN_NH];
            for (int a = 1; a < X.A; ++a)
                if (L.lg[tid * DQN_NH + a] > mx) { mx = L.lg[tid * DQN_NH + a]; best = a; }
            astar_s[tid] = best;
        }
        __syncthreads();
    }
    ppt_tile_load(T.tgt, T, X, D.obs, L);
    __syncthreads();
    ppt_tile_forward(T.tgt, T, X, L);
    if (tid < PPT_TM) {
        float y = 0.0f;
        if (tid < X.nrows) {
            y = ret_s[tid];
            if (L.src[tid] >= 0) {
                float boot;
                if constexpr (DOUBLE_Q) {
                    boot = L.lg[tid * DQN_NH + astar_s[tid]];
                } else {
                    boot = L.lg[tid * DQN_NH];
                    for (int a = 1; a < X.A; ++a) boot = L.lg[tid * DQN_NH + a] > boot ? L.lg[tid * DQN_NH + a] : boot;
                }
                y = y + disc_s[tid] * boot;
            }
        }
        T.y[(size_t)s * T.bpad_max + X.r0 + tid] = y;
    }
}

// ------------------------------------------------------------------------------------- 2. forward, loss, backward to dz1, per tile
__global__ void __launch_bounds__(PPT_T, 2) dqn_fwd_bwd_kernel(DqnTrainTab T, DqnBatch D) {
    __shared__ PptTileLds<DQN_NH> L;
    __shared__ float dl_s[PPT_TM * DQN_NH], lt_s[PPT_TM * DQN_NL];
    const PptTile X = ppt_tile(T, D.B);
    const int tid = X.tid, S = T.S, s = X.s, A = X.A;
    if (tid < PPT_TM) L.src[tid] = tid < X.nrows ? D.src(X.r0 + tid, s, S) : -1;
    __syncthreads();
    ppt_tile_load(T.par, T, X, D.obs, L);
    __syncthreads();
    ppt_tile_forward(T.par, T, X, L);
    // ---- the loss gradient of every row; rows past the minibatch contribute nothing
    if (tid < PPT_TM) {
        float dl[PPT_AMAX], tm = 0.0f;
        for (int a = 0; a < PPT_AMAX; ++a) dl[a] = 0.0f;
        if (tid < X.nrows) {
            float q[PPT_AMAX];
            for (int a = 0; a < PPT_AMAX; ++a) q[a] = a < A ? L.lg[tid * DQN_NH + a] : 0.0f;
            dqn_row_loss_grad(q, A, (int)D.act[(size_t)L.src[tid] * S + s], T.y[(size_t)s * T.bpad_max + X.r0 + tid], (float)D.B, dl, &tm);
        }
        for (int a = 0; a < PPT_AMAX; ++a) dl_s[tid * DQN_NH + a] = a < A ? dl[a] : 0.0f;
        lt_s[tid] = tm;
    }
    __syncthreads();
    ppt_tile_backward<DQN_NH, DQN_NL>(T, X, L, dl_s, lt_s);
}

__global__ void __launch_bounds__(PPT_T) dqn_fc1_bwd_kernel(DqnTrainTab T, DqnBatch D) { ppt_fc1_bwd_body(T, D); }
__global__ void __launch_bounds__(PPT_T) dqn_reduce_kernel(DqnTrainTab T, int B, float *loss_out) { ppt_reduce_body<DQN_NH, DQN_NL>(T, B, loss_out); }
__global__ void __launch_bounds__(PPT_T) dqn_adam_kernel(DqnTrainTab T, PpoStepConsts K) { ppt_adam_body<DQN_NH>(T, K, PpoPair{1.0f, 0.0f}); }
#endif
