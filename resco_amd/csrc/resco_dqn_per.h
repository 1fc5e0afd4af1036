// resco_dqn_per.h -- prioritised experience replay for the fused DQN update of IDQN (resco_dqn_train.h; rs_dqn_set_priorities /
// rs_dqn_per_rebuild / rs_dqn_per_fill / rs_dqn_per_commit of include/resco_sim.h).  Off by default: without rs_dqn_set_priorities
// nothing in this file is launched.
//
// The state is the caller's and sits beside the ring: prio f32 [T][N][S] (the layout of rew), a leaf q = (|delta| + eps)^alpha >= 0;
// ssum f32 [T][S], the sum of a slot's N leaves; pmax f32 [S], the largest q ever written for the signal.  Two levels: a draw picks a
// slot by ssum, then an environment by the slot's leaves, each with a random number of its own.
//
// THE sum of n weights (per_wave_total) has one order, whoever takes it: the weights in chunks of 64, inside a chunk the inclusive
// Hillis-Steele scan over the lanes of one wave (steps 1, 2, 4 .. 32: lane l adds the value of lane l - d), the chunk's cumulative
// values = carry + scan, carry = the cumulative value of lane 63, starting at 0.  The total is the last carry.  ssum is ALWAYS this
// total of the slot's leaves as they stand (rebuild, fill and commit re-sum, they never adjust by a difference), so the three agree bit
// for bit, and the cumulative values a draw compares with are the ones whose last is the stored total.  No float atomics anywhere:
// pmax is raised by an integer max on the bit pattern, which orders non-negative floats as their values.
//
// The draw (dqn_per_pick_seq is its sequential restatement): with threshold thr = r * total, the first entry k with weight > 0 and
// cumulative(k) > thr; none (rounding let thr fall past the end) -> the last entry with weight > 0; no positive weight at all -> entry
// 0.  A scan is not monotone in floating point, so an entry of weight 0 may show a cumulative value above its predecessor's: the
// weight > 0 condition is what keeps it from being drawn.
//
// Launches.  rs_dqn_sample: dqn_per_z_kernel (Z_s, the total of the valid slots' ssum, one wave per signal), dqn_per_sample_kernel (one
// wave per draw).  rs_dqn_grad: dqn_per_z_kernel, dqn_per_weight_kernel (one workgroup per signal: the rows' importance weights and
// their maximum over the minibatch, which spans tiles), the target kernel as the options say, dqn_fwd_bwd_per_kernel, then as without.
// rs_dqn_per_commit: dqn_per_leaf_kernel (q of every row, pmax), dqn_per_resum_kernel (one wave per row re-sums its slot; a launch of
// its own: a slot's sum must see every leaf the minibatch wrote into it).
#pragma once
#include <math.h>
#include "resco_dqn_train.h"

#define DQN_PER_SEED 0x9E3779B9u        // the draw's two uniforms come from d_hash(seed ^ DQN_PER_SEED, u, s, i, j): not the uniform draw's stream

// ---------------------------------------------------------------------------------------------------------------- scalar pieces
// uniform j (0: the slot, 1: the environment) of draw i of signal s in update u: 24 bits, exact in fp32, in [0, 1)
RS_DQN_DEV float dqn_per_uniform(uint32_t seed, uint32_t u, uint32_t s, uint32_t i, uint32_t j) {
    return (float)(d_hash(seed ^ DQN_PER_SEED, u, s, i, j) >> 8) * 5.9604644775390625e-8f;
}
// the exponent of the importance weights after u Adam steps: in double, rounded once (as gt_epsilon); beta_steps 0: constant
RS_PPO_HD float dqn_per_beta(double beta0, int64_t beta_steps, int64_t u) {
    if (beta_steps <= 0) return (float)beta0;
    const double b = beta0 + (1.0 - beta0) * ((double)u / (double)beta_steps);
    return (float)(b < 1.0 ? b : 1.0);
}
// the leaf of a row with |delta| = ad.  An overflow to infinity (a diverged network) becomes 0: the row is not drawn again, and
// neither the sums nor pmax hold an infinity.
RS_PPO_HD float dqn_per_priority(float ad, float eps, float alpha) {
    const float q = powf(ad + eps, alpha);
    return q < INFINITY ? q : 0.0f;
}
// the importance weight of a row before the division by the minibatch's maximum: (M q / Z)^-beta, M = (count - 1) N.  A row of
// priority 0 cannot have been drawn; where a caller names one, its weight is 0.
RS_PPO_HD float dqn_per_row_weight(float q, float Z, float M, float beta) { return q > 0.0f && Z > 0.0f ? powf(M * q / Z, -beta) : 0.0f; }
// the pick among n weights w[k * stride], summed one after the other (the device sums in per_wave_total's order)
RS_PPO_HD int dqn_per_pick_seq(const float *w, int n, long long stride, float thr) {
    float c = 0.0f;
    int last = 0;
    for (int k = 0; k < n; ++k) {
        const float x = w[k * stride];
        c = c + x;
        if (x > 0.0f) {
            if (c > thr) return k;
            last = k;
        }
    }
    return last;
}

#ifdef __HIPCC__
struct DqnPer {
    float *prio, *ssum, *pmax;              // the caller's: [T][N][S], [T][S], [S]
    float *z, *w, *ad;                      // the handle's: Z_s [S]; the rows' weights and |delta| [S][bpad_max]
    int32_t T, N, S, bpad_max;
    float alpha, eps, beta;
};
#define DQN_PER_WAVES (PPT_T / 64)          // one wave per unit of work, DQN_PER_WAVES of them per workgroup

__device__ __forceinline__ int per_unit() { return (int)blockIdx.x * DQN_PER_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6); }
// the inclusive scan of one value per lane
__device__ __forceinline__ float per_scan64(float x, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const float y = __shfl_up(x, d, 64);
        if (lane >= d) x = x + y;
    }
    return x;
}
// THE sum of the weights w(0 .. n - 1); n is the same in every lane, every lane returns the total
template <class F> __device__ __forceinline__ float per_wave_total(int n, int lane, F w) {
    float carry = 0.0f;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        carry = __shfl(carry + per_scan64(k < n ? w(k) : 0.0f, lane), 63, 64);
    }
    return carry;
}
// the draw among the weights w(0 .. n - 1) against thr, with the same cumulative values; every lane returns the entry
template <class F> __device__ __forceinline__ int per_wave_pick(int n, int lane, float thr, F w) {
    float carry = 0.0f;
    int last = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const float x = k < n ? w(k) : 0.0f, cum = carry + per_scan64(x, lane);
        const unsigned long long pos = __ballot(x > 0.0f), hit = __ballot(x > 0.0f && cum > thr);
        if (hit) return k0 + __ffsll(hit) - 1;
        if (pos) last = k0 + 63 - __clzll((long long)pos);
        carry = __shfl(cum, 63, 64);
    }
    return last;
}
// valid slot k = 0 .. count - 2 of a ring, counted from the oldest
__device__ __forceinline__ int per_slot(int k, int T, int head, int count) { return (int)((uint32_t)(head - count + T + k) % (uint32_t)T); }

// Z_s: grid ceil(S / DQN_PER_WAVES)
__global__ void __launch_bounds__(PPT_T) dqn_per_z_kernel(DqnPer P, int head, int count) {
    const int s = per_unit(), lane = threadIdx.x & 63;
    if (s >= P.S) return;
    const float z = per_wave_total(count - 1, lane, [&](int k) { return P.ssum[(size_t)per_slot(k, P.T, head, count) * P.S + s]; });
    if (lane == 0) P.z[s] = z;
}

// the draws: grid ceil(B S / DQN_PER_WAVES); idx [B][S][2]
__global__ void __launch_bounds__(PPT_T) dqn_per_sample_kernel(DqnPer P, uint32_t seed, uint32_t u, int head, int count, int B, int32_t *idx) {
    const int o = per_unit(), lane = threadIdx.x & 63, S = P.S;
    if (o >= B * S) return;
    const int i = o / S, s = o - i * S;
    const float r0 = dqn_per_uniform(seed, u, (uint32_t)s, (uint32_t)i, 0u), r1 = dqn_per_uniform(seed, u, (uint32_t)s, (uint32_t)i, 1u);
    const int k = per_wave_pick(count - 1, lane, r0 * P.z[s], [&](int j) { return P.ssum[(size_t)per_slot(j, P.T, head, count) * S + s]; });
    const int t = per_slot(k, P.T, head, count);
    const float *leaf = P.prio + (size_t)t * P.N * S + s;
    const int e = per_wave_pick(P.N, lane, r1 * P.ssum[(size_t)t * S + s], [&](int j) { return leaf[(size_t)j * S]; });
    if (lane == 0) { idx[(size_t)o * 2] = t; idx[(size_t)o * 2 + 1] = e; }
}

// the rows' weights w_i = raw_i / max_j raw_j: grid S.  The maximum is a max, so its order does not matter.
__global__ void __launch_bounds__(PPT_T) dqn_per_weight_kernel(DqnPer P, DqnBatch D, int count) {
    __shared__ float mx_s[PPT_T];
    const int s = blockIdx.x, tid = threadIdx.x, S = P.S;
    const float Z = P.z[s], M = (float)((long long)(count - 1) * P.N);
    float *w = P.w + (size_t)s * P.bpad_max;
    float mx = 0.0f;
    for (int i = tid; i < D.B; i += PPT_T) {
        const float raw = dqn_per_row_weight(P.prio[(size_t)D.src(i, s, S) * S + s], Z, M, P.beta);
        w[i] = raw;
        mx = fmaxf(mx, raw);
    }
    mx_s[tid] = mx;
    __syncthreads();
    for (int d = PPT_T / 2; d > 0; d >>= 1) {
        if (tid < d) mx_s[tid] = fmaxf(mx_s[tid], mx_s[tid + d]);
        __syncthreads();
    }
    mx = mx_s[0];
    for (int i = tid; i < D.B; i += PPT_T) w[i] = mx > 0.0f ? w[i] / mx : 0.0f;     // (a thread divides what it wrote itself)
}

// dqn_fwd_bwd_kernel (launch 2 of a gradient) with the rows' weights: row i of signal s multiplies its loss term and its dQ by
// w[s][i] and leaves |delta| in ad[s][i] for the commit.  A kernel of its own that restates the default one's few lines around the
// shared tile functions, so that the default kernel's source stays as it is (the compiler still allocates its registers a little
// differently with a second caller of those functions: profiles/r24_idqn_per_kernel_resources.txt).
__global__ void __launch_bounds__(PPT_T, 2) dqn_fwd_bwd_per_kernel(DqnTrainTab T, DqnBatch D, const float *w, float *ad) {
    __shared__ PptTileLds<DQN_NH> L;
    __shared__ float dl_s[PPT_TM * DQN_NH], lt_s[PPT_TM * DQN_NL];
    const PptTile X = ppt_tile(T, D.B);
    const int tid = X.tid, S = T.S, s = X.s, A = X.A;
    if (tid < PPT_TM) L.src[tid] = tid < X.nrows ? D.src(X.r0 + tid, s, S) : -1;
    __syncthreads();
    ppt_tile_load(T.par, T, X, D.obs, L);
    __syncthreads();
    ppt_tile_forward(T.par, T, X, L);
    if (tid < PPT_TM) {
        float dl[PPT_AMAX], tm = 0.0f;
        for (int a = 0; a < PPT_AMAX; ++a) dl[a] = 0.0f;
        if (tid < X.nrows) {
            float q[PPT_AMAX];
            for (int a = 0; a < PPT_AMAX; ++a) q[a] = a < A ? L.lg[tid * DQN_NH + a] : 0.0f;
            const size_t at = (size_t)s * T.bpad_max + X.r0 + tid;
            const int action = (int)D.act[(size_t)L.src[tid] * S + s];
            const float y = T.y[at], wi = w[at];
            dqn_row_loss_grad(q, A, action, y, (float)D.B, dl, &tm);
            for (int a = 0; a < PPT_AMAX; ++a) dl[a] = wi * dl[a];
            tm = wi * tm;
            ad[at] = fabsf(q[action < 0 ? 0 : (action >= A ? A - 1 : action)] - y);        // (dqn_row_loss_grad's clamp of the action)
        }
        for (int a = 0; a < PPT_AMAX; ++a) dl_s[tid * DQN_NH + a] = a < A ? dl[a] : 0.0f;
        lt_s[tid] = tm;
    }
    __syncthreads();
    ppt_tile_backward<DQN_NH, DQN_NL>(T, X, L, dl_s, lt_s);
}

// the commit's leaves: grid ceil(B S / PPT_T).  Two rows of a minibatch that name the same (t, e) of a signal are the same row of the
// ring: the same observation, action and target through the same arithmetic, so the same delta and the same bits of q.  Both write
// them to the same leaf -- a benign race.
__global__ void __launch_bounds__(PPT_T) dqn_per_leaf_kernel(DqnPer P, DqnBatch D) {
    const int o = blockIdx.x * PPT_T + threadIdx.x, S = P.S;
    if (o >= D.B * S) return;
    const int i = o / S, s = o - i * S;
    const float q = dqn_per_priority(P.ad[(size_t)s * P.bpad_max + i], P.eps, P.alpha);
    P.prio[(size_t)D.src(i, s, S) * S + s] = q;
    atomicMax((int *)P.pmax + s, __float_as_int(q));        // q >= 0: the integer order of the bit patterns is the order of the values
}
// ... and the sums of the slots they touched: grid ceil(B S / DQN_PER_WAVES).  Rows of one slot write the same total.
__global__ void __launch_bounds__(PPT_T) dqn_per_resum_kernel(DqnPer P, DqnBatch D) {
    const int o = per_unit(), lane = threadIdx.x & 63, S = P.S;
    if (o >= D.B * S) return;
    const int i = o / S, s = o - i * S;
    int t, e;
    D.at(i, s, S, &t, &e);
    const float *leaf = P.prio + (size_t)t * P.N * S + s;
    const float z = per_wave_total(P.N, lane, [&](int j) { return leaf[(size_t)j * S]; });
    if (lane == 0) P.ssum[(size_t)t * S + s] = z;
}

// a new slot enters at the maximum priority: every leaf <- pmax[s] (every thread, grid-stride) and the slot's sums, which need no
// leaf read back: wave s sums N copies of pmax[s] in THE order.  grid >= ceil(S / DQN_PER_WAVES)
__global__ void __launch_bounds__(PPT_T) dqn_per_fill_kernel(DqnPer P, int slot) {
    const int S = P.S, n = P.N * S, lane = threadIdx.x & 63;
    float *leaf = P.prio + (size_t)slot * n;
    for (int o = blockIdx.x * PPT_T + threadIdx.x; o < n; o += gridDim.x * PPT_T) leaf[o] = P.pmax[o % S];
    const int s = per_unit();
    if (s >= S) return;
    const float pm = P.pmax[s], z = per_wave_total(P.N, lane, [&](int) { return pm; });
    if (lane == 0) P.ssum[(size_t)slot * S + s] = z;
}

// every sum from the leaves: grid ceil(T S / DQN_PER_WAVES)
__global__ void __launch_bounds__(PPT_T) dqn_per_rebuild_kernel(DqnPer P) {
    const int o = per_unit(), lane = threadIdx.x & 63, S = P.S;
    if (o >= P.T * S) return;
    const float *leaf = P.prio + (size_t)(o / S) * P.N * S + (o % S);
    const float z = per_wave_total(P.N, lane, [&](int j) { return leaf[(size_t)j * S]; });
    if (lane == 0) P.ssum[o] = z;
}
#endif
