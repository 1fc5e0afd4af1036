// resco_ppo.h -- generalised advantage estimation and the per-signal advantage standardisation of the IPPO learner, fused
// (rs_ppo_gae of include/resco_sim.h).
//
// What it replaces (resco_amd/agents/ippo.py: gae() and the last lines of BatchedPPOLearner.make_dataset; the reference gets both
// from pfrl.agents.PPO, resco_benchmark/agents/pfrl_ppo.py:38-75 with standardize_advantages=True):
//     for t = T-1 .. 0:  nd = 1 - done[t];  delta = rew[t] + gamma nd V[t+1] - V[t];  last = delta + gamma lambda nd last;  adv[t] = last
//     ret = adv + V;     adv = (adv - mean_s) / (std_s + 1e-8)     per signal s over its T * N samples, std biased
// As tensor operations that is a Python loop of T dependent launches of a few hundred bytes each, then four reductions.
//
// Here: rew / value / adv / ret are [T][N][S] = [T][C] with C = N * S columns (env, signal).
//   pass 1 (ppo_gae_column, one thread per column): walks T backwards -- the columns of a step are adjacent in memory, so a wave reads
//           256 contiguous bytes per step -- writes the raw advantage and the return and leaves the column's sum in scratch[col];
//   pass 2 (one workgroup of PPO_B threads per signal): mean from the column sums, then sum (x - mean)^2 over the signal's samples
//           (two passes over the data: no E[x^2] - mean^2 cancellation), then the standardisation in place.
// Every sum has ONE order, fixed by (T, N, S) alone: a column front to back in t = T-1 .. 0, a thread's columns e = tid, tid + PPO_B, ..
// in that order, then a halving tree over the PPO_B partial sums.  No float atomics: two runs give the same bits.
//
// The arithmetic is plain C++ (RS_PPO_HD functions of (tid, column)); the kernels below only hand out thread indices and put
// barriers between the phases.  ppo_gae_host runs the same functions phase by phase in a loop over tid -- with the same
// contraction setting (-ffp-contract=off, as the library is built) a host compiler produces the device's bits
// (tests/ppo_host/ppo_host.cpp).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RS_PPO_HD __host__ __device__ static inline
#else
#define RS_PPO_HD static inline
#endif

#define PPO_B 256           // threads of a per-signal workgroup = partial sums of its reductions

struct PpoArgs {
    const float *rew, *value, *last_value;  // [T][C], [T][C], [C]
    const uint8_t *done;                    // [T]: the episode ended after step t -- no bootstrap across it
    int32_t T, N, S;
    float gamma, lambda;
    float *adv, *ret;                       // [T][C]
    float *colsum;                          // scratch [C]
};

// pass 1: column col = e * S + s
RS_PPO_HD void ppo_gae_column(const PpoArgs &A, int col) {
    const size_t C = (size_t)A.N * A.S;
    const float gl = A.gamma * A.lambda;
    float nv = A.last_value[col], last = 0.0f, sum = 0.0f;
    for (int t = A.T - 1; t >= 0; --t) {
        const size_t o = (size_t)t * C + col;
        const float nd = A.done[t] ? 0.0f : 1.0f, v = A.value[o];
        const float delta = A.rew[o] + A.gamma * nd * nv - v;
        last = delta + gl * nd * last;
        A.adv[o] = last;
        A.ret[o] = last + v;
        sum += last;
        nv = v;
    }
    A.colsum[col] = sum;
}

// pass 2, the pieces between the barriers, for thread tid of signal s's workgroup; p[PPO_B] = the workgroup's partial sums
RS_PPO_HD float ppo_partial_mean(const PpoArgs &A, int s, int tid) {
    float a = 0.0f;
    for (int e = tid; e < A.N; e += PPO_B) a += A.colsum[(size_t)e * A.S + s];
    return a;
}
RS_PPO_HD float ppo_partial_var(const PpoArgs &A, int s, int tid, float mean) {
    const size_t C = (size_t)A.N * A.S;
    float a = 0.0f;
    for (int e = tid; e < A.N; e += PPO_B)
        for (int t = 0; t < A.T; ++t) { const float d = A.adv[(size_t)t * C + (size_t)e * A.S + s] - mean; a += d * d; }
    return a;
}
RS_PPO_HD void ppo_tree_step(float *p, int off, int tid) { if (tid < off) p[tid] += p[tid + off]; }
RS_PPO_HD void ppo_standardise(const PpoArgs &A, int s, int tid, float mean, float var_sum) {
    const size_t C = (size_t)A.N * A.S;
    const float den = sqrtf(var_sum / (float)((size_t)A.T * A.N)) + 1e-8f;
    for (int e = tid; e < A.N; e += PPO_B)
        for (int t = 0; t < A.T; ++t) { float &x = A.adv[(size_t)t * C + (size_t)e * A.S + s]; x = (x - mean) / den; }
}

#ifdef __HIPCC__
__global__ void __launch_bounds__(256) rs_ppo_gae_columns_kernel(PpoArgs A) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col < A.N * A.S) ppo_gae_column(A, col);
}

__global__ void __launch_bounds__(PPO_B) rs_ppo_standardise_kernel(PpoArgs A) {
    __shared__ float p[PPO_B];
    const int s = blockIdx.x, tid = threadIdx.x;
    p[tid] = ppo_partial_mean(A, s, tid);
    __syncthreads();
    for (int off = PPO_B / 2; off > 0; off >>= 1) { ppo_tree_step(p, off, tid); __syncthreads(); }
    const float mean = p[0] / (float)((size_t)A.T * A.N);
    __syncthreads();
    p[tid] = ppo_partial_var(A, s, tid, mean);
    __syncthreads();
    for (int off = PPO_B / 2; off > 0; off >>= 1) { ppo_tree_step(p, off, tid); __syncthreads(); }
    ppo_standardise(A, s, tid, mean, p[0]);
}
#else
// the same phases, thread after thread: the host build of the tests (tests/ppo_host), not compiled into the library
static inline void ppo_gae_host(const PpoArgs &A) {
    for (int col = 0; col < A.N * A.S; ++col) ppo_gae_column(A, col);
    float p[PPO_B];
    for (int s = 0; s < A.S; ++s) {
        for (int tid = 0; tid < PPO_B; ++tid) p[tid] = ppo_partial_mean(A, s, tid);
        for (int off = PPO_B / 2; off > 0; off >>= 1)
            for (int tid = 0; tid < off; ++tid) ppo_tree_step(p, off, tid);
        const float mean = p[0] / (float)((size_t)A.T * A.N);
        for (int tid = 0; tid < PPO_B; ++tid) p[tid] = ppo_partial_var(A, s, tid, mean);
        for (int off = PPO_B / 2; off > 0; off >>= 1)
            for (int tid = 0; tid < off; ++tid) ppo_tree_step(p, off, tid);
        const float vs = p[0];
        for (int tid = 0; tid < PPO_B; ++tid) ppo_standardise(A, s, tid, mean, vs);
    }
}
#endif
