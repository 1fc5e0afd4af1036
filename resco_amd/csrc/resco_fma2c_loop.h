// resco_fma2c_loop.h -- what joins the fused FMA2C acting kernel (resco_fma2c.h), the step kernel and the fused A2C update
// (resco_fma2c_train.h) into a training loop that one call enqueues (rs_group_fma2c_train of include/resco_sim.h): the reward of
// rewards.fma2c / fma2c_full for all agents with the recorder of a step (rs_fma2c_record), the done words of a segment, the state
// hand-over of an update and the launch-free bookkeeping of a step.
//
// What it replaces, per env-step of tools/fma2c_train.py --device-update: VecMultiSignal.fma2c_rewards (five casts, a cat and a dense
// [N, 3 O + 2 S] @ [3 O + 2 S, K] product against a matrix that is almost all zeros), the stack of its K columns, the cat + long() of
// the actions, `ret += rew`, the two copy_ into the segment and the host-to-device scalar write of dones_dev[t + 1].
//
// Everything here is plain C++ over (first index, stride) that a host compiler builds as well (tests/fma2c_loop_host).  The build's
// contraction is off (-ffp-contract=off, both compilers), so `acc = acc + g * w` is a rounded product and a rounded sum on either
// side: host and device give the same bits.
#pragma once
#include "resco_group_train.h"

// ------------------------------------------------------------------------------------------------ the reward and the recorder
// The reward matrix W [3 O + 2 S][K] of VecMultiSignal._fma2c_tables (resco_amd/multi_signal.py: fma2c_reward_matrix) as the non-zeros
// of its columns, rows ascending (CSR over the K agents, managers first): column k is off[k] .. off[k + 1] - 1 of (idx, w).  The row
// vector G of an environment is never materialised; row r of it reads
//     r < O        lane_agg[e][r][0]           (queue)
//     r < 2 O      lane_agg[e][r - O][3]       (max_wait)
//     r < 3 O      (float)lane_arr[e][r - 2 O] (lane arrivals)
//     r < 3 O + S  (float)arrivals[e][r - 3 O]
//     otherwise    (float)departures[e][r - 3 O - S]
// The table's contents are NOT checked here (0 <= idx < 3 O + 2 S, off non-decreasing from 0): whoever builds the table does
// (resco_amd/sim.py: Fma2cRewardTable asserts it before the upload).
struct FlRec {
    int32_t K, M, O, S, N;                  // agents, managers, observed lanes, signals, environments
    const int32_t *off, *idx;               // [K + 1], [off[K]]
    const float *w;                         // [off[K]]
    const float *lane_agg;                  // [N][O][5]
    const int32_t *lane_arr, *arrivals, *departures;       // [N][O], [N][S], [N][S]
    const int32_t *macts, *actions;         // [N][M] the managers' actions of these environments, [N][S] the workers' (RS_BUF_ACTIONS)
    float *rew;                             // [N][K] the RAW reward (the learner normalises and clips)
    int32_t *acts;                          // [N][K] or NULL
    float *ret;                             // [N][K] or NULL: ret += reward
};
GT_HD float fl_g(const FlRec &R, int e, int r) {
    const int O = R.O, S = R.S;
    if (r < O) return R.lane_agg[((size_t)e * O + r) * 5];
    if (r < 2 * O) return R.lane_agg[((size_t)e * O + (r - O)) * 5 + 3];
    if (r < 3 * O) return (float)R.lane_arr[(size_t)e * O + (r - 2 * O)];
    if (r < 3 * O + S) return (float)R.arrivals[(size_t)e * S + (r - 3 * O)];
    return (float)R.departures[(size_t)e * S + (r - 3 * O - S)];
}
// the column's entries in stored order.  A thread's entries are a chain of dependent loads (idx, then G): four entries are read
// before their sums so that their loads are in flight together; the sums themselves stay one after the other, in stored order.
GT_HD float fl_reward(const FlRec &R, int e, int k) {
    float acc = 0.0f;
    int q = R.off[k];
    const int end = R.off[k + 1];
    for (; q + 4 <= end; q += 4) {
        const int r0 = R.idx[q], r1 = R.idx[q + 1], r2 = R.idx[q + 2], r3 = R.idx[q + 3];
        const float w0 = R.w[q], w1 = R.w[q + 1], w2 = R.w[q + 2], w3 = R.w[q + 3];
        const float g0 = fl_g(R, e, r0), g1 = fl_g(R, e, r1), g2 = fl_g(R, e, r2), g3 = fl_g(R, e, r3);
        acc = acc + g0 * w0;
        acc = acc + g1 * w1;
        acc = acc + g2 * w2;
        acc = acc + g3 * w3;
    }
    for (; q < end; ++q) acc = acc + fl_g(R, e, R.idx[q]) * R.w[q];
    return acc;
}
// element i = e * K + k of the three outputs, for the "threads" i0, i0 + stride, ..
GT_HD void fl_record(const FlRec &R, int64_t i0, int64_t stride) {
    const int64_t n = (int64_t)R.N * R.K;
    for (int64_t i = i0; i < n; i += stride) {
        const int e = (int)(i / R.K), k = (int)(i - (int64_t)e * R.K);
        const float r = fl_reward(R, e, k);
        R.rew[i] = r;
        if (R.acts) R.acts[i] = k < R.M ? R.macts[(size_t)e * R.M + k] : R.actions[(size_t)e * R.S + (k - R.M)];
        if (R.ret) R.ret[i] = R.ret[i] + r;
    }
}

// ------------------------------------------------------------------------------------------------ the done words
// gt_done of resco_group_train.h over the learner's int32 dones [T + 1] (resco_fma2c_train.h): the post-step dones of the slots a call
// fills from one slot on to the next update, under the name the host build of the tests calls (tests/fma2c_loop_host)
GT_HD void fl_done(int32_t *done, int32_t m, int32_t hit, int i0, int stride) { gt_done(done, m, hit, i0, stride); }

// ------------------------------------------------------------------------------------------------ the state hand-over
// After an update the acting state becomes the next segment's start state (states_bw <- states_fw); at an episode's end the start
// state is zeroed right afterwards (model.reset()), which leaves zeros: one pass does either.
GT_HD void fl_state(float *dst, const float *src, size_t n, int zero, size_t i0, size_t stride) {
    for (size_t i = i0; i < n; i += stride) dst[i] = zero ? 0.0f : src[i];
}

// ------------------------------------------------------------------------------------------------ the bookkeeping of a step
// Step k of a call that starts at env-step t0 with slot0 slots of the segment filled: what FusedA2CLearner.observe decides on the
// host.  The step is recorded into `slot`; `done`: the horizon is reached at this step (only a call's last step can be: a call does
// not run past a done); `update`: the step fills the segment's last slot or ends the episode, and the update that follows runs on the
// first n_slots slots; key: the step's key of the policy's draws.  A segment is cut at the episode's end: the caller goes on with
// slot 0 after a done, and with (slot0 + n) mod T otherwise, and t0 + n either way -- then any split of the same steps into calls
// gives the same plans.
struct FlStep {
    int32_t slot, done, update, n_slots;
    uint32_t key;
};
GT_HD FlStep fl_plan(int32_t T, int32_t slot0, int64_t t0, int32_t done_step, int32_t k) {
    FlStep s;
    s.slot = (int32_t)(((int64_t)slot0 + k) % T);
    s.done = k == done_step;
    s.update = s.slot == T - 1 || s.done;
    s.n_slots = s.slot + 1;
    s.key = (uint32_t)((t0 + k) & 0xFFFFFFFFll);
    return s;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------------ kernels (grid-stride: any grid covers any size)
// one thread per (environment, agent): a few hundred loads out of cache-resident buffers, no LDS, no atomics, no workspace
__global__ void __launch_bounds__(256) rs_fma2c_record_kernel(FlRec R) {
    fl_record(R, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
}
// dones[0] = dones[n]: the post-step done of an update's last slot is the pre-step done of the next segment's first
__global__ void rs_fma2c_done_carry_kernel(int32_t *dones, int32_t n) {
    if (blockIdx.x == 0 && threadIdx.x == 0) dones[0] = dones[n];
}
__global__ void __launch_bounds__(256) rs_fma2c_state_kernel(float *dst, const float *src, size_t n, int zero) {
    fl_state(dst, src, n, zero, (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256);
}
#endif
