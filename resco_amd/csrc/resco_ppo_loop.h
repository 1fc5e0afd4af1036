// resco_ppo_loop.h -- what joins the actor-critic rollout, the fused GAE, the fused PPO update and the actor-critic pack into a
// training loop that one call enqueues (rs_group_ppo_train of include/resco_sim.h), beside the pack itself (resco_group_train.h:
// gt_pack_unit_value): the shuffle of an update (rs_ppo_perm), the done bytes of a segment and the launch-free bookkeeping of a step.
//
// What it replaces, per segment of tools/ippo_train.py --device-update: two host synchronisations, the dataset glue of
// BatchedPPOLearner.dataset_from_rollout (casts, empty_like), `epochs` torch.randperm calls and FusedIPPO.refresh_on_device (three
// index_select + mul_ + casting copy_, the fc3_with_value scatter and the b3 fill).
//
// Everything here is plain C++ that a host compiler builds as well (tests/ppo_loop_host).  The shuffle draws with d_hash, on the
// device resco_step.h's; the host build of the tests brings one of its own, as for resco_dqn_train.h.
#pragma once
#include "resco_group_train.h"

#ifdef __HIPCC__
#define GP_DEV __device__ static inline     // (d_hash of resco_step.h is a device function)
#else
#define GP_DEV static inline
#endif

// ------------------------------------------------------------------------------------------------ the shuffle
// Row e of the permutations of update `key`: a bijection of 0 .. n - 1 that is a pure function of (seed, key, e, n), every element
// computed on its own -- no sort, no atomics, no workspace.  A four-round Feistel network over 2 h bits, h = max(1, ceil(bits(n - 1)
// / 2)), is a bijection of 0 .. 4^h - 1 whatever its round function is; the round function is the project's counter hash.  Walking
// the cycle of i until a value below n turns up restricts it to a bijection of 0 .. n - 1: the walk leaves 0 .. n - 1 at i and the
// first return to it is unique to i (two starts that met at one value would have met one step earlier, back to the starts).  It
// ends, because the cycle of a bijection returns to i < n itself; 4^h < 4 n, so fewer than four applications on average.  n = 1: {0}.
// n below 2^31 gives h <= 16: a half fits 16 bits, and (round << 16) | half is a word of the hash that no other round shares.
#define GP_PERM_SALT 0x9C3A71E5u        // distinct from the minibatch draws of the DQN learners (resco_frap_train.h) and the policies' draws
GT_HD int gp_perm_half_bits(int32_t n) {
    int bits = 0;
    for (uint32_t m = (uint32_t)(n - 1); m; m >>= 1) ++bits;
    const int h = (bits + 1) / 2;
    return h < 1 ? 1 : h;
}
GP_DEV uint32_t gp_perm_feistel(uint32_t x, int h, uint32_t seed, uint32_t key, uint32_t e, uint32_t n) {
    const uint32_t mask = (1u << h) - 1u;
    uint32_t l = x >> h, r = x & mask;
    for (uint32_t round = 0; round < 4; ++round) {
        const uint32_t f = d_hash(seed ^ GP_PERM_SALT, key, e, n, (round << 16) | r) & mask;
        const uint32_t t = l ^ f;
        l = r; r = t;
    }
    return (l << h) | r;
}
GP_DEV int32_t gp_perm_at(uint32_t seed, uint32_t key, int32_t e, int32_t n, int32_t i) {
    const int h = gp_perm_half_bits(n);
    uint32_t x = (uint32_t)i;
    do x = gp_perm_feistel(x, h, seed, key, (uint32_t)e, (uint32_t)n); while (x >= (uint32_t)n);
    return (int32_t)x;
}
// perm [epochs][n], row e, for the "threads" i0, i0 + stride, ..
GP_DEV void gp_perm_row(uint32_t seed, uint32_t key, int32_t e, int32_t n, int32_t *perm, int64_t i0, int64_t stride) {
    int32_t *row = perm + (size_t)e * (size_t)n;
    for (int64_t i = i0; i < n; i += stride) row[i] = gp_perm_at(seed, key, e, n, (int32_t)i);
}

// ------------------------------------------------------------------------------------------------ the done bytes
// gt_done of resco_group_train.h over bytes, under the name the host build of the tests calls (tests/ppo_loop_host)
GT_HD void gp_done(uint8_t *done, int32_t m, int32_t hit, int i0, int stride) { gt_done(done, m, hit, i0, stride); }

// ------------------------------------------------------------------------------------------------ the bookkeeping of a step
// Step k of a call that starts at env-step t0 with slot0 slots of the segment filled and update0 updates finished: what one iteration
// of tools/ippo_train.py's --device-update loop decides on the host.  The step is recorded into `slot`; `done`: the horizon is
// reached at this step; `update`: the step fills the segment's last slot, and the update that follows shuffles with update_key (the
// number of updates finished before it); key: the step's key of the actor-critic draws.  A function of t0 + k, slot0 + k and update0
// only: any split of the same steps into calls gives the same plans, when the caller advances (slot0 + n) mod T, t0 + n and
// update0 + (slot0 + n) / T.
struct GpLoop {
    int32_t T, slot0, done_step;
    int64_t t0, update0;
};
struct GpStep {
    int32_t slot, done, update;
    uint32_t update_key, key;
};
GT_HD GpStep gp_plan(const GpLoop &L, int32_t k) {
    GpStep s;
    const int64_t pos = (int64_t)L.slot0 + k;
    s.slot = (int32_t)(pos % L.T);
    s.done = k == L.done_step;
    s.update = s.slot == L.T - 1;
    s.update_key = (uint32_t)((L.update0 + pos / L.T) & 0xFFFFFFFFll);
    s.key = (uint32_t)((L.t0 + k) & 0xFFFFFFFFll);
    return s;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------------ kernels (grid-stride: any grid covers any size)
// grid (x, epochs)
__global__ void __launch_bounds__(256) rs_ppo_perm_kernel(uint32_t seed, uint32_t key, int32_t n, int32_t *perm) {
    gp_perm_row(seed, key, (int32_t)blockIdx.y, n, perm, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
}
#endif
