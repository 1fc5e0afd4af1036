// group_train_host.cpp -- the launch-free pieces of the in-library training loop (resco_amd/csrc/resco_group_train.h: the pack's
// analytic fragment index and conversion, the recorder's and the target sync's bodies, the bookkeeping of a step) compiled for the
// HOST (TEST INFRASTRUCTURE, never shipped).  tests/test_group_train_cpu.py compares them with idqn_fused.repack_index /
// pack_idqn_weights, with numpy and with a Python restatement of the tools' loop.  The bodies take (first index, stride) as a kernel's
// thread does: `threads` here plays the grid, one "thread" after the other.
#include "resco_group_train.h"

extern "C" int gt_host_pack_index(int32_t which, int32_t lmax, int32_t amax, int32_t *out) {
    if (which < 0 || which > 2 || lmax < 2 || lmax > 17 || amax < 1 || amax > 8) return -1;
    const int n = gt_pack_count(which, lmax);
    for (int o = 0; o < n; ++o) out[o] = gt_pack_src(which, o, lmax, amax);
    return n;
}

extern "C" int gt_host_pack(int32_t S, int32_t lmax, int32_t amax, const float *fc1_w, const float *fc2_w, const float *fc3_w, const float *fc3_b,
                            uint16_t *w1, uint16_t *w2, uint16_t *w3, float *b3, int32_t threads) {
    if (S < 1 || lmax < 2 || lmax > 17 || amax < 1 || amax > 8 || threads < 1) return -1;
    const GtPack P{fc1_w, fc2_w, fc3_w, fc3_b, w1, w2, w3, b3, lmax, amax};
    const int n = gt_pack_units(lmax);
    for (int s = 0; s < S; ++s)
        for (int i0 = 0; i0 < threads; ++i0)
            for (int u = i0; u < n; u += threads) gt_pack_unit(P, s, u);
    return n;
}

extern "C" uint16_t gt_host_f2h(float f) { return gt_f2h(f); }

extern "C" int gt_host_record(const void *obs_src, void *obs_dst, int32_t n_obs, int32_t obs_kind, int32_t vec, const int32_t *act_src, int16_t *act_dst,
                              const void *rew_src, float *rew_dst, float *ret, int32_t n_sig, int32_t rew_i32, uint8_t *done_dst, int32_t done,
                              int32_t threads) {
    if (threads < 1 || (vec && ((((uintptr_t)obs_src | (uintptr_t)obs_dst) & 15) != 0))) return -1;
    const GtRec R{obs_src, obs_dst, n_obs, obs_kind, vec, act_src, act_dst, rew_src, rew_dst, ret, n_sig, rew_i32, done_dst, done};
    for (int i0 = 0; i0 < threads; ++i0) gt_record(R, i0, threads);
    return 0;
}

extern "C" int gt_host_sync(const float *src, float *dst, int64_t n, int32_t threads) {
    if (threads < 1) return -1;
    GtSync Y{};
    Y.count = 1; Y.src[0] = src; Y.dst[0] = dst; Y.n[0] = n;
    for (int i0 = 0; i0 < threads; ++i0) gt_sync_tensor(Y, 0, i0, threads);
    return 0;
}

// the plans of steps 0 .. n_steps - 1 of one call: out [n_steps][8] = slot, head, count, sync, update, done, key, epsilon's float bits
extern "C" int gt_host_plan(int32_t capacity, int64_t pool, int32_t batch, int32_t target_update, int32_t updates_per_step, int64_t t0, int32_t head,
                            int32_t count, int32_t done_step, double eps_start, double eps_end, int32_t decay_steps, int32_t n_steps, uint32_t *out) {
    if (capacity < 2 || target_update < 1 || n_steps < 1) return -1;
    GtLoop L{};
    L.capacity = capacity; L.batch = batch; L.target_update = target_update; L.updates_per_step = updates_per_step; L.decay_steps = decay_steps;
    L.done_step = done_step; L.pool = pool; L.t0 = t0; L.head = head; L.count = count; L.eps_start = eps_start; L.eps_end = eps_end;
    for (int k = 0; k < n_steps; ++k) {
        const GtStep s = gt_plan(L, k);
        uint32_t *o = out + (size_t)k * 8;
        o[0] = (uint32_t)s.slot; o[1] = (uint32_t)s.head; o[2] = (uint32_t)s.count; o[3] = (uint32_t)s.sync; o[4] = (uint32_t)s.update;
        o[5] = (uint32_t)s.done; o[6] = s.key; o[7] = gt_f2u(s.epsilon);
    }
    return 0;
}
