// ppo_loop_host.cpp -- the launch-free pieces of the in-library PPO training loop (resco_amd/csrc/resco_ppo_loop.h: the shuffle, the
// done bytes, the bookkeeping of a step; resco_group_train.h: the actor-critic pack's index and values) compiled for the HOST (TEST
// INFRASTRUCTURE, never shipped).  tests/test_ppo_loop_cpu.py compares them with ippo_fused.ippo_repack_index / pack_ippo_weights and
// with a Python restatement of the tool's loop; tests/test_gpu_ppo_loop.py compares rs_ppo_perm with gp_host_perm.
#include <stdint.h>

// The header draws with d_hash, on the device resco_step.h's.  That file is the simulator's kernel and needs its includer's device
// qualifiers, so the host build restates the hash here (as tests/dqn_train_host does; the permutation test holds it against
// resco_amd.sim._murmur, the package's own restatement).
static inline uint32_t gp_host_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
static inline uint32_t d_hash(uint32_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    uint32_t h = seed;
    const uint32_t w[4] = {a, b, c, d};
    for (int i = 0; i < 4; ++i) {
        uint32_t k = w[i];
        k *= 0xcc9e2d51u; k = gp_host_rotl32(k, 15); k *= 0x1b873593u;
        h ^= k; h = gp_host_rotl32(h, 13); h = h * 5u + 0xe6546b64u;
    }
    h ^= 16u;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
#include "resco_ppo_loop.h"

extern "C" uint32_t gp_host_hash(uint32_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return d_hash(seed, a, b, c, d); }
extern "C" int gp_host_half_bits(int32_t n) { return n < 1 ? -1 : gp_perm_half_bits(n); }

// perm [epochs][n] as rs_ppo_perm_kernel fills it: `threads` plays the grid, one "thread" after the other
extern "C" int gp_host_perm(int32_t n, int32_t epochs, uint32_t seed, uint32_t key, int32_t *perm, int32_t threads) {
    if (n < 1 || epochs < 1 || !perm || threads < 1) return -1;
    for (int e = 0; e < epochs; ++e)
        for (int i0 = 0; i0 < threads; ++i0) gp_perm_row(seed, key, e, n, perm, i0, threads);
    return 0;
}

extern "C" int gp_host_done(uint8_t *done, int32_t m, int32_t hit, int32_t threads) {
    if (threads < 1) return -1;
    for (int i0 = 0; i0 < threads; ++i0) gp_done(done, m, hit, i0, threads);
    return 0;
}

// the plans of steps 0 .. n_steps - 1 of one call: out [n_steps][5] = slot, done, update, update_key, key
extern "C" int gp_host_plan(int32_t T, int32_t slot0, int32_t done_step, int64_t t0, int64_t update0, int32_t n_steps, uint32_t *out) {
    if (T < 1 || slot0 < 0 || slot0 >= T || n_steps < 1) return -1;
    const GpLoop L{T, slot0, done_step, t0, update0};
    for (int k = 0; k < n_steps; ++k) {
        const GpStep s = gp_plan(L, k);
        uint32_t *o = out + (size_t)k * 5;
        o[0] = (uint32_t)s.slot; o[1] = (uint32_t)s.done; o[2] = (uint32_t)s.update; o[3] = s.update_key; o[4] = s.key;
    }
    return 0;
}

// value != 0: the actor-critic pack's index (w3 into the virtual [64][9] matrix), else the IDQN pack's
extern "C" int gp_host_pack_index(int32_t value, int32_t which, int32_t lmax, int32_t amax, int32_t *out) {
    if (which < 0 || which > 2 || lmax < 2 || lmax > 17 || amax < 1 || amax > 8) return -1;
    const int n = gt_pack_count(which, lmax);
    for (int o = 0; o < n; ++o) out[o] = value ? gt_pack_src_value(which, o, lmax, amax) : gt_pack_src(which, o, lmax, amax);
    return n;
}

extern "C" int gp_host_pack_value(int32_t S, int32_t lmax, int32_t amax, const float *fc1_w, const float *fc2_w, const float *fc3_w, const float *fc3_b,
                                  const float *v_w, const float *v_b, uint16_t *w1, uint16_t *w2, uint16_t *w3, float *b3, int32_t threads) {
    if (S < 1 || lmax < 2 || lmax > 17 || amax < 1 || amax > 8 || threads < 1) return -1;
    const GtPackValue P{{fc1_w, fc2_w, fc3_w, fc3_b, w1, w2, w3, b3, lmax, amax}, v_w, v_b};
    const int n = gt_pack_units(lmax);
    for (int s = 0; s < S; ++s)
        for (int i0 = 0; i0 < threads; ++i0)
            for (int u = i0; u < n; u += threads) gt_pack_unit_value(P, s, u);
    return n;
}
