// dqn_train_host.cpp -- the scalar pieces of the fused DQN update (resco_amd/csrc/resco_dqn_train.h: the per-row loss gradient, the
// minibatch draw) compiled for the HOST (TEST INFRASTRUCTURE, never shipped).  tests/test_dqn_train_cpu.py compares them with
// autograd of the float64 loss and with the oracle's counter hash (tests/dqn_train_ref.py).
#include <stdint.h>

// The header draws with d_hash, on the device resco_step.h's.  That file is the simulator's kernel and needs its includer's device
// qualifiers, so the host build restates the hash here; the sampling test holds it against the oracle's own implementation.
static inline uint32_t dqn_host_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
static inline uint32_t d_hash(uint32_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    uint32_t h = seed;
    const uint32_t w[4] = {a, b, c, d};
    for (int i = 0; i < 4; ++i) {
        uint32_t k = w[i];
        k *= 0xcc9e2d51u; k = dqn_host_rotl32(k, 15); k *= 0x1b873593u;
        h ^= k; h = dqn_host_rotl32(h, 13); h = h * 5u + 0xe6546b64u;
    }
    h ^= 16u;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
#include "resco_dqn_train.h"

// n samples of one signal with A actions: q / dq [n][8]
extern "C" int dqn_train_rows(const float *q, int32_t A, int32_t n, const int32_t *action, const float *tgt, float batch, float *dq, float *terms) {
    if (A < 1 || A > PPT_AMAX || n < 0) return -1;
    for (int i = 0; i < n; ++i) dqn_row_loss_grad(q + i * PPT_AMAX, A, action[i], tgt[i], batch, dq + i * PPT_AMAX, terms + i);
    return 0;
}

// the minibatch of update u: idx [B][S][2], as dqn_sample_kernel fills it
extern "C" int dqn_train_sample(uint32_t seed, uint32_t u, int32_t S, int32_t T, int32_t N, int32_t head, int32_t count, int32_t B, int32_t *idx) {
    if (S < 1 || T < 2 || N < 1 || head < 0 || head >= T || count < 2 || count > T || B < 0) return -1;
    for (int i = 0; i < B; ++i)
        for (int s = 0; s < S; ++s) dqn_sample_index(seed, u, (uint32_t)s, (uint32_t)i, T, N, head, count, idx + ((size_t)i * S + s) * 2);
    return 0;
}
