// dqn_per_host.cpp -- the scalar pieces of prioritised replay in the fused DQN update (resco_amd/csrc/resco_dqn_per.h: the uniform
// from the counter hash, the weight of a row, the priority of a row, the beta schedule, the sequential restatement of the two-stage
// pick) compiled for the HOST (TEST INFRASTRUCTURE, never shipped).  tests/test_dqn_per_cpu.py compares them with numpy in float64.
#include <stdint.h>

// The header draws with d_hash, on the device resco_step.h's; the host build restates it (as tests/dqn_train_host does) and the
// test holds it against the oracle's own implementation.
static inline uint32_t per_host_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
static inline uint32_t d_hash(uint32_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    uint32_t h = seed;
    const uint32_t w[4] = {a, b, c, d};
    for (int i = 0; i < 4; ++i) {
        uint32_t k = w[i];
        k *= 0xcc9e2d51u; k = per_host_rotl32(k, 15); k *= 0x1b873593u;
        h ^= k; h = per_host_rotl32(h, 13); h = h * 5u + 0xe6546b64u;
    }
    h ^= 16u;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
#include "resco_dqn_per.h"

extern "C" uint32_t dqn_per_host_seed_constant(void) { return DQN_PER_SEED; }
extern "C" float dqn_per_host_uniform(uint32_t seed, uint32_t u, uint32_t s, uint32_t i, uint32_t j) { return dqn_per_uniform(seed, u, s, i, j); }
extern "C" float dqn_per_host_beta(double beta0, int64_t beta_steps, int64_t u) { return dqn_per_beta(beta0, beta_steps, u); }
extern "C" float dqn_per_host_priority(float ad, float eps, float alpha) { return dqn_per_priority(ad, eps, alpha); }
extern "C" float dqn_per_host_row_weight(float q, float Z, float M, float beta) { return dqn_per_row_weight(q, Z, M, beta); }

// the two-stage pick on prio [T][N][S] and ssum [T][S] for signal s at ring position (head, count) with uniforms (r0, r1) and
// Z = the sequential total of the valid slots' ssum: out = (slot, environment)
extern "C" int dqn_per_host_pick(const float *prio, const float *ssum, int32_t T, int32_t N, int32_t S, int32_t s, int32_t head, int32_t count, float r0,
                                 float r1, int32_t *out) {
    if (!prio || !ssum || !out || T < 2 || N < 1 || S < 1 || s < 0 || s >= S || head < 0 || head >= T || count < 2 || count > T) return -1;
    // the valid slots k = 0 .. count - 2 from the oldest, gathered so that the pick sees them in order
    float valid[4096];
    if (count - 1 > 4096) return -1;
    float Z = 0.0f;
    for (int k = 0; k < count - 1; ++k) {
        valid[k] = ssum[(size_t)((head - count + T + k) % T) * S + s];
        Z = Z + valid[k];
    }
    const int k = dqn_per_pick_seq(valid, count - 1, 1, r0 * Z);
    const int t = (head - count + T + k) % T;
    out[0] = t;
    out[1] = dqn_per_pick_seq(prio + (size_t)t * N * S + s, N, S, r1 * ssum[(size_t)t * S + s]);
    return 0;
}
