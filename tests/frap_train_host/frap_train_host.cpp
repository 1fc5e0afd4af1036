// frap_train_host.cpp -- the host-compilable pieces of the fused MPLight update (resco_amd/csrc/resco_frap_train.h: the tile's phases, its
// gradient entries, the reduction with its two one-time chains, the minibatch draw) compiled for the HOST (TEST INFRASTRUCTURE,
// never shipped).  frap_train_grad runs whole minibatches through them as frap_dqn_tile_kernel and frap_dqn_reduce_kernel do -- the
// lanes of a phase one after the other where the kernel puts a barrier -- and tests/test_frap_train_cpu.py compares the result with
// autograd of the float64 loss (tests/frap_train_ref.py); frap_train_sample is held against the oracle's counter hash.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#define RS_HD
// The headers draw with d_hash, on the device resco_step.h's.  That file is the simulator's kernel and needs its includer's device
// qualifiers, so the host build restates the hash here; the sampling test holds it against the oracle's own implementation.
static inline uint32_t frap_host_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
static inline uint32_t d_hash(uint32_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    uint32_t h = seed;
    const uint32_t w[4] = {a, b, c, d};
    for (int i = 0; i < 4; ++i) {
        uint32_t k = w[i];
        k *= 0xcc9e2d51u; k = frap_host_rotl32(k, 15); k *= 0x1b873593u;
        h ^= k; h = frap_host_rotl32(h, 13); h = h * 5u + 0xe6546b64u;
    }
    h ^= 16u;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
static inline float d_u01(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }
#include "resco_frap.h"
#include "resco_frap_train.h"

// The gradient (packed layout, 1365 + 4 D floats) and the mean loss of the minibatch idx [B][3] = (t, e, s) on the ring obs [T][N][S][1 + 12 D],
// act, rew [T][N][S], done [T].  The stage is filled with NaN before every tile: a phase that read what no earlier phase wrote
// would show in the result.
extern "C" int frap_train_grad(const float *w, const float *wt, int32_t D, int32_t P, const int32_t *pairs, const float *obs, const int16_t *act,
                               const float *rew, const uint8_t *done, int32_t T, int32_t N, int32_t S, const int32_t *idx, int32_t B, double gamma,
                               float *grad, float *loss, float *dy_out /* [B]: every row's d loss / d y, or NULL */) {
    if ((D != 1 && D != 4) || P < 2 || P > FRAP_PMAX || T < 2 || N < 1 || S < 1 || B < 1) return -1;
    const int W = 1 + FRAP_MV * D, tiles = (B + FPT_TM - 1) / FPT_TM, n = FrapOff(D).n;
    std::vector<fpt_t> part((size_t)tiles * FG_N);
    std::vector<FrapStage> stage(1);
    FrapStage &L = stage[0];
    for (int tile = 0; tile < tiles; ++tile) {
        memset((void *)&L, 0xFF, sizeof(L));
        for (int k = 0; k < 144; ++k) fpt_prep(L, w, wt, D, k);
        for (int r = 0; r < FPT_TM; ++r) {
            const int row = tile * FPT_TM + r;
            const bool ok = row < B;
            int t = 0, e = 0, s = 0;
            if (ok) {
                const int32_t *p = idx + (size_t)row * 3;
                t = p[0] < 0 ? 0 : (p[0] >= T ? T - 1 : p[0]);
                e = p[1] < 0 ? 0 : (p[1] >= N ? N - 1 : p[1]);
                s = p[2] < 0 ? 0 : (p[2] >= S ? S - 1 : p[2]);
            }
            const bool boot = ok && !done[t];
            const size_t cur = ((size_t)t * N + e) * S + s, nxt = ((size_t)(t + 1 == T ? 0 : t + 1) * N + e) * S + s;
            for (int q = 0; q < FPT_W; ++q) {
                L.obs[r][q] = ok && q < W ? obs[cur * W + q] : 0.0f;
                L.nxt[r][q] = boot && q < W ? obs[nxt * W + q] : 0.0f;
            }
            const int a = ok ? (int)act[cur] : 0;
            L.ok[r] = ok; L.boot[r] = boot;
            L.g[r] = a < 0 ? 0 : (a >= P ? P - 1 : a);
            L.rew[r] = ok ? rew[cur] : 0.0f;
        }
#define FPT_LANES(stmt) for (int r = 0; r < FPT_TM; ++r) for (int j = 0; j < FPT_G; ++j) { stmt; }
        FPT_LANES(fpt_target_ab(L, wt, D, P, pairs, r, j))
        FPT_LANES(fpt_target_q(L, wt, D, P, pairs, r, j))
        FPT_LANES(if (j == 0) fpt_target_value(L, P, gamma, r); if (j < FRAP_MV) fpt_mv_forward(L, w, D, P, pairs, r, j))
        FPT_LANES(fpt_pair_forward(L, w, D, P, pairs, r, j))
        FPT_LANES(fpt_item_forward(L, w, D, P, pairs, r, j))
        FPT_LANES(if (j == 0) fpt_row_loss(L, P, B, r))
        FPT_LANES(fpt_item_backward(L, w, D, P, r, j))
        FPT_LANES(if (j == L.g[r]) fpt_row_backward(L, w, D, P, r))
        FPT_LANES(if (j < FRAP_MV) fpt_mv_backward(L, w, D, P, pairs, r, j))
#undef FPT_LANES
        for (int r = 0; dy_out && r < FPT_TM; ++r)
            if (L.ok[r]) dy_out[tile * FPT_TM + r] = (float)L.dy[r];
        for (int e = 0; e < FG_N; ++e) part[(size_t)tile * FG_N + e] = frap_tile_entry(L, P, D, e);
    }
    fpt_t gPE[32], gR[2 * FRAP_C];
    for (int k = 0; k < 32; ++k) gPE[k] = frap_reduce_entry(part.data(), tiles, FG_PE + k);
    for (int k = 0; k < 2 * FRAP_C; ++k) gR[k] = frap_reduce_entry(part.data(), tiles, FG_DR + k);
    for (int i = 0; i < n; ++i) grad[i] = frap_grad_element(w, D, i, part.data(), tiles, gPE, gR);
    *loss = frap_loss_mean(part.data(), tiles, B);
    return 0;
}

// the minibatch of update u: idx [B][3], as frap_dqn_sample_kernel fills it
extern "C" int frap_train_sample(uint32_t seed, uint32_t u, int32_t T, int32_t N, int32_t S, int32_t head, int32_t count, int32_t B, int32_t *idx) {
    if (S < 1 || T < 2 || N < 1 || head < 0 || head >= T || count < 2 || count > T || B < 0) return -1;
    for (int i = 0; i < B; ++i) frap_dqn_sample_index(seed, u, (uint32_t)i, T, N, S, head, count, idx + (size_t)i * 3);
    return 0;
}

// the tile size the GPU tests name their batch sizes from
extern "C" int frap_train_tile_rows(void) { return FPT_TM; }
