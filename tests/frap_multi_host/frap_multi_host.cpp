// frap_multi_host.cpp -- the host-compilable pieces of the multi-map MPLight update (resco_amd/csrc/resco_frap_multi.h: the draw over
// several rings, the grouping, the prefix table, the row load) compiled for the HOST next to those of resco_frap_train.h (TEST
// INFRASTRUCTURE, never shipped).  frap_multi_grad runs whole grouped minibatches through them as frap_multi_tile_kernel and
// frap_multi_reduce_kernel do; frap_multi_sample places the draws as frap_multi_sample_kernel does, a chunk at a time;
// tests/test_mplight_multi_cpu.py compares both with the yardstick of tests/frap_train_ref.py and a Python restatement of the draw.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#define RS_HD
// the simulator's counter hash, restated as in tests/frap_train_host (resco_step.h needs its includer's device qualifiers)
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
#include "resco_frap_multi.h"

extern "C" uint32_t frap_multi_hash_of(uint32_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return frap_multi_hash(seed, a, b, c, d); }
extern "C" uint32_t frap_multi_d_hash_of(uint32_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return d_hash(seed, a, b, c, d); }
extern "C" int frap_multi_max_maps(void) { return FPM_MAPS; }

static int pools_of(int32_t n_maps, const int32_t *T, const int32_t *N, const int32_t *S, const int32_t *head, const int32_t *count, FrapMultiPools &Q) {
    if (n_maps < 1 || n_maps > FPM_MAPS) return -1;
    Q = FrapMultiPools{};
    Q.n_maps = n_maps;
    for (int m = 0; m < n_maps; ++m) {
        if (T[m] < 2 || N[m] < 1 || S[m] < 1 || head[m] < 0 || head[m] >= T[m] || count[m] < 0 || count[m] > T[m]) return -1;
        const uint64_t pool = frap_multi_pool(N[m], S[m], count[m]);
        if (pool >= (1ull << 31)) return -1;
        Q.cum[m + 1] = Q.cum[m] + pool;
        Q.T[m] = T[m]; Q.N[m] = N[m]; Q.S[m] = S[m]; Q.head[m] = head[m]; Q.count[m] = count[m];
    }
    return Q.cum[n_maps] == 0 ? -1 : 0;
}

// the minibatch of update u: idx [B][4] grouped by map and counts [n_maps], placed as the kernel places them: the group bases from
// frap_multi_counts, then chunk by chunk base + the rows taken in earlier chunks + the rank inside the chunk
extern "C" int frap_multi_sample(uint32_t seed, uint32_t u, int32_t n_maps, const int32_t *T, const int32_t *N, const int32_t *S, const int32_t *head,
                                 const int32_t *count, int32_t B, int32_t *idx, int32_t *counts) {
    FrapMultiPools Q;
    if (pools_of(n_maps, T, N, S, head, count, Q) || B < 0) return -1;
    frap_multi_counts(seed, u, B, Q, counts);
    int32_t fill[FPM_MAPS];
    for (int m = 0, row = 0; m < n_maps; ++m) { Q.base[m] = fill[m] = row; row += counts[m]; }
    for (int c0 = 0; c0 < B; c0 += FPM_CHUNK) {
        int32_t rows[FPM_CHUNK][4];
        const int n = B - c0 < FPM_CHUNK ? B - c0 : FPM_CHUNK;
        for (int k = 0; k < n; ++k) frap_multi_sample_index(seed, u, (uint32_t)(c0 + k), Q, rows[k]);
        for (int k = 0; k < n; ++k) {
            int rank = 0;
            for (int j = 0; j < k; ++j) rank += rows[j][0] == rows[k][0];
            const int pos = fill[rows[k][0]] + rank;
            if (pos < 0 || pos >= B) return -2;
            memcpy(idx + (size_t)pos * 4, rows[k], sizeof(rows[k]));
        }
        for (int k = 0; k < n; ++k) fill[rows[k][0]] += 1;
    }
    return 0;
}

// The gradient (packed layout) and the mean loss of the grouped minibatch idx [B][4] = (map, t, e, s), counts [n_maps], on the maps'
// rings (arrays of n_maps pointers and sizes).  The stage is filled with NaN bytes before every tile.
extern "C" int frap_multi_grad(const float *w, const float *wt, int32_t D, int32_t n_maps, const int32_t *P, const int32_t *const *pairs,
                               const float *const *obs, const int16_t *const *act, const float *const *rew, const uint8_t *const *done, const int32_t *T,
                               const int32_t *N, const int32_t *S, const int32_t *idx, const int32_t *counts, double gamma, float *grad, float *loss) {
    if ((D != 1 && D != 4) || n_maps < 1 || n_maps > FPM_MAPS) return -1;
    FrapMultiBatch B{};
    B.n_maps = n_maps; B.idx = idx;
    for (int m = 0; m < n_maps; ++m) {
        if (P[m] < 2 || P[m] > FRAP_PMAX || T[m] < 2 || N[m] < 1 || S[m] < 1 || counts[m] < 0) return -1;
        B.map[m] = FrapMultiRing{obs[m], act[m], rew[m], done[m], pairs[m], T[m], N[m], S[m], 1 + FRAP_MV * D, P[m], 0, 0, 0};
    }
    const int tiles = frap_multi_layout(B, counts), n = FrapOff(D).n;
    if (B.B < 1) return -1;
    std::vector<fpt_t> part((size_t)tiles * FG_N);
    std::vector<FrapStage> stage(1);
    FrapStage &L = stage[0];
    for (int tile = 0; tile < tiles; ++tile) {
        const FrapMultiRing &R = B.map[frap_multi_tile_map(B, tile)];
        const int Pm = R.P;
        const int32_t *pr = R.pairs;
        memset((void *)&L, 0xFF, sizeof(L));
        for (int k = 0; k < 144; ++k) fpt_prep<FPM_TAG>(L, w, wt, D, k);
#define FPT_LANES(stmt) for (int r = 0; r < FPT_TM; ++r) for (int j = 0; j < FPT_G; ++j) { stmt; }
        FPT_LANES(frap_multi_load(L, R, idx, tile, r, j))
        FPT_LANES(fpt_target_ab<FPM_TAG>(L, wt, D, Pm, pr, r, j))
        FPT_LANES(fpt_target_q<FPM_TAG>(L, wt, D, Pm, pr, r, j))
        FPT_LANES(if (j == 0) fpt_target_value<FPM_TAG>(L, Pm, gamma, r); if (j < FRAP_MV) fpt_mv_forward<FPM_TAG>(L, w, D, Pm, pr, r, j))
        FPT_LANES(fpt_pair_forward<FPM_TAG>(L, w, D, Pm, pr, r, j))
        FPT_LANES(fpt_item_forward<FPM_TAG>(L, w, D, Pm, pr, r, j))
        FPT_LANES(if (j == 0) fpt_row_loss<FPM_TAG>(L, Pm, B.B, r))
        FPT_LANES(fpt_item_backward<FPM_TAG>(L, w, D, Pm, r, j))
        FPT_LANES(if (j == L.g[r]) fpt_row_backward<FPM_TAG>(L, w, D, Pm, r))
        FPT_LANES(if (j < FRAP_MV) fpt_mv_backward<FPM_TAG>(L, w, D, Pm, pr, r, j))
#undef FPT_LANES
        for (int e = 0; e < FG_N; ++e) part[(size_t)tile * FG_N + e] = frap_tile_entry<FPM_TAG>(L, Pm, D, e);
    }
    fpt_t gPE[32], gR[2 * FRAP_C];
    for (int k = 0; k < 32; ++k) gPE[k] = frap_reduce_entry(part.data(), tiles, FG_PE + k);
    for (int k = 0; k < 2 * FRAP_C; ++k) gR[k] = frap_reduce_entry(part.data(), tiles, FG_DR + k);
    for (int i = 0; i < n; ++i) grad[i] = frap_grad_element<FPM_TAG>(w, D, i, part.data(), tiles, gPE, gR);
    *loss = frap_loss_mean<FPM_TAG>(part.data(), tiles, B.B);
    return 0;
}
