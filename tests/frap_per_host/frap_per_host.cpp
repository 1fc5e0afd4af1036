// frap_per_host.cpp -- prioritised replay of the fused MPLight update (resco_amd/csrc/resco_frap_per.h) compiled for the HOST (TEST
// INFRASTRUCTURE, never shipped): the uniform from the counter hash, the three-stage pick as dqn_per_pick_seq applied three times,
// the weighted row loss (fpt_row_loss_per) inside whole minibatches run through the phases in the order of frap_per_tile_kernel /
// frap_per_tile_opt_kernel -- the lanes of a phase one after the other where the kernel puts a barrier -- and the layout of
// rs_mplight_per as the C compiler sees it.  tests/test_frap_per_cpu.py compares them with numpy and float64 autograd
// (tests/frap_per_ref.py).
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/resco_sim.h"

#define RS_HD
// The header draws with d_hash, on the device resco_step.h's; the host build restates it (as tests/dqn_per_host does) and the test
// holds it against the oracle's own implementation.
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
static inline float d_u01(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }
#include "resco_frap.h"
#include "resco_frap_train.h"
#include "resco_frap_per.h"

extern "C" float frap_per_host_uniform(uint32_t seed, uint32_t u, uint32_t i, uint32_t j) { return frap_per_uniform(seed, u, i, j); }

// sizeof and the offsets of rs_mplight_per's eleven members, in declaration order: out int64 [12]
extern "C" void frap_per_host_layout(int64_t *out) {
    out[0] = (int64_t)sizeof(rs_mplight_per);
    out[1] = offsetof(rs_mplight_per, prio); out[2] = offsetof(rs_mplight_per, esum); out[3] = offsetof(rs_mplight_per, ssum);
    out[4] = offsetof(rs_mplight_per, pmax); out[5] = offsetof(rs_mplight_per, capacity); out[6] = offsetof(rs_mplight_per, n_envs);
    out[7] = offsetof(rs_mplight_per, n_signals); out[8] = offsetof(rs_mplight_per, alpha); out[9] = offsetof(rs_mplight_per, beta0);
    out[10] = offsetof(rs_mplight_per, eps); out[11] = offsetof(rs_mplight_per, beta_steps);
}

// the three-stage pick on prio [T][N][S], esum [T][N], ssum [T] at ring position (head, count) with uniforms (r0, r1, r2) and
// Z = the sequential total of the valid slots' ssum: out = (slot, environment, signal)
extern "C" int frap_per_host_pick(const float *prio, const float *esum, const float *ssum, int32_t T, int32_t N, int32_t S, int32_t head, int32_t count,
                                  float r0, float r1, float r2, int32_t *out) {
    if (!prio || !esum || !ssum || !out || T < 2 || N < 1 || S < 1 || head < 0 || head >= T || count < 2 || count > T) return -1;
    std::vector<float> valid((size_t)count - 1);        // the valid slots k = 0 .. count - 2 from the oldest, in order
    float Z = 0.0f;
    for (int k = 0; k < count - 1; ++k) {
        valid[k] = ssum[(head - count + T + k) % T];
        Z = Z + valid[k];
    }
    const int k = dqn_per_pick_seq(valid.data(), count - 1, 1, r0 * Z);
    const int t = (head - count + T + k) % T;
    const int e = dqn_per_pick_seq(esum + (size_t)t * N, N, 1, r1 * ssum[t]);
    out[0] = t; out[1] = e;
    out[2] = dqn_per_pick_seq(prio + ((size_t)t * N + e) * S, S, 1, r2 * esum[(size_t)t * N + e]);
    return 0;
}

#define FPT_LANES(stmt) for (int r = 0; r < FPT_TM; ++r) for (int j = 0; j < FPT_G; ++j) { stmt; }
// the phases behind the target, with the weighted row loss: the tail of frap_per_tile_kernel and of frap_per_tile_opt_kernel
static void per_tail(FrapStage &L, const float *w, int D, int P, const int32_t *pairs, int B, const float *wrow, float *ad) {
    FPT_LANES(fpt_pair_forward(L, w, D, P, pairs, r, j))
    FPT_LANES(fpt_item_forward(L, w, D, P, pairs, r, j))
    FPT_LANES(if (j == 0) fpt_row_loss_per<0>(L, P, B, r, wrow, ad))
    FPT_LANES(fpt_item_backward(L, w, D, P, r, j))
    FPT_LANES(if (j == L.g[r]) fpt_row_backward(L, w, D, P, r))
    FPT_LANES(if (j < FRAP_MV) fpt_mv_backward(L, w, D, P, pairs, r, j))
}
template <bool DOUBLE_Q>
static void per_opt_tile(FrapStage &L, FrapOptRows &O, const float *w, const float *wt, int D, int P, const int32_t *pairs, const float *obs, int W, int B,
                         const float *wrow, float *ad) {
    FPT_LANES(fpt_opt_load_next(L, O, obs, W, r, j))
    if (DOUBLE_Q) {
        FPT_LANES((fpt_target_ab<0, 0>(L, w, D, P, pairs, r, j)))
        FPT_LANES((fpt_target_q<0, 0>(L, w, D, P, pairs, r, j)))
        FPT_LANES(if (j == 0) fpt_opt_astar(L, O, P, r))
    }
    FPT_LANES((fpt_target_ab<0, 1>(L, wt, D, P, pairs, r, j)))
    FPT_LANES((fpt_target_q<0, 1>(L, wt, D, P, pairs, r, j)))
    FPT_LANES(if (j == 0) (fpt_opt_target_value<0, DOUBLE_Q>(L, O, P, r)); if (j < FRAP_MV) fpt_mv_forward(L, w, D, P, pairs, r, j))
    per_tail(L, w, D, P, pairs, B, wrow, ad);
}

// The weighted gradient (packed layout), the weighted mean loss and the rows' |delta| (ad [B]) of the minibatch idx [B][3] with the
// rows' weights wrow [B], on the ring obs [T][N][S][1 + 12 D], act, rew [T][N][S], done [T] whose next slot to write is head.  With
// (n_step, double_q) = (1, 0) the phases are the plain kernel's (frap_per_tile_kernel), else the option kernel's.  The stage is filled
// with 0xFF bytes (NaN) before every tile: a phase that read what no earlier phase wrote would show in the result.
extern "C" int frap_per_host_grad(const float *w, const float *wt, int32_t D, int32_t P, const int32_t *pairs, const float *obs, const int16_t *act,
                                  const float *rew, const uint8_t *done, int32_t T, int32_t N, int32_t S, int32_t head, const int32_t *idx, int32_t B,
                                  double gamma, int32_t n_step, int32_t double_q, const float *wrow, float *grad, float *loss, float *ad) {
    if ((D != 1 && D != 4) || P < 2 || P > FRAP_PMAX || T < 2 || N < 1 || S < 1 || B < 1 || n_step < 1 || n_step > 32) return -1;
    const int W = 1 + FRAP_MV * D, tiles = (B + FPT_TM - 1) / FPT_TM, n = FrapOff(D).n;
    const bool plain = n_step == 1 && !double_q;
    std::vector<fpt_t> part((size_t)tiles * FG_N);
    std::vector<FrapStage> stage(1);
    FrapStage &L = stage[0];
    FrapOptRows O;
    for (int tile = 0; tile < tiles; ++tile) {
        memset((void *)&L, 0xFF, sizeof(L));
        memset((void *)&O, 0xFF, sizeof(O));
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
            if (!plain) {
                for (int j = 0; j < FPT_G; ++j) fpt_opt_load_row(L, O, obs, act, rew, done, T, N, S, W, P, head, ok, t, e, s, n_step, gamma, r, j);
                continue;
            }
            // the load of frap_per_tile_kernel
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
        const float *wr = wrow + (size_t)tile * FPT_TM;
        float *adr = ad + (size_t)tile * FPT_TM;
        if (plain) {
            FPT_LANES(fpt_target_ab(L, wt, D, P, pairs, r, j))
            FPT_LANES(fpt_target_q(L, wt, D, P, pairs, r, j))
            FPT_LANES(if (j == 0) fpt_target_value(L, P, gamma, r); if (j < FRAP_MV) fpt_mv_forward(L, w, D, P, pairs, r, j))
            per_tail(L, w, D, P, pairs, B, wr, adr);
        } else if (double_q) per_opt_tile<true>(L, O, w, wt, D, P, pairs, obs, W, B, wr, adr);
        else per_opt_tile<false>(L, O, w, wt, D, P, pairs, obs, W, B, wr, adr);
        for (int e = 0; e < FG_N; ++e) part[(size_t)tile * FG_N + e] = frap_tile_entry(L, P, D, e);
    }
    fpt_t gPE[32], gR[2 * FRAP_C];
    for (int k = 0; k < 32; ++k) gPE[k] = frap_reduce_entry(part.data(), tiles, FG_PE + k);
    for (int k = 0; k < 2 * FRAP_C; ++k) gR[k] = frap_reduce_entry(part.data(), tiles, FG_DR + k);
    for (int i = 0; i < n; ++i) grad[i] = frap_grad_element(w, D, i, part.data(), tiles, gPE, gR);
    *loss = frap_loss_mean(part.data(), tiles, B);
    return 0;
}
