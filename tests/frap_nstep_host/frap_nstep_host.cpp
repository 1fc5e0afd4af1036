// frap_nstep_host.cpp -- the phases of the target's options of the fused MPLight update (resco_amd/csrc/resco_frap_train.h:
// fpt_opt_load_row with the n-step walk, fpt_opt_load_next, the online pass of Double DQN through fpt_target_ab / fpt_target_q with
// NET 0, fpt_opt_astar, fpt_opt_target_value) compiled for the HOST (TEST INFRASTRUCTURE, never shipped).  frap_nstep_grad runs whole
// minibatches through them in the order of frap_dqn_tile_opt_kernel -- the lanes of a phase one after the other where the kernel puts
// a barrier -- and tests/test_frap_nstep_cpu.py compares the result with autograd of the float64 definition (tests/frap_nstep_ref.py).
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#define RS_HD
// (the headers' draw needs a d_hash; nothing here draws)
static inline uint32_t d_hash(uint32_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return seed ^ a ^ b ^ c ^ d; }
static inline float d_u01(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }
#include "resco_frap.h"
#include "resco_frap_train.h"

template <bool DOUBLE_Q>
static void nstep_tile(FrapStage &L, FrapOptRows &O, const float *w, const float *wt, int D, int P, const int32_t *pairs, const float *obs, int W, int B) {
#define FPT_LANES(stmt) for (int r = 0; r < FPT_TM; ++r) for (int j = 0; j < FPT_G; ++j) { stmt; }
    FPT_LANES(fpt_opt_load_next(L, O, obs, W, r, j))
    if (DOUBLE_Q) {
        FPT_LANES((fpt_target_ab<0, 0>(L, w, D, P, pairs, r, j)))
        FPT_LANES((fpt_target_q<0, 0>(L, w, D, P, pairs, r, j)))
        FPT_LANES(if (j == 0) fpt_opt_astar(L, O, P, r))
    }
    FPT_LANES((fpt_target_ab<0, 1>(L, wt, D, P, pairs, r, j)))
    FPT_LANES((fpt_target_q<0, 1>(L, wt, D, P, pairs, r, j)))
    FPT_LANES(if (j == 0) (fpt_opt_target_value<0, DOUBLE_Q>(L, O, P, r)); if (j < FRAP_MV) fpt_mv_forward(L, w, D, P, pairs, r, j))
    FPT_LANES(fpt_pair_forward(L, w, D, P, pairs, r, j))
    FPT_LANES(fpt_item_forward(L, w, D, P, pairs, r, j))
    FPT_LANES(if (j == 0) fpt_row_loss(L, P, B, r))
    FPT_LANES(fpt_item_backward(L, w, D, P, r, j))
    FPT_LANES(if (j == L.g[r]) fpt_row_backward(L, w, D, P, r))
    FPT_LANES(if (j < FRAP_MV) fpt_mv_backward(L, w, D, P, pairs, r, j))
#undef FPT_LANES
}

// The gradient (packed layout, 1365 + 4 D floats) and the mean loss of the minibatch idx [B][3] = (t, e, s) on the ring obs [T][N][S][1 + 12 D],
// act, rew [T][N][S], done [T] whose next slot to write is head, under (n_step, double_q).  The stage and the rows' scalars are filled
// with 0xFF bytes (NaN) before every tile: a phase that read what no earlier phase wrote would show in the result.  m_out, astar_out
// [B] or NULL: every row's walk length (the bootstrap slot is (t + m) mod T) and a* (0 without double_q or where the walk was cut).
extern "C" int frap_nstep_grad(const float *w, const float *wt, int32_t D, int32_t P, const int32_t *pairs, const float *obs, const int16_t *act,
                               const float *rew, const uint8_t *done, int32_t T, int32_t N, int32_t S, int32_t head, const int32_t *idx, int32_t B,
                               double gamma, int32_t n_step, int32_t double_q, float *grad, float *loss, int32_t *m_out, int32_t *astar_out) {
    if ((D != 1 && D != 4) || P < 2 || P > FRAP_PMAX || T < 2 || N < 1 || S < 1 || B < 1 || n_step < 1 || n_step > 32) return -1;
    const int W = 1 + FRAP_MV * D, tiles = (B + FPT_TM - 1) / FPT_TM, n = FrapOff(D).n;
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
            for (int j = 0; j < FPT_G; ++j) fpt_opt_load_row(L, O, obs, act, rew, done, T, N, S, W, P, head, ok, t, e, s, n_step, gamma, r, j);
            if (ok && m_out) {
                int m, cut;
                dqn_nstep_walk(done, T, head < 0 ? 0 : (head >= T ? T - 1 : head), t, n_step, &m, &cut);
                m_out[row] = m;
            }
        }
        if (double_q) nstep_tile<true>(L, O, w, wt, D, P, pairs, obs, W, B);
        else nstep_tile<false>(L, O, w, wt, D, P, pairs, obs, W, B);
        for (int r = 0; astar_out && r < FPT_TM; ++r)
            if (L.ok[r]) astar_out[tile * FPT_TM + r] = O.astar[r];
        for (int e = 0; e < FG_N; ++e) part[(size_t)tile * FG_N + e] = frap_tile_entry(L, P, D, e);
    }
    fpt_t gPE[32], gR[2 * FRAP_C];
    for (int k = 0; k < 32; ++k) gPE[k] = frap_reduce_entry(part.data(), tiles, FG_PE + k);
    for (int k = 0; k < 2 * FRAP_C; ++k) gR[k] = frap_reduce_entry(part.data(), tiles, FG_DR + k);
    for (int i = 0; i < n; ++i) grad[i] = frap_grad_element(w, D, i, part.data(), tiles, gPE, gR);
    *loss = frap_loss_mean(part.data(), tiles, B);
    return 0;
}
