// fma2c_loop_host.cpp -- the launch-free pieces of the in-library FMA2C training loop (resco_amd/csrc/resco_fma2c_loop.h: the reward
// and the recorder of a step, the done words, the state hand-over, the bookkeeping of a step) compiled for the HOST (TEST
// INFRASTRUCTURE, never shipped).  tests/test_fma2c_loop_cpu.py holds the reward against float64 and the bookkeeping against a Python
// restatement of FusedA2CLearner.observe; tests/test_gpu_fma2c_loop.py compares rs_fma2c_record with fl_host_record bit for bit.
#include <stdint.h>
#include <stddef.h>

#include "resco_fma2c_loop.h"

// the three outputs as rs_fma2c_record_kernel fills them: `threads` plays the grid, one "thread" after the other.
// acts and ret may be NULL (then macts and actions are not read).
extern "C" int fl_host_record(int32_t K, int32_t M, int32_t O, int32_t S, int32_t N, const int32_t *off, const int32_t *idx, const float *w,
                              const float *lane_agg, const int32_t *lane_arr, const int32_t *arrivals, const int32_t *departures,
                              const int32_t *macts, const int32_t *actions, float *rew, int32_t *acts, float *ret, int32_t threads) {
    if (K < 1 || M < 0 || M > K || O < 1 || S < 1 || N < 1 || threads < 1 || !off || !idx || !w || !rew) return -1;
    const int n_rows = 3 * O + 2 * S;
    if (off[0] != 0) return -2;
    for (int k = 0; k < K; ++k)
        if (off[k + 1] < off[k]) return -2;
    for (int q = 0; q < off[K]; ++q)
        if (idx[q] < 0 || idx[q] >= n_rows) return -3;
    const FlRec R{K, M, O, S, N, off, idx, w, lane_agg, lane_arr, arrivals, departures, macts, actions, rew, acts, ret};
    for (int i0 = 0; i0 < threads; ++i0) fl_record(R, i0, threads);
    return 0;
}

extern "C" int fl_host_done(int32_t *done, int32_t m, int32_t hit, int32_t threads) {
    if (threads < 1) return -1;
    for (int i0 = 0; i0 < threads; ++i0) fl_done(done, m, hit, i0, threads);
    return 0;
}

extern "C" int fl_host_state(float *dst, const float *src, int64_t n, int32_t zero, int32_t threads) {
    if (threads < 1 || n < 0) return -1;
    for (int i0 = 0; i0 < threads; ++i0) fl_state(dst, src, (size_t)n, zero, (size_t)i0, (size_t)threads);
    return 0;
}

// the plans of steps 0 .. n_steps - 1 of one call: out [n_steps][5] = slot, done, update, n_slots, key
extern "C" int fl_host_plan(int32_t T, int32_t slot0, int64_t t0, int32_t done_step, int32_t n_steps, uint32_t *out) {
    if (T < 1 || slot0 < 0 || slot0 >= T || n_steps < 1) return -1;
    for (int k = 0; k < n_steps; ++k) {
        const FlStep s = fl_plan(T, slot0, t0, done_step, k);
        uint32_t *o = out + (size_t)k * 5;
        o[0] = (uint32_t)s.slot; o[1] = (uint32_t)s.done; o[2] = (uint32_t)s.update; o[3] = (uint32_t)s.n_slots; o[4] = s.key;
    }
    return 0;
}
