// dqn_nstep_host.cpp -- the n-step walk of the fused DQN update (resco_amd/csrc/resco_dqn_train.h: dqn_nstep_walk) compiled for the
// HOST (TEST INFRASTRUCTURE, never shipped).  tests/test_dqn_nstep_cpu.py compares it exhaustively with the Python twin
// (tests/dqn_nstep_ref.py: walk).
#include <stdint.h>

// the header's draw calls d_hash, on the device resco_step.h's; nothing here draws, so a declaration is all the host build needs
static inline uint32_t d_hash(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) { return 0u; }
#include "resco_dqn_train.h"

// the walk of slot t: out = (m, cut)
extern "C" int dqn_nstep_walk_host(const uint8_t *done, int32_t T, int32_t head, int32_t t, int32_t n_step, int32_t *out) {
    if (!done || !out || T < 1 || head < 0 || head >= T || t < 0 || t >= T) return -1;
    int m = 0, cut = 0;
    dqn_nstep_walk(done, T, head, t, n_step, &m, &cut);
    out[0] = m; out[1] = cut;
    return 0;
}
