// ppo_host.cpp -- the fused GAE + per-signal standardisation (resco_amd/csrc/resco_ppo.h) compiled for the HOST (TEST
// INFRASTRUCTURE, never shipped).  ppo_gae_host runs the kernels' own functions phase by phase, thread after thread, in the
// kernels' reduction order; tests/test_ippo_fused_cpu.py compares it with gae() + the standardisation of resco_amd/agents/ippo.py,
// tests/test_gpu_ippo.py with the device.
#include "resco_ppo.h"

extern "C" int ppo_gae(const float *rew, const float *value, const float *last_value, const uint8_t *done, int32_t T, int32_t n_envs,
                       int32_t n_signals, float gamma, float lambda, float *adv, float *ret, float *scratch) {
    if (T <= 0 || n_envs <= 0 || n_signals <= 0) return -1;
    ppo_gae_host(PpoArgs{rew, value, last_value, done, T, n_envs, n_signals, gamma, lambda, adv, ret, scratch});
    return 0;
}
