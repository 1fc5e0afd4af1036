// ppo_train_host.cpp -- the scalar pieces of the fused PPO update (resco_amd/csrc/resco_ppo_train.h: the per-row loss gradient, the
// clip scale, the Adam element update) compiled for the HOST (TEST INFRASTRUCTURE, never shipped).  tests/test_ppo_train_cpu.py
// compares them with autograd of the float64 loss and with torch.optim.Adam (tests/ppo_train_ref.py).
#include "resco_ppo_train.h"

// n samples of one signal with A actions: logits / dlogits [n][8], terms [n][3]
extern "C" int ppo_train_rows(const float *logits, int32_t A, int32_t n, const float *value, const int32_t *action, const float *logp_old,
                              const float *adv, const float *ret, float inv_b, float clip_eps, float entropy_coef, float value_coef,
                              float *dlogits, float *dvalue, float *terms) {
    if (A < 1 || A > PPT_AMAX || n < 0) return -1;
    for (int i = 0; i < n; ++i)
        ppo_row_loss_grad(logits + i * PPT_AMAX, A, value[i], action[i], logp_old[i], adv[i], ret[i], inv_b, clip_eps, entropy_coef, value_coef,
                          dlogits + i * PPT_AMAX, dvalue + i, terms + i * 3);
    return 0;
}

// the clip scale of a signal from its squared gradient norm, as the pair the Adam kernel multiplies the gradients with: out[2]
extern "C" void ppo_train_clip(double sq_norm, double max_grad_norm, float *out) {
    const PpoStepConsts K = ppo_step_consts(1.0, 1.0, 0.9, 0.999, max_grad_norm, 1);
    const PpoPair s = ppo_clip_scale(ppo_pair_of(sq_norm), K);
    out[0] = s.hi; out[1] = s.lo;
}

// n elements of step t: the gradient times the clip scale, then the Adam element update
extern "C" int ppo_train_adam(float *p, float *m, float *v, const float *g, const float *scale, int32_t n, double lr, double adam_eps, double beta1,
                              double beta2, int32_t t) {
    const PpoStepConsts K = ppo_step_consts(lr, adam_eps, beta1, beta2, 0.5, t);
    for (int i = 0; i < n; ++i) ppo_adam_element(p + i, m + i, v + i, g[i], PpoPair{scale[0], scale[1]}, K);
    return 0;
}
