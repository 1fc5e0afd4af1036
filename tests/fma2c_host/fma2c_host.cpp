// fma2c_host.cpp -- the per-row pieces of the fused FMA2C kernel (resco_amd/csrc/resco_fma2c.h), compiled for the HOST (TEST
// INFRASTRUCTURE, never shipped).  fma2c_host_act walks the agents in the kernel's launch order -- managers, then workers -- and the
// rows one after the other, and glues the pieces as rs_fma2c_kernel does: input row, three fc layers, LSTM, head, softmax and draw,
// fingerprint into the other buffer, parity flip.  The state arrays are the caller's (host copies of what the library owns).
// tests/test_fma2c_cpu.py compares it with the float64 restatement of the reference (tests/fma2c_ref.py).
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "resco_sim.h"

#define RS_HD
#define RS_SMEM nullptr
// the simulator's counter hash (resco_amd/csrc/resco_step.h: d_hash, d_u01), which the device build takes from there
static inline uint32_t rs_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
static inline uint32_t d_hash(uint32_t seed, uint32_t env, uint32_t trip, uint32_t tick, uint32_t stream) {
    uint32_t h = seed;
    const uint32_t w[4] = {env, trip, tick, stream};
    for (int i = 0; i < 4; ++i) {
        uint32_t k = w[i];
        k *= 0xcc9e2d51u; k = rs_rotl32(k, 15); k *= 0x1b873593u;
        h ^= k; h = rs_rotl32(h, 13); h = h * 5u + 0xe6546b64u;
    }
    h ^= 16u;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
static inline float d_u01(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }
#include "resco_fma2c.h"

extern "C" uint32_t fma2c_host_hash(uint32_t seed, uint32_t genv, uint32_t k, uint32_t step_key) { return d_hash(seed ^ FM_SALT, genv, k, step_key, 0u); }

// u_override: NULL (the counter hash) or the uniforms [N][K] to draw with.  value_only: the bootstrap call.  Returns W.
extern "C" int fma2c_host_act(const rs_fma2c_desc *d, const float *weights, int max_envs, float *state, float *fp, int32_t *macts,
                              int32_t *parity, const float *lane_agg, int N, int env_base, uint32_t seed, uint32_t step_key,
                              const float *u_override, int value_only, int32_t *actions, float *pi_out, float *value_out, float *rows_out) {
    Fma2cTab T{};
    T.w = weights; T.n_a = d->n_a; T.n_s = d->n_s; T.n_w = d->n_w; T.n_f = d->n_f; T.g_off = d->gather_off; T.g_idx = d->gather_idx;
    T.g_scale = d->gather_scale; T.fp_off = d->fp_off; T.fp_src = d->fp_src; T.m_off = d->mgr_off; T.m_src = d->mgr_src;
    T.state = state; T.fp = fp; T.macts = macts; T.parity = parity;
    T.K = d->K; T.M = d->M; T.S = d->S; T.O = d->n_obs; T.full = d->full; T.max_envs = max_envs;
    T.norm_wave = d->norm_wave; T.clip_wave = d->clip_wave; T.norm_wait = d->norm_wait; T.clip_wait = d->clip_wait;
    for (int k = 0; k < T.K; ++k) {
        T.NS = d->n_s[k] > T.NS ? d->n_s[k] : T.NS; T.NW = d->n_w[k] > T.NW ? d->n_w[k] : T.NW; T.NF = d->n_f[k] > T.NF ? d->n_f[k] : T.NF;
        const int w = d->n_s[k] + d->n_w[k] + d->n_f[k];
        T.W = w > T.W ? w : T.W;
    }
    const int K = T.K;
    const Fma2cOff o(K, T.NS, T.NW, T.NF);
    std::vector<float> x((size_t)T.W), hc(FM_HID), z(4 * FM_L), hn(FM_L);
    // the parities of a call are read before anybody flips: agent k of environment e reads buffer parity[e][k] as it is at ITS turn,
    // and only its own word has changed by then
    for (int k = 0; k < K; ++k)
        for (int e = 0; e < N; ++e) {
            const size_t ge = (size_t)(env_base + e);
            const int n_a = T.n_a[k], n_s = T.n_s[k], n_w = T.n_w[k], n_f = T.n_f[k], W = n_s + n_w + n_f;
            const int par = parity[ge * K + k];
            for (int j = 0; j < T.W; ++j) {
                x[j] = j < W ? fm_row_elem(T, k, j, lane_agg + (size_t)e * T.O * 5, macts + ge * T.M, fp + (((size_t)par * max_envs + ge) * K) * FM_AMAX) : 0.0f;
                if (rows_out) rows_out[((size_t)e * K + k) * T.W + j] = x[j];
            }
            float logit[FM_AMAX];
            for (int net = value_only ? 1 : 0; net < 2; ++net) {
                const size_t kn = (size_t)k * 2 + net;
                for (int c = 0; c < FM_FW; ++c) hc[c] = fm_fc_col(x.data(), n_s, weights + o.fcw_w + kn * T.NS * FM_FW, FM_FW, c, weights[o.fcw_b + kn * FM_FW + c]);
                for (int c = 0; c < FM_FP; ++c) hc[FM_FW + c] = fm_fc_col(x.data() + n_s + n_w, n_f, weights + o.fcf_w + kn * T.NF * FM_FP, FM_FP, c, weights[o.fcf_b + kn * FM_FP + c]);
                if (n_w > 0)
                    for (int c = 0; c < FM_FT; ++c) hc[FM_FW + FM_FP + c] = fm_fc_col(x.data() + n_s, n_w, weights + o.fct_w + kn * T.NW * FM_FT, FM_FT, c, weights[o.fct_b + kn * FM_FT + c]);
                float *st = state + ((ge * K + k) * 4 + 2 * net) * FM_L;
                const int n_in = n_w > 0 ? FM_HID : FM_FW + FM_FP;
                for (int c = 0; c < 4 * FM_L; ++c)
                    z[c] = fm_lstm_z(hc.data(), n_in, st + FM_L, weights + o.wx + kn * FM_HID * 4 * FM_L, weights + o.wh + kn * FM_L * 4 * FM_L, c, weights[o.lb + kn * 4 * FM_L + c]);
                for (int u = 0; u < FM_L; ++u) {
                    float c, h;
                    fm_lstm_gate(z[u], z[FM_L + u], z[2 * FM_L + u], z[3 * FM_L + u], st[u], &c, &h);
                    hn[u] = h;
                    if (!value_only) st[u] = c;
                }
                if (!value_only) memcpy(st + FM_L, hn.data(), FM_L * sizeof(float));
                const float *hw = weights + o.head_w + kn * FM_L * FM_AMAX, *hb = weights + o.head_b + kn * FM_AMAX;
                if (net == 0) for (int a = 0; a < n_a; ++a) logit[a] = fm_head(hn.data(), hw, a, hb[a]);
                else if (value_out) value_out[(size_t)e * K + k] = fm_head(hn.data(), hw, 0, hb[0]);
            }
            if (value_only) continue;
            float pi[FM_AMAX];
            const float u = u_override ? u_override[(size_t)e * K + k] : fm_uniform(seed, (uint32_t)ge, (uint32_t)k, step_key);
            const int act = fm_softmax_draw(logit, n_a, u, pi);
            float *fw = fp + (((size_t)(par ^ 1) * max_envs + ge) * K + k) * FM_AMAX;
            for (int a = 0; a < FM_AMAX; ++a) {
                fw[a] = pi[a];
                if (pi_out) pi_out[((size_t)e * K + k) * FM_AMAX + a] = pi[a];
            }
            parity[ge * K + k] = par ^ 1;
            if (k < T.M) macts[ge * T.M + k] = act;
            else if (actions) actions[(size_t)e * T.S + (k - T.M)] = act;
        }
    return T.W;
}
