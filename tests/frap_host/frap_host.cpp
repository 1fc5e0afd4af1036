// frap_host.cpp -- the per-lane pieces of the fused MPLight kernel (resco_amd/csrc/resco_frap.h), compiled for the HOST (TEST
// INFRASTRUCTURE, never shipped).  frap_rows runs the lanes of every row one after the other and glues them as the kernel's
// frap_body does with shuffles: Q_i = sum over j != i of y_ij, the first maximum over the valid pairs in dict order, the
// epsilon-greedy draw of the model's counter hash.  tests/test_mplight_cpu.py compares it with the reference's fixtures,
// tests/test_frap_ref_cpu.py with the float64 reference (tests/frap_ref.py) on synthetic phase-pair sets.
#include <stdio.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "resco_sim.h"

#define RS_DEV static inline
#define RS_HD
#define RS_MEM inline
#define RS_CARVE static inline
static char *g_smem = nullptr;
#define RS_SMEM g_smem
// an invariant of the kernel source the emulation checks (the device build compiles it out)
#define RS_ASSERT(c) if (!(c)) { fprintf(stderr, "rs_emu: invariant violated: %s (resco_step.h:%d)\n", #c, __LINE__); abort(); }
static inline void rs_atomic_min(int32_t *p, int32_t v) { if (v < *p) *p = v; }
static inline void rs_atomic_min(uint32_t *p, uint32_t v) { if (v < *p) *p = v; }
static inline void rs_atomic_max(int32_t *p, int32_t v) { if (v > *p) *p = v; }
static inline void rs_atomic_add(int32_t *p, int32_t v) { *p += v; }
static inline int32_t rs_atomic_fetch_add(int32_t *p, int32_t v) { const int32_t o = *p; *p += v; return o; }
static inline int32_t rs_wave_ticket(int32_t *p) { return (*p)++; }
static inline void rs_wave_add(int32_t *p, int32_t v) { *p += v; }
static inline void rs_wave_max(int32_t *p, int32_t v) { if (v > *p) *p = v; }
static inline void rs_atomic_or(uint32_t *p, uint32_t v) { *p |= v; }
static inline uint32_t rs_atomic_fetch_or(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p |= v; return o; }
static inline void rs_atomic_and(uint32_t *p, uint32_t v) { *p &= v; }
static inline uint32_t rs_atomic_cas(uint32_t *p, uint32_t cmp, uint32_t v) { uint32_t o = *p; if (o == cmp) *p = v; return o; }
static inline int rs_ffsll(unsigned long long x) { return __builtin_ffsll((long long)x); }
static inline int rs_clzll(unsigned long long x) { return __builtin_clzll(x); }
static inline int rs_ffs(uint32_t x) { return __builtin_ffs((int)x); }
static inline int rs_popc(uint32_t x) { return __builtin_popcount(x); }
static inline float rs_int_as_float(int x) { float f; memcpy(&f, &x, 4); return f; }
static inline int rs_float_as_int(float x) { int i; memcpy(&i, &x, 4); return i; }
// float -> IEEE half bits, round to nearest even (what __float2half does)
static inline uint16_t rs_f2h(float f) {
    uint32_t x; memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    int32_t e = (int32_t)((x >> 23) & 0xFF) - 127 + 15;
    uint32_t m = x & 0x7FFFFFu;
    if (((x >> 23) & 0xFF) == 0xFF) return (uint16_t)(sign | 0x7C00u | (m ? 0x200u : 0u));
    if (e >= 31) return (uint16_t)(sign | 0x7C00u);
    if (e <= 0) {
        if (e < -10) return (uint16_t)sign;
        m |= 0x800000u;
        const int shift = 14 - e;
        uint32_t r = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (r & 1u))) r += 1;
        return (uint16_t)(sign | r);
    }
    uint32_t r = ((uint32_t)e << 10) | (m >> 13);
    const uint32_t rem = m & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) r += 1;
    return (uint16_t)(sign | r);
}
#include "resco_step.h"
#include "resco_frap.h"

extern "C" int frap_rows(const float *w, int D, int P, const int32_t *pairs, int S, const int32_t *valid, const int32_t *order,
                         const float *obs /* [N][S][1 + 12 D] */, int N, int env_base, float eps, uint32_t seed, uint32_t step_key,
                         int want_q, int32_t *actions, int32_t *pair_out, float *q_out /* [N][S][16] */) {
    float PE[32], R[40];
    for (int k = 0; k < 72; ++k) (k < 32 ? PE[k] : R[k - 32]) = frap_prep_value(w, D, k);
    const int W = 1 + FRAP_MV * D;
    for (int m = 0; m < N; ++m)
        for (int s = 0; s < S; ++s) {
            const float *o = obs + ((size_t)m * S + s) * W;
            int nv = 0;
            while (nv < P && order[s * P + nv] >= 0) ++nv;
            const int k = frap_draw(seed, (uint32_t)(env_base + m), (uint32_t)s, step_key, eps, nv);
            int ph = (int)o[0];
            ph = ph < 0 ? 0 : (ph >= P ? P - 1 : ph);
            const int p0 = pairs[2 * ph], p1 = pairs[2 * ph + 1];
            float A[FRAP_PMAX][FRAP_C], B[FRAP_PMAX][FRAP_C], Q[FRAP_PMAX];
            int g = 0;
            if (k < 0 || want_q) {
                for (int j = 0; j < P; ++j) {
                    const int a = pairs[2 * j], b = pairs[2 * j + 1];
                    frap_lane_ab(w, D, PE, a, b, a == p0 || a == p1, b == p0 || b == p1, [&](int mv, int t) { return o[1 + mv + t]; }, A[j], B[j]);
                }
                for (int i = 0; i < P; ++i) {
                    Q[i] = 0.0f;
                    for (int j = 0; j < P; ++j)
                        if (j != i) Q[i] += frap_lane_y(w, D, A[i], B[j], R + FRAP_C * frap_comp(pairs, i, j));
                }
                g = order[s * P];
                for (int t = 1; t < nv; ++t)
                    if (Q[order[s * P + t]] > Q[g]) g = order[s * P + t];
                if (want_q)
                    for (int t = 0; t < FRAP_PMAX; ++t) q_out[((size_t)m * S + s) * FRAP_PMAX + t] = t < P ? Q[t] : -INFINITY;
            }
            if (k >= 0) g = order[s * P + k];
            actions[(size_t)m * S + s] = valid[s * P + g];
            pair_out[(size_t)m * S + s] = g;
        }
    return 0;
}
