// resco_frap.h -- fused epsilon-greedy forward of MPLight's shared FRAP network for all N x S (environment, signal) rows.
//
// The reference network (resco_benchmark/agents/mplight.py:48-130), restated.  P = len(phase_pairs) (<= 16), 12 movements,
// demand_shape D (1: states.mplight rows, 4: states.mplight_full rows).  For one observation row o:
//   pp = phase_pairs[o[0]]                              o[0] is the LOCAL green index of the signal, used as a GLOBAL pair index (a quirk
//                                                       of the reference, kept); movement m has phase bit 1 iff m is in pp
//   e_m = relu(LE . [sigmoid(p[bit_m]), sigmoid(d . o[1+m .. 1+m+D-1] + d_b)] + LE_b)      16 wide; the demand windows of D = 4 overlap
//   pair_i = e_a + e_b                                  (a, b) = phase_pairs[i]
//   x_ij = relu(LC . [pair_i, pair_j] + LC_b) * relu(RC . relu(RE[comp_ij]) + RC_b)           20 wide, i != j
//   y_ij = BM . relu(H . x_ij + H_b) + BM_b,  Q_i = sum_{j != i} y_ij                          comp_ij = the pairs share one movement
//
// Three regroupings make it cheap (they change rounding only):
//   * LC splits by linearity: LC . [pair_i, pair_j] = A_i + B_j with A_i = LC[:, :16] . pair_i, B_j = LC[:, 16:] . pair_j + LC_b,
//     computed once per pair and row; the relation factor R[comp][c] has two values per channel and the phase term of the lane
//     embedding LE[:, :4] . sigmoid(p[bit]) + LE_b two per unit: both are derived once per workgroup into LDS (frap_prep_value).
//     What remains per (i, j) is the 20 x 20 hidden layer.
//   * Pruning: greedy acting reads only Q of the signal's valid pairs (ingolstadt21: 3.2 of 13 on average), and a row that explores
//     needs none; all P rows are computed only when the caller asks for the Q-values.
//   * The weights (~1.4 k floats) are read with wave-uniform addresses: scalar loads through the constant cache.
//
// Mapping: G = 4, 8 or 16 lanes per row (the smallest power of two >= P); lane j of a row owns pair j: its A_j, B_j and, for every
// needed i, y_ij.  A_i reaches the row's lanes by shuffles, Q_i is a butterfly sum over the G lanes.  One workgroup = 256 / G rows of
// ONE signal (grid: env tiles x S), so the loop over the signal's valid pairs is uniform in the workgroup.
//
// The per-lane pieces (frap_prep_value, frap_lane_ab, frap_lane_y, frap_draw) are written for the host as well (RS_HD): a CPU test
// compiles them with the host compiler (tests/frap_host) and checks the kernel's own arithmetic against the reference.
//
// Packed weight layout (float32, the order of FRAP's parameters in its state_dict, each tensor row-major, 1365 + 4 D floats):
//   p.weight [2][4], d.weight [4][D], d.bias [4], lane_embedding.weight [16][8], lane_embedding.bias [16],
//   lane_conv.weight [20][32], lane_conv.bias [20], relation_embedding.weight [2][4], relation_conv.weight [20][4],
//   relation_conv.bias [20], hidden_layer.weight [20][20], hidden_layer.bias [20], before_merge.weight [20], before_merge.bias [1]
#pragma once

#define FRAP_MV 12          // movements per signal
#define FRAP_E 16           // lane embedding units
#define FRAP_C 20           // lane_conv / relation_conv / hidden_layer channels
#define FRAP_PMAX 16        // at most 16 phase pairs (the width of the q output)
#define FRAP_SALT 0x3F4A9E1Bu   // exploration draws: d_hash(seed ^ FRAP_SALT; env_base + env, signal, step_key, 0 | 1)

// offsets into the packed weights for demand_shape D
struct FrapOff {
    int p, dw, db, le, leb, lc, lcb, re, rc, rcb, h, hb, bm, bmb, n;
    RS_HD explicit FrapOff(int D) {
        p = 0; dw = 8; db = dw + 4 * D; le = db + 4; leb = le + 128; lc = leb + 16; lcb = lc + 640; re = lcb + 20; rc = re + 8;
        rcb = rc + 80; h = rcb + 20; hb = h + 400; bm = hb + 20; bmb = bm + 20; n = bmb + 1;
    }
};

RS_HD inline float frap_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
RS_HD inline float frap_relu(float x) { return x > 0.0f ? x : 0.0f; }

// value k of the per-workgroup derived table: k < 32: PE[bit][u] = LE[u][0:4] . sigmoid(p[bit]) + LE_b[u] (k = 16 bit + u);
// 32 <= k < 72: R[comp][c] = relu(RC[c] . relu(RE[comp]) + RC_b[c]) (k = 32 + 20 comp + c)
RS_HD inline float frap_prep_value(const float *__restrict__ w, int D, int k) {
    const FrapOff o(D);
    if (k < 32) {
        const int bit = k >> 4, u = k & 15;
        float a = w[o.leb + u];
        for (int t = 0; t < 4; ++t) a = fmaf(w[o.le + u * 8 + t], frap_sigmoid(w[o.p + bit * 4 + t]), a);
        return a;
    }
    const int comp = (k - 32) / FRAP_C, c = (k - 32) % FRAP_C;
    float a = w[o.rcb + c];
    for (int t = 0; t < 4; ++t) a = fmaf(w[o.rc + c * 4 + t], frap_relu(w[o.re + comp * 4 + t]), a);
    return frap_relu(a);
}

// lane j of a row: A_j = LC[:, :16] . pair_j and B_j = LC[:, 16:] . pair_j + LC_b.  dem(m, t) = o[1 + m + t] as float; bits: phase bit
// of movements a and b; PE: the derived phase terms [2][16]
template <class WP, class Dem>
RS_HD inline void frap_lane_ab(WP w, int D, const float *PE, int a, int b, int bit_a, int bit_b, Dem dem,
                               float A[FRAP_C], float B[FRAP_C]) {
    const FrapOff o(D);
    float pr[FRAP_E];
#pragma unroll
    for (int u = 0; u < FRAP_E; ++u) pr[u] = 0.0f;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int m = side ? b : a, bit = side ? bit_b : bit_a;
        float sd[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float z = w[o.db + t];
            for (int v = 0; v < D; ++v) z = fmaf(w[o.dw + t * D + v], dem(m, v), z);
            sd[t] = frap_sigmoid(z);
        }
#pragma unroll
        for (int u = 0; u < FRAP_E; ++u) {
            float e = PE[bit * 16 + u];
#pragma unroll
            for (int t = 0; t < 4; ++t) e = fmaf(w[o.le + u * 8 + 4 + t], sd[t], e);
            pr[u] += frap_relu(e);
        }
    }
#pragma unroll
    for (int c = 0; c < FRAP_C; ++c) {
        float x = 0.0f, y = w[o.lcb + c];
#pragma unroll
        for (int u = 0; u < FRAP_E; ++u) {
            x = fmaf(w[o.lc + c * 32 + u], pr[u], x);
            y = fmaf(w[o.lc + c * 32 + 16 + u], pr[u], y);
        }
        A[c] = x; B[c] = y;
    }
}

// y_ij from A_i, B_j and the relation factor row R[comp_ij] (20)
template <class WP>
RS_HD inline float frap_lane_y(WP w, int D, const float Ai[FRAP_C], const float Bj[FRAP_C], const float *Rc) {
    const FrapOff o(D);
    float x[FRAP_C];
#pragma unroll
    for (int c = 0; c < FRAP_C; ++c) x[c] = frap_relu(Ai[c] + Bj[c]) * Rc[c];
    float y = w[o.bmb];
#pragma unroll
    for (int k = 0; k < FRAP_C; ++k) {
        float h = w[o.hb + k];
#pragma unroll
        for (int c = 0; c < FRAP_C; ++c) h = fmaf(w[o.h + k * FRAP_C + c], x[c], h);
        y = fmaf(w[o.bm + k], frap_relu(h), y);
    }
    return y;
}

// 1 when phase pairs i and j name exactly three distinct movements (mplight.py:19-28: len(set(pair_a + pair_b)) == 3).  For pairs of
// two distinct movements that is "they share one"; a pair that names one movement twice ([3, 3] against [4, 5]) counts as the
// reference counts it
RS_HD inline int frap_comp(const int32_t *pairs, int i, int j) {
    const int a0 = pairs[2 * i], a1 = pairs[2 * i + 1], b0 = pairs[2 * j], b1 = pairs[2 * j + 1];
    const int distinct = 1 + (a1 != a0) + (b0 != a0 && b0 != a1) + (b1 != a0 && b1 != a1 && b1 != b0);
    return distinct == 3;
}

// the exploration draw of a row: returns -1 (greedy) or k in [0, n_valid): the k-th entry of the signal's valid list
RS_HD inline int frap_draw(uint32_t seed, uint32_t genv, uint32_t s, uint32_t step_key, float eps, int n_valid) {
    if (!(eps > 0.0f)) return -1;
    const float u = d_u01(d_hash(seed ^ FRAP_SALT, genv, s, step_key, 0u));
    if (!(u < eps)) return -1;
    return (int)(d_hash(seed ^ FRAP_SALT, genv, s, step_key, 1u) % (uint32_t)n_valid);
}

struct FrapTab {            // device pointers
    const float *w;         // packed weights (layout above)
    const int32_t *pairs;   // [P][2]
    const int32_t *valid;   // [S][P] local action of pair g, -1 = not valid for the signal
    const int32_t *order;   // [S][P] the valid pairs in the reference's (dict) order, -1 padded
    const int32_t *nvalid;  // [S]
    int32_t P, S, D;
};

#if defined(__HIPCC__)      // the kernel itself: hipcc only (the pieces above also compile with a host compiler)
typedef const __attribute__((address_space(4))) float *FrapW;
template <int G>
__device__ __forceinline__ void frap_body(const FrapTab &F, const void *__restrict__ obs, int n_envs, int env_base, float eps, uint32_t seed,
                                          uint32_t step_key, int32_t *__restrict__ actions, int32_t *__restrict__ pair_out,
                                          float *__restrict__ q_out, const float *PE, const float *R) {
    constexpr int ROWS = 256 / G;
    const int s = blockIdx.y, tid = threadIdx.x;
    const int j = tid & (G - 1), row = tid / G;
    const int m = blockIdx.x * ROWS + row;
    if (m >= n_envs) return;                        // whole rows leave together: the shuffles below stay inside live rows
    const int P = F.P, S = F.S, D = F.D;
    const FrapW w = (FrapW)F.w;                     // constant address space: wave-uniform loads become scalar loads
    const int nv = F.nvalid[s];
    const size_t r = (size_t)m * S + s;
    const int base = (threadIdx.x & 63) & ~(G - 1);  // first lane of the row in its wave

    const int k = frap_draw(seed, (uint32_t)(env_base + m), (uint32_t)s, step_key, eps, nv);
    const bool want_q = q_out != nullptr;
    int g = 0;
    float myq = 0.0f;
    if (k < 0 || want_q) {
        // the row's observation: phase (local green index) and the 12 movement demands
        int ph;
        if (D == 1) ph = ((const int32_t *)obs)[r * 13];
        else ph = (int)((const float *)obs)[r * 49];
        ph = ph < 0 ? 0 : (ph >= P ? P - 1 : ph);
        const int p0 = F.pairs[2 * ph], p1 = F.pairs[2 * ph + 1];
        const int jj = j < P ? j : 0;
        const int a = F.pairs[2 * jj], b = F.pairs[2 * jj + 1];
        float A[FRAP_C], B[FRAP_C];
        if (D == 1) {
            const int32_t *o = (const int32_t *)obs + r * 13 + 1;
            frap_lane_ab(w, 1, PE, a, b, a == p0 || a == p1, b == p0 || b == p1, [&](int mv, int) { return (float)o[mv]; }, A, B);
        } else {
            const float *o = (const float *)obs + r * 49 + 1;
            frap_lane_ab(w, D, PE, a, b, a == p0 || a == p1, b == p0 || b == p1, [&](int mv, int t) { return o[mv + t]; }, A, B);
        }
        // greedy: Q of the valid pairs only (order[s][0 .. nv)), or of all P pairs when the caller wants the Q-values
        const int n_need = want_q ? P : nv;
        for (int t = 0; t < n_need; ++t) {
            const int i = want_q ? t : F.order[s * P + t];
            FrapW wl = w;
            asm volatile("" : "+s"(wl));            // the hidden layer's weights are re-read (scalar loads) per i, not hoisted into ~440 SGPRs
            float Ai[FRAP_C];
#pragma unroll
            for (int c = 0; c < FRAP_C; ++c) Ai[c] = __shfl(A[c], base + i, 64);
            float y = 0.0f;
            if (j < P && j != i) y = frap_lane_y(wl, D, Ai, B, R + FRAP_C * frap_comp(F.pairs, i, j));
#pragma unroll
            for (int msk = 1; msk < G; msk <<= 1) y += __shfl_xor(y, msk, 64);
            if (j == i) myq = y;
        }
        if (want_q && j < FRAP_PMAX) {
            float *q = q_out + r * FRAP_PMAX;
            q[j] = j < P ? myq : -INFINITY;
            if (G < FRAP_PMAX) for (int t = G + j; t < FRAP_PMAX; t += G) q[t] = -INFINITY;
        }
        // first maximum over the valid pairs in dict order, strict >
        g = F.order[s * P];
        float best = __shfl(myq, base + g, 64);
        for (int t = 1; t < nv; ++t) {
            const int gi = F.order[s * P + t];
            const float v = __shfl(myq, base + gi, 64);
            if (v > best) { best = v; g = gi; }
        }
    }
    if (k >= 0) g = F.order[s * P + k];
    if (j == 0) {
        actions[r] = F.valid[s * P + g];
        if (pair_out) pair_out[r] = g;
    }
}

__global__ void __launch_bounds__(256)
rs_mplight_act_kernel(FrapTab F, const void *__restrict__ obs, int n_envs, int env_base, float eps, uint32_t seed, uint32_t step_key,
                      const uint32_t *__restrict__ dyn, int32_t *__restrict__ actions, int32_t *__restrict__ pair_out, float *__restrict__ q_out) {
    // dyn != NULL: epsilon (float bits) and step key from device memory (graph replay, as rs_idqn_act)
    if (dyn) { eps = __uint_as_float(dyn[0]); step_key = dyn[1]; }
    __shared__ float sPE[32], sR[2 * FRAP_C];
    if (threadIdx.x < 72) {
        const float v = frap_prep_value(F.w, F.D, (int)threadIdx.x);
        if (threadIdx.x < 32) sPE[threadIdx.x] = v;
        else sR[threadIdx.x - 32] = v;
    }
    __syncthreads();
    if (F.P <= 4) frap_body<4>(F, obs, n_envs, env_base, eps, seed, step_key, actions, pair_out, q_out, sPE, sR);
    else if (F.P <= 8) frap_body<8>(F, obs, n_envs, env_base, eps, seed, step_key, actions, pair_out, q_out, sPE, sR);
    else frap_body<16>(F, obs, n_envs, env_base, eps, seed, step_key, actions, pair_out, q_out, sPE, sR);
}
#endif
