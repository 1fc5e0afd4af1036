// resco_fma2c.h -- fused acting step of FMA2C: input assembly, both LSTM actor-critic nets and the draw for all K agents of N
// environments, with the LSTM state, the fingerprints and the managers' actions kept on the device.
//
// The reference (resco_benchmark/agents/fma2c.py:103-132 act, ma2c.py:124-131 MA2CAgent.act, :411-456 FPLstmACPolicy, :482-532 fc /
// lstm), restated.  K = M managers + S workers, managers first (fma2c.py:41-70).  Agent k has n_a actions and an input row
//   x = [manager actions (workers: own manager's, then its neighbours'; as floats)] ++ states.fma2c row ++ fingerprints
// that splits as [0, n_s) | [n_s, n_s + n_w) waits | [n_s + n_w, .. + n_f) fingerprints (the states row ends with the n_w waits).
// pi and v are two separate nets (net 0, net 1), each
//   hc = concat(relu(x[:n_s] fcw + b) 128, relu(x[n_s + n_w:] fcf + b) 64, relu(x[n_s:n_s + n_w] fct + b) 32 if n_w > 0)
//   z = hc wx + h wh + b;  i, f, o, u = split(z);  c = sig(f) c + sig(i) tanh(u);  h = sig(o) tanh(c)          (64 units)
//   net 0: pi = softmax(h head_w[:, :n_a] + head_b);  net 1: v = h head_w[:, 0] + head_b[0]
// A fingerprint is an agent's own pi of its PREVIOUS act (zeros before the first).  Managers act first; workers see the managers'
// actions of this step.  The forward is always called with done = False; only the acting call moves the LSTM state, the bootstrap
// call (value only) reads it.
//
// Launches: one kernel, launched twice per act on the caller's stream -- the managers (agents 0 .. M-1), then the workers, which
// read the actions the first launch wrote.  No workgroup waits for another one.  Grid = (tiles of FM_TM = 32 environments) x (agents
// of the launch), 256 threads; the agent's widths are uniform in the workgroup and padded widths are skipped, not multiplied.
//
// Fingerprints are double-buffered: agent (e, k) reads its neighbours' pi from buffer parity[e][k] and writes its own into the
// OTHER buffer, then flips its parity word.  All agents of an environment act in every call, so their parities agree when a call
// starts, and nobody writes the buffer anybody reads: the race of a single buffer (a neighbour's workgroup overwriting what this
// one has yet to read) cannot happen.  The parity word is device state private to its (e, k): no host-side flip, so a batch split
// over pipes (env_base) and a captured graph behave as the single call.
//
// Arithmetic: fp32 throughout.  The matrix products run on v_mfma_f32_32x32x2_f32, whose result is bit-for-bit a k-ascending fmaf
// chain from 0 in fp32; the bias is added after the chain.  The per-row pieces below (RS_HD) spell that same order out, so a host
// build (tests/fma2c_host) reproduces the kernel's arithmetic up to expf / tanhf of the two maths libraries.
//
// Packed weights (float32; resco_amd/agents/fma2c.py: BatchedFMA2C.packed): eleven tensors in this order, each row-major, each
// padded to the map's largest widths NS = max n_s, NW = max n_w, NF = max n_f and indexed [k][net] first:
//   fcw_w [K][2][NS][128], fcw_b [K][2][128], fcf_w [K][2][NF][64], fcf_b [K][2][64], fct_w [K][2][NW][32], fct_b [K][2][32],
//   wx [K][2][224][256] (rows: fcw, fcf, fct units; a manager uses the first 192), wh [K][2][64][256], lb [K][2][256] (columns: gates
//   i, f, o, u, 64 each), head_w [K][2][64][8], head_b [K][2][8] (net 0: columns < n_a; net 1: column 0)
#pragma once

#define FM_TM 32            // environments per workgroup (one M tile of the 32x32x2 MFMA)
#define FM_AMAX 8           // widest action set = the width of a fingerprint
#define FM_FW 128
#define FM_FP 64
#define FM_FT 32
#define FM_L 64
#define FM_HID 224          // FM_FW + FM_FP + FM_FT
#define FM_NS_MAX 256       // documented limits of rs_fma2c_create
#define FM_NW_MAX 32
#define FM_NF_MAX 32
#define FM_W_MAX 320
#define FM_SALT 0x5A2C9D47u // action draws: d_hash(seed ^ FM_SALT; env_base + env, agent, step_key, 0)
#define FM_HS 289           // LDS row stride of hc | h (224 + 64, odd against bank conflicts)
#define FM_ZS 257

struct Fma2cOff {           // offsets of the eleven tensors in the packed weights
    size_t fcw_w, fcw_b, fcf_w, fcf_b, fct_w, fct_b, wx, wh, lb, head_w, head_b, n;
    RS_HD Fma2cOff(int K, int NS, int NW, int NF) {
        const size_t k2 = (size_t)K * 2;
        fcw_w = 0; fcw_b = fcw_w + k2 * NS * FM_FW; fcf_w = fcw_b + k2 * FM_FW; fcf_b = fcf_w + k2 * NF * FM_FP; fct_w = fcf_b + k2 * FM_FP;
        fct_b = fct_w + k2 * NW * FM_FT; wx = fct_b + k2 * FM_FT; wh = wx + k2 * FM_HID * 4 * FM_L; lb = wh + k2 * FM_L * 4 * FM_L;
        head_w = lb + k2 * 4 * FM_L; head_b = head_w + k2 * FM_L * FM_AMAX; n = head_b + k2 * FM_AMAX;
    }
};

struct Fma2cTab {           // device pointers (the host build: host pointers)
    const float *w;         // packed weights
    const int32_t *n_a, *n_s, *n_w, *n_f;          // [K]
    const int32_t *g_off, *g_idx; const float *g_scale;    // [K + 1], gather (index into F, scale) of the states row
    const int32_t *fp_off, *fp_src;                 // [K + 1], the agents whose fingerprints are appended, in order
    const int32_t *m_off, *m_src;                   // [K + 1], the managers whose actions lead the row
    float *state;           // [max_envs][K][4][64]: pi c, pi h, v c, v h
    float *fp;              // [2][max_envs][K][8]
    int32_t *macts;         // [max_envs][M]
    int32_t *parity;        // [max_envs][K]: the fingerprint buffer the agent's next act READS
    int32_t K, M, S, O, full, NS, NW, NF, W, max_envs;
    float norm_wave, clip_wave, norm_wait, clip_wait;
};

RS_HD inline float fm_clip(float x, float hi) { return x < 0.0f ? 0.0f : (x > hi ? hi : x); }
RS_HD inline float fm_relu(float x) { return x > 0.0f ? x : 0.0f; }
RS_HD inline float fm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// element `idx` of the feature vector F of VecMultiSignal.fma2c_states (states.py:162-305) from one environment's lane aggregates
// agg [O][5] = queue, approach, total_wait, max_wait, speed_sum.  Blocks of O: wave, [full: total_wait / 28, speed / 20 / 28], max_wait
RS_HD inline float fm_feature(const Fma2cTab &T, const float *agg, int idx) {
    const int b = idx / T.O, l = idx - b * T.O;
    const float *a = agg + (size_t)l * 5;
    if (b == 0) return fm_clip((a[0] + a[1]) / T.norm_wave, T.clip_wave);
    if (T.full && b == 1) return fm_clip(a[2] / 28.0f / T.norm_wave, T.clip_wave);
    if (T.full && b == 2) return fm_clip(a[4] / 20.0f / 28.0f / T.norm_wave, T.clip_wave);
    return fm_clip(a[3] / T.norm_wait, T.clip_wait);
}

// element j of agent k's input row (0 beyond its width): agg = the environment's lane aggregates, macts = its managers' actions
// [M], fp = the fingerprint buffer it reads [K][8]
RS_HD inline float fm_row_elem(const Fma2cTab &T, int k, int j, const float *agg, const int32_t *macts, const float *fp) {
    const int nm = T.m_off[k + 1] - T.m_off[k], ng = T.g_off[k + 1] - T.g_off[k];
    if (j < nm) return (float)macts[T.m_src[T.m_off[k] + j]];
    j -= nm;
    if (j < ng) { const int g = T.g_off[k] + j; return fm_feature(T, agg, T.g_idx[g]) * T.g_scale[g]; }
    j -= ng;
    for (int q = T.fp_off[k]; q < T.fp_off[k + 1]; ++q) {
        const int src = T.fp_src[q], na = T.n_a[src];
        if (j < na) return fp[src * FM_AMAX + j];
        j -= na;
    }
    return 0.0f;
}

// one output column of an fc layer: relu(b + sum_k x[k] w[k][col]), the sum as the MFMA forms it (k ascending, fmaf, from 0)
RS_HD inline float fm_fc_col(const float *x, int n_in, const float *w, int ncols, int col, float b) {
    float acc = 0.0f;
    for (int k = 0; k < n_in; ++k) acc = fmaf(x[k], w[(size_t)k * ncols + col], acc);
    return fm_relu(acc + b);
}
// one column of the LSTM's pre-activation: hc wx (n_in rows), continued over h wh, then the bias
RS_HD inline float fm_lstm_z(const float *hc, int n_in, const float *h, const float *wx, const float *wh, int col, float b) {
    float acc = 0.0f;
    for (int k = 0; k < n_in; ++k) acc = fmaf(hc[k], wx[(size_t)k * 4 * FM_L + col], acc);
    for (int k = 0; k < FM_L; ++k) acc = fmaf(h[k], wh[(size_t)k * 4 * FM_L + col], acc);
    return acc + b;
}
RS_HD inline void fm_lstm_gate(float zi, float zf, float zo, float zu, float c_prev, float *c, float *h) {
    const float cn = fm_sigmoid(zf) * c_prev + fm_sigmoid(zi) * tanhf(zu);
    *c = cn;
    *h = fm_sigmoid(zo) * tanhf(cn);
}
RS_HD inline float fm_head(const float *h, const float *w, int col, float b) {
    float acc = 0.0f;
    for (int k = 0; k < FM_L; ++k) acc = fmaf(h[k], w[k * FM_AMAX + col], acc);
    return acc + b;
}
// softmax over the n_a logits into pi[8] (0 beyond n_a) and the inverse-CDF draw: the first action whose running sum exceeds u
RS_HD inline int fm_softmax_draw(const float *logit, int n_a, float u, float pi[FM_AMAX]) {
    float mx = logit[0];
    for (int a = 1; a < n_a; ++a) mx = logit[a] > mx ? logit[a] : mx;
    float s = 0.0f;
    for (int a = 0; a < FM_AMAX; ++a) { pi[a] = a < n_a ? expf(logit[a] - mx) : 0.0f; s += pi[a]; }
    int act = n_a - 1;
    float cum = 0.0f;
    bool found = false;
    for (int a = 0; a < n_a; ++a) {
        pi[a] = pi[a] / s;
        cum += pi[a];
        if (!found && u < cum) { act = a; found = true; }
    }
    return act;
}
RS_HD inline float fm_uniform(uint32_t seed, uint32_t genv, uint32_t k, uint32_t step_key) {
    return d_u01(d_hash(seed ^ FM_SALT, genv, k, step_key, 0u));
}

struct Fma2cOut {           // device pointers of one call, any may be NULL; rows of the CALL (0 .. n_envs - 1)
    int32_t *actions;       // [n_envs][S] the workers' local actions
    float *pi, *value, *rows;       // [n_envs][K][8], [n_envs][K], [n_envs][K][W]
};

#if defined(__HIPCC__)
typedef float fm_f16 __attribute__((ext_vector_type(16)));

// ACT: the acting call (both nets, draw, state / fingerprints / parity written).  !ACT: the bootstrap call (net 1 only, nothing of
// the library's state written).  k0: the first agent of the launch (blockIdx.y counts from it).
template <bool ACT>
__global__ void __launch_bounds__(256)
rs_fma2c_kernel(Fma2cTab T, const float *__restrict__ lane_agg, int n_envs, int env_base, int k0, uint32_t seed, uint32_t step_key,
                const uint32_t *__restrict__ dyn, Fma2cOut out) {
    if (dyn) step_key = dyn[1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 31, g = lane >> 5;
    const int k = k0 + blockIdx.y, e0 = blockIdx.x * FM_TM;
    const int rows = n_envs - e0 < FM_TM ? n_envs - e0 : FM_TM;
    const int n_a = T.n_a[k], n_s = T.n_s[k], n_w = T.n_w[k], n_f = T.n_f[k], W = n_s + n_w + n_f, K = T.K;
    const int XS = T.W + 1;
    float *xs = (float *)RS_SMEM;                   // [32][XS] the input rows
    float *hc = xs + FM_TM * XS;                    // [32][FM_HS] fc outputs (224) | h of the net in hand (64)
    float *zz = hc + FM_TM * FM_HS;                 // [32][FM_ZS] LSTM pre-activations
    float *lg = zz + FM_TM * FM_ZS;                 // [32][8] logits
    const Fma2cOff o(K, T.NS, T.NW, T.NF);

    // ---- 1. the input rows (fm_row_elem), zero beyond the agent's width and for the rows a short last tile pads
    for (int idx = tid; idx < FM_TM * T.W; idx += 256) {
        const int r = idx / T.W, j = idx - r * T.W;
        float v = 0.0f;
        if (r < rows) {
            const size_t ge = (size_t)(env_base + e0 + r);
            if (j < W) {
                const int par = T.parity[ge * K + k];
                v = fm_row_elem(T, k, j, lane_agg + (size_t)(e0 + r) * T.O * 5, T.macts + ge * T.M, T.fp + (((size_t)par * T.max_envs + ge) * K) * FM_AMAX);
            }
            if (out.rows) out.rows[((size_t)(e0 + r) * K + k) * T.W + j] = v;
        }
        xs[r * XS + j] = v;
    }
    __syncthreads();

    for (int net = ACT ? 0 : 1; net < 2; ++net) {
        const size_t kn = (size_t)k * 2 + net;
        // ---- 2. the three fc layers: 7 column tiles of 32 (4 fcw, 2 fcf, 1 fct) over the four waves
        for (int t = wv; t < 7; t += 4) {
            if (t == 6 && n_w == 0) continue;
            const int xoff = t < 4 ? 0 : (t < 6 ? n_s + n_w : n_s), n_in = t < 4 ? n_s : (t < 6 ? n_f : n_w);
            const int ncols = t < 4 ? FM_FW : (t < 6 ? FM_FP : FM_FT), col = (t < 4 ? t : (t < 6 ? t - 4 : 0)) * 32 + i;
            const float *w = T.w + (t < 4 ? o.fcw_w + kn * T.NS * FM_FW : (t < 6 ? o.fcf_w + kn * T.NF * FM_FP : o.fct_w + kn * T.NW * FM_FT));
            const float b = T.w[(t < 4 ? o.fcw_b + kn * FM_FW : (t < 6 ? o.fcf_b + kn * FM_FP : o.fct_b + kn * FM_FT)) + col];
            fm_f16 acc;
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            for (int kk = 0; kk < n_in; kk += 2) {
                const int kq = kk + g;
                const bool in = kq < n_in;              // an odd width: the last k-step's second product is 0 * 0
                const float a = in ? xs[i * XS + xoff + kq] : 0.0f;
                const float bb = in ? w[(size_t)kq * ncols + col] : 0.0f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
            }
            for (int r = 0; r < 16; ++r) hc[((r & 3) + 8 * (r >> 2) + 4 * g) * FM_HS + t * 32 + i] = fm_relu(acc[r] + b);
        }
        for (int idx = tid; idx < FM_TM * FM_L; idx += 256) {
            const int r = idx >> 6, u = idx & 63;
            hc[r * FM_HS + FM_HID + u] = r < rows ? T.state[(((size_t)(env_base + e0 + r) * K + k) * 4 + 2 * net + 1) * FM_L + u] : 0.0f;
        }
        __syncthreads();
        // ---- 3. z = hc wx + h wh + b: 8 column tiles, two per wave on two accumulators
        {
            const int n_in = n_w > 0 ? FM_HID : FM_FW + FM_FP;
            const float *wx = T.w + o.wx + kn * FM_HID * 4 * FM_L, *wh = T.w + o.wh + kn * FM_L * 4 * FM_L;
            const int c0 = wv * 32 + i, c1 = (wv + 4) * 32 + i;
            fm_f16 acc0, acc1;
            for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
            for (int kk = 0; kk < n_in; kk += 2) {
                const int kq = kk + g;
                const float a = hc[i * FM_HS + kq];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wx[(size_t)kq * 4 * FM_L + c0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wx[(size_t)kq * 4 * FM_L + c1], acc1, 0, 0, 0);
            }
#pragma unroll 4
            for (int kk = 0; kk < FM_L; kk += 2) {
                const int kq = kk + g;
                const float a = hc[i * FM_HS + FM_HID + kq];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wh[(size_t)kq * 4 * FM_L + c0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wh[(size_t)kq * 4 * FM_L + c1], acc1, 0, 0, 0);
            }
            const float b0 = T.w[o.lb + kn * 4 * FM_L + c0], b1 = T.w[o.lb + kn * 4 * FM_L + c1];
            for (int r = 0; r < 16; ++r) {
                const int rr = (r & 3) + 8 * (r >> 2) + 4 * g;
                zz[rr * FM_ZS + c0] = acc0[r] + b0;
                zz[rr * FM_ZS + c1] = acc1[r] + b1;
            }
        }
        __syncthreads();
        // ---- 4. the gates; the new h replaces the old one in LDS, the new (c, h) go to the library's state (acting call only)
        for (int idx = tid; idx < FM_TM * FM_L; idx += 256) {
            const int r = idx >> 6, u = idx & 63;
            float *st = T.state + (((size_t)(env_base + e0 + (r < rows ? r : 0)) * K + k) * 4 + 2 * net) * FM_L;
            const float *z = zz + r * FM_ZS;
            float c, h;
            fm_lstm_gate(z[u], z[FM_L + u], z[2 * FM_L + u], z[3 * FM_L + u], r < rows ? st[u] : 0.0f, &c, &h);
            hc[r * FM_HS + FM_HID + u] = h;
            if (ACT && r < rows) { st[u] = c; st[FM_L + u] = h; }
        }
        __syncthreads();
        // ---- 5. the head: thread (row, column)
        {
            const int r = tid >> 3, a = tid & 7;
            const float *hw = T.w + o.head_w + kn * FM_L * FM_AMAX, *hb = T.w + o.head_b + kn * FM_AMAX;
            if (net == 0) { if (a < n_a) lg[r * FM_AMAX + a] = fm_head(hc + r * FM_HS + FM_HID, hw, a, hb[a]); }
            else if (a == 0 && r < rows && out.value) out.value[(size_t)(e0 + r) * K + k] = fm_head(hc + r * FM_HS + FM_HID, hw, 0, hb[0]);
        }
        __syncthreads();
        // ---- 6. softmax, draw, fingerprint into the OTHER buffer, parity flip: one thread per row
        if (ACT && net == 0 && tid < rows) {
            const int r = tid;
            const size_t ge = (size_t)(env_base + e0 + r);
            float pi[FM_AMAX];
            const int act = fm_softmax_draw(lg + r * FM_AMAX, n_a, fm_uniform(seed, (uint32_t)ge, (uint32_t)k, step_key), pi);
            const int par = T.parity[ge * K + k];
            float *fw = T.fp + (((size_t)(par ^ 1) * T.max_envs + ge) * K + k) * FM_AMAX;
            for (int a = 0; a < FM_AMAX; ++a) {
                fw[a] = pi[a];
                if (out.pi) out.pi[((size_t)(e0 + r) * K + k) * FM_AMAX + a] = pi[a];
            }
            T.parity[ge * K + k] = par ^ 1;
            if (k < T.M) T.macts[ge * T.M + k] = act;
            else if (out.actions) out.actions[(size_t)(e0 + r) * T.S + (k - T.M)] = act;
        }
        __syncthreads();
    }
}

// rs_fma2c_reset: zero the state of environments env_base .. + n; with clear also both fingerprint buffers and the parity words
__global__ void rs_fma2c_reset_kernel(Fma2cTab T, int env_base, int n, int clear) {
    const size_t per = (size_t)T.K * 4 * FM_L, idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * per) return;
    T.state[(size_t)env_base * per + idx] = 0.0f;
    if (clear && idx < (size_t)n * T.K * FM_AMAX) {
        T.fp[(size_t)env_base * T.K * FM_AMAX + idx] = 0.0f;
        T.fp[((size_t)T.max_envs + env_base) * T.K * FM_AMAX + idx] = 0.0f;
        if (idx < (size_t)n * T.K) T.parity[(size_t)env_base * T.K + idx] = 0;
    }
}
#endif
