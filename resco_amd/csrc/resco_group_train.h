// resco_group_train.h -- what joins the policy kernels, the step kernel and the fused DQN learners into a training loop that one
// call enqueues (rs_group_train of include/resco_sim.h), and the three entry points it is made of (rs_idqn_pack_weights,
// rs_dqn_sync_target / rs_mplight_dqn_sync_target, the ring recorder).
//
// What it replaces, per env-step of tools/idqn_train.py / tools/mplight_train.py --device-update: replay.stage and replay.commit
// (four copy launches, three scalar host-to-device stores), `ret += rew`, the target's copy_ per tensor, and
// FusedIDQN.refresh_on_device (three index_select + mul_ + casting copy_ and the b3 fill) -- about twenty launches and as many
// trips through the Python interpreter -- by two recorder launches per pipe, one copy launch per target sync and one pack launch per
// update.
//
// Everything here is a GT_HD function in plain C++ over (first index, stride), which the kernels call with their thread's grid-stride
// position and a host compiler builds as well (tests/group_train_host): the pack's analytic fragment index and its element
// conversion, the recorder's bodies, the copy of the target sync, and the launch-free bookkeeping of a step (gt_plan).
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define GT_HD __host__ __device__ static inline
#else
#define GT_HD static inline
#endif

struct alignas(16) GtVec16 { uint32_t x, y, z, w; };       // one 16-byte word of the vector paths

// ------------------------------------------------------------------------------------------------ the pack of the IDQN policy
// The three linear layers as f16 MFMA B-fragments (resco_policy.h; resco_amd/agents/idqn_fused.py: _b_fragments): element
// (kk, nt, lane, j) of a [K][N] matrix is row kk * 8 + (lane >> 5) * 4 + j, column nt * 32 + (lane & 31), zero outside the matrix.
//   w1 [64 c][hp][2][64][4] from fc1_w[s] = [64 c][H * 4][64] (K = H * 4 per conv channel, hp = lmax / 2 k-steps, N = 64)
//   w2 [8][2][64][4]        from fc2_w[s] = [64][64]
//   w3 [8][64][4]           from fc3_w[s] = [64][amax]  (one column tile; columns amax .. 31 are padding)
// gt_pack_src: the flat index into the signal's source matrix of output element o of fragment buffer `which` (0, 1, 2), -1 where the
// element is padding -- idqn_fused.repack_index(lmax, amax)[w1 / w2 / w3][o] for every lmax in 2 .. 17 and amax in 1 .. 8
// (tests/test_group_train_cpu.py).  No gather table is read.
GT_HD int gt_pack_count(int which, int lmax) { return which == 0 ? 64 * (lmax / 2) * 512 : (which == 1 ? 4096 : 2048); }
// VALUE: the actor-critic pack (rs_ippo_pack_weights).  Its w3 is gathered from the virtual [64][9] matrix of
// resco_amd/agents/ippo_fused.py: fc3_with_value -- columns 0 .. amax - 1 fc3_w, zeros up to 7, the value head v_w in column 8 -- and the
// index is ippo_repack_index(lmax, amax)['w3'] (amax does not enter it); w1 and w2 are the same.  Without VALUE: an IDQN pack, as ever.
#define GT_VALUE_COL 8      // POL_QMAX: the value head's column of the fc3 tile, its bias in b3[s][8]
template <bool VALUE> GT_HD int gt_pack_src_t(int which, int o, int lmax, int amax) {
    const int j = o & 3, lane = (o >> 2) & 63;
    const int krow = (lane >> 5) * 4 + j, col = lane & 31;
    if (which == 0) {
        const int H4 = (lmax - 1) * 4, per_c = (lmax / 2) * 512;
        const int c = o / per_c, r = o - c * per_c;
        const int k = (r >> 9) * 8 + krow, n = ((r >> 8) & 1) * 32 + col;
        return k < H4 ? (c * H4 + k) * 64 + n : -1;
    }
    if (which == 1) return ((o >> 9) * 8 + krow) * 64 + ((o >> 8) & 1) * 32 + col;
    if (VALUE) return col <= GT_VALUE_COL ? ((o >> 8) * 8 + krow) * (GT_VALUE_COL + 1) + col : -1;
    return col < amax ? ((o >> 8) * 8 + krow) * amax + col : -1;
}
GT_HD int gt_pack_src(int which, int o, int lmax, int amax) { return gt_pack_src_t<false>(which, o, lmax, amax); }
GT_HD int gt_pack_src_value(int which, int o, int lmax, int amax) { return gt_pack_src_t<true>(which, o, lmax, amax); }

// fp32 -> fp16 bits, round to nearest even, overflow to infinity, denormals kept: what a casting copy_ and numpy's astype do.  On the
// device this is one v_cvt_f16_f32 (the default rounding mode is nearest-even and the kernels here never change it).
GT_HD uint16_t gt_f2h(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __half_as_ushort(__float2half(f));
#else
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, ax = x & 0x7FFFFFFFu;
    if (ax >= 0x7F800000u) return (uint16_t)(sign | (ax > 0x7F800000u ? 0x7E00u : 0x7C00u));      // NaN, infinity
    if (ax >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);                                       // rounds to 65520 or more: infinity
    if (ax < 0x33000001u) return (uint16_t)sign;                                                    // at most 2^-25: zero
    const int e = (int)(ax >> 23) - 127;
    uint32_t man = (ax & 0x7FFFFFu) | 0x800000u;
    const int shift = e < -14 ? 13 + (-14 - e) : 13;                                                // a denormal result loses more bits
    const uint32_t half = 1u << (shift - 1), rest = man & ((1u << shift) - 1u);
    man >>= shift;
    if (rest > half || (rest == half && (man & 1u))) man += 1u;                                     // (a carry walks into the exponent: right)
    return (uint16_t)(sign | ((e < -14 ? 0u : (uint32_t)(e + 15) << 10) + (e < -14 ? man : man - 0x400u)));
#endif
}

// The pack of ONE signal as a flat list of work units, four output elements each (j = 0 .. 3: one 8-byte store; the four share their
// column and their padding status): units of w1, then of w2, then of w3, then the 32 floats of b3 one per unit.
struct GtPack {
    const float *fc1_w, *fc2_w, *fc3_w, *fc3_b;     // the learner's fp32 parameters, all signals
    uint16_t *w1, *w2, *w3;                         // the policy's fragment buffers, all signals
    float *b3;                                      // [S][32]
    int32_t lmax, amax;
};
struct GtPackValue : GtPack {                       // the actor-critic pack: also the value head [S][64][1], [S][1].  (A struct of its own:
    const float *v_w, *v_b;                         // the IDQN kernel keeps its argument layout and with it its instructions)
};
GT_HD int gt_pack_units(int lmax) { return (gt_pack_count(0, lmax) + 4096 + 2048) / 4 + 32; }
template <bool VALUE, class Pack> GT_HD void gt_pack_unit_t(const Pack &P, int s, int u) {
    const int n1 = gt_pack_count(0, P.lmax) / 4, n2 = 1024, n3 = 512;
    int which = 0;
    if (u >= n1 + n2 + n3) {                        // b3: zero beyond the signal set's amax columns (VALUE: but for v_b in column 8)
        const int a = u - (n1 + n2 + n3);
        if constexpr (VALUE) P.b3[(size_t)s * 32 + a] = a < P.amax ? P.fc3_b[(size_t)s * P.amax + a] : (a == GT_VALUE_COL ? P.v_b[s] : 0.0f);
        else P.b3[(size_t)s * 32 + a] = a < P.amax ? P.fc3_b[(size_t)s * P.amax + a] : 0.0f;
        return;
    }
    if (u >= n1 + n2) { which = 2; u -= n1 + n2; } else if (u >= n1) { which = 1; u -= n1; }
    const size_t per_src = which == 0 ? (size_t)64 * (P.lmax - 1) * 4 * 64 : (which == 1 ? (size_t)4096 : (size_t)64 * P.amax);
    const float *src = (which == 0 ? P.fc1_w : (which == 1 ? P.fc2_w : P.fc3_w)) + (size_t)s * per_src;
    uint16_t *dst = (which == 0 ? P.w1 : (which == 1 ? P.w2 : P.w3)) + (size_t)s * gt_pack_count(which, P.lmax) + (size_t)u * 4;
    uint16_t h[4];
    for (int j = 0; j < 4; ++j) {
        const int i = gt_pack_src_t<VALUE>(which, u * 4 + j, P.lmax, P.amax);
        if constexpr (VALUE) {
            if (which == 2) {                       // element (k, c) of the virtual [64][9] matrix: fc3_w, zeros, v_w
                const int k = i / (GT_VALUE_COL + 1), c = i - k * (GT_VALUE_COL + 1);
                h[j] = i < 0 ? (uint16_t)0 : (c < P.amax ? gt_f2h(src[k * P.amax + c]) : (c == GT_VALUE_COL ? gt_f2h(P.v_w[(size_t)s * 64 + k]) : (uint16_t)0));
                continue;
            }
        }
        h[j] = i >= 0 ? gt_f2h(src[i]) : (uint16_t)0;
    }
    uint32_t lo = (uint32_t)h[0] | ((uint32_t)h[1] << 16), hi = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
    ((uint32_t *)dst)[0] = lo;                      // (a fragment buffer is a torch allocation: its elements 4 u .. 4 u + 3 are 8-byte aligned)
    ((uint32_t *)dst)[1] = hi;
}
GT_HD void gt_pack_unit(const GtPack &P, int s, int u) { gt_pack_unit_t<false, GtPack>(P, s, u); }
GT_HD void gt_pack_unit_value(const GtPackValue &P, int s, int u) { gt_pack_unit_t<true, GtPackValue>(P, s, u); }

// ------------------------------------------------------------------------------------------------ copies
// n elements of 2 or 4 bytes from src to dst for the "threads" i0, i0 + stride, ..: 16-byte words where `vec` (the caller found both
// pointers 16-byte aligned), the tail and everything else element by element.  conv: the 4-byte source elements are int32 and
// become float (exact below 2^24: the counts of states.mplight and rewards.pressure).
template <class E> GT_HD void gt_copy(E *dst, const E *src, int n, int vec, int i0, int stride) {
    const int per = 16 / (int)sizeof(E), nv = vec ? n / per : 0;
    for (int i = i0; i < nv; i += stride) ((GtVec16 *)dst)[i] = ((const GtVec16 *)src)[i];
    for (int i = nv * per + i0; i < n; i += stride) dst[i] = src[i];
}
GT_HD uint32_t gt_f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
GT_HD void gt_copy_i32_f32(float *dst, const int32_t *src, int n, int vec, int i0, int stride) {
    const int nv = vec ? n / 4 : 0;
    for (int i = i0; i < nv; i += stride) {
        const GtVec16 v = ((const GtVec16 *)src)[i];
        ((GtVec16 *)dst)[i] = GtVec16{gt_f2u((float)(int32_t)v.x), gt_f2u((float)(int32_t)v.y), gt_f2u((float)(int32_t)v.z), gt_f2u((float)(int32_t)v.w)};
    }
    for (int i = nv * 4 + i0; i < n; i += stride) dst[i] = (float)src[i];
}

// ------------------------------------------------------------------------------------------------ the ring recorder
// One launch of ONE pipe into its own rows of ONE ring slot; every part is optional (a NULL source).  Before the policy kernel: the
// observation it is about to see.  After the step kernel: the action taken, the reward, the running return and -- the first pipe's
// launch only -- the slot's done byte.
enum { GT_OBS_F16 = 0, GT_OBS_I32_F32 = 1, GT_OBS_F32 = 2 };
struct GtRec {
    const void *obs_src;        // the pipe's observation buffer: f16 (IDQN), int32 (MPLight) or f32 (MPLightFULL)
    void *obs_dst;              // the pipe's first row of the slot: f16 / f32 / f32
    int32_t n_obs, obs_kind, vec;
    const int32_t *act_src;     // int32 [n][S]: RS_BUF_ACTIONS (IDQN) or the global pair indices (MPLight)
    int16_t *act_dst;
    const void *rew_src;        // f32 RS_BUF_WAIT_NORM, or int32 RS_BUF_PRESSURE when rew_i32
    float *rew_dst;
    float *ret;                 // NULL, or the pipe's rows of the running return: ret += rew, one fp32 addition
    int32_t n_sig, rew_i32;     // n_sig = the pipe's n_envs * S
    uint8_t *done_dst;          // NULL, or the slot's byte
    int32_t done;
};
GT_HD void gt_record(const GtRec &R, int i0, int stride) {
    if (R.obs_src) {
        if (R.obs_kind == GT_OBS_F16) gt_copy((uint16_t *)R.obs_dst, (const uint16_t *)R.obs_src, R.n_obs, R.vec, i0, stride);
        else if (R.obs_kind == GT_OBS_F32) gt_copy((uint32_t *)R.obs_dst, (const uint32_t *)R.obs_src, R.n_obs, R.vec, i0, stride);
        else gt_copy_i32_f32((float *)R.obs_dst, (const int32_t *)R.obs_src, R.n_obs, R.vec, i0, stride);
    }
    if (R.act_src)
        for (int i = i0; i < R.n_sig; i += stride) R.act_dst[i] = (int16_t)R.act_src[i];
    if (R.rew_src)
        for (int i = i0; i < R.n_sig; i += stride) {
            const float r = R.rew_i32 ? (float)((const int32_t *)R.rew_src)[i] : ((const float *)R.rew_src)[i];
            R.rew_dst[i] = r;
            if (R.ret) R.ret[i] = R.ret[i] + r;
        }
    if (R.done_dst && i0 == 0) *R.done_dst = (uint8_t)(R.done != 0);
}

// ------------------------------------------------------------------------------------------------ the target sync
// target <- params for up to eight tensors in one launch (blockIdx.y = tensor): the element counts travel with the pointers.
struct GtSync {
    const float *src[8];
    float *dst[8];
    int64_t n[8];
    int32_t count;
};
GT_HD void gt_sync_tensor(const GtSync &Y, int t, int i0, int stride) {
    const float *src = Y.src[t];
    float *dst = Y.dst[t];
    const int64_t n = Y.n[t];
    const int vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const int64_t nv = vec ? n / 4 : 0;
    for (int64_t i = i0; i < nv; i += stride) ((GtVec16 *)dst)[i] = ((const GtVec16 *)src)[i];
    for (int64_t i = nv * 4 + i0; i < n; i += stride) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------ the done flags of a segment
// done[j] = (j == hit) for j < m: the slots a segment loop (resco_ppo_loop.h: bytes; resco_fma2c_loop.h: the learner's int32 words)
// fills from one slot on to the segment's or the call's end, in one launch; hit = the step at which the horizon is reached, counted
// from the first of them (anything outside 0 .. m - 1: none of them).
template <class E> GT_HD void gt_done(E *done, int32_t m, int32_t hit, int i0, int stride) {
    for (int j = i0; j < m; j += stride) done[j] = (E)(j == hit);
}

// ------------------------------------------------------------------------------------------------ the bookkeeping of a step
// Step k of a call that starts at agent step t0 with the ring at (head, count): what one iteration of the tools' --device-update
// loops decides on the host.  The observation and the transition go into `slot`; afterwards the ring stands at (head, count), which
// is what the learner is told; `sync`: learner.t = t0 + k + 1 is a multiple of target_update; `update`: the ring holds a minibatch,
// len(replay) = (count - 1) * pool >= batch with pool = n_envs (DeviceReplay) or n_envs * n_signals (MPLightReplay), and at least one
// update per step is asked for.  epsilon: idqn_learn.linear_epsilon(t0 + k, start, end, decay_steps) in double, rounded to float once
// (what passing a Python float through ctypes.c_float does).  A function of t0 + k and of the position before step k only: any split
// of the same steps into calls gives the same plans.
struct GtLoop {
    int32_t capacity, batch, target_update, updates_per_step, decay_steps, done_step;
    int64_t pool, t0;
    int32_t head, count;
    double eps_start, eps_end;
};
struct GtStep {
    int32_t slot, head, count, sync, update, done;
    uint32_t key;
    float epsilon;
};
GT_HD float gt_epsilon(int64_t t, double start, double end, int32_t decay_steps) {
    if (t >= (int64_t)decay_steps) return (float)end;
    return (float)(start + (end - start) * ((double)t / (double)decay_steps));
}
GT_HD GtStep gt_plan(const GtLoop &L, int32_t k) {
    GtStep s;
    s.slot = (int32_t)(((int64_t)L.head + k) % L.capacity);
    s.head = (int32_t)(((int64_t)L.head + k + 1) % L.capacity);
    const int64_t c = (int64_t)L.count + k + 1;
    s.count = c < L.capacity ? (int32_t)c : L.capacity;
    const int64_t t = L.t0 + k;
    s.sync = (t + 1) % L.target_update == 0;
    s.update = L.updates_per_step >= 1 && (int64_t)(s.count - 1) * L.pool >= (int64_t)L.batch;
    s.done = k == L.done_step;
    s.key = (uint32_t)(t & 0xFFFFFFFFll);
    s.epsilon = gt_epsilon(t, L.eps_start, L.eps_end, L.decay_steps);
    return s;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------------ kernels (grid-stride: any grid covers any size)
__global__ void __launch_bounds__(256) rs_train_record_kernel(GtRec R) { gt_record(R, (int)(blockIdx.x * 256 + threadIdx.x), (int)(gridDim.x * 256)); }
// grid (x, S): the units of signal blockIdx.y
__global__ void __launch_bounds__(256) rs_idqn_pack_kernel(GtPack P) {
    const int n = gt_pack_units(P.lmax);
    for (int u = blockIdx.x * 256 + threadIdx.x; u < n; u += gridDim.x * 256) gt_pack_unit(P, (int)blockIdx.y, u);
}
// the same grid for the actor-critic pack (rs_ippo_pack_weights)
__global__ void __launch_bounds__(256) rs_ippo_pack_kernel(GtPackValue P) {
    const int n = gt_pack_units(P.lmax);
    for (int u = blockIdx.x * 256 + threadIdx.x; u < n; u += gridDim.x * 256) gt_pack_unit_value(P, (int)blockIdx.y, u);
}
// grid (x, tensors)
__global__ void __launch_bounds__(256) rs_sync_target_kernel(GtSync Y) { gt_sync_tensor(Y, (int)blockIdx.y, (int)(blockIdx.x * 256 + threadIdx.x), (int)(gridDim.x * 256)); }
// E = uint8_t (rs_group_ppo_train) or int32_t (rs_group_fma2c_train)
template <class E> __global__ void __launch_bounds__(256) rs_done_kernel(E *done, int32_t m, int32_t hit) {
    gt_done(done, m, hit, (int)(blockIdx.x * 256 + threadIdx.x), (int)(gridDim.x * 256));
}
#endif
