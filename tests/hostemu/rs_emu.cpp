// rs_emu.cpp -- HOST EMULATION of the step kernel (TEST INFRASTRUCTURE, never shipped, never loaded by resco_amd/).
//
// Compiles resco_amd/csrc/resco_step.h -- the very source of the HIP kernel -- and resco_host.h -- reset, re-init, the static agents,
// the buffer table and scenario -> tables as the library has them -- with g++ and runs the "threads" of a
// workgroup one after the other, phase by phase (HostExec::phase), in a selectable order (ascending, descending,
// shuffled).  The CPU tests compare it with the oracle bit for bit: that pins the kernel's LOGIC (and its independence
// of the thread order inside a phase) without a GPU; the -m gpu tests then pin the real thing.  The library exports the
// subset of the C ABI of include/resco_sim.h the tests need, so tests/hostemu/emu.py can reuse the ctypes wrapper.
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
#define RS_EMU_CHECK_MAIL 1
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

#ifdef RS_EMU_DEBUG
#include <stdio.h>
static int rs_dbg_slot = getenv("RS_DBG_SLOT") ? atoi(getenv("RS_DBG_SLOT")) : -1;
static int rs_dbg_t = getenv("RS_DBG_T") ? atoi(getenv("RS_DBG_T")) : -1;
static long rs_dbg_chain = 0;         // chain-walk steps of the current phase (reset by HostExec::phase)
#endif
#include "resco_host.h"

struct HostExec {
    unsigned long long role_begin() const { return 0ull; }
    void role_end(int, unsigned long long) const {}
    int wave_of(int tid) const { return tid >> 6; }
    // chunk of work for wave w on its i-th call in a phase (n waves): the GPU hands chunks out dynamically; here a fixed
    // assignment that depends on the thread order under test -- every chunk goes to exactly one wave either way
    int next_chunk(int32_t *, int w, int i, int n) const { return i * n + (order == 0 ? w : (order == 1 ? n - 1 - w : (w + n / 2 + 1) % n)); }
    int B;
    int order;          // 0 ascending, 1 descending, 2 shuffled (a different permutation in every phase)
    uint32_t rng = 12345u;
    template <class F> void phase(int id, F f) {
#ifdef RS_EMU_DEBUG
        if (getenv("RS_DBG_PHASES")) { printf("phase %d\n", id); fflush(stdout); }
        rs_dbg_chain = 0;
#endif
        if (order == 0) for (int t = 0; t < B; ++t) f(t);
        else if (order == 1) for (int t = B - 1; t >= 0; --t) f(t);
        else {
            std::vector<int> p((size_t)B);
            for (int i = 0; i < B; ++i) p[i] = i;
            for (int i = B - 1; i > 0; --i) { rng = rng * 1664525u + 1013904223u; std::swap(p[i], p[(rng >> 8) % (uint32_t)(i + 1)]); }
            for (int t : p) f(t);
        }
    }
};

struct rs_sim {
    KTab K{};
    State G{};
    Out O{};
    KParams P{};
    Lds L{};
    int n_envs = 0, block = 0, order = 0, ratio = 1;
    size_t lds = 0;
    std::vector<char> slab, outb, smem;
    std::vector<int32_t> env, tls, actions, trip_log, pairs, valid, ordr;
    uint32_t out_mask = OUT_ALL;
    std::vector<long long> stats;
    std::vector<uint16_t> dep_next;
    std::vector<uint32_t> mail;
    // the tables of K: copies of the packed tables AND of the caller's arrays (which it may free).  Byte blocks: the 16-byte records rest
    // on operator new's alignment, and an empty table is 16 zero bytes, not a null pointer (a read of one does not fault here)
    std::vector<std::vector<char>> keep;
    Buf bufs[RS_BUF_COUNT]{};
    std::string err;
    int n_pairs = 0;
};
static std::string g_err;
static const void *keep_copy(rs_sim *h, const void *src, size_t bytes) {
    h->keep.emplace_back((const char *)src, (const char *)src + bytes);
    if (h->keep.back().empty()) h->keep.back().resize(16, 0);
    return h->keep.back().data();
}

static void run_step(rs_sim *h, int n_ticks, int do_fsm, int do_observe = 1) {
    KParams P = h->P;
    P.n_ticks = n_ticks; P.do_fsm = do_fsm; P.do_observe = do_observe; P.out_mask = h->out_mask; P.prof = nullptr;
    for (int env = 0; env < h->n_envs; ++env) {
        std::fill(h->smem.begin(), h->smem.end(), (char)0xA5);      // LDS is not zero on the GPU either
        g_smem = h->smem.data();
        HostExec ex;
        ex.B = h->block; ex.order = h->order;
        ex.rng = 777u + (uint32_t)env;
        switch (h->K.capacity) {
            case 128: rs_step_body<128>(ex, h->L, h->K, h->G, h->O, P, h->actions.data(), env); break;
            case 256: rs_step_body<256>(ex, h->L, h->K, h->G, h->O, P, h->actions.data(), env); break;
            case 896: rs_step_body<896>(ex, h->L, h->K, h->G, h->O, P, h->actions.data(), env); break;
            case 1024: rs_step_body<1024>(ex, h->L, h->K, h->G, h->O, P, h->actions.data(), env); break;
            default: rs_step_body<0>(ex, h->L, h->K, h->G, h->O, P, h->actions.data(), env); break;
        }
    }
}

extern "C" {
// block_threads < 0 selects thread order: -1 descending, -2 shuffled (with one thread per slot); order > 0 as given
int rs_create(const rs_scenario *sc, const rs_params *p, int32_t n_envs, int32_t env_base, int32_t device_id, int32_t block_threads, rs_handle *out) {
    rs_sim *h = new rs_sim();
    PackedTables PT;
    if (const char *msg = rs_pack_tables(PT, sc)) { g_err = msg; delete h; return RS_ELIMIT; }
    const int C = sc->capacity;
    h->order = device_id;           // the emulation has no device: the argument carries the thread order
    h->block = block_threads > 0 ? block_threads : (C > 1024 ? 1024 : C);
    h->n_envs = n_envs;
    KTab &K = h->K;
#define KEEP(dst, type, src, count) dst = (const type *)keep_copy(h, src, (size_t)(count) * sizeof(type));
    RS_KTAB_TABLES(KEEP, K, PT, sc)
#undef KEEP
    h->ratio = rs_step_ratio(p);
    rs_ktab_scalars(K, PT, sc, h->ratio);
    h->P = rs_kparams(p, env_base, n_envs);
    const size_t N = (size_t)n_envs, NC = N * C, S = (size_t)sc->n_signals;
    h->G.nc = NC; h->slab.assign(State::bytes(NC), 0); h->G.base = h->slab.data();
    h->O.n = n_envs; h->O.o = sc->n_obs; h->O.s = sc->n_signals; h->O.lm = PT.lmax;
    h->outb.assign(h->O.bytes(), 0); h->O.base = h->outb.data();
    h->env.assign(N * 4, 0); h->tls.assign(N * S * TLS_W, 0); h->stats.assign(N * ST_N, 0); h->actions.assign(N * S, 0);
    h->dep_next.assign(N * K.n_dep, 0);
    h->mail.assign(N * (size_t)((C + 31) / 32), 0u);
    h->G.env = h->env.data(); h->G.tls = h->tls.data(); h->G.stats = h->stats.data(); h->G.dep_next = h->dep_next.data(); h->G.mail = h->mail.data();
    h->G.trip_log = nullptr;
    if (p->trip_log) { h->trip_log.assign(N * (size_t)sc->n_trips * 4, 0); h->G.trip_log = h->trip_log.data(); }
    h->lds = lds_carve(&h->L, C, K.n_cells, K.n_arr, K.n_dep, sc->n_obs, sc->n_signals, sc->n_vtypes, K.tls_maxl);
    if (!lds_fix_matches(h->L, C)) { g_err = "the layout of the working memory does not match the kernel's literals (lds_carve / LdsFix)"; delete h; return RS_EINVAL; }
    h->L.cell_inv = PT.cell_inv;
    h->smem.assign(h->lds + 64, 0);
    rs_fill_bufs(h->bufs, h->G, h->O, h->actions.data(), BufDims{n_envs, C, sc->n_signals, sc->n_obs, PT.lmax, K.n_dep, p->trip_log ? sc->n_trips : 0});
    *out = h;
    return rs_reset(h, nullptr);
}
void rs_destroy(rs_handle h) { delete h; }
const char *rs_last_error(rs_handle h) { return h ? h->err.c_str() : g_err.c_str(); }
int rs_reset(rs_handle h, void *) {
    for (int env = 0; env < h->n_envs; ++env) rs_reset_env(h->K, h->G, h->P, env, 0, 1);
    run_step(h, 0, 0);
    return RS_OK;
}
int rs_step(rs_handle h, const int32_t *actions, int32_t, void *) {
    if (actions) memcpy(h->actions.data(), actions, h->actions.size() * 4);
    run_step(h, h->K.step_length * h->ratio, 1);
    return RS_OK;
}
int rs_ticks(rs_handle h, int32_t n, void *) { run_step(h, n, 0); return RS_OK; }
int rs_step_sim(rs_handle h, int32_t n, void *) { run_step(h, n, 0, 0); return RS_OK; }
int rs_set_outputs(rs_handle h, uint64_t buffer_mask) {
    h->out_mask = rs_out_mask(buffer_mask);
    return RS_OK;
}
int rs_sync(rs_handle) { return RS_OK; }
int rs_reinit_signals(rs_handle h, void *) {
    for (int env = 0; env < h->n_envs; ++env) rs_reinit_env(h->K, h->G, h->P, env, 0, 1);
    run_step(h, 0, 0);
    return RS_OK;
}
int rs_act_random(rs_handle h, uint32_t step_key, void *) {
    for (int i = 0; i < h->n_envs * h->K.n_signals; ++i) h->actions[i] = rs_random_action(h->K, h->P, step_key, i);
    return RS_OK;
}
int rs_act_maxwave(rs_handle h, const int32_t *phase_pairs, int32_t n_pairs, const int32_t *valid, const int32_t *order, int32_t use_pressure, void *) {
    const int S = h->K.n_signals;
    if (!(h->out_mask & (use_pressure ? OUT_MPLIGHT : OUT_WAVE))) return RS_EINVAL;     // (as the HIP library: the rows it would read are switched off)
    if (phase_pairs) {
        h->pairs.assign(phase_pairs, phase_pairs + n_pairs * 2); h->valid.assign(valid, valid + S * n_pairs); h->ordr.assign(order, order + S * n_pairs);
        h->n_pairs = n_pairs;
    }
    for (int i = 0; i < h->n_envs * S; ++i)
        h->actions[i] = rs_maxwave_action(h->K, h->pairs.data(), h->n_pairs, h->valid.data(), h->ordr.data(), use_pressure, h->O.mplight(), h->O.wave(), i);
    return RS_OK;
}
// the static agents + the step of a group of handles in one call (include/resco_sim.h); the policy network is device code only
int rs_group_step(const rs_handle *hs, int32_t n, const rs_group_agent *agent, int32_t n_steps) {
    if (!hs || n <= 0 || n_steps <= 0) return RS_EINVAL;
    const int kind = agent ? agent->kind : RS_AGENT_NONE;
    if (kind == RS_AGENT_IDQN || kind < 0 || kind > RS_AGENT_IDQN) return RS_EINVAL;
    for (int i = 0; i < n; ++i)
        if ((kind == RS_AGENT_MAXWAVE || kind == RS_AGENT_MAXPRESSURE) && hs[i]->n_pairs == 0) return RS_EINVAL;
    for (int k = 0; k < n_steps; ++k)
        for (int i = 0; i < n; ++i) {
            int rc = RS_OK;
            if (kind == RS_AGENT_RANDOM) rc = rs_act_random(hs[i], agent->step_key + (uint32_t)k, nullptr);
            else if (kind == RS_AGENT_MAXWAVE || kind == RS_AGENT_MAXPRESSURE) rc = rs_act_maxwave(hs[i], nullptr, hs[i]->n_pairs, nullptr, nullptr, kind == RS_AGENT_MAXPRESSURE, nullptr);
            if (rc != RS_OK) return rc;
            rs_step(hs[i], nullptr, 1, nullptr);
        }
    return RS_OK;
}
int rs_get_buffer(rs_handle h, int32_t which, void **dev_ptr, int64_t shape[4], int32_t *ndim, int32_t *dtype) {
    if (!h || which < 0 || which >= RS_BUF_COUNT) return RS_EINVAL;
    rs_buf_describe(h->bufs[which], dev_ptr, shape, ndim, dtype);
    return RS_OK;
}
int rs_read_buffer(rs_handle h, int32_t which, void *host_dst, int64_t nbytes) {
    auto &B = h->bufs[which];
    if ((size_t)nbytes != B.bytes) return RS_EINVAL;
    if (B.bytes) memcpy(host_dst, B.ptr, B.bytes);
    return RS_OK;
}
int rs_stats(rs_handle h, int64_t *out) { return rs_read_buffer(h, RS_BUF_STATS, out, (int64_t)h->n_envs * ST_N * 8); }
int rs_set_seed(rs_handle h, uint32_t seed) { h->P.seed = seed; return RS_OK; }
// snapshots: every buffer, in id order
struct Snap { std::vector<std::vector<char>> b; };
int rs_snapshot(rs_handle h, void **snap) {
    Snap *S = new Snap();
    for (int i = 0; i < RS_BUF_COUNT; ++i) S->b.emplace_back((char *)h->bufs[i].ptr, (char *)h->bufs[i].ptr + (h->bufs[i].ptr ? h->bufs[i].bytes : 0));
    *snap = S;
    return RS_OK;
}
int rs_restore(rs_handle h, const void *snap) {
    const Snap *S = (const Snap *)snap;
    for (int i = 0; i < RS_BUF_COUNT; ++i) if (!S->b[i].empty()) memcpy(h->bufs[i].ptr, S->b[i].data(), S->b[i].size());
    return RS_OK;
}
void rs_snapshot_free(rs_handle, void *snap) { delete (Snap *)snap; }
int rs_timing(rs_handle, int32_t) { return RS_OK; }
int rs_timing_read(rs_handle, float *ms, int32_t *n) { if (ms) *ms = 0.0f; if (n) *n = 0; return RS_OK; }
int rs_phase_profile(rs_handle, int32_t, uint64_t *out) { if (out) memset(out, 0, 16 * 8); return RS_OK; }
int rs_info(rs_handle h, int32_t *n_envs, int32_t *block_threads, int32_t *lds_bytes, int32_t *max_lanes) {
    rs_info_describe(h->n_envs, h->block, h->lds, h->K.lmax, n_envs, block_threads, lds_bytes, max_lanes);
    return RS_OK;
}
}
