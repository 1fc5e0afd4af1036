// resco_host.h -- what surrounds the step body and is the same for the HIP library (resco_sim.hip) and for the host emulation of
// the CPU tests (tests/hostemu/rs_emu.cpp): the per-element bodies of reset, re-init and the static agents, the buffer-mask ->
// OUT_* mapping, the table of the RS_BUF_* buffers, and scenario -> KTab / KParams.  Written like resco_step.h: the includer
// supplies the qualifier macros, nothing here calls HIP.  The library wraps the bodies in kernels and uploads the tables; the
// emulation calls the bodies in loops and keeps the tables in host memory.
#pragma once
#include <stdio.h>

#include "resco_step.h"

// ------------------------------------------------------------------------------------------------ reset / re-init (device or host)
// Each body does the share of "thread" `first` of `stride` for ONE environment: the kernels pass (threadIdx.x, blockDim.x), the
// emulation (0, 1).
// reset an environment: no vehicles, every backlog at its first trip, TLS programs freshly installed
// (Signal.__init__, traffic_signal.py:93-100)
RS_DEV void rs_reset_env(const KTab &T, const State &G, const KParams &P, int env, int first, unsigned stride) {
    const int C = T.capacity, S = T.n_signals;
    const size_t eo = (size_t)env * C;
    for (int s = first; s < C; s += stride) {
        G.lane()[eo + s] = LANE_NONE; G.trip()[eo + s] = TRIP_NONE; G.owner()[eo + s] = OWNER_NONE;
        G.rwait()[eo + s] = 0; G.swait()[eo + s] = 0; G.cursor()[eo + s] = 0; G.depart()[eo + s] = 0; G.wtot()[eo + s] = 0;
        G.pos()[eo + s] = 0.0f; G.speed()[eo + s] = 0.0f; G.accel()[eo + s] = 0.0f; G.tloss()[eo + s] = 0.0f; G.sf()[eo + s] = 1.0f;
        G.coop(0)[eo + s] = COOP_NONE; G.coop(1)[eo + s] = COOP_NONE; G.cooplead(0)[eo + s] = COOP_NONE; G.cooplead(1)[eo + s] = COOP_NONE;
    }
    for (int s = first; s < S; s += stride) {
        int ph, left;
        if (P.fixed_program) { ph = T.cold.fix_init_phase[s]; left = T.cold.fix_init_left[s]; }
        else { ph = T.cold.tls_init_phase[s]; left = T.cold.tls_dur[T.cold.tls_dur_off[s] + ph]; }
        G.tls[(env * S + s) * TLS_W + 0] = ph; G.tls[(env * S + s) * TLS_W + 1] = left; G.tls[(env * S + s) * TLS_W + 2] = 0; G.tls[(env * S + s) * TLS_W + 3] = 0;
    }
    // (every backlog starts at the first trip of the environment's OWN demand: rs_set_demand)
    const uint16_t *dep_first = T.dem_ ? Demand<true, KTab>(T, env).dep_first() : T.cold.dep_first;
    for (int d = first; d < T.n_dep; d += stride) G.dep_next[(size_t)env * T.n_dep + d] = dep_first[d];
    for (int i = first; i < (C + 31) / 32; i += stride) G.mail[(size_t)env * ((C + 31) / 32) + i] = 0u;
    for (int i = first; i < 4; i += stride) G.env[env * 4 + i] = 0;
    for (int i = first; i < ST_N; i += stride) G.stats[(size_t)env * ST_N + i] = 0;
    if (G.trip_log)
        for (int i = first; i < T.n_trips * 4; i += stride) G.trip_log[(size_t)env * T.n_trips * 4 + i] = 0;
}
// fresh Signal objects on the running simulation (rs_reinit_signals)
RS_DEV void rs_reinit_env(const KTab &T, const State &G, const KParams &P, int env, int first, unsigned stride) {
    const int C = T.capacity, S = T.n_signals;
    const size_t eo = (size_t)env * C;
    for (int s = first; s < C; s += stride) { G.owner()[eo + s] = OWNER_NONE; G.rwait()[eo + s] = 0; }
    for (int s = first; s < S; s += stride) {
        if (!P.fixed_program) G.tls[(env * S + s) * TLS_W + 1] = T.cold.tls_dur[T.cold.tls_dur_off[s] + G.tls[(env * S + s) * TLS_W + 0]];
        G.tls[(env * S + s) * TLS_W + 2] = 0; G.tls[(env * S + s) * TLS_W + 3] = 0;
    }
}

// ------------------------------------------------------------------------------------------------ static agents (device or host)
// The action of flat index i = env * n_signals + signal, i < n_envs * n_signals.
// STOCHASTIC (agents/stochastic.py:17-18): uniform green index per (env, signal, step)
RS_DEV int32_t rs_random_action(const KTab &T, const KParams &P, uint32_t step_key, int i) {
    const int S = T.n_signals;
    const int env = i / S, s = i - env * S;
    const uint32_t h = d_hash(P.seed ^ 0xA5A5A5A5u, (uint32_t)(P.env_base + env), (uint32_t)s, step_key, 7u);
    return (int32_t)(h % (uint32_t)T.cold.tls_ngreen[s]);
}
// MAXWAVE / MAXPRESSURE (agents/maxwave.py:18-38, maxpressure.py:13-18): first maximum over the valid
// phase pairs (in the reference's iteration order) of obs[pair0] + obs[pair1]
RS_DEV int32_t rs_maxwave_action(const KTab &T, const int32_t *pairs, int n_pairs, const int32_t *valid, const int32_t *order, int use_pressure,
                                 const int32_t *mplight, const int32_t *wave, int i) {
    const int s = i % T.n_signals;
    const int32_t *obs = use_pressure ? mplight + (size_t)i * 13 + 1 : wave + (size_t)i * 12;
    bool have = false;
    int best = 0, best_act = 0;
    for (int j = 0; j < n_pairs; ++j) {
        const int p = order[s * n_pairs + j];     // the reference walks valid_acts in dict order; ties keep the first
        if (p < 0) break;
        const int act = valid[s * n_pairs + p];
        if (act < 0) continue;
        const int press = obs[pairs[p * 2]] + obs[pairs[p * 2 + 1]];
        if (!have || press > best) { have = true; best = press; best_act = act; }
    }
    return best_act;
}

// ------------------------------------------------------------------------------------------------ host side
// which output buffers an observe writes (rs_set_outputs: bit b = buffer id b) as the kernel's OUT_* groups
static inline uint32_t rs_out_mask(uint64_t buffer_mask) {
    uint32_t m = 0;
    if (buffer_mask & (1ull << RS_BUF_LANE_AGG)) m |= OUT_LANE_AGG;
    if (buffer_mask & (1ull << RS_BUF_DRQ_NORM)) m |= OUT_DRQ_NORM;
    if (buffer_mask & (1ull << RS_BUF_DRQ_NORM_F16)) m |= OUT_DRQ_F16;
    if (buffer_mask & (1ull << RS_BUF_LANE_ARRIVALS)) m |= OUT_LANE_ARR;
    if (buffer_mask & (1ull << RS_BUF_MPLIGHT)) m |= OUT_MPLIGHT;
    if (buffer_mask & (1ull << RS_BUF_WAVE)) m |= OUT_WAVE;
    if (buffer_mask & (1ull << RS_BUF_MPLIGHT_FULL)) m |= OUT_MPLIGHT_FULL;
    if (buffer_mask & (1ull << RS_BUF_VEH_ACCEL)) m |= OUT_VEH_ACCEL;
    return m;
}

// ---- the RS_BUF_* buffers: X(id, pointer, dtype, ndim, shape[0..3]) over G (State), O (Out), `actions` and the dimensions of BufDims
struct Buf { void *ptr; int64_t shape[4]; int ndim; int dtype; size_t bytes; };
struct BufDims { int64_t n, c, s, o, lmax, n_dep, n_trips; };      // envs, capacity, signals, observed lanes, .., trips (0: no trip log)
static const size_t kDtypeSize[] = {4, 4, 2, 1, 2, 8, 4};
#define RS_BUF_TABLE(X)                                                                                                               \
    X(LANE_AGG, O.lane_agg(), F32, 3, n, o, 5, 1)           X(DRQ_NORM, O.drq_norm(), F32, 3, n, o, 5, 1)                             \
    X(PHASE, O.phase(), I32, 2, n, s, 1, 1)                 X(MPLIGHT, O.mplight(), I32, 3, n, s, 13, 1)                              \
    X(WAVE, O.wave(), I32, 3, n, s, 12, 1)                  X(WAIT, O.wait(), F32, 2, n, s, 1, 1)                                     \
    X(WAIT_NORM, O.wait_norm(), F32, 2, n, s, 1, 1)         X(PRESSURE, O.pressure(), I32, 2, n, s, 1, 1)                             \
    X(QUEUE_SUM, O.queue_sum(), I32, 2, n, s, 1, 1)         X(QUEUE_MAX, O.queue_max(), I32, 2, n, s, 1, 1)                           \
    X(ACTIONS, actions, I32, 2, n, s, 1, 1)                 X(ENV, G.env, I32, 2, n, 4, 1, 1)                                         \
    X(TLS, G.tls, I32, 3, n, s, TLS_W, 1)                                                                                             \
    X(VEH_POS, G.pos(), F32, 2, n, c, 1, 1)                 X(VEH_SPEED, G.speed(), F32, 2, n, c, 1, 1)                               \
    X(VEH_ACCEL, G.accel(), F32, 2, n, c, 1, 1)             X(VEH_TLOSS, G.tloss(), F32, 2, n, c, 1, 1)                               \
    X(VEH_LANE, G.lane(), U16, 2, n, c, 1, 1)               X(VEH_TRIP, G.trip(), U16, 2, n, c, 1, 1)                                 \
    X(VEH_CURSOR, G.cursor(), U16, 2, n, c, 1, 1)           X(VEH_SWAIT, G.swait(), U16, 2, n, c, 1, 1)                               \
    X(VEH_RWAIT, G.rwait(), U16, 2, n, c, 1, 1)             X(VEH_DEPART, G.depart(), U16, 2, n, c, 1, 1)                             \
    X(VEH_OWNER, G.owner(), U8, 2, n, c, 1, 1)              X(STATS, G.stats, I64, 2, n, ST_N, 1, 1)                                  \
    X(DRQ_NORM_F16, O.drq_f16(), F16, 4, n, s, lmax, 5)     X(VEH_SF, G.sf(), F32, 2, n, c, 1, 1)                                     \
    X(VEH_WTOT, G.wtot(), U16, 2, n, c, 1, 1)               X(TRIP_LOG, G.trip_log, I32, 3, n, n_trips, 4, 1)                         \
    X(DEP_NEXT, G.dep_next, U16, 2, n, n_dep, 1, 1)                                                                                   \
    X(VEH_COOP, G.coop(0), U32, 2, n, c, 1, 1)              X(VEH_COOPLEAD, G.cooplead(0), U32, 2, n, c, 1, 1)                        \
    X(ARRIVALS, O.arrivals(), I32, 2, n, s, 1, 1)           X(DEPARTURES, O.departures(), I32, 2, n, s, 1, 1)                         \
    X(MPLIGHT_FULL, O.mplight_full(), F32, 3, n, s, 49, 1)  X(LANE_ARRIVALS, O.lane_arr(), I32, 2, n, o, 1, 1)                        \
    X(VEH_COOP_ODD, G.coop(1), U32, 2, n, c, 1, 1)          X(VEH_COOPLEAD_ODD, G.cooplead(1), U32, 2, n, c, 1, 1)                    \
    X(VEH_MAIL, G.mail, U32, 2, n, (c + 31) / 32, 1, 1)
#define RS_BUF_BIT(id, ptr, dt, nd, a, b, c_, d) | (1ull << RS_BUF_##id)
static_assert((0ull RS_BUF_TABLE(RS_BUF_BIT)) == (1ull << RS_BUF_COUNT) - 1, "RS_BUF_TABLE must describe every buffer id below RS_BUF_COUNT");
#undef RS_BUF_BIT
#define RS_BUF_ONE(id, ptr, dt, nd, a, b, c_, d) + 1
static_assert((0 RS_BUF_TABLE(RS_BUF_ONE)) == RS_BUF_COUNT, "RS_BUF_TABLE must describe every buffer id once");
#undef RS_BUF_ONE
static inline void rs_fill_bufs(Buf *bufs, const State &G, const Out &O, int32_t *actions, const BufDims &D) {
    const int64_t n = D.n, c = D.c, s = D.s, o = D.o, lmax = D.lmax, n_dep = D.n_dep, n_trips = D.n_trips;
#define RS_BUF_SET(id, ptr_, dt, nd, a, b, c_, d)                                                                  \
    { Buf &B = bufs[RS_BUF_##id];                                                                                  \
      B.ptr = (void *)(ptr_); B.dtype = RS_##dt; B.ndim = nd;                                                      \
      B.shape[0] = (a); B.shape[1] = (b); B.shape[2] = (c_); B.shape[3] = (d);                                     \
      B.bytes = (size_t)(B.shape[0] * B.shape[1] * B.shape[2] * B.shape[3]) * kDtypeSize[RS_##dt]; }
    RS_BUF_TABLE(RS_BUF_SET)
#undef RS_BUF_SET
}
// the bodies of rs_get_buffer and of rs_info behind the argument checks
static inline void rs_buf_describe(const Buf &B, void **ptr, int64_t shape[4], int32_t *ndim, int32_t *dtype) {
    if (ptr) *ptr = B.ptr;
    if (shape) for (int i = 0; i < 4; ++i) shape[i] = B.shape[i];
    if (ndim) *ndim = B.ndim;
    if (dtype) *dtype = B.dtype;
}
static inline void rs_info_describe(int n_envs_, int block_, size_t lds_, int lmax_, int32_t *n_envs, int32_t *block_threads, int32_t *lds_bytes,
                                    int32_t *max_lanes_per_signal) {
    if (n_envs) *n_envs = n_envs_;
    if (block_threads) *block_threads = block_;
    if (lds_bytes) *lds_bytes = (int32_t)lds_;
    if (max_lanes_per_signal) *max_lanes_per_signal = lmax_;
}

// ---- scenario -> tables
// The packed tables with the grid cell length of this scenario: build once to learn the sizes that do not depend on it, choose, build
// for good.  Returns the error text, or NULL.
static inline const char *rs_pack_tables(PackedTables &PT, const rs_scenario *sc) {
    PackedTables probe;
    if (!probe.build(sc)) { PT.err = probe.err; return PT.err.c_str(); }
    if (!PT.build(sc, pick_cell_len(sc, probe.n_arr, probe.n_dep, probe.tls_maxl))) return PT.err.c_str();
    return nullptr;
}
// the table members of KTab K: X(member, element type, source on the host, element count) -- the library uploads each, the
// emulation keeps a host copy
#define RS_KTAB_TABLES(X, K, PT, sc)                                                                                                  \
    X(K.lanes_, LaneRec, PT.lanes.data(), PT.lanes.size()) X(K.links_, LinkRec, PT.links.data(), PT.links.size())                     \
    X(K.foes_, FoeRec, PT.foes.data(), PT.foes.size()) X(K.rsteps_, RStep, PT.rsteps.data(), PT.rsteps.size())                        \
    X(K.routes_, RouteRec, PT.routes.data(), PT.routes.size()) X(K.next_link_, uint16_t, PT.next_link.data(), PT.next_link.size())    \
    X(K.trip_route_, uint16_t, PT.trip_route.data(), PT.trip_route.size()) X(K.trip_vtype_, uint8_t, PT.trip_vtype.data(), PT.trip_vtype.size()) \
    X(K.route_cont_, float, PT.route_cont.data(), PT.route_cont.size()) X(K.notbest_, uint16_t, PT.notbest.data(), PT.notbest.size()) \
    X(K.cold.trip_depart, int32_t, sc->trip_depart, sc->n_trips) X(K.cold.trip_next, uint16_t, PT.trip_next.data(), PT.trip_next.size()) \
    X(K.cold.dep_lane, uint16_t, PT.dep_lane.data(), PT.dep_lane.size()) X(K.cold.dep_info, DepInfo, PT.dep_info.data(), PT.dep_info.size()) \
    X(K.cold.dep_first, uint16_t, PT.dep_first.data(), PT.dep_first.size())                                                           \
    X(K.cold.vtype_params, float, sc->vtype_params, sc->n_vtypes * VT_COLS)                                                           \
    X(K.cold.tls8, uint8_t, PT.tls8.data(), PT.tls8.size()) X(K.cold.fix8, uint8_t, PT.fix8.data(), PT.fix8.size())                   \
    X(K.cold.tls_nphase, int32_t, sc->tls_nphase, sc->n_signals) X(K.cold.tls_ngreen, int32_t, sc->tls_ngreen, sc->n_signals)         \
    X(K.cold.tls_nlinks, int32_t, sc->tls_nlinks, sc->n_signals) X(K.cold.tls_state_off, int32_t, PT.tls_off_p.data(), sc->n_signals) \
    X(K.cold.tls_dur_off, int32_t, sc->tls_dur_off, sc->n_signals) X(K.cold.tls_yel_off, int32_t, sc->tls_yel_off, sc->n_signals)     \
    X(K.cold.tls_dur, int32_t, sc->tls_dur, sc->n_tls_dur) X(K.cold.tls_yellow, int32_t, sc->tls_yellow, sc->n_tls_yellow)            \
    X(K.cold.tls_init_phase, int32_t, sc->tls_init_phase, sc->n_signals)                                                              \
    X(K.cold.fix_nphase, int32_t, sc->fix_nphase, sc->n_signals) X(K.cold.fix_state_off, int32_t, PT.fix_off_p.data(), sc->n_signals) \
    X(K.cold.fix_dur_off, int32_t, sc->fix_dur_off, sc->n_signals) X(K.cold.fix_dur, int32_t, sc->fix_dur, sc->n_fix_dur)             \
    X(K.cold.fix_init_phase, int32_t, sc->fix_init_phase, sc->n_signals) X(K.cold.fix_init_left, int32_t, sc->fix_init_left, sc->n_signals) \
    X(K.cold.lane_obs, int16_t, PT.lane_obs16.data(), PT.lane_obs16.size()) X(K.cold.obs_sig, int32_t, PT.obs_sig.data(), PT.obs_sig.size()) \
    X(K.cold.sig_obs_start, int32_t, sc->sig_obs_start, sc->n_signals + 1)                                                            \
    X(K.cold.mv_in_start, int32_t, sc->mv_in_start, sc->n_signals * 12 + 1) X(K.cold.mv_in_idx, int32_t, sc->mv_in_idx, sc->n_mv_in)  \
    X(K.cold.mv_out_start, int32_t, sc->mv_out_start, sc->n_signals * 12 + 1) X(K.cold.mv_out_idx, int32_t, sc->mv_out_idx, sc->n_mv_out) \
    X(K.cold.pr_out_start, int32_t, sc->pr_out_start, sc->n_signals + 1) X(K.cold.pr_out_idx, int32_t, sc->pr_out_idx, sc->n_pr_out)  \
    X(K.cold.trips_cum, int32_t, sc->trips_cum, sc->horizon + 2)
// rs_params.step_ratio: simulation ticks per step_sim() call
static inline int rs_step_ratio(const rs_params *p) { return p->step_ratio > 1 ? p->step_ratio : 1; }
// the scalar members of KTab
static inline void rs_ktab_scalars(KTab &K, const PackedTables &PT, const rs_scenario *sc, int ratio) {
    K.maxlen = PT.maxlen; K.occ_unit = PT.occ_unit;
    K.n_trips = sc->n_trips; K.tls_maxl = PT.tls_maxl; K.kmax = sc->kmax;
    K.n_lanes = sc->n_lanes; K.n_cells = PT.n_cells; K.n_signals = sc->n_signals; K.n_obs = sc->n_obs; K.n_vtypes = sc->n_vtypes;
    // the kernel counts ticks: Signal.set_phase comes after yellow_length x step_ratio of them (multi_signal.py:102-105, 175-180);
    // step_length stays what Signal.observe adds to a waiting time (traffic_signal.py:196)
    K.horizon = sc->horizon; K.capacity = sc->capacity; K.step_length = sc->step_length; K.yellow_length = sc->yellow_length * ratio; K.lmax = PT.lmax;
    K.n_arr = PT.n_arr; K.n_dep = PT.n_dep;
}
// ---- scenario -> the constants of a handle (resco_step.h: ScnConsts).  No device is touched: rs_create computes them this way, and so
// does the build, ahead of the HIP compile, for the literals of the per-map step kernels (resco_scn_consts.cpp).
// From the packed tables of the scenario; `L` (optional) receives the layout of the working memory they describe.  The budget is the
// one of the default workgroup shape: rs_create puts in what its block_threads argument selects.
static inline void rs_scn_consts_from(const PackedTables &PT, const rs_scenario *sc, int ratio, ScnConsts *c, Lds *L = nullptr) {
    KTab K{};
    rs_ktab_scalars(K, PT, sc, ratio);
    Lds l{};
    const size_t bytes = lds_carve(&l, sc->capacity, K.n_cells, K.n_arr, K.n_dep, sc->n_obs, sc->n_signals, sc->n_vtypes, K.tls_maxl);
    l.cell_inv = PT.cell_inv;
#define X(n) c->n = K.n;
    RS_SCN_KTAB(X)
#undef X
#define X(n) memcpy(&c->n##_bits, &K.n, 4);
    RS_SCN_KTAB_F(X)
#undef X
    scn_consts_layout(c, l, bytes);
    c->budget = rs_default_budget(sc->capacity, bytes);
    if (L) *L = l;
}
// from the scenario itself (packs the tables first); false: the scenario exceeds a limit of the tables
static inline bool rs_scn_consts_of(const rs_scenario *sc, int ratio, ScnConsts *c) {
    PackedTables PT;
    if (rs_pack_tables(PT, sc)) return false;
    rs_scn_consts_from(PT, sc, ratio, c);
    return true;
}
// ---- demand variants (rs_set_demand): what a handle remembers of its scenario for them, and the check + packing of a call.  The library
// uploads what pack() builds and points KTab::dem_ / dem_env_ at it; the emulation keeps it in host memory.
struct DemandHost {
    std::vector<int16_t> route_dep;     // RouteRec::dep_idx of every route
    int n_trips = 0, n_dep = 1, n_vtypes = 0, horizon = 0, common_vt = 0;
    uint32_t generation = 0;            // bumped by every successful rs_set_demand; a snapshot records it
    int n_variants = 0;                 // in force (0: the scenario's own trips)
    std::vector<int32_t> env_variant;   // [n_envs] in force
    void init(const PackedTables &PT, const rs_scenario *sc) {
        route_dep = PT.route_dep; n_trips = sc->n_trips; n_dep = PT.n_dep; n_vtypes = sc->n_vtypes; horizon = sc->horizon; common_vt = PT.common_vt;
    }
    // Checks a call's arguments (n_variants > 0) -- everything a kernel will index with -- and builds the variants' tables (`arena`:
    // n_variants blocks in the layout of resco_tables.h: dem_off_*) and every environment's block offset.  Returns the refusal's text,
    // empty: fine.  Changes nothing of *this: the caller commits (n_variants, env_variant, generation) once its copies succeeded.
    std::string pack(int n_envs, int n_var, const rs_demand *variants, const int32_t *env_var, std::vector<char> &arena, std::vector<uint32_t> &env_off) const {
        char msg[192];
        if (!variants || !env_var) return "rs_set_demand: NULL variants / env_variant";
        const uint32_t stride = dem_stride(n_trips, n_dep, horizon);
        if ((uint64_t)stride * (uint64_t)n_var >= ((uint64_t)1 << 32)) return "rs_set_demand: the variants' tables exceed 4 GiB";
        for (int e = 0; e < n_envs; ++e)
            if (env_var[e] < 0 || env_var[e] >= n_var) {
                snprintf(msg, sizeof(msg), "rs_set_demand: env_variant[%d] = %d is outside 0 .. %d", e, env_var[e], n_var - 1); return msg;
            }
        for (int v = 0; v < n_var; ++v) {
            const rs_demand &V = variants[v];
            if (!V.trip_depart || !V.trip_route || !V.trip_vtype) { snprintf(msg, sizeof(msg), "rs_set_demand: variant %d has a NULL table", v); return msg; }
            for (int k = 0; k < n_trips; ++k) {
                const int dp = V.trip_depart[k];
                if (dp < 0 || dp > 65534 || (k > 0 && dp < V.trip_depart[k - 1])) {
                    snprintf(msg, sizeof(msg), "rs_set_demand: variant %d, trip %d: depart %d (departs must be non-decreasing in 0 .. 65534)", v, k, dp); return msg;
                }
                if (V.trip_route[k] < 0 || V.trip_route[k] >= (int)route_dep.size()) {
                    snprintf(msg, sizeof(msg), "rs_set_demand: variant %d, trip %d: route %d is outside 0 .. %d", v, k, V.trip_route[k], (int)route_dep.size() - 1); return msg;
                }
                if (V.trip_vtype[k] < 0 || V.trip_vtype[k] >= n_vtypes) {
                    snprintf(msg, sizeof(msg), "rs_set_demand: variant %d, trip %d: vehicle type %d is outside 0 .. %d", v, k, V.trip_vtype[k], n_vtypes - 1); return msg;
                }
            }
            const int cv = PackedTables::common_vtype(n_vtypes, n_trips, V.trip_vtype);
            if (cv != common_vt) {
                snprintf(msg, sizeof(msg), "rs_set_demand: variant %d: its most common vehicle type is %d, the scenario's is %d (the queue unit of the lane occupancy is a constant of the handle)", v, cv, common_vt);
                return msg;
            }
        }
        arena.assign((size_t)stride * (size_t)n_var, 0);
        for (int v = 0; v < n_var; ++v) {
            const rs_demand &V = variants[v];
            char *b = arena.data() + (size_t)stride * (size_t)v;
            int32_t *depart = (int32_t *)(b + dem_off_depart(n_trips, n_dep, horizon)), *cum = (int32_t *)(b + dem_off_cum(n_trips, n_dep, horizon));
            if (n_trips) memcpy(depart, V.trip_depart, (size_t)n_trips * 4);
            for (int t = 0, k = 0; t < horizon + 2; ++t) {      // trips_cum[t] = trips with depart <= t (scenario.py: compile_scenario)
                while (k < n_trips && V.trip_depart[k] <= t) ++k;
                cum[t] = k;
            }
            PackedTables::pack_trips(route_dep.data(), n_dep, n_trips, V.trip_route, V.trip_vtype, (uint16_t *)(b + dem_off_route(n_trips, n_dep, horizon)),
                                     (uint8_t *)(b + dem_off_vtype(n_trips, n_dep, horizon)), (uint16_t *)(b + dem_off_next(n_trips, n_dep, horizon)),
                                     (uint16_t *)(b + dem_off_first(n_trips, n_dep, horizon)));
        }
        env_off.resize((size_t)n_envs);
        for (int e = 0; e < n_envs; ++e) env_off[(size_t)e] = stride * (uint32_t)env_var[e];
        return std::string();
    }
    // the body of rs_demand_info behind the argument checks
    void describe(int32_t *n_var, int32_t *env_variant_out) const {
        if (n_var) *n_var = n_variants;
        if (env_variant_out && n_variants > 0) memcpy(env_variant_out, env_variant.data(), env_variant.size() * 4);
    }
};
// the parameters of a handle that every launch starts from (launch_step / run_step fill in the per-launch members)
static inline KParams rs_kparams(const rs_params *p, int32_t env_base, int32_t n_envs) {
    KParams P{};
    P.seed = p->seed; P.env_base = env_base; P.max_distance = p->max_distance; P.sigma = p->sigma;
    P.speed_dev = p->speed_dev; P.fixed_program = p->fixed_program; P.tls_expiry = p->tls_hold == 0; P.n_envs = n_envs;
    return P;
}
