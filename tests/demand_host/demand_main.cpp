// demand_main.cpp -- a program of its own around the host emulation with per-environment demand (rs_emu_demand.cpp), for the sanitizers:
// tests/test_demand_cpu.py builds it with -fsanitize=address,undefined and runs it.  It creates a handle from a scenario dump, sets
// the variants of the dump, runs env-steps, walks the refusals and the snapshot rule, and prints the trips every environment inserted.
//
// The dump (written by the test): int32 counts[23] (the scalars of rs_scenario in order); per pointer member of rs_scenario, in order,
// int64 bytes + the array; int32 n_envs, K; K x (trip_depart, trip_route, trip_vtype: int32 [n_trips] each); int32 env_variant[n_envs].
#include "rs_emu_demand.cpp"

#include <stddef.h>
#include <stdio.h>

static bool read_all(FILE *f, void *dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: demand_main DUMP STEPS\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror("demand_main"); return 2; }
    const int steps = atoi(argv[2]);
    rs_scenario sc;
    memset(&sc, 0, sizeof(sc));
    const size_t n_counts = offsetof(rs_scenario, lane_len) / 4, n_ptrs = (sizeof(rs_scenario) - offsetof(rs_scenario, lane_len)) / sizeof(void *);
    if (!read_all(f, &sc, n_counts * 4)) return 2;
    std::vector<std::vector<char>> arrays(n_ptrs);
    const void **pp = (const void **)((char *)&sc + offsetof(rs_scenario, lane_len));
    for (size_t i = 0; i < n_ptrs; ++i) {
        int64_t bytes = 0;
        if (!read_all(f, &bytes, 8) || bytes < 0) return 2;
        arrays[i].resize((size_t)bytes);                    // exactly sized: a read past a table's end is a heap overflow
        if (!read_all(f, arrays[i].data(), (size_t)bytes)) return 2;
        pp[i] = arrays[i].data();
    }
    int32_t n_envs = 0, K = 0;
    if (!read_all(f, &n_envs, 4) || !read_all(f, &K, 4) || n_envs < 1 || K < 1) return 2;
    std::vector<std::vector<int32_t>> tabs((size_t)K * 3, std::vector<int32_t>((size_t)sc.n_trips));
    for (auto &t : tabs) if (!read_all(f, t.data(), t.size() * 4)) return 2;
    std::vector<int32_t> env_variant((size_t)n_envs);
    if (!read_all(f, env_variant.data(), env_variant.size() * 4)) return 2;
    fclose(f);
    std::vector<rs_demand> variants((size_t)K);
    for (int k = 0; k < K; ++k) variants[k] = rs_demand{tabs[3 * k].data(), tabs[3 * k + 1].data(), tabs[3 * k + 2].data()};

    rs_params p;
    memset(&p, 0, sizeof(p));
    p.seed = 5; p.max_distance = 200.0f; p.sigma = -1.0f; p.speed_dev = 1; p.trip_log = 1;
    rs_handle h = nullptr;
    if (rs_create(&sc, &p, n_envs, 1, 2, 0, &h) != RS_OK) { fprintf(stderr, "rs_create: %s\n", rs_last_error(nullptr)); return 1; }
    void *snap = nullptr;
    if (rs_snapshot(h, &snap) != RS_OK) return 1;
    if (rs_set_demand(h, K, variants.data(), env_variant.data()) != RS_OK) { fprintf(stderr, "rs_set_demand: %s\n", rs_last_error(h)); return 1; }
    if (rs_restore(h, snap) != RS_EINVAL) { fprintf(stderr, "a snapshot of another demand set was restored\n"); return 1; }
    rs_snapshot_free(h, snap);
    // the refusals change nothing
    {
        std::vector<int32_t> bad = env_variant;
        bad[0] = K;
        if (rs_set_demand(h, K, variants.data(), bad.data()) != RS_EINVAL) return 1;
        std::vector<int32_t> route = tabs[1];
        if (sc.n_trips) route[(size_t)sc.n_trips / 2] = sc.n_routes;
        rs_demand v0 = variants[0];
        v0.trip_route = route.data();
        std::vector<rs_demand> bv = variants;
        bv[0] = v0;
        if (rs_set_demand(h, K, bv.data(), env_variant.data()) != RS_EINVAL) return 1;
        if (rs_set_demand(h, -1, nullptr, nullptr) != RS_EINVAL || rs_set_demand(h, K, nullptr, env_variant.data()) != RS_EINVAL) return 1;
    }
    int32_t k_now = -1;
    std::vector<int32_t> ev((size_t)n_envs, -1);
    if (rs_demand_info(h, &k_now, ev.data()) != RS_OK || k_now != K || ev != env_variant) { fprintf(stderr, "rs_demand_info differs\n"); return 1; }
    rs_reset(h, nullptr);
    std::vector<int32_t> acts((size_t)n_envs * sc.n_signals);
    uint32_t rng = 2463534242u;
    for (int s = 0; s < steps; ++s) {
        for (int e = 0; e < n_envs; ++e)
            for (int i = 0; i < sc.n_signals; ++i) { rng = rng * 1664525u + 1013904223u; acts[(size_t)e * sc.n_signals + i] = (int32_t)((rng >> 8) % (uint32_t)sc.tls_ngreen[i]); }
        rs_step(h, acts.data(), 0, nullptr);
    }
    std::vector<int64_t> st((size_t)n_envs * ST_N);
    rs_stats(h, st.data());
    printf("demand_main: inserted");
    for (int e = 0; e < n_envs; ++e) printf(" %lld", (long long)st[(size_t)e * ST_N + ST_INSERTED]);
    printf("\n");
    if (rs_set_demand(h, 0, nullptr, nullptr) != RS_OK) return 1;
    rs_reset(h, nullptr);
    rs_step(h, acts.data(), 0, nullptr);
    rs_destroy(h);
    return 0;
}
