// record_load_host.cpp -- the whole-record loads of the scenario tables (resco_amd/csrc/resco_tables.h: rec_load16, rec_load8,
// link_load) as the host sees them, as a program of its own: tests/test_record_load_cpu.py builds it with
// -fsanitize=address,undefined and runs it.  For every record type, arrays of EXACTLY 1, 2 and 3 records on the heap, filled with
// seeded random bytes: the helper's result must equal the struct copy byte for byte at every index, and must not read a byte
// outside the array -- the last record of an exactly sized array is where a 16-byte read of an 8-byte record, or a second half
// read behind a LinkRec, would show (the sanitizer's red zone begins right behind it).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "resco_tables.h"

static uint32_t g_rng = 0x9E3779B9u;
static uint8_t next_byte() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5;      // xorshift32
    return (uint8_t)(g_rng >> 11);
}

static int g_checked = 0, g_failed = 0;

template <class R, class Load> static void check(const char *name, Load load) {
    for (int n = 1; n <= 3; ++n) {
        R *tab = (R *)aligned_alloc(alignof(R), (size_t)n * sizeof(R));     // exactly n records: no slack behind the last one
        if (!tab || ((uintptr_t)tab % alignof(R)) != 0) { printf("%s: allocation failed\n", name); exit(2); }
        for (size_t b = 0; b < (size_t)n * sizeof(R); ++b) ((uint8_t *)tab)[b] = next_byte();
        for (int i = 0; i < n; ++i) {
            const R got = load(tab, i);
            const R want = tab[i];
            g_checked += 1;
            if (memcmp(&got, &want, sizeof(R)) != 0 || memcmp(&got, (const uint8_t *)tab + (size_t)i * sizeof(R), sizeof(R)) != 0) {
                printf("%s: record %d of %d differs from the struct copy\n", name, i, n);
                g_failed += 1;
            }
        }
        // the same through index types the kernel uses (uint16_t ids, size_t products)
        const R a = load(tab, (uint16_t)(n - 1)), b = load(tab, (size_t)(n - 1));
        if (memcmp(&a, &tab[n - 1], sizeof(R)) != 0 || memcmp(&b, &tab[n - 1], sizeof(R)) != 0) { printf("%s: index type\n", name); g_failed += 1; }
        free(tab);
    }
}

int main(int argc, char **argv) {
    if (argc > 1) g_rng = (uint32_t)strtoul(argv[1], nullptr, 0) | 1u;
    check<LaneRec>("LaneRec", [](const LaneRec *t, auto i) { return rec_load16(t, i); });
    check<FoeRec>("FoeRec", [](const FoeRec *t, auto i) { return rec_load16(t, i); });
    check<RouteRec>("RouteRec", [](const RouteRec *t, auto i) { return rec_load16(t, i); });
    check<LinkRec>("LinkRec", [](const LinkRec *t, auto i) { return link_load(t, i); });
    check<RStep>("RStep", [](const RStep *t, auto i) { return rec_load8(t, i); });
    check<DepInfo>("DepInfo", [](const DepInfo *t, auto i) { return rec_load8(t, i); });
#ifdef RECORD_LOAD_OVERREAD     // (the test's control: what the sanitizer must catch -- a 16-byte read of the last 8-byte record)
    {
        RStep *tab = (RStep *)aligned_alloc(alignof(RStep), sizeof(RStep));
        memset(tab, 1, sizeof(RStep));
        RecRaw16 r;
        __builtin_memcpy(&r, tab, 16);
        printf("overread %u\n", r.d);
        free(tab);
    }
#endif
#ifdef RS_FIELD_LOADS
    const char *mode = "field";
#else
    const char *mode = "whole";
#endif
    printf("record_load_host %s: %d records checked, %d failed\n", mode, g_checked, g_failed);
    return g_failed ? 1 : 0;
}
