// rs_emu_count.cpp -- the host emulation of the step kernel (tests/hostemu/rs_emu.cpp, included UNCHANGED) with the RS_COUNT hook of
// resco_step.h defined: every kind of thing the two long paths of the plan phase do -- the hop loop of phase_plan<true>, foe_blocked,
// phase_lc_decide -- bumps a counter, and rs_longpath_counts reads and resets them.  TEST INFRASTRUCTURE, never shipped.
//
// A run that equals the oracle bit for bit says nothing about a path it never took: tests/test_long_paths_cpu.py asks for every kind.
#include <stdint.h>

static long long g_rs_count[64];
#define RS_COUNT(id) { g_rs_count[id] += 1; }
#include "../hostemu/rs_emu.cpp"

static_assert(RC_COUNT <= 64, "g_rs_count holds 64 kinds");

extern "C" {
// copy the counters (RC_COUNT of them, in the order of resco_step.h's RsCount) into out[0 .. cap) and clear them; returns RC_COUNT
int rs_longpath_counts(long long *out, int cap) {
    for (int i = 0; i < RC_COUNT; ++i) {
        if (out && i < cap) out[i] = g_rs_count[i];
        g_rs_count[i] = 0;
    }
    return RC_COUNT;
}
}
