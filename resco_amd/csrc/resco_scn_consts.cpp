// resco_scn_consts.cpp -- HOST ONLY: the constants of a handle (ScnConsts, resco_step.h) for a scenario, computed without a device.
// resco_amd/build.py compiles this file with g++ before the HIP compile, calls it for every shipped scenario and writes what it
// returns as literals into the generated header (resco_scn_fix.h) that the per-map step kernels are instantiated from.  It is the very
// code rs_create runs (resco_host.h: rs_scn_consts_of), so the literals of a map are what a handle of that map computes.
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <string>

#include "resco_sim.h"

// the layout half of resco_step.h needs no atomics and no working memory: qualifiers only
#define RS_DEV static inline
#define RS_HD
#define RS_MEM inline
#define RS_CARVE static inline
#define RS_SMEM ((char *)0)
#define RS_LAYOUT_ONLY
#include "resco_host.h"

extern "C" {
// the constants of a handle of `sc` with the default parameters (step_ratio 1) and the default workgroup shape; RS_OK or RS_ELIMIT
int rs_scn_consts(const rs_scenario *sc, ScnConsts *out) {
    if (!sc || !out) return RS_EINVAL;
    return rs_scn_consts_of(sc, 1, out) ? RS_OK : RS_ELIMIT;
}
// the members of ScnConsts (all 32 bits wide) in order, comma separated
const char *rs_scn_const_names(void) { return RS_SCN_NAMES; }
// where the constant argument block of the step kernels (resco_step.h: StepArgs) keeps what: "member:class:offset:bytes," -- class
// `const` (fixed for the handle: a scalar of the tables, a member of the working-memory layout), `pointer` or `state` (follows from the
// number of environments).  tools/isa_sloads.py names the scalar loads of a kernel's ISA with it.
const char *rs_step_args_layout(void) {
    static std::string s;
    if (!s.empty()) return s.c_str();
    auto add = [&](const char *name, const char *cls, size_t off, size_t bytes) {
        s += std::string(name) + ":" + cls + ":" + std::to_string(off) + ":" + std::to_string(bytes) + ",";
    };
    const size_t T = offsetof(StepArgs, T), G = offsetof(StepArgs, G), O = offsetof(StepArgs, O), L = offsetof(StepArgs, L), GP = offsetof(StepArgs, GP);
    add("T.tables", "pointer", T, offsetof(KTab, cold));
    add("T.cold", "pointer", T + offsetof(KTab, cold), sizeof(KCold));
#define X(n) add("T." #n, "const", T + offsetof(KTab, n), 4);
    RS_SCN_KTAB(X) RS_SCN_KTAB_F(X)
#undef X
    add("G.base", "pointer", G + offsetof(State, base), 8);
    add("G.nc", "state", G + offsetof(State, nc), 8);
    add("G.pointers", "pointer", G + offsetof(State, trip_log), sizeof(State) - offsetof(State, trip_log));
    add("O.base", "pointer", O + offsetof(Out, base), 8);
    add("O.dims", "state", O + offsetof(Out, n), 16);
#define X(n, tp) add("L." #n, "const", L + offsetof(Lds, n), 4);
    RS_SCN_LDS(X)
#undef X
    add("L.gstride", "const", L + offsetof(Lds, gstride), 4);
    add("L.lcap", "const", L + offsetof(Lds, lcap), 4);
    add("L.cell_inv", "const", L + offsetof(Lds, cell_inv), 4);
    add("GP", "pointer", GP, sizeof(StateP));
    return s.c_str();
}
}
