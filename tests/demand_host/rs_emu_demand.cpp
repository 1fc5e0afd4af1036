// rs_emu_demand.cpp -- the host emulation of the step kernel (tests/hostemu/rs_emu.cpp, included UNCHANGED) plus the per-environment
// demand of include/resco_sim.h: rs_set_demand / rs_demand_info on that file's rs_sim.  TEST INFRASTRUCTURE, never shipped.
//
// The check and the packing of a call are the library's (resco_host.h: DemandHost::pack), the selection of an environment's tables is the
// kernel source's (resco_step.h: Demand, resco_host.h: rs_reset_env): this file only keeps the tables in host memory and points the
// emulation's KTab at them.  What a handle has to remember of its scenario lives beside the handle, keyed by it: rs_create, rs_destroy
// and the snapshot calls of rs_emu.cpp are taken under other names and wrapped.
#include "resco_sim.h"

#define rs_create rs_emu_create
#define rs_destroy rs_emu_destroy
#define rs_snapshot rs_emu_snapshot
#define rs_restore rs_emu_restore
#define rs_snapshot_free rs_emu_snapshot_free
#include "../hostemu/rs_emu.cpp"
#undef rs_create
#undef rs_destroy
#undef rs_snapshot
#undef rs_restore
#undef rs_snapshot_free

#include <map>

struct DemState {
    DemandHost dem;
    std::vector<char> arena;            // the variants' tables (K.dem_)
    std::vector<uint32_t> env_off;      // [n_envs] block offsets (K.dem_env_)
};
static std::map<rs_sim *, DemState> g_dem;
struct DemSnap { void *snap; uint32_t generation; };

extern "C" {
int rs_create(const rs_scenario *sc, const rs_params *p, int32_t n_envs, int32_t env_base, int32_t device_id, int32_t block_threads, rs_handle *out) {
    const int rc = rs_emu_create(sc, p, n_envs, env_base, device_id, block_threads, out);
    if (rc != RS_OK) return rc;
    PackedTables PT;
    if (const char *msg = rs_pack_tables(PT, sc)) { g_err = msg; rs_emu_destroy(*out); *out = nullptr; return RS_ELIMIT; }
    g_dem[*out].dem.init(PT, sc);
    return RS_OK;
}
void rs_destroy(rs_handle h) {
    if (!h) return;
    g_dem.erase(h);
    rs_emu_destroy(h);
}
int rs_set_demand(rs_handle h, int32_t n_variants, const rs_demand *variants, const int32_t *env_variant) {
    if (!h) return RS_EINVAL;
    if (n_variants < 0) { h->err = "rs_set_demand: n_variants < 0"; return RS_EINVAL; }
    DemState &D = g_dem[h];
    if (n_variants == 0 && D.dem.n_variants == 0) return RS_OK;        // (as the library: no new demand generation)
    std::vector<char> arena;
    std::vector<uint32_t> env_off;
    if (n_variants > 0) {
        const std::string msg = D.dem.pack(h->n_envs, n_variants, variants, env_variant, arena, env_off);
        if (!msg.empty()) { h->err = msg; return RS_EINVAL; }
    }
    D.arena.swap(arena); D.env_off.swap(env_off);
    h->K.dem_ = n_variants > 0 ? D.arena.data() : nullptr;
    h->K.dem_env_ = n_variants > 0 ? D.env_off.data() : nullptr;
    D.dem.n_variants = n_variants;
    if (n_variants > 0) D.dem.env_variant.assign(env_variant, env_variant + h->n_envs);
    else D.dem.env_variant.clear();
    D.dem.generation += 1;
    return RS_OK;
}
int rs_demand_info(rs_handle h, int32_t *n_variants, int32_t *env_variant_out) {
    if (!h) return RS_EINVAL;
    g_dem[h].dem.describe(n_variants, env_variant_out);
    return RS_OK;
}
int rs_snapshot(rs_handle h, void **snap) {
    if (!h || !snap) return RS_EINVAL;
    void *base = nullptr;
    const int rc = rs_emu_snapshot(h, &base);
    if (rc != RS_OK) return rc;
    *snap = new DemSnap{base, g_dem[h].dem.generation};
    return RS_OK;
}
int rs_restore(rs_handle h, const void *snap) {
    if (!h || !snap) return RS_EINVAL;
    const DemSnap *S = (const DemSnap *)snap;
    if (S->generation != g_dem[h].dem.generation) { h->err = "rs_restore: the snapshot was taken under another demand set (rs_set_demand since)"; return RS_EINVAL; }
    return rs_emu_restore(h, S->snap);
}
void rs_snapshot_free(rs_handle h, void *snap) {
    if (!snap) return;
    DemSnap *S = (DemSnap *)snap;
    rs_emu_snapshot_free(h, S->snap);
    delete S;
}
}
