// resco_frap_multi.h -- MPLight's ONE shared FRAP network trained on several maps at once: the DQN update of resco_frap_train.h over
// M replay rings, one per map (rs_mplight_multi_create / _sample / _grad / _step / _update of include/resco_sim.h).
//
// Why it is cheap: FRAP's parameter vector (1365 + 4 D floats) does not depend on a map's signal count, lane counts or number of phase
// pairs P; the network sees a map only through pairs [P][2] and the 12 movement demands of a row.  The tile of resco_frap_train.h reads
// its rows in its first lines and is map-independent after that except for P and pairs, which are run-time values already.  So a
// minibatch may hold rows of several maps as long as a TILE holds rows of one map: P stays workgroup-uniform, the phases (fpt_*), the
// entries (frap_tile_entry), the reduction with its chains (frap_grad_element) and the Adam element are the ones of
// resco_frap_train.h, called, not restated (as this file's own instantiations, FPM_TAG: the single-map kernels' code stays what it was).  What is new here: the draw over several rings, the grouping of the draws by map, and a
// tile kernel that finds its map in a small prefix table in its arguments.
//
// The draw (frap_multi_draw, frap_multi_map_of, frap_multi_row): uniform over ALL stored transitions of all maps that have a
// successor -- what one replay buffer shared by the maps would give.  pool_m = (count_m - 1) N_m S_m (0 where count_m < 2), total =
// the sum; r = ((uint64) hash(seed ^ FRAP_TRAIN_SALT, u, i, 0, 3) << 32 | hash(.., 4)) % total; map m = the first with r < pool_0 + ..
// + pool_m, r' = r - the pools before it; s = r' % S_m, e = (r' / S_m) % N_m, k = r' / (S_m N_m), t = (head_m - count_m + T_m + k) %
// T_m.  (hash % n: with total below 2^34 the bias of a 64-bit value is under 2^-30 relative, accepted as in frap_dqn_sample_index.)
// The rows leave the sampler GROUPED by map, maps ascending, the draw order kept inside a map (stable): idx [B][4] = (map, t, e, s).
// Every input of the draw is passed by value, so the host computes the group sizes from the same hash (frap_multi_counts) without
// asking the device: they size the tile launch and are what the caller gets as counts_out.
//
// Launches of one update: frap_multi_sample_kernel (ONE workgroup: the stable rank of a draw inside its map is a count over the
// draws before it, taken in LDS, 256 draws at a time), frap_multi_tile_kernel (one workgroup per tile; map m owns tiles tile0_m ..
// tile0_m + ceil(count_m / FPT_TM) - 1 and rows row0_m .. row0_m + count_m - 1 of idx; a map's last tile may be ragged: its missing
// rows are the ok = 0 rows of the stage and add exact zeros), frap_multi_reduce_kernel (frap_dqn_reduce_kernel with the tile count
// given: it is no longer ceil(B / FPT_TM)), frap_dqn_adam_kernel.  Four launches whatever the number of maps.
//
// The map tag idx[i][0] is NOT read by the gradient: a row's map is its group's, known to the host, so no table is indexed by a
// device value the host never saw.  t, e, s are held inside the map's ring whatever idx says, as in frap_dqn_tile_kernel.
// The loss is the mean over all B rows (fpt_row_loss divides by B, not by the group size); the target's max runs over all P_m outputs
// of the row's own map.  With one map the tiles, their order and every operation are those of rs_mplight_dqn_grad: the same bits.
// Every sum has one order fixed by (count_0, .., count_M-1) alone; no floating-point atomics.
//
// The hash: resco_step.h's d_hash is a device function, and the group sizes are needed on the host, so frap_multi_hash restates the
// project's counter hash as a host-and-device function; tests/frap_multi_host holds it against d_hash word for word and the GPU
// sampler test against resco_amd/sim.py's.
// Needs resco_frap.h and resco_frap_train.h before it.
#pragma once
#include "resco_frap_train.h"

#define FPM_MAPS 8                      // the most maps of one learner (the prefix table lives in the kernel arguments)
#define FPM_CHUNK 256                   // draws the sampler ranks at a time
#define FPM_TAG 1                       // these kernels' own instantiations of the phases of resco_frap_train.h (the TAG there)

RS_HD inline uint32_t frap_multi_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
RS_HD inline uint32_t frap_multi_hash(uint32_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    uint32_t h = seed;
    const uint32_t w[4] = {a, b, c, d};
    for (int i = 0; i < 4; ++i) {
        uint32_t k = w[i];
        k *= 0xcc9e2d51u; k = frap_multi_rotl(k, 15); k *= 0x1b873593u;
        h ^= k; h = frap_multi_rotl(h, 13); h = h * 5u + 0xe6546b64u;
    }
    h ^= 16u;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// the rings' positions and the pools, by value: what a draw depends on
struct FrapMultiPools {
    uint64_t cum[FPM_MAPS + 1];         // cum[m] = pool_0 + .. + pool_(m-1); cum[n_maps] = total
    int32_t T[FPM_MAPS], N[FPM_MAPS], S[FPM_MAPS], head[FPM_MAPS], count[FPM_MAPS];
    int32_t base[FPM_MAPS];             // the first row of map m's group in idx (the sampler's kernel alone reads it)
    int32_t n_maps;
};
// pool_m; needs the ring checked (capacity >= 2, 1 <= n_envs, 1 <= n_signals, 0 <= count <= capacity).  Below 2^63 for any int32 sizes
RS_HD inline uint64_t frap_multi_pool(int N, int S, int count) { return count < 2 ? 0u : (uint64_t)(count - 1) * (uint64_t)N * (uint64_t)S; }
// draw i of update u: r in 0 .. total - 1 (total >= 1)
RS_HD inline uint64_t frap_multi_draw(uint32_t seed, uint32_t u, uint32_t i, uint64_t total) {
    const uint32_t hi = frap_multi_hash(seed ^ FRAP_TRAIN_SALT, u, i, 0u, 3u), lo = frap_multi_hash(seed ^ FRAP_TRAIN_SALT, u, i, 0u, 4u);
    return (((uint64_t)hi << 32) | (uint64_t)lo) % total;
}
// the first map with r < cum[m + 1] (r < cum[n_maps]): a map whose pool is empty is never the first
RS_HD inline int frap_multi_map_of(const uint64_t *cum, int n_maps, uint64_t r) {
    int m = 0;
    while (m + 1 < n_maps && r >= cum[m + 1]) ++m;
    return m;
}
// r' < pool_m < 2^31 -> (t, e, s) of map m's ring
RS_HD inline void frap_multi_row(uint32_t rp, int T, int N, int S, int head, int count, int32_t *out) {
    const uint32_t s = rp % (uint32_t)S, q = rp / (uint32_t)S, e = q % (uint32_t)N, k = q / (uint32_t)N;
    out[0] = (int32_t)(((uint32_t)(head - count + T) + k) % (uint32_t)T);
    out[1] = (int32_t)e;
    out[2] = (int32_t)s;
}
// draw i whole: out = (map, t, e, s)
RS_HD inline void frap_multi_sample_index(uint32_t seed, uint32_t u, uint32_t i, const FrapMultiPools &Q, int32_t *out) {
    const uint64_t r = frap_multi_draw(seed, u, i, Q.cum[Q.n_maps]);
    const int m = frap_multi_map_of(Q.cum, Q.n_maps, r);
    out[0] = m;
    frap_multi_row((uint32_t)(r - Q.cum[m]), Q.T[m], Q.N[m], Q.S[m], Q.head[m], Q.count[m], out + 1);
}
// the group sizes of update u's B draws (the host's side of the sampler)
inline void frap_multi_counts(uint32_t seed, uint32_t u, int B, const FrapMultiPools &Q, int32_t *counts) {
    for (int m = 0; m < Q.n_maps; ++m) counts[m] = 0;
    for (int i = 0; i < B; ++i) counts[frap_multi_map_of(Q.cum, Q.n_maps, frap_multi_draw(seed, u, (uint32_t)i, Q.cum[Q.n_maps]))] += 1;
}

// one map of a minibatch: its ring, its pairs, and where its group lies
struct FrapMultiRing {
    const float *obs;                   // [T][N][S][W]
    const int16_t *act;                 // [T][N][S]
    const float *rew;                   // [T][N][S]
    const uint8_t *done;                // [T]
    const int32_t *pairs;               // device [P][2]
    int32_t T, N, S, W, P;
    int32_t tile0, row0, rows;          // the group's first tile, its first row of idx, its row count
    int32_t head;                       // the ring's next slot to write (the n-step walk of the option kernels stops before head - 1)
};
struct FrapMultiBatch {
    FrapMultiRing map[FPM_MAPS];
    const int32_t *idx;                 // [B][4]: (map, t, e, s), grouped by map
    int32_t n_maps, B, tiles;
};
// the prefix table from the group sizes -> the tile count
RS_HD inline int frap_multi_layout(FrapMultiBatch &D, const int32_t *counts) {
    int tile = 0, row = 0;
    for (int m = 0; m < D.n_maps; ++m) {
        D.map[m].tile0 = tile; D.map[m].row0 = row; D.map[m].rows = counts[m];
        tile += (counts[m] + FPT_TM - 1) / FPT_TM; row += counts[m];
    }
    D.B = row; D.tiles = tile;
    return tile;
}
// the map that owns tile b (b < D.tiles): the last whose first tile is not behind b -- a map without rows shares its first tile with
// the next one and is passed over
RS_HD inline int frap_multi_tile_map(const FrapMultiBatch &D, int b) {
    int m = 0;
    for (int k = 1; k < FPM_MAPS; ++k)
        if (k < D.n_maps && b >= D.map[k].tile0) m = k;
    return m;
}
// row r of tile b of map R into the stage (lane j of FPT_G reads its share of the observation; lane 0 the scalars): what the first
// lines of frap_dqn_tile_kernel do for one ring
RS_HD inline void frap_multi_load(FrapStage &L, const FrapMultiRing &R, const int32_t *idx, int b, int r, int j) {
    const int local = (b - R.tile0) * FPT_TM + r;
    const bool ok = local < R.rows;
    int t = 0, e = 0, s = 0;
    if (ok) {
        const int32_t *p = idx + (size_t)(R.row0 + local) * 4;      // (p[0], the map tag, is not read: the row's map is its group's)
        t = p[1] < 0 ? 0 : (p[1] >= R.T ? R.T - 1 : p[1]);
        e = p[2] < 0 ? 0 : (p[2] >= R.N ? R.N - 1 : p[2]);
        s = p[3] < 0 ? 0 : (p[3] >= R.S ? R.S - 1 : p[3]);
    }
    const bool boot = ok && !R.done[t];
    const size_t cur = ((size_t)t * R.N + e) * R.S + s, nxt = ((size_t)(t + 1 == R.T ? 0 : t + 1) * R.N + e) * R.S + s;
    for (int q = j; q < FPT_W; q += FPT_G) {
        L.obs[r][q] = ok && q < R.W ? R.obs[cur * R.W + q] : 0.0f;
        L.nxt[r][q] = boot && q < R.W ? R.obs[nxt * R.W + q] : 0.0f;
    }
    if (j == 0) {
        const int a = ok ? (int)R.act[cur] : 0;
        L.ok[r] = ok; L.boot[r] = boot;
        L.g[r] = a < 0 ? 0 : (a >= R.P ? R.P - 1 : a);
        L.rew[r] = ok ? R.rew[cur] : 0.0f;
    }
}

// the same row under the target's options (rs_mplight_maps_set_target): its own observation, its scalars and its walk
// (fpt_opt_load_row of resco_frap_train.h); the bootstrap row is loaded a barrier later (fpt_opt_load_next)
template <int TAG>
RS_HD inline void frap_multi_opt_load(FrapStage &L, FrapOptRows &O, const FrapMultiRing &R, const int32_t *idx, int b, int r, int j, int n_step, fpt_t gamma) {
    const int local = (b - R.tile0) * FPT_TM + r;
    const bool ok = local < R.rows;
    int t = 0, e = 0, s = 0;
    if (ok) {
        const int32_t *p = idx + (size_t)(R.row0 + local) * 4;
        t = p[1] < 0 ? 0 : (p[1] >= R.T ? R.T - 1 : p[1]);
        e = p[2] < 0 ? 0 : (p[2] >= R.N ? R.N - 1 : p[2]);
        s = p[3] < 0 ? 0 : (p[3] >= R.S ? R.S - 1 : p[3]);
    }
    fpt_opt_load_row<TAG>(L, O, R.obs, R.act, R.rew, R.done, R.T, R.N, R.S, R.W, R.P, R.head, ok, t, e, s, n_step, gamma, r, j);
}

#if defined(__HIPCC__)      // ------------------------------------------------------------------------------------------ the kernels
// ONE workgroup of FPM_CHUNK threads.  Draw i goes to row base[m] + (draws j < i of the same map): the draws of a chunk leave their map
// in LDS, a thread counts the entries before its own, and fill[m] carries the rows map m has taken in earlier chunks.
__global__ void __launch_bounds__(FPM_CHUNK) frap_multi_sample_kernel(uint32_t seed, uint32_t u, FrapMultiPools Q, int B, int32_t *idx) {
    __shared__ FrapMultiPools sQ;
    __shared__ int32_t fill[FPM_MAPS];
    __shared__ uint8_t mp[FPM_CHUNK];
    const int tid = threadIdx.x;
    if (tid == 0) sQ = Q;
    if (tid < FPM_MAPS) fill[tid] = tid < Q.n_maps ? Q.base[tid] : 0;
    __syncthreads();
    for (int c0 = 0; c0 < B; c0 += FPM_CHUNK) {
        const int i = c0 + tid;
        int32_t row[4] = {FPM_MAPS, 0, 0, 0};           // (FPM_MAPS: no map -- a thread past the last draw)
        if (i < B) frap_multi_sample_index(seed, u, (uint32_t)i, sQ, row);
        mp[tid] = (uint8_t)row[0];
        __syncthreads();
        if (i < B) {
            int rank = 0;
            for (int j = 0; j < tid; ++j) rank += mp[j] == (uint8_t)row[0];
            const int pos = fill[row[0]] + rank;
            if (pos >= 0 && pos < B) {                  // (always: the host's group sizes come from the same draws)
                int32_t *o = idx + (size_t)pos * 4;
                o[0] = row[0]; o[1] = row[1]; o[2] = row[2]; o[3] = row[3];
            }
        }
        __syncthreads();
        if (tid < Q.n_maps) {
            int n = 0;
            for (int j = 0; j < FPM_CHUNK; ++j) n += mp[j] == (uint8_t)tid;
            fill[tid] += n;
        }
        __syncthreads();
    }
}

// frap_dqn_tile_kernel over the groups: the workgroup's map from the prefix table, then the same phases with that map's P and pairs
__global__ void __launch_bounds__(FPT_T) frap_multi_tile_kernel(FrapTrainTab T, FrapMultiBatch D) {
    __shared__ FrapStage L;
    const int tid = threadIdx.x, r = tid / FPT_G, j = tid % FPT_G, b = blockIdx.x;
    const FrapMultiRing R = D.map[frap_multi_tile_map(D, b)];       // (workgroup-uniform: scalar loads from the argument table)
    const int P = R.P, Dm = T.D;
    const int32_t *pairs = R.pairs;
    const float *w = T.par, *wt = T.tgt;
    for (int k = tid; k < 144; k += FPT_T) fpt_prep<FPM_TAG>(L, T.par, T.tgt, Dm, k);
    frap_multi_load(L, R, D.idx, b, r, j);
    __syncthreads();
    fpt_target_ab<FPM_TAG>(L, wt, Dm, P, pairs, r, j);
    __syncthreads();
    fpt_target_q<FPM_TAG>(L, wt, Dm, P, pairs, r, j);
    __syncthreads();
    if (j == 0) fpt_target_value<FPM_TAG>(L, P, T.gamma, r);
    if (j < FRAP_MV) fpt_mv_forward<FPM_TAG>(L, w, Dm, P, pairs, r, j);
    __syncthreads();
    fpt_pair_forward<FPM_TAG>(L, w, Dm, P, pairs, r, j);
    __syncthreads();
    fpt_item_forward<FPM_TAG>(L, w, Dm, P, pairs, r, j);
    __syncthreads();
    if (j == 0) fpt_row_loss<FPM_TAG>(L, P, D.B, r);
    __syncthreads();
    fpt_item_backward<FPM_TAG>(L, w, Dm, P, r, j);
    __syncthreads();
    if (j == L.g[r]) fpt_row_backward<FPM_TAG>(L, w, Dm, P, r);
    __syncthreads();
    if (j < FRAP_MV) fpt_mv_backward<FPM_TAG>(L, w, Dm, P, pairs, r, j);
    __syncthreads();
    fpt_t *part = T.part + (size_t)b * FG_N;
    for (int e = tid; e < FG_N; e += FPT_T) part[e] = frap_tile_entry<FPM_TAG>(L, P, Dm, e);
}

// frap_dqn_tile_opt_kernel over the groups (launched only when an option is on; instantiations FPM_OPT_TAG + DOUBLE_Q)
#define FPM_OPT_TAG 4
template <bool DOUBLE_Q> __global__ void __launch_bounds__(FPT_T) frap_multi_tile_opt_kernel(FrapTrainTab T, FrapMultiBatch D, int n_step) {
    constexpr int TAG = FPM_OPT_TAG + (DOUBLE_Q ? 1 : 0);
    __shared__ FrapStage L;
    __shared__ FrapOptRows O;
    const int tid = threadIdx.x, r = tid / FPT_G, j = tid % FPT_G, b = blockIdx.x;
    const FrapMultiRing R = D.map[frap_multi_tile_map(D, b)];
    for (int k = tid; k < 144; k += FPT_T) fpt_prep<TAG>(L, T.par, T.tgt, T.D, k);
    frap_multi_opt_load<TAG>(L, O, R, D.idx, b, r, j, n_step, T.gamma);
    __syncthreads();
    frap_opt_tile_body<TAG, DOUBLE_Q>(L, O, T, R.obs, R.W, R.P, R.pairs, D.B, T.part + (size_t)b * FG_N, tid, r, j);
}

// frap_dqn_reduce_kernel with the tile count given
__global__ void __launch_bounds__(256) frap_multi_reduce_kernel(FrapTrainTab T, int tiles, int B, float *loss_out) {
    __shared__ fpt_t gPE[32], gR[2 * FRAP_C];
    const int tid = threadIdx.x;
    if (tid < 32) gPE[tid] = frap_reduce_entry(T.part, tiles, FG_PE + tid);
    else if (tid < 72) gR[tid - 32] = frap_reduce_entry(T.part, tiles, FG_DR + tid - 32);
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    if (i < T.n) T.grad[i] = frap_grad_element<FPM_TAG>(T.par, T.D, i, T.part, tiles, gPE, gR);
    if (loss_out && i == 0) *loss_out = frap_loss_mean<FPM_TAG>(T.part, tiles, B);
}
#endif
