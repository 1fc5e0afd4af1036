"""Tests-only helpers of the multi-map MPLight update (resco_amd/csrc/resco_frap_multi.h), built on tests/frap_train_ref.py: the maps
of one shared network, the yardstick of a grouped minibatch, the Python restatement of the draw, and the host build
(tests/frap_multi_host).

The maps.  frap_train_ref.case(P, D, T, N, S, seed=1) draws the network and the target from the seed alone, so the cases of different
P at one D ARE the maps of one shared network (shared_weights asserts it), each kink-free under those weights.

The yardstick.  A grouped minibatch of B = sum B_m rows is the B_m-row minibatches of frap_train_ref.reference(P, D, T, N, S, B_m), one
per map; the mean loss over B rows and its gradient are the B_m / B weighted sums of the per-map ones, so
    truth  g64 = sum (B_m / B) g64_m
    e_ref      = max(sum (B_m / B) e_ref_m, one ulp32 of the tensor's largest |truth|)
(the project's per-tensor e_ref carried through the triangle inequality), the loss likewise; the device and the host build get 4 e_ref.
"""
import ctypes as C
import functools

import numpy as np

import frap_train_ref as ft
from resco_amd.sim import _murmur
from train_ref import build_host

MAPS_D1 = ((4, 6, 3, 1), (3, 5, 2, 2), (9, 4, 2, 3))        # (P, T, N, S)
MAPS_D4 = ((4, 6, 3, 1), (13, 4, 2, 3))
# (D, maps, counts): with tiles of ft.TILE_ROWS = 4 rows -- a map across a tile boundary, a ragged single tile and one whole tile;
# whole tiles only; the first and the last map empty; demand_shape 4 with the widest lane group
CASES = [(1, MAPS_D1, (5, 3, 4)), (1, MAPS_D1, (4, 4, 4)), (1, MAPS_D1, (0, 7, 0)), (4, MAPS_D4, (6, 2))]
MAX_MAPS = 8
# rings (T, N, S, head, count) per map, every one a state a ring can be in (count < T: head = count): full rings whose head lies
# anywhere (the oldest slot wraps), a ring without a transition (count 1), one with a single slot to draw, an unwritten one
RING_SETS = [[(6, 3, 1, 2, 6), (5, 2, 2, 0, 5), (4, 2, 3, 3, 4)],
             [(6, 3, 1, 1, 6), (5, 2, 2, 1, 1), (4, 2, 3, 2, 2)],
             [(7, 4, 2, 0, 0), (9, 5, 3, 3, 9)],
             [(8, 11, 4, 7, 7)]]


def map_cases(D, maps):
    return [ft.case(P, D, T, N, S) for P, T, N, S in maps]


def shared_weights(cases):
    """the maps' networks and targets hold the same tensors -> (net, target) of map 0"""
    for c in cases[1:]:
        for a, b in ((cases[0]['net'], c['net']), (cases[0]['target'], c['target'])):
            sa, sb = a.state_dict(), b.state_dict()
            assert list(sa) == list(sb) and all(np.array_equal(sa[k].numpy(), sb[k].numpy()) for k in sa), 'the cases do not share one network'
    return cases[0]['net'], cases[0]['target']


@functools.lru_cache(maxsize=None)
def reference(D, maps, counts):
    """(idx int32 [B, 4] grouped by map, truth gradients, e_ref per tensor, truth loss, e_ref of the loss): computed once, shared,
    never changed"""
    B = sum(counts)
    idx, g64, e_ref, l64, e_loss = [], None, None, 0.0, 0.0
    for m, ((P, T, N, S), Bm) in enumerate(zip(maps, counts)):
        if Bm == 0:
            continue
        i_m, g_m, e_m, l_m, el_m = ft.reference(P, D, T, N, S, Bm)[:5]
        idx.append(np.concatenate((np.full((Bm, 1), m, np.int32), i_m), -1))
        w = Bm / B
        g64 = {k: w * v for k, v in g_m.items()} if g64 is None else {k: g64[k] + w * v for k, v in g_m.items()}
        e_ref = {k: w * v for k, v in e_m.items()} if e_ref is None else {k: e_ref[k] + w * v for k, v in e_m.items()}
        l64, e_loss = l64 + w * l_m, e_loss + w * el_m
    e_ref = {k: max(v, float(ft.ulp32(np.abs(g64[k]).max()))) for k, v in e_ref.items()}
    return np.concatenate(idx).astype(np.int32), g64, e_ref, l64, max(e_loss, float(ft.ulp32(l64)))


# ---- the draw
def pools_of(rings):
    """rings: (T, N, S, head, count) per map -> cumulative pools [n_maps + 1]"""
    cum = [0]
    for T, N, S, head, count in rings:
        cum.append(cum[-1] + (max(count - 1, 0) * N * S if count >= 2 else 0))
    return cum


def predict_sample(seed, u, rings, B):
    """rs_mplight_multi_sample restated from its rule: -> (idx int32 [B, 4] = (map, t, e, s) grouped by map, maps ascending, the draw
    order kept inside a map; counts [n_maps])"""
    cum = pools_of(rings)
    total = cum[-1]
    assert total > 0
    sd = (seed ^ ft.FRAP_TRAIN_SALT) & 0xFFFFFFFF
    groups = [[] for _ in rings]
    for i in range(B):
        r = ((_murmur(sd, (u, i, 0, 3)) << 32) | _murmur(sd, (u, i, 0, 4))) % total
        m = next(k for k in range(len(rings)) if r < cum[k + 1])
        T, N, S, head, count = rings[m]
        rp = r - cum[m]
        s, e, k = rp % S, (rp // S) % N, rp // (S * N)
        groups[m].append((m, (head - count + T + k) % T, e, s))
    idx = np.array([row for g in groups for row in g], np.int32).reshape(B, 4)
    return idx, [len(g) for g in groups]


def check_grouped(idx, counts, rings):
    """what every grouped minibatch must satisfy: the tags ascending with the stated group sizes, every group a valid draw of its ring"""
    assert len(idx) == sum(counts) and list(idx[:, 0]) == [m for m, c in enumerate(counts) for _ in range(c)]
    for m, (T, N, S, head, count) in enumerate(rings):
        rows = idx[idx[:, 0] == m][:, 1:]
        if count < 2:
            assert len(rows) == 0, 'a ring without a transition was drawn'
        elif len(rows):
            ft.check_sample(rows, T, N, S, head, count)


def build_frap_multi_host(out_dir):
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    return build_host('frap_multi', out_dir, dict(frap_multi_grad=[vp, vp, i32, i32] + [vp] * 11 + [C.c_double, vp, vp],
                                                  frap_multi_sample=[u32, u32, i32, vp, vp, vp, vp, vp, i32, vp, vp],
                                                  frap_multi_hash_of=([u32] * 5, u32), frap_multi_d_hash_of=([u32] * 5, u32),
                                                  frap_multi_max_maps=[]))


def host_sample(host, seed, u, rings, B):
    cols = [np.ascontiguousarray([r[k] for r in rings], np.int32) for k in range(5)]
    idx, counts = np.full((B, 4), -9, np.int32), np.full(len(rings), -9, np.int32)
    rc = host.frap_multi_sample(seed, u, len(rings), *[c.ctypes.data for c in cols], B, idx.ctypes.data, counts.ctypes.data)
    return rc, idx, counts.tolist()


def host_grads(host, cases, idx, counts):
    """frap_multi_grad on the maps' rings -> (dict name -> float32 gradient, float32 loss)"""
    from resco_amd.agents.mplight import pack_mplight_weights
    net, target = shared_weights(cases)
    w, wt = (np.ascontiguousarray(pack_mplight_weights(n).numpy(), np.float32) for n in (net, target))
    keep = [[np.ascontiguousarray(c['obs'], np.float32), np.ascontiguousarray(c['act'], np.int16), np.ascontiguousarray(c['rew'], np.float32),
             np.ascontiguousarray(c['done'], np.uint8), np.ascontiguousarray(c['pairs'], np.int32)] for c in cases]
    ptrs = lambda k: (C.c_void_p * len(cases))(*[a[k].ctypes.data for a in keep])
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    P, T, N, S = (ints([c[k] if k == 'P' else c['obs'].shape[i] for c in cases]) for k, i in (('P', 0), ('T', 0), ('N', 1), ('S', 2)))
    idx, cnt = np.ascontiguousarray(idx, np.int32), ints(counts)
    grad, loss = np.full(len(w), np.nan, np.float32), np.full(1, np.nan, np.float32)
    p = lambda a: a.ctypes.data
    rc = host.frap_multi_grad(p(w), p(wt), cases[0]['D'], len(cases), p(P), ptrs(4), ptrs(0), ptrs(1), ptrs(2), ptrs(3), p(T), p(N), p(S), p(idx), p(cnt),
                              ft.GAMMA, p(grad), p(loss))
    assert rc == 0
    return ft.unpack(grad, net), float(loss[0])
