"""Tests-only float64 reference of MPLight's FRAP network, written in the reference's own formulation (agents/mplight.py:19-28, 72-130),
and what the tests of the fused kernel (rs_mplight_act, resco_amd/csrc/resco_frap.h) share: synthetic phase-pair sets for every pair
count 2..16, four classes of observation rows, the kernel's epilogue restated in Python, and the yardstick.

frap_ref is plain numpy in float64: per ordered pair (i, j) the concatenation [pair_i, pair_j] through lane_conv, the relation factor
from len(set(pair_i + pair_j)) == 3, the hidden layer, before_merge, the sum over j != i.  It neither splits lane_conv as the kernel
does nor calls resco_amd's FRAP.forward (fp32); tests/test_frap_ref_cpu.py holds it to the reference's own Q-values
(tests/golden/mplight_frap.npz).

The yardstick (the convention of tests/ppo_train_ref.py): truth = float64, e_ref = max |fp32 PyTorch FRAP on the CPU - truth| over a
class of rows; a candidate gets 4 e_ref + 2 ulp32(|truth|) per element (with fresh weights e_ref can fall below one fp32 spacing of Q).
"""
import types

import numpy as np
import torch

from resco_amd.agents.mplight import FRAP
from resco_amd.sim import _murmur

N_MOVEMENTS = 12
FRAP_SALT = 0x3F4A9E1B      # resco_frap.h
CLASSES = ('zero', 'small', 'wide', 'sat')
# the 0 < epsilon < 1 fixture of the kernel tests; tests/test_frap_ref_cpu.py checks from the hash alone that 20-55 % of its rows explore
EPS_CASE = dict(eps=0.37, seed=0x5EED1234, env_base=1000, step_key=0x9E3779B9)


def _sigmoid(z):
    """stable for |z| of several thousand: exp only of non-positive arguments"""
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _relu(x):
    return np.maximum(x, 0.0)


def frap_ref(state_dict, phase_pairs, D, obs):
    """Q [B, P] in float64.  state_dict: FRAP's parameters (tensors or arrays, the reference's names); obs: rows [B, 1 + 12 D] (any
    leading shape), column 0 the phase index (clamped to [0, P) where the reference would raise)."""
    w = {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, 'detach') else v, np.float64) for k, v in state_dict.items()}
    pairs = [[int(a), int(b)] for a, b in phase_pairs]
    P = len(pairs)
    obs = np.asarray(obs)
    rows = obs.reshape(-1, obs.shape[-1]).astype(np.float64)
    assert rows.shape[1] == 1 + N_MOVEMENTS * D
    B = rows.shape[0]
    ph = np.clip(np.trunc(rows[:, 0]).astype(np.int64), 0, P - 1)
    x = rows[:, 1:]
    p_w, d_w, d_b = w['p.weight'], w['d.weight'], w['d.bias']
    le_w, le_b = w['lane_embedding.weight'], w['lane_embedding.bias']
    lc_w, lc_b = w['lane_conv.weight'].reshape(20, 32), w['lane_conv.bias']
    re_w = w['relation_embedding.weight']
    rc_w, rc_b = w['relation_conv.weight'].reshape(20, 4), w['relation_conv.bias']
    h_w, h_b = w['hidden_layer.weight'].reshape(20, 20), w['hidden_layer.bias']
    bm_w, bm_b = w['before_merge.weight'].reshape(20), w['before_merge.bias'].reshape(())
    # movement m carries phase bit 1 iff it is in phase_pairs[phase]
    bits = np.zeros((B, N_MOVEMENTS), np.int64)
    for b in range(B):
        bits[b, pairs[ph[b]][0]] = 1
        bits[b, pairs[ph[b]][1]] = 1
    lanes = []
    for m in range(N_MOVEMENTS):
        phase = _sigmoid(p_w[bits[:, m]])                               # [B, 4]
        demand = _sigmoid(x[:, m:m + D] @ d_w.T + d_b)                  # [B, 4]: the windows of D = 4 overlap
        lanes.append(_relu(np.concatenate((phase, demand), -1) @ le_w.T + le_b))
    pair = [lanes[a] + lanes[b] for a, b in pairs]                      # P x [B, 16]
    q = np.zeros((B, P))
    for i in range(P):
        for j in range(P):
            if i == j:
                continue
            comp = int(len(set(pairs[i] + pairs[j])) == 3)
            rot = _relu(np.concatenate((pair[i], pair[j]), -1) @ lc_w.T + lc_b)
            rel = _relu(rc_w @ _relu(re_w[comp]) + rc_b)                # [20]
            h = _relu((rot * rel) @ h_w.T + h_b)
            q[:, i] += h @ bm_w + bm_b
    return q


# ---- fixtures
def synthetic_signal_set(P, S, rng, repeated_movement=False, counts=None):
    """P distinct phase pairs of distinct movements out of 12 and valid_acts tables for S signals -> (pairs [P][2] int32, valid [S][P],
    order [S][P], scenario stand-in for FusedMPLight / mplight_tables).

    The numbers of valid pairs cover P, 1, 2 and an intermediate value (counts: given instead); every signal with more than one
    valid pair lists them in an order that does not start with its smallest pair index (hence is not ascending); the local actions
    run 0 .. n-1 in dict order, as rs_mplight_create requires.  repeated_movement: pair 0 names one movement twice, [m, m], and
    pair 1 shares nothing with it -- the case where "three distinct movements" and "one shared movement" differ."""
    combos = [(a, b) for a in range(N_MOVEMENTS) for b in range(a + 1, N_MOVEMENTS)]
    pick = rng.choice(len(combos), P, replace=False)
    pairs = []
    for c in pick:
        a, b = combos[c]
        pairs.append([a, b] if rng.random() < 0.5 else [b, a])
    if repeated_movement:
        m = pairs[0][0]
        pairs[0] = [m, m]
        other = [v for v in range(N_MOVEMENTS) if v != m]
        free = [(a, b) for a in other for b in other if a < b and not any(set(p) == {a, b} for p in pairs[2:])]
        pairs[1] = list(free[rng.integers(len(free))])
    if counts is None:
        base = [P, 1, 2, max(3, (P + 1) // 2) if P >= 4 else 2]
        counts = [base[s] if s < 4 else int(rng.integers(1, P + 1)) for s in range(S)]
    assert len(counts) == S
    signal_ids = ['tl%d' % s for s in range(S)]
    valid_acts = {}
    for s, n in enumerate(counts):
        lst = sorted(rng.choice(P, n, replace=False).tolist())
        if n > 1:
            while True:
                perm = rng.permutation(lst).tolist()
                if perm[0] != min(lst):
                    break
            lst = perm
        valid_acts[signal_ids[s]] = {int(g): k for k, g in enumerate(lst)}
    sc = types.SimpleNamespace(n_signals=S, signal_ids=signal_ids, phase_pairs=[list(p) for p in pairs], valid_acts=valid_acts)
    valid = np.full((S, P), -1, np.int32)
    order = np.full((S, P), -1, np.int32)
    for s, sid in enumerate(signal_ids):
        for k, (g, a) in enumerate(valid_acts[sid].items()):
            valid[s, g], order[s, k] = a, g
    return np.asarray(pairs, np.int32), valid, order, sc


def obs_classes(P, D, n, S, rng):
    """{class: rows [n, S, 1 + 12 D]} (int32 for D = 1, float32 for D = 4, the kernel's input types).  The phase column cycles through
    -2 .. P + 2 in every class (shuffled), so every pair index and both clamps occur once n S >= P + 5."""
    W = 1 + N_MOVEMENTS * D
    out = {}
    for name in CLASSES:
        shape = (n, S, W - 1)
        if name == 'zero':
            dem = np.zeros(shape)
        elif name == 'sat':
            dem = rng.choice([-1000.0, 1000.0], shape)
        elif D == 1:
            lim = 8 if name == 'small' else 80
            dem = rng.integers(-lim, lim + 1, shape).astype(np.float64)
        else:
            dem = rng.normal(0.0, 3.0 if name == 'small' else 25.0, shape)
        phases = np.arange(-2, P + 3)
        ph = np.resize(phases, n * S) if n * S >= len(phases) else rng.choice(phases, n * S, replace=False)
        ph = rng.permutation(ph).reshape(n, S)
        rows = np.concatenate((ph[..., None].astype(np.float64), dem), -1)
        out[name] = np.ascontiguousarray(rows.astype(np.int32 if D == 1 else np.float32))
    return out


def make_net(pairs, D, scale=1.0, seed=3):
    """FRAP on the CPU with the reference's initialisation, every parameter times `scale`"""
    net = FRAP(len(pairs), [list(map(int, p)) for p in pairs], D).init_like_reference(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(float(scale))
    return net


def fp32_frap(net, obs):
    """the fp32 PyTorch FRAP on the CPU (the yardstick's fp32 side) -> [..., P] float64 array of fp32 values"""
    import copy
    cpu = copy.deepcopy(net).cpu().float()
    obs = np.asarray(obs)
    with torch.no_grad():
        q = cpu(torch.as_tensor(obs.astype(np.float32))).numpy()
    return q.reshape(obs.shape[:-1] + (net.oshape,)).astype(np.float64)


# ---- the yardstick
def ulp32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def q_tolerance(q64, q32):
    """(element-wise bound 4 e_ref + 2 ulp32(|Q64|), e_ref = max |Q32 - Q64| over the arrays given)"""
    e_ref = float(np.abs(q32 - q64).max())
    return 4.0 * e_ref + 2.0 * ulp32(q64), e_ref


def greedy_check(pair, q64, order, e_ref):
    """The margin rule on pair [n, S] against q64 [n, S, P]: where the float64 margin between the best and the second-best valid Q
    exceeds 8 e_ref the pair is the float64 pair (first maximum in dict order); elsewhere its float64 Q is within 8 e_ref of the
    maximum.  Returns the share of rows below the margin."""
    n, S = pair.shape
    excluded = 0
    for s in range(S):
        lst = [int(g) for g in order[s] if g >= 0]
        assert np.all(np.isin(pair[:, s], lst)), ('signal %d: a pair outside the valid list' % s)
        v = q64[:, s, lst]
        best = np.asarray(lst)[np.argmax(v, axis=1)]                    # first maximum in dict order
        if len(lst) > 1:
            srt = np.sort(v, axis=1)
            clear = srt[:, -1] - srt[:, -2] > 8.0 * e_ref
        else:
            clear = np.ones(n, bool)
        np.testing.assert_array_equal(pair[clear, s], best[clear], err_msg='signal %d' % s)
        mine = q64[np.arange(n), s, pair[:, s]]
        assert np.all(mine[~clear] >= v.max(axis=1)[~clear] - 8.0 * e_ref), 'signal %d: a pair far from the maximum' % s
        excluded += int((~clear).sum())
    return excluded / float(n * S)


# ---- the kernel's epilogue (resco_frap.h: frap_draw, frap_body)
def _u01(h):
    return np.float32(h >> 8) * np.float32(1.0 / 16777216.0)           # d_u01, in float32 as tests/idqn_kernel_ref.py restates it


def explores(seed, genv, s, key, eps):
    """does row (global environment genv, signal s) explore at step key `key`?"""
    eps = np.float32(eps)
    if not eps > 0:
        return False
    return bool(_u01(_murmur((seed ^ FRAP_SALT) & 0xFFFFFFFF, (genv & 0xFFFFFFFF, s, key & 0xFFFFFFFF, 0))) < eps)


def select_pairs(q, order, eps=0.0, seed=0, env_base=0, step_key=0, greedy=None):
    """(pair [n, S], explore mask [n, S]).  Greedy rows: the first maximum of q [n, S, >= P] over the valid pairs in dict order, strict >
    (greedy: take these pairs instead of deriving them from q); exploring rows: the k-th valid pair, k = word-1 hash mod n_valid."""
    n, S = q.shape[:2] if greedy is None else greedy.shape
    pair = np.zeros((n, S), np.int32)
    mask = np.zeros((n, S), bool)
    for s in range(S):
        lst = [int(g) for g in order[s] if g >= 0]
        for m in range(n):
            if explores(seed, env_base + m, s, step_key, eps):
                mask[m, s] = True
                k = _murmur((seed ^ FRAP_SALT) & 0xFFFFFFFF, ((env_base + m) & 0xFFFFFFFF, s, step_key & 0xFFFFFFFF, 1)) % len(lst)
                pair[m, s] = lst[k]
            elif greedy is not None:
                pair[m, s] = greedy[m, s]
            else:
                g = lst[0]
                for gi in lst[1:]:
                    if q[m, s, gi] > q[m, s, g]:
                        g = gi
                pair[m, s] = g
    return pair, mask
