"""Tests-only: the truth of prioritised replay in the fused DQN update (rs_dqn_set_priorities of include/resco_sim.h;
resco_amd/csrc/resco_dqn_per.h).  The rings, networks, the n-step walk and the target are tests/dqn_nstep_ref.py's, unchanged; this adds
the priorities of a case, the draw's uniforms from the oracle's counter hash, the importance weights and the weighted loss with its
autograd gradient in float64 and in float32 (the yardstick is the project's: truth = float64, e_ref = float32 against it, the device
gets 4 e_ref per tensor and on the loss), and the priorities a commit must write.

`reference` asserts on the references alone what lets a case tell a right kernel from a wrong one: the weights spread (the smallest is
below 0.5, the largest is 1), and the weighted truth differs from the unweighted truth by more than 100 e_ref in at least one tensor."""
import functools

import numpy as np
import torch

from dqn_nstep_ref import NAMES, ring_case, rows, valid_slots
from oracle_batch import murmur_hash
from resco_amd.agents.trunk import fc1_row_mask
from train_ref import net_as

PER_SEED = 0x9E3779B9           # DQN_PER_SEED of resco_dqn_per.h
PER = dict(alpha=0.6, beta0=0.4, beta_steps=0, eps=1e-6)
S = 3
LOSS_ORDERS = 8


def uniforms(seed, u, n_signals, B):
    """(r0, r1): float64 [B, S], the two uniforms of every draw of update u (exact: 24 bits)"""
    r = np.zeros((2, B, n_signals))
    for i in range(B):
        for s in range(n_signals):
            for j in range(2):
                r[j, i, s] = (murmur_hash((seed ^ PER_SEED) & 0xFFFFFFFF, u, s, i, j) >> 8) * 2.0 ** -24
    return r[0], r[1]


def beta_at(beta0, beta_steps, u):
    """the schedule in double, rounded once to float32"""
    b = beta0 if beta_steps <= 0 else min(1.0, beta0 + (1.0 - beta0) * (u / float(beta_steps)))
    return np.float32(b)


@functools.lru_cache(maxsize=None)
def priorities(T, N, head, count, seed=0, zero_slot=True):
    """float32 [T, N, S] of non-negative priorities over five decades with a third of exact zeros, every signal of one valid slot all
    zero (zero_slot), and values in the unwritten and the newest slots as well (the draw must leave those out by position)"""
    rng = np.random.default_rng(1000 * T + N + seed)
    q = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), (T, N, S))).astype(np.float32)
    q[rng.random((T, N, S)) < 1.0 / 3.0] = 0.0
    ok = valid_slots(T, head, count)
    if zero_slot and len(ok) > 1:
        q[ok[len(ok) // 2]] = 0.0
    for t in ok:                                        # every other valid slot keeps a positive leaf per signal
        if not (zero_slot and len(ok) > 1 and t == ok[len(ok) // 2]):
            e = rng.integers(0, N)
            q[t, e, :] = np.maximum(q[t, e, :], np.float32(0.25))
    q.setflags(write=False)
    return q


def weights(prio, idx, head, count, beta, dtype):
    """the importance weights of the rows idx [B, S, 2] in dtype (np.float64 / np.float32) -> [B, S]: (M q / Z)^-beta over its maximum
    per signal, Z the sum of prio over the valid slots (in float32: slot by slot, one after the other)"""
    T, N = prio.shape[:2]
    ok = valid_slots(T, head, count)
    p = prio.astype(dtype)
    Z = np.zeros(S, dtype)
    for t in ok:
        Z = (Z + p[t].sum(0, dtype=dtype)).astype(dtype)
    M = dtype((count - 1) * N)
    q = p[idx[..., 0], idx[..., 1], np.arange(S)[None, :]]
    assert (q > 0).all(), 'a reference row of priority 0: no draw gives one'
    raw = np.power((M * q / Z).astype(dtype), dtype(-beta)).astype(dtype)
    return (raw / raw.max(0, keepdims=True)).astype(dtype)


def torch_grads(c, idx, dtype, head, n_step, double_q, w):
    """dqn_nstep_ref.torch_grads with row weights w [B, S] (None: unweighted) -> (gradients name -> float64 numpy with the fc1 mask,
    float64 [S] loss, float64 [B, S] delta)"""
    net, tgt_net = net_as(c['net'], dtype), net_as(c['target'], dtype)
    npd = np.float64 if dtype == torch.float64 else np.float32
    wk = rows(c, idx, head, n_step, npd)
    idx = np.asarray(idx)
    t, e, s = idx[..., 0], idx[..., 1], np.arange(idx.shape[1])[None, :]
    o2 = c['obs'][wk['u_m'], e, s].copy()
    o2[wk['cut']] = 0
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    o, a, cut = f(c['obs'][t, e, s]), f(c['act'][t, e, s]).long(), f(wk['cut'])
    y = net(o).gather(-1, a.unsqueeze(-1)).squeeze(-1)
    with torch.no_grad():
        q_t, q_o = tgt_net(f(o2)), net(f(o2))
        boot = q_t.gather(-1, q_o.argmax(-1).unsqueeze(-1)).squeeze(-1) if double_q else q_t.max(-1).values
        R, g = f(wk['R']), f(wk['g'])
        target = torch.where(cut, R, R + g * boot)
    per = torch.nn.functional.smooth_l1_loss(y, target, reduction='none')
    if w is not None:
        per = f(w.astype(npd)) * per
    per = per.mean(0)
    per.sum().backward()
    grads = {k: getattr(net, k).grad.detach().double() for k in NAMES}
    grads['fc1_w'] = grads['fc1_w'] * fc1_row_mask(net.lanes, net.lmax, torch.float64)
    return {k: v.numpy() for k, v in grads.items()}, per.detach().double().numpy(), (y - target).detach().double().numpy()


def draw_positive(prio, B, slots):
    """rows [B, S, 2] among `slots` whose priority is positive, per signal"""
    T, N = prio.shape[:2]
    rng = np.random.default_rng(B + 7 * N)
    idx = np.zeros((B, S, 2), np.int32)
    for s in range(S):
        t, e = np.nonzero(prio[np.asarray(slots)][:, :, s] > 0)
        pick = rng.integers(0, len(t), B)
        idx[:, s, 0], idx[:, s, 1] = np.asarray(slots)[t[pick]], e[pick]
    return idx


@functools.lru_cache(maxsize=None)
def reference(lmax, T, N, B, head, count, n_step, double_q, done_slots=(), beta=0.4):
    """(idx, prio, truth gradients, float32 gradients, truth loss, float32 losses, truth delta, float32 delta): computed once, shared,
    never changed.  The float32 losses are [LOSS_ORDERS, S]: a signal's loss is ONE number, and one float32 evaluation of a mean of B
    terms agrees with the truth to a fraction of an ulp by chance often enough (it did at B = 7) that its distance from the truth
    measured once is no yardstick.  So the float32 reference is evaluated with the minibatch's rows in LOSS_ORDERS orders (the same
    rows, weights and mean: only the float32 summation order differs) and check_4_e_ref takes e_ref over all of them."""
    c = ring_case(lmax, T, N, done_slots)
    prio = priorities(T, N, head, count)
    idx = draw_positive(prio, B, valid_slots(T, head, count))
    w64, w32 = weights(prio, idx, head, count, beta, np.float64), weights(prio, idx, head, count, beta, np.float32)
    print('(%d, %d, %d) B %d: weights %.3e .. %.3e' % (lmax, T, N, B, w64.min(), w64.max()))
    assert w64.max() == 1.0 and w64.min() < 0.5
    g64, l64, d64 = torch_grads(c, idx, torch.float64, head, n_step, double_q, w64)
    g32, l32, d32 = torch_grads(c, idx, torch.float32, head, n_step, double_q, w32)
    rng = np.random.default_rng(B)
    orders = [rng.permutation(B) for _ in range(LOSS_ORDERS - 1)]
    l32 = np.stack([l32] + [torch_grads(c, idx[o], torch.float32, head, n_step, double_q, w32[o])[1] for o in orders])
    # ... and that yardstick must not inflate unnoticed: a float32 loss is a handful of dependent roundings behind a Q value that is
    # itself a few ulp off, so its distance from the truth stays within 8 float32 ulp of the largest loss (1.1 - 2.7 were seen)
    ulp = np.spacing(np.float32(np.abs(l64).max())).astype(np.float64)
    assert np.abs(l32 - l64).max() <= 8 * ulp, (np.abs(l32 - l64).max() / ulp)
    plain = torch_grads(c, idx, torch.float64, head, n_step, double_q, None)[0]
    assert any(np.abs(g64[k] - plain[k]).max() > 100 * np.abs(g32[k] - g64[k]).max() for k in NAMES), 'the weights change nothing here'
    return idx, prio, g64, g32, l64, l32, d64, d32


def committed(delta, eps, alpha, dtype):
    """the leaves a commit writes for the rows' delta, in dtype"""
    return np.power((np.abs(delta).astype(dtype) + dtype(eps)).astype(dtype), dtype(alpha)).astype(dtype)


def pick_sequential(w, thr):
    """the draw's definition on float64 weights, summed one after the other: the first entry of positive weight whose inclusive
    cumulative sum exceeds thr, else the last entry of positive weight (nothing positive: 0)"""
    c, last = 0.0, 0
    for k, x in enumerate(w):
        c += float(x)
        if x > 0:
            if c > thr:
                return k
            last = k
    return last
