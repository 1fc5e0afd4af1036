"""Tests-only: the truth of the target's options of the IDQN learners (n-step returns, Double DQN; rs_dqn_set_target of
include/resco_sim.h, nstep_walk of resco_amd/agents/idqn_learn.py).  The rings, the networks and the forward are tests/dqn_train_ref.py's,
unchanged; this adds a scalar Python twin of the walk, the target restated row by row in float64 and in float32, and autograd
gradients in the form dqn_train_ref.torch_grads gives them.  The yardstick is the project's: truth = float64, e_ref = float32
against it, the device gets 4 e_ref per tensor and on the loss.

`reference` asserts, on the references alone and with no row left out, what makes a case able to tell a right kernel from a wrong one:
  1. the argmax margin: on every row of the ring the online network's best and second-best Q differ by at least 256 x the largest
     |Q32 - Q64| of the case (so float32 and float64 choose the same action, and so does any fp32 summation order);
  2. the Huber branches: the share of rows with |delta| > 1 lies in 0.2 .. 0.8 and no |delta| is within 1e-4 of 1;
  3. with double_q at least a quarter of the bootstrapped rows have argmax_online != argmax_target, and the truth gradient differs
     from the truth without double_q by more than 100 e_ref in at least one tensor;
  4. with n_step > 1 the truth gradient differs from the one-step truth by more than 100 e_ref in at least one tensor.
A kernel that ignores an option therefore cannot pass."""
import functools

import numpy as np
import torch

from dqn_train_ref import NAMES, case, forward_all
from resco_amd.agents.trunk import fc1_row_mask
from train_ref import net_as

GAMMA = 0.99


def walk(done, T, head, t, n_step):
    """the scalar walk -> (m, cut): the twin of dqn_nstep_walk of resco_amd/csrc/resco_dqn_train.h"""
    newest = (head - 1) % T
    u, j = t, 0
    while True:
        d = bool(done[u])
        j += 1
        if d or j >= n_step or (u + 1) % T == newest:
            return j, d
        u = (u + 1) % T


def valid_slots(T, head, count):
    """the slots the draw can name: written, with a written successor"""
    return [(head - count + k) % T for k in range(count - 1)]


def rows(c, idx, head, n_step, np_dtype):
    """the walk of every row idx [B, S, 2] in np_dtype, in the defined order (R = rew_0, g = gamma; R = R + g rew_j, g = g gamma)
    -> dict(R, g [B, S] np_dtype; m, u_m [B, S] int; cut [B, S] bool; read: the set of slots whose reward was taken)"""
    idx = np.asarray(idx)
    B, S = idx.shape[:2]
    T = c['obs'].shape[0]
    out = dict(R=np.zeros((B, S), np_dtype), g=np.zeros((B, S), np_dtype), m=np.zeros((B, S), np.int64), u_m=np.zeros((B, S), np.int64),
               cut=np.zeros((B, S), bool), read=set())
    gamma = np_dtype(GAMMA)
    for i in range(B):
        for s in range(S):
            t, e = int(idx[i, s, 0]), int(idx[i, s, 1])
            m, cut = walk(c['done'], T, head, t, n_step)
            R, g = np_dtype(c['rew'][t, e, s]), gamma
            out['read'].add(t)
            for j in range(1, m):
                u = (t + j) % T
                out['read'].add(u)
                R = np_dtype(R + np_dtype(g * np_dtype(c['rew'][u, e, s])))
                g = np_dtype(g * gamma)
            out['R'][i, s], out['g'][i, s], out['m'][i, s], out['u_m'][i, s], out['cut'][i, s] = R, g, m, (t + m) % T, cut
    return out


def torch_grads(c, idx, dtype, head, n_step=1, double_q=False):
    """The loss on rows idx [B, S, 2] in dtype and its backward, as dqn_train_ref.torch_grads gives them: (dict name -> float64 numpy
    gradient with the fc1 mask; float64 numpy [S] loss; float64 numpy [B, S] delta), and a fourth: dict(m, cut, a_online, a_target)"""
    net, tgt_net = net_as(c['net'], dtype), net_as(c['target'], dtype)
    w = rows(c, idx, head, n_step, np.float64 if dtype == torch.float64 else np.float32)
    idx = np.asarray(idx)
    t, e, s = idx[..., 0], idx[..., 1], np.arange(idx.shape[1])[None, :]
    o2 = c['obs'][w['u_m'], e, s].copy()
    o2[w['cut']] = 0                       # whatever the ring holds behind a cut must never matter
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    o, a, cut = f(c['obs'][t, e, s]), f(c['act'][t, e, s]).long(), f(w['cut'])
    y = net(o).gather(-1, a.unsqueeze(-1)).squeeze(-1)
    with torch.no_grad():
        q_t, q_o = tgt_net(f(o2)), net(f(o2))
        a_t, a_o = q_t.argmax(-1), q_o.argmax(-1)
        boot = q_t.gather(-1, a_o.unsqueeze(-1)).squeeze(-1) if double_q else q_t.max(-1).values
        R, g = f(w['R']), f(w['g'])
        target = torch.where(cut, R, R + g * boot)
    per = torch.nn.functional.smooth_l1_loss(y, target, reduction='none').mean(0)
    per.sum().backward()
    grads = {k: getattr(net, k).grad.detach().double() for k in NAMES}
    grads['fc1_w'] = grads['fc1_w'] * fc1_row_mask(net.lanes, net.lmax, torch.float64)
    info = dict(m=w['m'], cut=w['cut'], a_online=a_o.numpy(), a_target=a_t.numpy(), read=w['read'], u_m=w['u_m'])
    return {k: v.numpy() for k, v in grads.items()}, per.detach().double().numpy(), (y - target).detach().double().numpy(), info


@functools.lru_cache(maxsize=None)
def ring_case(lmax, T, N, done_slots=(1,)):
    """case(lmax, T, N, seed=lmax) and condition 1 on every row of its ring"""
    c = case(lmax, T, N, seed=lmax, done_slots=done_slots)
    S = c['obs'].shape[2]
    flat = torch.from_numpy(c['obs'].reshape(T * N, S, lmax, 5))
    with torch.no_grad():
        q64 = forward_all(net_as(c['net'], torch.float64), flat)[3].numpy()
        q32 = forward_all(net_as(c['net'], torch.float32), flat)[3].double().numpy()
    real = np.isfinite(q64)
    err = np.abs(np.where(real, q32, 0.0) - np.where(real, q64, 0.0)).max()
    top = np.sort(np.where(real, q64, -np.inf), -1)
    several = np.asarray(c['net'].actions) > 1                  # a signal with one action has no second best
    margin = (top[..., -1] - top[..., -2])[:, several].min()
    print('ring (%d, %d, %d): smallest argmax margin %.3e, largest |Q32 - Q64| %.3e' % (lmax, T, N, margin, err))
    assert margin >= 256 * err, (margin, err)
    assert np.array_equal(np.where(real, q64, -np.inf).argmax(-1), np.where(real, q32, -np.inf).argmax(-1))
    return c


def draw_idx(T, N, B, slots):
    rng = np.random.default_rng(B)
    return np.stack([rng.choice(np.asarray(slots), (B, 3)), rng.integers(0, N, (B, 3))], -1).astype(np.int32)


def _far(a, b, e):
    """does truth a differ from truth b by more than 100 e_ref (e: name -> e_ref) in at least one tensor?"""
    return any(np.abs(a[k] - b[k]).max() > 100 * e[k] for k in NAMES)


@functools.lru_cache(maxsize=None)
def reference(lmax, T, N, B, head, count, n_step, double_q, done_slots=(1,), slots=None):
    """(idx, truth gradients, float32 gradients, truth loss, float32 loss, info): computed once, shared, never changed.  The rows are
    drawn from `slots` (default: every slot the draw can name); conditions 2 - 4 of the module docstring are asserted here."""
    c = ring_case(lmax, T, N, done_slots)
    ok = valid_slots(T, head, count)
    slots = tuple(ok) if slots is None else tuple(slots)
    assert set(slots) <= set(ok)
    idx = draw_idx(T, N, B, slots)
    g64, l64, d64, info = torch_grads(c, idx, torch.float64, head, n_step, double_q)
    g32, l32, _, info32 = torch_grads(c, idx, torch.float32, head, n_step, double_q)
    assert np.array_equal(info['a_online'], info32['a_online']) and np.array_equal(info['a_target'], info32['a_target'])
    ad = np.abs(d64)
    frac = (ad > 1).mean()
    print('(%d, %d, %d) B %d n %d dq %d: share of |delta| > 1 %.2f, nearest to 1 %.2e' % (lmax, T, N, B, n_step, double_q, frac, np.abs(ad - 1).min()))
    assert 0.2 <= frac <= 0.8, 'both branches of the Huber loss must be well populated: %.2f' % frac
    assert np.abs(ad - 1).min() >= 1e-4
    e_ref = {k: np.abs(g32[k] - g64[k]).max() for k in NAMES}
    if double_q:
        boot = ~info['cut']
        differ = (info['a_online'] != info['a_target'])[boot].mean()
        assert differ >= 0.25, differ
        assert _far(g64, torch_grads(c, idx, torch.float64, head, n_step, False)[0], e_ref), 'double_q changes nothing here'
    if n_step > 1:
        assert (info['m'] > 1).any()
        assert _far(g64, torch_grads(c, idx, torch.float64, head, 1, double_q)[0], e_ref), 'n_step changes nothing here'
    return idx, g64, g32, l64, l32, info
