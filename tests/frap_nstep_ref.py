"""Tests-only: the truth of the target's options of the MPLight learners (n-step returns, Double DQN; rs_mplight_dqn_set_target and
rs_mplight_maps_set_target of include/resco_sim.h, the option kernels of resco_amd/csrc/resco_frap_train.h), built on
tests/frap_train_ref.py: its networks, its kink-free rings, its float64 restatement of FRAP's forward and its yardstick -- truth =
float64; e_ref of a tensor = the worst distance from the truth over a family of float32 evaluations (the batch as drawn, 7 row
permutations, chunks of 16 rows), floored at 1 ulp32 of the tensor's largest |truth|; the device and the host build get 4 e_ref per
tensor and on the loss.

The definition, for the row (t, e, s) of a ring of T slots whose next slot to write is head (newest = (head - 1) mod T):
    the walk (walk below, the twin of dqn_nstep_walk): u_0 = t; step j takes rew[u_j][e][s] and the walk stops after it where
    done[u_j] (cut), where j + 1 == n_step, or where (u_j + 1) mod T == newest; m = j + 1.
    R = rew_0, g = gamma; for j = 1 .. m - 1: R = R + g rew_j, g = g gamma; tgt = R where cut, else R + g boot;
    boot = max over ALL P outputs of Q_target(obs[(t + m) mod T][e][s]), or with double_q Q_target[a*], a* = argmax over ALL P outputs
    of Q_online of the same row, the lowest index among equal maxima.

What makes a case able to tell a right kernel from a wrong one is asserted here, on the references alone; the generator redraws
until it holds (observation rows as frap_train_ref.case redraws them for kinks, the minibatch by its seed):
  1. argmax agreement: on EVERY row of the ring the float32 and the float64 online network agree on a* (the rule frap_train_ref.case
     applies to ReLU masks: without it the family's e_ref blows up and the bound proves nothing);
  2. Huber branches: the rewards are chosen so that between a quarter and three quarters of the minibatch rows have |delta| > 1
     under the n-step target;
  3. walk coverage: the minibatch rows cover every walk length m = 1 .. n_step, at least one cut walk and, where n_step > 1 (a
     one-step walk cannot be truncated), at least one truncated walk: m < n_step without a cut;
  4. the options matter: the truth differs from the truth of the same ring without double_q / at n_step 1 by more than 100 e_ref in
     at least one tensor or in the loss, and with double_q at least one bootstrapped row has argmax_online != argmax_target (double_q's half where
     P > 2: with two pairs the online and the target network of these cases name the same pair on all rows but one of the ring).
A shape that cannot meet them is not used: the smallest ring that has a cut walk, a truncated walk and both lengths at n_step 2 has
T = 4 (three rows that can be drawn), and n_step 5 beside a cut needs 7 such slots."""
import copy
import ctypes as C
import functools

import numpy as np
import torch

import frap_train_ref as ft
from frap_train_ref import CHUNK, GAMMA, N_PERMS, compare, frap_forward, ulp32, weights_as      # noqa: F401 (compare: for the tests)
from train_ref import build_host

# (P, D, T, N, S, B, head, count, n_step, double_q, done_slots): the smallest ring that meets the conditions (B crosses a tile); a full
# ring whose head lies inside with an episode end, at n_step 3 alone, with double_q, and double_q alone; a ring that is not full (slots
# 8 and 9 were never written) with many tiles and a ragged last one
SHAPES = [(2, 1, 4, 4, 2, 5, 0, 4, 2, True, (0,)),
          (8, 4, 8, 5, 3, 11, 3, 8, 3, False, (5,)),
          (8, 4, 8, 5, 3, 11, 3, 8, 3, True, (5,)),
          (8, 4, 8, 5, 3, 11, 3, 8, 1, True, (5,)),
          (16, 1, 10, 6, 2, 45, 8, 8, 5, True, (1,))]
SEMANTICS = SHAPES[2]
# two maps of one shared network (frap_train_ref.case draws the weights from the seed alone) in one minibatch: other P, ring size, head
# and episode end; 5 and 7 rows, so that either group ends in a ragged tile
TWO_MAPS = [(4, 1, 8, 4, 2, 5, 3, 8, 3, True, (5,)), (8, 1, 6, 3, 3, 7, 2, 6, 3, True, (4,))]
SEMANTICS_SLOTS = (3, 4, 5, 0, 1)       # cut after 3 / 2 / 1 rewards; truncated at the newest slot, 2, after 2 / 1


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
    """the slots the draw can name: written, with a written successor; oldest first"""
    return [(head - count + k) % T for k in range(count - 1)]


def _detached(net, dtype):
    return {k: v.detach() for k, v in weights_as(net, dtype).items()}


def _bad_rows(net, pairs, D, obs, act):
    """bool [n]: rows the generator must redraw -- a pre-activation near a kink, a ReLU mask or an online argmax on which float32 and
    float64 disagree"""
    w64, w32 = _detached(net, torch.float64), _detached(net, torch.float32)
    o = torch.from_numpy(obs)
    rows, g = torch.arange(len(obs)), torch.from_numpy(act).long()
    with torch.no_grad():
        a, b = frap_forward(w64, pairs, D, o.double(), True), frap_forward(w32, pairs, D, o, True)
    bad = torch.from_numpy(ft._near_kinks(w64, pairs, D, obs, act)) | (a[0].argmax(-1) != b[0].argmax(-1))
    for x, y in zip(a[1:], b[1:]):
        sel = (lambda t: t) if x.dim() == 3 else (lambda t: t[rows, g])
        bad |= ((sel(x) > 0) != (sel(y) > 0)).flatten(1).any(-1)
    return bad.numpy()


@functools.lru_cache(maxsize=None)
def ring_case(P, D, T, N, S, head, count, n_step, double_q, done_slots=(), tie=False, seed=1):
    """frap_train_ref.case(P, D, T, N, S, seed) at the ring position (head, count), with condition 1 on every row and the rewards of
    condition 2: delta of a row is 1.5 x a standard normal draw under the options' target (the slots solved newest first: a row's
    later rewards are newer slots').  tie: before_merge.weight of the online network is zero, so that all its Q are equal.  The
    rewards of slots no row can be drawn from are zero (the tests overwrite them with NaN).  Shared and never changed."""
    base = ft.case(P, D, T, N, S, seed=seed, done_slots=tuple(done_slots))
    c = dict(base, head=head, count=count, n_step=n_step, double_q=bool(double_q))
    pairs, W = base['pairs'], 1 + 12 * D
    if tie:
        c['net'] = copy.deepcopy(base['net'])
        with torch.no_grad():
            c['net'].before_merge.weight.zero_()
    rng = np.random.default_rng(77 + 1000 * P + 10 * D + seed)
    obs, act = base['obs'].reshape(-1, W).copy(), np.ascontiguousarray(base['act'].reshape(-1))
    for _ in range(200):
        bad = _bad_rows(c['net'], pairs, D, obs, act)
        if not bad.any():
            break
        obs[bad] = ft._draw_obs(P, D, int(bad.sum()), rng)
    assert not _bad_rows(c['net'], pairs, D, obs, act).any(), 'the case generator left a row on which float32 and float64 disagree'
    with torch.no_grad():
        o = torch.from_numpy(obs).double()
        q_o, q_t = frap_forward(_detached(c['net'], torch.float64), pairs, D, o), frap_forward(_detached(c['target'], torch.float64), pairs, D, o)
        y = q_o.gather(-1, torch.from_numpy(act).long().unsqueeze(-1)).squeeze(-1).reshape(T, N, S).numpy()
        boot = (q_t.gather(-1, q_o.argmax(-1, keepdim=True)).squeeze(-1) if double_q else q_t.max(-1).values).reshape(T, N, S).numpy()
    if tie:
        assert (q_o.argmax(-1) == 0).all() and (q_t.argmax(-1) != 0).float().mean() > 0.25
    want = 1.5 * rng.standard_normal((T, N, S))
    rew = np.zeros((T, N, S), np.float32)
    for t in reversed(valid_slots(T, head, count)):
        m, cut = walk(base['done'], T, head, t, n_step)
        tail = sum(GAMMA ** j * rew[(t + j) % T].astype(np.float64) for j in range(1, m))
        if not cut:
            tail = tail + GAMMA ** m * boot[(t + m) % T]
        rew[t] = (y[t] - want[t] - tail).astype(np.float32)
    c['obs'], c['rew'] = obs.reshape(T, N, S, W), rew
    return c


def rows(c, idx, np_dtype):
    """the walk of every row idx [B, 3] in np_dtype, in the defined order -> dict(R, g [B]; m, u_m [B] int; cut [B] bool; read: the slots
    whose reward was taken)"""
    idx = np.asarray(idx)
    B, T = len(idx), c['obs'].shape[0]
    out = dict(R=np.zeros(B, np_dtype), g=np.zeros(B, np_dtype), m=np.zeros(B, np.int64), u_m=np.zeros(B, np.int64), cut=np.zeros(B, bool), read=set())
    gamma = np_dtype(GAMMA)
    for i, (t, e, s) in enumerate(idx.tolist()):
        m, cut = walk(c['done'], T, c['head'], t, c['n_step'])
        R, g = np_dtype(c['rew'][t, e, s]), gamma
        out['read'].add(t)
        for j in range(1, m):
            u = (t + j) % T
            out['read'].add(u)
            R = np_dtype(R + np_dtype(g * np_dtype(c['rew'][u, e, s])))
            g = np_dtype(g * gamma)
        out['R'][i], out['g'][i], out['m'][i], out['u_m'][i], out['cut'][i] = R, g, m, (t + m) % T, cut
    return out


def torch_grads(c, idx, dtype, chunk=None, n_step=None, double_q=None):
    """The mean Huber loss of the rows idx [B, 3] under the case's options (or the ones given) in dtype and its backward -> (dict name ->
    float64 numpy gradient, float64 loss, float64 numpy delta [B], info: dict(m, cut, u_m, read, a_online, a_target)).  chunk: the rows
    in chunks of that many, the chunk gradients accumulated in dtype."""
    c = dict(c, n_step=c['n_step'] if n_step is None else n_step)
    double_q = c['double_q'] if double_q is None else double_q
    idx = np.asarray(idx)
    w = weights_as(c['net'], dtype)
    wd, wt = {k: v.detach() for k, v in w.items()}, _detached(c['target'], dtype)
    r = rows(c, idx, np.float64 if dtype == torch.float64 else np.float32)
    t, e, s = idx[:, 0], idx[:, 1], idx[:, 2]
    o2 = c['obs'][r['u_m'], e, s].copy()
    o2[r['cut']] = 0                        # whatever the ring holds behind a cut must never matter
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    o, o2 = f(c['obs'][t, e, s]).to(dtype), f(o2).to(dtype)
    g = f(np.clip(c['act'][t, e, s].astype(np.int64), 0, c['P'] - 1))
    R, disc, cut = f(r['R']), f(r['g']), f(r['cut'])
    B = len(idx)
    step = B if chunk is None else int(chunk)
    total, deltas, a_on, a_tg = torch.zeros((), dtype=dtype), [], [], []
    for i in range(0, B, step):
        k = slice(i, i + step)
        y = frap_forward(w, c['pairs'], c['D'], o[k]).gather(-1, g[k].unsqueeze(-1)).squeeze(-1)
        with torch.no_grad():
            q_t, q_o = frap_forward(wt, c['pairs'], c['D'], o2[k]), frap_forward(wd, c['pairs'], c['D'], o2[k])
            best = q_o.argmax(-1)           # (the first of equal maxima)
            boot = q_t.gather(-1, best.unsqueeze(-1)).squeeze(-1) if double_q else q_t.max(-1).values
            tgt = torch.where(cut[k], R[k], R[k] + disc[k] * boot)
        part = torch.nn.functional.smooth_l1_loss(y, tgt, reduction='none').sum() / B
        part.backward()
        total = total + part.detach()
        deltas.append((y - tgt).detach())
        a_on.append(best)
        a_tg.append(q_t.argmax(-1))
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().double().numpy() for k, v in w.items()}
    info = dict(m=r['m'], cut=r['cut'], u_m=r['u_m'], read=r['read'], a_online=torch.cat(a_on).numpy(), a_target=torch.cat(a_tg).numpy())
    return grads, float(total.double()), torch.cat(deltas).double().numpy(), info


def draw_idx(c, B, slots, seed):
    T, N, S = c['obs'].shape[:3]
    rng = np.random.default_rng(B + 7919 * seed)
    return np.stack([rng.choice(np.asarray(slots), B), rng.integers(0, N, B), rng.integers(0, S, B)], -1).astype(np.int32)


def covers(info, n_step):
    """condition 3 on the walks of a minibatch"""
    truncated = (~info['cut'] & (info['m'] < n_step)).any() or n_step == 1
    return set(info['m'].tolist()) == set(range(1, n_step + 1)) and info['cut'].any() and truncated


def _far(c, idx, truth, e, **other):
    """does the truth (gradients, loss) differ from the truth under `other` options by more than 100 e_ref (e: per tensor, of the loss)
    in at least one tensor or in the loss?  (Where the changed rows all sit on the linear branch of the Huber loss, the loss alone.)"""
    g, l = torch_grads(c, idx, torch.float64, **other)[:2]
    return any(np.abs(truth[0][k] - g[k]).max() > 100 * e[0][k] for k in g) or abs(truth[1] - l) > 100 * e[1]


@functools.lru_cache(maxsize=None)
def reference(P, D, T, N, S, B, head, count, n_step, double_q, done_slots=(), slots=None, tie=False):
    """(idx, truth gradients, e_ref per tensor, truth loss, e_ref of the loss, the float32 family, delta64, info): computed once,
    shared, never changed.  The rows are drawn from `slots` (default: every slot the draw can name; given: each of them at least once), the draw's seed the first under
    which conditions 2 and 3 hold; condition 4 is asserted.  family: list of (label, gradients, loss)."""
    c = ring_case(P, D, T, N, S, head, count, n_step, double_q, tuple(done_slots), tie)
    ok = valid_slots(T, head, count)
    every = slots is not None               # slots given: every one of them is drawn from
    slots = tuple(ok) if slots is None else tuple(slots)
    assert set(slots) <= set(ok)
    need_differ = bool(double_q) and not tie and P > 2
    for seed in range(400):
        idx = draw_idx(c, B, slots, seed)
        if not covers(rows(c, idx, np.float64), n_step) or (every and set(idx[:, 0].tolist()) != set(slots)):
            continue
        g64, l64, d64, info = torch_grads(c, idx, torch.float64)
        differ = bool((info['a_online'] != info['a_target'])[~info['cut']].any())
        if 0.25 <= float((np.abs(d64) > 1).mean()) <= 0.75 and (differ or not need_differ):
            break
    else:
        raise AssertionError('no minibatch of this shape meets the conditions: change the shape')
    assert covers(info, n_step) and 0.25 <= float((np.abs(d64) > 1).mean()) <= 0.75
    print('(%d, %d, %d, %d, %d) B %d at (%d, %d) n %d dq %d: draw %d, walks %s, cut %d, share of |delta| > 1 %.2f' % (
        P, D, T, N, S, B, head, count, n_step, double_q, seed, sorted(set(info['m'].tolist())), int(info['cut'].sum()), (np.abs(d64) > 1).mean()))
    rng = np.random.default_rng(B)
    family = []
    for label, rows_, kw in [('as drawn', idx, {})] + [('permutation %d' % k, idx[rng.permutation(B)], {}) for k in range(N_PERMS)] + \
                            [('chunks of %d' % CHUNK, idx, dict(chunk=CHUNK))]:
        g32, l32, _, info32 = torch_grads(c, rows_, torch.float32, **kw)
        family.append((label, g32, l32))
        if label == 'as drawn':             # (condition 1 on the rows that bootstrap; a cut row's a* is of a row of zeros and is not used)
            assert np.array_equal(info32['a_online'][~info['cut']], info['a_online'][~info['cut']])
    e_ref = {k: max(max(np.abs(g[k] - g64[k]).max() for _, g, _ in family), float(ulp32(np.abs(g64[k]).max()))) for k in g64}
    e_loss = max(max(abs(l - l64) for _, _, l in family), float(ulp32(l64)))
    if need_differ:
        assert _far(c, idx, (g64, l64), (e_ref, e_loss), double_q=False), 'double_q changes nothing here'
    if tie:
        assert (info['a_online'] == 0).all() and _far(c, idx, (g64, l64), (e_ref, e_loss), double_q=False), 'the tie changes nothing here'
    if n_step > 1:
        assert _far(c, idx, (g64, l64), (e_ref, e_loss), n_step=1), 'n_step changes nothing here'
    return idx, g64, e_ref, l64, e_loss, family, d64, info


@functools.lru_cache(maxsize=None)
def two_map_reference():
    """the grouped minibatch of TWO_MAPS -> (idx int32 [B, 4] = (map, t, e, s), counts, truth gradients, e_ref per tensor, truth loss,
    e_ref of the loss): the per-map references weighted by B_m / B, as tests/frap_multi_ref.py combines them (e_ref through the
    triangle inequality, floored at one ulp32 of the combined truth)"""
    refs = [reference(*shape) for shape in TWO_MAPS]
    counts = [len(r[0]) for r in refs]
    B = sum(counts)
    for a, b in zip(*[(ring_case(*(sh[:5] + sh[6:]))[k].state_dict() for k in ('net', 'target')) for sh in TWO_MAPS]):
        assert list(a) == list(b) and all(np.array_equal(a[k].numpy(), b[k].numpy()) for k in a), 'the cases do not share one network'
    idx = np.concatenate([np.concatenate((np.full((n, 1), m, np.int32), r[0]), -1) for m, (r, n) in enumerate(zip(refs, counts))]).astype(np.int32)
    g64 = {k: sum(n / B * r[1][k] for r, n in zip(refs, counts)) for k in refs[0][1]}
    e_ref = {k: max(sum(n / B * r[2][k] for r, n in zip(refs, counts)), float(ulp32(np.abs(g64[k]).max()))) for k in g64}
    l64 = sum(n / B * r[3] for r, n in zip(refs, counts))
    return idx, counts, g64, e_ref, l64, max(sum(n / B * r[4] for r, n in zip(refs, counts)), float(ulp32(l64)))


# ---- the host build of the option phases (tests/frap_nstep_host)
def build_frap_nstep_host(out_dir):
    vp, i32 = C.c_void_p, C.c_int32
    return build_host('frap_nstep', out_dir, dict(frap_nstep_grad=[vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, C.c_double, i32, i32,
                                                                   vp, vp, vp, vp]))


def host_grads(host, c, idx, arrays=None):
    """frap_nstep_grad on the case's ring (arrays: (obs, act, rew) in place of the case's) under its options -> (dict name -> float32
    gradient, float32 loss, m [B], a* [B])"""
    from resco_amd.agents.mplight import pack_mplight_weights
    w, wt = (np.ascontiguousarray(pack_mplight_weights(n).numpy(), np.float32) for n in (c['net'], c['target']))
    T, N, S = c['obs'].shape[:3]
    obs, act, rew = (c['obs'], c['act'], c['rew']) if arrays is None else arrays
    arrs = [np.ascontiguousarray(obs, np.float32), np.ascontiguousarray(act, np.int16), np.ascontiguousarray(rew, np.float32), np.ascontiguousarray(c['done'], np.uint8),
            np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(c['pairs'], np.int32)]
    B = len(idx)
    grad, loss = np.full(len(w), np.nan, np.float32), np.full(1, np.nan, np.float32)
    m, astar = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    p = lambda a: a.ctypes.data
    rc = host.frap_nstep_grad(p(w), p(wt), c['D'], c['P'], p(arrs[5]), p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), T, N, S, c['head'], p(arrs[4]), B,
                              GAMMA, c['n_step'], int(c['double_q']), p(grad), p(loss), p(m), p(astar))
    assert rc == 0
    return ft.unpack(grad, c['net']), float(loss[0]), m, astar


def sentinel_arrays(c, unreadable=()):
    """(obs, act, rew) of the case's ring with what must not be read replaced: NaN observations / NaN rewards / action -777 in every
    unwritten and every `unreadable` slot, NaN reward and action -777 in the newest slot (its observations are intact)"""
    T = c['obs'].shape[0]
    newest = (c['head'] - 1) % T
    keep = set(valid_slots(T, c['head'], c['count'])) - set(unreadable)
    obs, act, rew = c['obs'].copy(), c['act'].copy(), c['rew'].copy()
    for t in range(T):
        if t not in keep:
            act[t], rew[t] = -777, np.nan
            if t != newest or t in unreadable:
                obs[t] = np.nan
    return obs, act, rew
