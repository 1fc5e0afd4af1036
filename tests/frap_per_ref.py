"""Tests-only: the truth of prioritised replay in the fused shared-DQN update of MPLight (rs_mplight_dqn_set_priorities of
include/resco_sim.h; resco_amd/csrc/resco_frap_per.h).  The rings, networks, the n-step walk and the target are tests/frap_nstep_ref.py's
and the scalar definitions tests/dqn_per_ref.py's, both unchanged; this adds the priorities of a case over three axes, the draw's three
uniforms from the oracle's counter hash, THE order of the sums restated in numpy float32 (the chunked Hillis-Steele scan) with the
three-level draw on top of it, the importance weights over the pooled minibatch, and the weighted loss with its autograd gradient.

The yardstick is the project's: truth = float64; e_ref of a tensor = the worst distance from the truth over a family of float32
evaluations of the WEIGHTED loss (the batch as drawn, 7 row permutations, chunks of 16 rows), floored at 1 ulp32 of the tensor's
largest |truth|; the device and the host build get 4 e_ref per tensor and on the loss.

`reference` asserts on the references alone what lets a case tell a right kernel from a wrong one: the weights spread (the smallest
is below 0.5, the largest is 1), and the weighted truth differs from the unweighted truth by more than 100 e_ref in at least one
tensor."""
import ctypes as C
import functools

import numpy as np
import torch

import frap_nstep_ref as fn
from dqn_per_ref import PER, beta_at, committed, pick_sequential        # noqa: F401 (for the tests)
from frap_train_ref import CHUNK, FRAP_TRAIN_SALT, N_PERMS, frap_forward, ulp32, unpack, weights_as
from oracle_batch import murmur_hash
from train_ref import build_host

F = np.float32


def uniforms(seed, u, B):
    """float64 [B, 3]: the three uniforms of every draw of update u (exact: 24 bits); the hash's fourth argument is 1"""
    sd = (seed ^ FRAP_TRAIN_SALT) & 0xFFFFFFFF
    return np.array([[(murmur_hash(sd, u, i, 1, j) >> 8) * 2.0 ** -24 for j in range(3)] for i in range(B)]).reshape(B, 3)


def uniform_draw_values(seed, u, B):
    """the 24-bit values the UNIFORM draw's hashes (fourth argument 0) would give for the same (seed, u, i): another stream"""
    sd = (seed ^ FRAP_TRAIN_SALT) & 0xFFFFFFFF
    return np.array([[(murmur_hash(sd, u, i, 0, j) >> 8) * 2.0 ** -24 for j in range(3)] for i in range(B)]).reshape(B, 3)


# ---- THE order of a sum (per_wave_total / per_wave_pick of resco_dqn_per.h) in numpy float32
def scan(w):
    """-> (cumulative values float32 [n], total float32): chunks of 64, inside a chunk the inclusive Hillis-Steele scan (steps 1, 2, 4
    .. 32: position l adds the value of position l - d), cumulative = carry + scan, carry = the cumulative value of position 63"""
    w = np.asarray(w, F)
    n = len(w)
    cum, carry = np.zeros(n, F), F(0)
    for k0 in range(0, n, 64):
        x = np.zeros(64, F)
        m = min(64, n - k0)
        x[:m] = w[k0:k0 + m]
        d = 1
        while d < 64:
            y = x.copy()
            y[d:] = x[d:] + x[:-d]
            x, d = y, d * 2
        c = (carry + x).astype(F)
        cum[k0:k0 + m] = c[:m]
        carry = c[63]
    return cum, F(carry)


def total(w):
    return scan(w)[1]


def pick(w, thr):
    """the draw among the weights w against thr with THE cumulative values: chunk by chunk, the first entry of positive weight whose
    cumulative value exceeds thr, else the last entry of positive weight, else 0"""
    w = np.asarray(w, F)
    cum = scan(w)[0]
    hit = np.nonzero((w > 0) & (cum > F(thr)))[0]
    if len(hit):
        return int(hit[0])
    pos = np.nonzero(w > 0)[0]
    return int(pos[-1]) if len(pos) else 0


def sums(prio):
    """(esum [T, N], ssum [T]) of prio [T, N, S] in THE order: what a rebuild writes, bit for bit"""
    T, N, S = prio.shape
    esum = np.array([[total(prio[t, e]) for e in range(N)] for t in range(T)], F).reshape(T, N)
    return esum, np.array([total(esum[t]) for t in range(T)], F)


def draw(prio, esum, ssum, head, count, seed, u, B):
    """the minibatch rs_mplight_dqn_sample draws by priority: int32 [B, 3]"""
    T, N, S = prio.shape
    ok = fn.valid_slots(T, head, count)
    r = uniforms(seed, u, B).astype(F)
    Z = total(ssum[ok])
    idx = np.zeros((B, 3), np.int32)
    for i in range(B):
        t = ok[pick(ssum[ok], F(r[i, 0] * Z))]
        e = pick(esum[t], F(r[i, 1] * ssum[t]))
        s = pick(prio[t, e], F(r[i, 2] * esum[t, e]))
        idx[i] = (t, e, s)
    return idx


@functools.lru_cache(maxsize=None)
def priorities(T, N, S, head, count, seed=0):
    """float32 [T, N, S] of non-negative priorities over five decades with a third of exact zeros; one valid slot all zero; one
    environment of another valid slot all zero; positive values left in the newest and the unwritten slots (the draw must leave
    those out by position); every other valid slot keeps a positive leaf"""
    rng = np.random.default_rng(1000 * T + 10 * N + S + seed)
    q = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), (T, N, S))).astype(F)
    q[rng.random((T, N, S)) < 1.0 / 3.0] = 0.0
    ok = fn.valid_slots(T, head, count)
    zero_slot = ok[len(ok) // 2] if len(ok) > 1 else None
    for t in ok:
        if t != zero_slot:
            e = int(rng.integers(0, N))
            q[t, e, int(rng.integers(0, S))] = F(0.25) + q[t, e].max()
            if N > 1 and t == [x for x in ok if x != zero_slot][0]:
                q[t, (e + 1) % N, :] = 0.0              # one environment of another slot all zero
    if zero_slot is not None:
        q[zero_slot] = 0.0
    for t in range(T):
        if t not in ok:
            q[t] = np.maximum(q[t], F(0.5))             # the newest and the unwritten slots: positive everywhere
    q.setflags(write=False)
    return q


def weights(prio, idx, head, count, beta, dtype):
    """the importance weights of the rows idx [B, 3] in dtype (np.float64 / np.float32) -> [B]: (M q / Z)^-beta over its maximum over
    the WHOLE minibatch, M = (count - 1) N S, Z the sum of prio over the valid slots (float32: THE total of the valid ssum)"""
    T, N, S = prio.shape
    ok = fn.valid_slots(T, head, count)
    if dtype == np.float32:
        Z = total(sums(np.asarray(prio))[1][ok])
    else:
        Z = prio[ok].astype(np.float64).sum()
    M = dtype((count - 1) * N * S)
    q = prio[idx[:, 0], idx[:, 1], idx[:, 2]].astype(dtype)
    assert (q > 0).all(), 'a reference row of priority 0: no draw gives one'
    raw = np.power((dtype(M * q) / dtype(Z)).astype(dtype), dtype(-beta)).astype(dtype)
    return (raw / raw.max()).astype(dtype)


def torch_grads(c, idx, dtype, w=None, chunk=None):
    """frap_nstep_ref.torch_grads with row weights w [B] (None: unweighted) under the case's options -> (gradients name -> float64
    numpy, float64 loss, float64 [B] delta)"""
    idx = np.asarray(idx)
    wts = weights_as(c['net'], dtype)
    wd, wt = {k: v.detach() for k, v in wts.items()}, fn._detached(c['target'], dtype)
    npd = np.float64 if dtype == torch.float64 else np.float32
    r = fn.rows(c, idx, npd)
    t, e, s = idx[:, 0], idx[:, 1], idx[:, 2]
    o2 = c['obs'][r['u_m'], e, s].copy()
    o2[r['cut']] = 0
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    o, o2 = f(c['obs'][t, e, s]).to(dtype), f(o2).to(dtype)
    g = f(np.clip(c['act'][t, e, s].astype(np.int64), 0, c['P'] - 1))
    R, disc, cut = f(r['R']), f(r['g']), f(r['cut'])
    wrow = torch.ones(len(idx), dtype=dtype) if w is None else f(np.asarray(w).astype(npd))
    B = len(idx)
    step = B if chunk is None else int(chunk)
    tot, deltas = torch.zeros((), dtype=dtype), []
    for i in range(0, B, step):
        k = slice(i, i + step)
        y = frap_forward(wts, c['pairs'], c['D'], o[k]).gather(-1, g[k].unsqueeze(-1)).squeeze(-1)
        with torch.no_grad():
            q_t, q_o = frap_forward(wt, c['pairs'], c['D'], o2[k]), frap_forward(wd, c['pairs'], c['D'], o2[k])
            boot = q_t.gather(-1, q_o.argmax(-1).unsqueeze(-1)).squeeze(-1) if c['double_q'] else q_t.max(-1).values
            tgt = torch.where(cut[k], R[k], R[k] + disc[k] * boot)
        part = (wrow[k] * torch.nn.functional.smooth_l1_loss(y, tgt, reduction='none')).sum() / B
        part.backward()
        tot = tot + part.detach()
        deltas.append((y - tgt).detach())
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().double().numpy() for k, v in wts.items()}
    return grads, float(tot.double()), torch.cat(deltas).double().numpy()


@functools.lru_cache(maxsize=None)
def case_priorities(shape, seed=0):
    """the priorities of a gradient case: log-uniform over 1e-3 .. 1e2, a third of exact zeros among the leaves the minibatch of
    frap_nstep_ref.reference does not name"""
    P, D, T, N, S = shape[:5]
    idx = fn.reference(*shape)[0]
    rng = np.random.default_rng(31 * T + 7 * N + S + 1000 * seed)
    q = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), (T, N, S))).astype(F)
    zero = rng.random((T, N, S)) < 1.0 / 3.0
    zero[idx[:, 0], idx[:, 1], idx[:, 2]] = False
    q[zero] = 0.0
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def reference(shape, beta=0.4):
    """(idx, prio, w64, truth gradients, e_ref per tensor, truth loss, e_ref of the loss, truth delta) of the minibatch
    frap_nstep_ref.reference draws for the shape, weighted: computed once, shared, never changed"""
    P, D, T, N, S, B, head, count, n_step, dq, done_slots = shape
    c = fn.ring_case(P, D, T, N, S, head, count, n_step, dq, tuple(done_slots))
    idx, plain = fn.reference(*shape)[:2]
    prio = case_priorities(shape)
    w64, w32 = weights(prio, idx, head, count, beta, np.float64), weights(prio, idx, head, count, beta, np.float32)
    assert w64.max() == 1.0 and w64.min() < 0.5, (w64.min(), w64.max())
    g64, l64, d64 = torch_grads(c, idx, torch.float64, w64)
    rng = np.random.default_rng(B)
    family = [('as drawn',) + torch_grads(c, idx, torch.float32, w32)[:2]]
    for k in range(N_PERMS):
        o = rng.permutation(B)
        family.append(('permutation %d' % k,) + torch_grads(c, idx[o], torch.float32, w32[o])[:2])
    family.append(('chunks of %d' % CHUNK,) + torch_grads(c, idx, torch.float32, w32, chunk=CHUNK)[:2])
    e_ref = {k: max(max(np.abs(g[k] - g64[k]).max() for _, g, _ in family), float(ulp32(np.abs(g64[k]).max()))) for k in g64}
    e_loss = max(max(abs(l - l64) for _, _, l in family), float(ulp32(l64)))
    far = max(np.abs(g64[k] - plain[k]).max() / e_ref[k] for k in g64)
    print('%s: weights %.3f .. %.3f, weighted against unweighted truth %.2e e_ref' % (shape[:6], w64.min(), w64.max(), far))
    assert far > 100, 'the weights change nothing here'
    return idx, prio, w64, g64, e_ref, l64, e_loss, d64


# ---- the host build of the weighted phases and the scalar pieces (tests/frap_per_host)
def build_frap_per_host(out_dir):
    vp, i32, u32, f32 = C.c_void_p, C.c_int32, C.c_uint32, C.c_float
    return build_host('frap_per', out_dir, dict(
        frap_per_host_uniform=([u32] * 4, f32), frap_per_host_pick=[vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, f32, vp],
        frap_per_host_layout=[vp],
        frap_per_host_grad=[vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, C.c_double, i32, i32, vp, vp, vp, vp]))


def host_grads(host, c, idx, w):
    """frap_per_host_grad on the case's ring under its options with the rows' weights w (float32 [B]) -> (dict name -> float32
    gradient, float32 loss, float32 |delta| [B])"""
    from resco_amd.agents.mplight import pack_mplight_weights
    par, tgt = (np.ascontiguousarray(pack_mplight_weights(n).numpy(), F) for n in (c['net'], c['target']))
    T, N, S = c['obs'].shape[:3]
    obs, act, rew = fn.sentinel_arrays(c)
    arrs = [np.ascontiguousarray(obs, F), np.ascontiguousarray(act, np.int16), np.ascontiguousarray(rew, F), np.ascontiguousarray(c['done'], np.uint8),
            np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(c['pairs'], np.int32), np.ascontiguousarray(w, F)]
    B = len(idx)
    grad, loss, ad = np.full(len(par), np.nan, F), np.full(1, np.nan, F), np.full(B, np.nan, F)
    p = lambda a: a.ctypes.data
    rc = host.frap_per_host_grad(p(par), p(tgt), c['D'], c['P'], p(arrs[5]), p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), T, N, S, c['head'], p(arrs[4]), B,
                                 fn.GAMMA, c['n_step'], int(c['double_q']), p(arrs[6]), p(grad), p(loss), p(ad))
    assert rc == 0
    return unpack(grad, c['net']), float(loss[0]), ad
