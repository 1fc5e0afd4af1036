"""GPU: prioritised experience replay in the fused shared-DQN update of MPLight (rs_mplight_dqn_set_priorities / _per_rebuild /
_per_fill / _per_commit of include/resco_sim.h; resco_amd/csrc/resco_frap_per.h; FusedMPLightLearner(per=...)).  The draw bit for bit
against the numpy restatement of THE order of the sums (tests/frap_per_ref.py); the weighted minibatch gradient against float64
autograd of the weighted loss (truth = float64, e_ref = the worst of a float32 family, the device gets 4 e_ref per tensor and on the
loss); what a commit writes and what it leaves; the sums against a rebuild, bit for bit; rs_mplight_dqn_update against its pieces; off
against a handle never touched; the refusals; the library's training loop against the Python-driven one on one and two pipes, and a
checkpoint of it at an episode boundary."""
import ctypes as C

import numpy as np
import pytest
import torch

import frap_nstep_ref as fn
import frap_per_ref as fp
import frap_train_ref as ft
from resco_amd import checkpoint
from resco_amd.agents.idqn_learn import linear_epsilon
from resco_amd.agents.mplight import FRAP, FusedMPLight, MPLightReplay, frap_from_scenario
from resco_amd.agents.mplight_learn_fused import FusedMPLightLearner
from resco_amd.agents.train_fused import DeviceTrainer
from resco_amd.sim import MPLightPer, load_library
from tools.train_pipes_ab import PipedEnvs, pair_of_action

pytestmark = pytest.mark.gpu

RS_EINVAL = -1
SEED = 0x5EED
MAX_BATCH = 33
PER = fp.PER
IDS = ['P%d-D%d-T%d-B%d-n%d-dq%d' % (s[0], s[1], s[2], s[5], s[8], s[9]) for s in fn.SHAPES]
#         T  N    S   head count
RINGS = [(4, 4, 2, 0, 4),           # the smallest
         (6, 5, 3, 4, 4),           # not full: slots 4 and 5 were never written
         (6, 5, 3, 2, 6),           # full and wrapped
         (8, 130, 3, 0, 8),         # the environment level crosses two chunk boundaries with a ragged end; head at 0
         (6, 3, 70, 3, 6),          # the signal level crosses a chunk
         (70, 2, 2, 5, 70)]         # the slot level crosses a chunk


def _case(shape):
    P, D, T, N, S, B, head, count, n_step, dq, done_slots = shape
    return fn.ring_case(P, D, T, N, S, head, count, n_step, dq, tuple(done_slots))


def _learner(c, B, S=None, per=PER, options=True, **kw):
    """a FusedMPLightLearner on a device copy of the case's network, its target the case's"""
    net = FRAP(c['net'].oshape, c['net'].phase_pairs, c['net'].demand_shape)
    net.load_state_dict(c['net'].state_dict())
    net = net.cuda()
    if options:
        kw = dict(dict(n_step=c['n_step'], double_q=c['double_q']), **kw)
    learner = FusedMPLightLearner(net, batch_size=B, seed=SEED, n_signals=c['obs'].shape[2] if S is None else S, per=per, **kw)
    learner.target.load_state_dict(c['target'].state_dict())
    return net, learner


def _device_ring(c, sentinels=True):
    """the case's ring on the device at its position.  sentinels: NaN observations / NaN rewards / action -777 wherever nothing may be
    read (frap_nstep_ref.sentinel_arrays) -- one of them read, and a gradient is NaN"""
    T, N, S, W = c['obs'].shape
    obs, act, rew = fn.sentinel_arrays(c) if sentinels else (c['obs'], c['act'], c['rew'])
    rp = MPLightReplay(T, N, S, W, device='cuda')
    rp.obs.copy_(torch.from_numpy(obs))
    rp.act.copy_(torch.from_numpy(act))
    rp.rew.copy_(torch.from_numpy(rew))
    rp.done.copy_(torch.from_numpy(c['done']))
    rp.head, rp.count = c['head'], c['count']
    return rp


def _set_priorities(learner, rp, prio):
    """the learner's priorities <- prio [T, N, S], its sums rebuilt"""
    learner.attach(rp)
    learner.prio.copy_(torch.from_numpy(np.array(prio)))
    learner.per_rebuild()
    torch.cuda.synchronize()


def _per_state(learner):
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy().copy() for x in (learner.prio, learner.esum, learner.ssum, learner.pmax))


def _state_np(learner):
    torch.cuda.synchronize()
    return tuple(x.detach().cpu().numpy().copy() for x in (learner.flat, learner._m, learner._v, learner._g, learner.loss_out))


def _grads_np(learner):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in learner.grads.items()}


# ---------------------------------------------------------------------------------------------------------------- 1. the draw
@pytest.mark.parametrize('B', [7, MAX_BATCH])
@pytest.mark.parametrize('T,N,S,head,count', RINGS)
def test_the_draw(T, N, S, head, count, B):
    c = _case(fn.SHAPES[0])
    net, learner = _learner(c, MAX_BATCH, S=S, options=False)
    rp = MPLightReplay(T, N, S, 13, device='cuda')          # (the draw reads nothing of the ring itself)
    rp.head, rp.count = head, count
    prio = fp.priorities(T, N, S, head, count)
    _set_priorities(learner, rp, prio)
    got_prio, esum, ssum, pmax = _per_state(learner)
    assert got_prio.tobytes() == prio.tobytes()
    want_esum, want_ssum = fp.sums(prio)
    assert esum.tobytes() == want_esum.tobytes() and ssum.tobytes() == want_ssum.tobytes(), 'a rebuild sums in THE order'
    ok = fn.valid_slots(T, head, count)
    seen = set()
    for u in (0, 1, 77):
        idx = learner.sample(rp, batch_size=B, update_key=u).cpu().numpy()
        assert idx.shape == (B, 3)
        ft.check_sample(idx, T, N, S, head, count)          # in the ring; neither the newest nor an unwritten slot
        want = fp.draw(prio, esum, ssum, head, count, SEED, u, B)
        assert idx.tobytes() == want.tobytes(), (u, np.nonzero((idx != want).any(1))[0])
        assert all(t in ok for t in idx[:, 0].tolist()) and (prio[idx[:, 0], idx[:, 1], idx[:, 2]] > 0).all(), 'an entry of weight 0 was drawn'
        assert (ssum[idx[:, 0]] > 0).all() and (esum[idx[:, 0], idx[:, 1]] > 0).all()
        seen |= set(idx[:, 0].tolist())
    if B == MAX_BATCH:          # 99 draws: a slot that holds a fifth of the mass is missed with probability 0.8^99
        s64 = prio.astype(np.float64).sum((1, 2))
        for t in ok:
            assert s64[t] < 0.2 * s64[ok].sum() or t in seen, t
    # priorities off on the same handle: the uniform draw again
    assert load_library().rs_mplight_dqn_set_priorities(learner._h, None) == 0
    learner.per = None
    assert np.array_equal(learner.sample(rp, batch_size=B, update_key=1).cpu().numpy(), ft.predict_sample(SEED, 1, T, N, S, head, count, B))
    learner.close()


# ------------------------------------------------------------------------------------------------------ 2. the gradient and the commit
@pytest.mark.parametrize('shape', fn.SHAPES, ids=IDS)
def test_weighted_gradient_and_commit(shape):
    P, D, T, N, S, B, head, count, n_step, dq, done_slots = shape
    c = _case(shape)
    idx, prio, w64, g64, e_ref, l64, e_loss, d64 = fp.reference(shape, beta=PER['beta0'])
    if shape == fn.SHAPES[4]:
        assert len({tuple(r) for r in idx.tolist()}) < len(idx), 'this minibatch names a row twice'
    net, learner = _learner(c, max(B, MAX_BATCH))
    rp = _device_ring(c)
    _set_priorities(learner, rp, prio)
    idx_t = torch.from_numpy(idx).cuda()
    learner.grad(rp, idx_t)
    got, loss = _grads_np(learner), learner.loss_out.cpu().numpy().copy()
    print(shape)
    worst = ft.compare(ft.names_of(net), got, loss, g64, e_ref, l64, e_loss)
    assert not worst, worst
    learner.grad(rp, idx_t)                                 # the same bits again
    again = _grads_np(learner)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    before = _per_state(learner)
    assert before[0].tobytes() == prio.tobytes(), 'a gradient writes no priority'

    # ---- |delta| itself: with alpha 1 and an eps far below half an ulp of every |delta| here, powf(|delta| + eps, 1) IS the |delta| the
    # gradient left in the workspace (the weights do not enter it), so a second handle's leaves show it
    net1, probe = _learner(c, max(B, MAX_BATCH), per=dict(PER, alpha=1.0, eps=1e-30))
    _set_priorities(probe, rp, prio)
    probe.grad(rp, idx_t)
    probe.per_commit(rp, idx_t)
    t, e, s = idx[:, 0], idx[:, 1], idx[:, 2]
    ad = _per_state(probe)[0][t, e, s]
    probe.close()
    want = np.abs(d64).astype(np.float32)
    print('  |delta|: |dev - truth| at most %.3f ulp32' % (np.abs(ad.astype(np.float64) - want) / ft.ulp32(want)).max())
    assert (np.abs(ad.astype(np.float64) - want) <= ft.ulp32(want)).all()

    # ---- the commit of those rows.  A leaf is DEFINED in float32, dqn_per_priority(ad, eps, alpha) = powf(ad + eps, alpha) of the fp32
    # |delta| checked above: two roundings and a powf of up to an ulp each, so the float64 power of the float64 delta is up to two
    # ulp32 away from a RIGHT leaf (printed, not asserted).  What a commit must write is committed(ad, eps, alpha, float32), the
    # definition in numpy float32 on the device's own |delta|: within 1 ulp32 (two powf implementations).
    learner.per_commit(rp, idx_t)
    after = _per_state(learner)
    q64 = fp.committed(d64, PER['eps'], PER['alpha'], np.float64)
    q32 = fp.committed(ad, PER['eps'], PER['alpha'], np.float32).astype(np.float64)
    print('  commit: |dev - float64 power of the truth\'s delta| at most %.3f ulp32' % (np.abs(after[0][t, e, s].astype(np.float64) - q64) / ft.ulp32(q64)).max())
    err = np.abs(after[0][t, e, s].astype(np.float64) - q32) / ft.ulp32(q32)
    print('  commit: |dev - committed(|delta|, float32)| at most %.3f ulp32' % err.max())
    assert (err <= 1).all(), err.max()
    touched = np.zeros(prio.shape, bool)
    touched[t, e, s] = True
    assert after[0][~touched].tobytes() == before[0][~touched].tobytes(), 'a leaf no row names was written'
    want_pmax = np.maximum(before[3], after[0][touched].max()).astype(np.float32)
    assert after[3].tobytes() == want_pmax.tobytes(), 'pmax is the bitwise max of what was written'
    e_touched = touched.any(2)
    assert after[1][~e_touched].tobytes() == before[1][~e_touched].tobytes() and after[2][~e_touched.any(1)].tobytes() == before[2][~e_touched.any(1)].tobytes()
    want_esum, want_ssum = fp.sums(after[0])
    assert after[1].tobytes() == want_esum.tobytes() and after[2].tobytes() == want_ssum.tobytes(), 'the touched sums are THE sums of what stands below'
    learner.per_rebuild()
    rebuilt = _per_state(learner)
    assert rebuilt[1].tobytes() == after[1].tobytes() and rebuilt[2].tobytes() == after[2].tobytes(), 'commit and rebuild sum in the same order'
    learner.close()


# ------------------------------------------------------------------------------------------------------------ 3. sums over a run
def test_sums_after_updates_wraps_and_fills_equal_a_rebuild():
    """six env-steps on a full ring (fill of the slot written, the ring moves on, two updates): then esum and ssum are what a rebuild
    writes, bit for bit, pmax bounds every leaf, and every leaf is positive"""
    c = _case(fn.SHAPES[2])
    T, N, S = c['obs'].shape[:3]
    net, learner = _learner(c, MAX_BATCH, per=dict(PER, beta_steps=6))
    rp = _device_ring(c, sentinels=False)
    learner.attach(rp)
    first = _per_state(learner)
    assert (first[0] == 1).all() and (first[1] == S).all() and (first[2] == N * S).all() and (first[3] == 1).all()
    for _ in range(T + 2):
        learner.per_fill(rp.head)
        rp.head = (rp.head + 1) % T
        learner.update(rp, updates=2)
    assert learner.n_updates == 2 * (T + 2)
    prio, esum, ssum, pmax = _per_state(learner)
    assert np.isfinite(prio).all() and (prio > 0).all() and (prio <= pmax[0]).all() and pmax[0] >= 1
    assert len(np.unique(prio)) > 20, 'the commits wrote nothing'
    want_esum, want_ssum = fp.sums(prio)
    assert esum.tobytes() == want_esum.tobytes() and ssum.tobytes() == want_ssum.tobytes()
    learner.per_rebuild()
    again = _per_state(learner)
    assert again[1].tobytes() == esum.tobytes() and again[2].tobytes() == ssum.tobytes()
    learner.close()


# ------------------------------------------------------------------------------------------------- 4. the loop of single calls
def test_update_is_the_loop_of_single_calls():
    """rs_mplight_dqn_update(n_updates = 3) against sample (keyed by the steps so far), grad, step, commit, three times, from the same
    state; beta moves from 0.4 to 1 over the three (beta_steps 2)"""
    shape = fn.SHAPES[2]
    c = _case(shape)
    T, N, S = c['obs'].shape[:3]
    rp = _device_ring(c, sentinels=False)
    prio = fp.priorities(T, N, S, c['head'], c['count'])

    def run(fused):
        net, learner = _learner(c, 21, per=dict(PER, beta_steps=2))
        _set_priorities(learner, rp, prio)
        if fused:
            learner.update(rp, updates=3)
        else:
            for _ in range(3):
                idx = learner.sample(rp)
                learner.grad(rp, idx)
                learner.step()
                learner.per_commit(rp, idx)
        assert learner.n_updates == 3
        out = _state_np(learner) + _per_state(learner)
        learner.close()
        return out

    one, loop, again = run(True), run(False), run(True)
    for other in (loop, again):
        for a, b in zip(one, other):
            assert a.tobytes() == b.tobytes()
    assert all(np.isfinite(a).all() for a in one)
    from resco_amd.agents.mplight import pack_mplight_weights
    assert np.abs(one[0] - pack_mplight_weights(c['net']).numpy()).max() > 1e-4
    assert one[5].tobytes() != prio.tobytes(), 'the update committed no priority'


# ------------------------------------------------------------------------------------------------------------- 5. off is off
@pytest.mark.parametrize('options', [(1, 0), (3, 1)])
def test_off_gives_the_bytes_of_a_handle_never_touched(options):
    shape = fn.SHAPES[2]
    c = _case(shape)
    T, N, S = c['obs'].shape[:3]
    idx = torch.from_numpy(fn.reference(*shape)[0]).cuda()
    rp = _device_ring(c, sentinels=False)
    L = load_library()
    prio = torch.from_numpy(np.array(fp.priorities(T, N, S, c['head'], c['count']))).cuda()
    esum, ssum, pmax = torch.zeros(T, N, device='cuda'), torch.zeros(T, device='cuda'), torch.ones(1, device='cuda')
    per = MPLightPer(prio.data_ptr(), esum.data_ptr(), ssum.data_ptr(), pmax.data_ptr(), T, N, S, 0.6, 0.4, 1e-6, 0)

    def run(calls):
        net, learner = _learner(c, len(idx), per=None, n_step=options[0], double_q=bool(options[1]))
        for on in calls:
            assert L.rs_mplight_dqn_set_priorities(learner._h, C.byref(per) if on else None) == 0
            if on:
                assert L.rs_mplight_dqn_per_rebuild(learner._h, None) == 0
        drawn = learner.sample(rp, update_key=5).cpu().numpy().copy()
        learner.grad(rp, idx)
        out = (drawn,) + _state_np(learner)[3:]
        learner.update(rp, updates=2)
        out += _state_np(learner)
        learner.close()
        return out

    plain, never, back, on = run(()), run(()), run((True, False)), run((True,))
    for other in (never, back):
        for a, b in zip(plain, other):
            assert a.tobytes() == b.tobytes()
    assert np.array_equal(plain[0], ft.predict_sample(SEED, 5, T, N, S, c['head'], c['count'], len(idx)))
    assert plain[0].tobytes() != on[0].tobytes() and plain[1].tobytes() != on[1].tobytes() and plain[3].tobytes() != on[3].tobytes()


# ------------------------------------------------------------------------------------------------------------ 6. the refusals
def test_refusals():
    T, N, S = 6, 5, 3
    c = _case(fn.SHAPES[0])
    net, learner = _learner(c, MAX_BATCH, S=S, per=None, options=False)
    L, h = load_library(), learner._h
    rp = MPLightReplay(T, N, S, 13, device='cuda')
    rp.head, rp.count = 4, 4
    prio, esum, ssum, pmax = torch.ones(T, N, S, device='cuda'), torch.zeros(T, N, device='cuda'), torch.zeros(T, device='cuda'), torch.ones(1, device='cuda')
    host = np.ones(1, np.float32)
    idx = torch.zeros(MAX_BATCH, 3, dtype=torch.int32, device='cuda')
    out, on = MPLightPer(), C.c_int32(-1)

    def state():
        assert L.rs_mplight_dqn_get_priorities(h, C.byref(out), C.byref(on)) == 0
        return on.value

    def arrays():
        torch.cuda.synchronize()
        return b''.join(x.cpu().numpy().tobytes() for x in (prio, esum, ssum, pmax))

    def per(**kw):
        d = dict(prio=prio.data_ptr(), esum=esum.data_ptr(), ssum=ssum.data_ptr(), pmax=pmax.data_ptr(), capacity=T, n_envs=N, n_signals=S, alpha=0.6,
                 beta0=0.4, eps=1e-6, beta_steps=0)
        d.update(kw)
        return MPLightPer(*[d[k] for k, _ in MPLightPer._fields_])

    assert state() == 0
    untouched = arrays()
    ring = learner._ring(rp)
    # while off: nothing of prioritised replay runs
    for call, name in ((lambda: L.rs_mplight_dqn_per_rebuild(h, None), b'rs_mplight_dqn_per_rebuild'), (lambda: L.rs_mplight_dqn_per_fill(h, 0, None), b'rs_mplight_dqn_per_fill'),
                       (lambda: L.rs_mplight_dqn_per_commit(h, C.byref(ring), idx.data_ptr(), 7, None), b'rs_mplight_dqn_per_commit')):
        assert call() == RS_EINVAL and L.rs_last_error(None).startswith(name) and b'off' in L.rs_last_error(None)
    for bad, word in ((dict(prio=None), b'NULL'), (dict(esum=None), b'NULL'), (dict(ssum=None), b'NULL'), (dict(pmax=None), b'NULL'),
                      (dict(pmax=host.ctypes.data), b'device'), (dict(alpha=1.5), b'alpha'), (dict(alpha=-0.1), b'alpha'), (dict(beta0=1.01), b'beta0'),
                      (dict(beta0=-1.0), b'beta0'), (dict(eps=0.0), b'eps'), (dict(eps=-1e-6), b'eps'), (dict(beta_steps=-1), b'beta_steps'),
                      (dict(capacity=1), b'capacity'), (dict(n_envs=0), b'n_envs'), (dict(n_signals=S + 1), b'n_signals')):
        assert L.rs_mplight_dqn_set_priorities(h, C.byref(per(**bad))) == RS_EINVAL, bad
        assert L.rs_last_error(None).startswith(b'rs_mplight_dqn_set_priorities') and word in L.rs_last_error(None), (bad, L.rs_last_error(None))
        assert state() == 0, 'a refused call leaves the handle as it was'
    assert L.rs_mplight_dqn_set_priorities(None, C.byref(per())) == RS_EINVAL and L.rs_mplight_dqn_get_priorities(h, None, C.byref(on)) == RS_EINVAL
    assert L.rs_mplight_dqn_set_priorities(h, C.byref(per(alpha=1.0, beta0=0.0, beta_steps=9))) == 0 and state() == 1
    assert (out.capacity, out.n_envs, out.n_signals, out.alpha, out.beta0, out.eps, out.beta_steps, out.prio, out.esum) == \
        (T, N, S, 1.0, 0.0, 1e-6, 9, prio.data_ptr(), esum.data_ptr())
    assert L.rs_mplight_dqn_set_priorities(h, C.byref(per(alpha=2.0))) == RS_EINVAL and state() == 1 and out.alpha == 1.0
    # a ring of other sizes than the priorities', at every call that takes one
    for T2, N2 in ((T + 1, N), (T, N + 1)):
        other = MPLightReplay(T2, N2, S, 13, device='cuda')
        other.head, other.count = 3, 3
        r2 = FusedMPLightLearner._ring(learner, other)
        for call in (lambda: L.rs_mplight_dqn_sample(h, C.byref(r2), 7, SEED, 0, idx.data_ptr(), None),
                     lambda: L.rs_mplight_dqn_grad(h, C.byref(r2), idx.data_ptr(), 7, None, None),
                     lambda: L.rs_mplight_dqn_update(h, C.byref(r2), 7, SEED, 1, None, None),
                     lambda: L.rs_mplight_dqn_per_commit(h, C.byref(r2), idx.data_ptr(), 7, None)):
            assert call() == RS_EINVAL and b'priorities' in L.rs_last_error(None), L.rs_last_error(None)
    assert learner.n_updates == 0
    for slot in (-1, T):
        assert L.rs_mplight_dqn_per_fill(h, slot, None) == RS_EINVAL and b'slot' in L.rs_last_error(None)
    # a commit without a gradient: refused; nothing so far has launched anything, the arrays are what they were
    assert L.rs_mplight_dqn_per_commit(h, C.byref(ring), idx.data_ptr(), 7, None) == RS_EINVAL and b'rs_mplight_dqn_grad' in L.rs_last_error(None)
    assert arrays() == untouched and state() == 1 and out.alpha == 1.0
    # ... and with another batch than the gradient's
    rp.obs.zero_()
    assert L.rs_mplight_dqn_per_rebuild(h, None) == 0
    assert L.rs_mplight_dqn_grad(h, C.byref(ring), idx.data_ptr(), 7, None, None) == 0
    assert L.rs_mplight_dqn_per_commit(h, C.byref(ring), idx.data_ptr(), 8, None) == RS_EINVAL
    assert L.rs_mplight_dqn_per_commit(h, C.byref(ring), None, 7, None) == RS_EINVAL
    assert L.rs_mplight_dqn_per_commit(h, C.byref(ring), idx.data_ptr(), 7, None) == 0
    assert L.rs_mplight_dqn_set_priorities(h, None) == 0 and state() == 0
    torch.cuda.synchronize()
    learner.close()
    # a checkpoint with the ring before the learner has seen its replay: told what to do, on the way out and on the way in
    fresh, seen = _learner(c, MAX_BATCH, S=S)[1], _learner(c, MAX_BATCH, S=S)[1]
    seen.attach(rp)
    with pytest.raises(RuntimeError, match=r'attach\(replay\)'):
        fresh.state_dict()
    with pytest.raises(RuntimeError, match=r'attach\(replay\)'):
        fresh.load_state_dict(seen.state_dict())
    assert 'per' not in fresh.state_dict(replay=False)['state']
    with pytest.raises(ValueError, match='sized for a ring'):
        seen.attach(MPLightReplay(T + 1, N, S, 13, device='cuda'))
    fresh.close()
    seen.close()


# ----------------------------------------------------------------------------------------------------------- 7. the library loop
# cologne1 x 8 environments, a ring of 8 slots (it wraps), batch 16, target_update 5, two episodes of 12 env-steps
N_ENVS, CAPACITY, BATCH, TARGET_UPDATE, STEPS, DECAY = 8, 8, 16, 5, 12, 20
LOOP_PER = dict(alpha=0.6, beta0=0.4, beta_steps=16, eps=1e-6)


def _loop_objects(pipes, per=LOOP_PER):
    pe = PipedEnvs('cologne1', N_ENVS, pipes, states=('mplight',), rewards=('pressure',), seed=0, outputs=('mplight',))
    for e in pe.envs:
        e.horizon_steps = STEPS                 # short episodes
    net = frap_from_scenario(pe.scenario, 1).cuda()
    net.init_like_reference(0)
    learner = FusedMPLightLearner(net, gamma=0.99, lr=1e-3, target_update=TARGET_UPDATE, batch_size=BATCH, seed=0, n_signals=pe.n_signals, n_step=3,
                                  double_q=True, per=per)
    policy = FusedMPLight(net, pe.scenario, seed=7)
    policy.share_weights(learner.flat)
    replay = MPLightReplay(CAPACITY, N_ENVS, pe.n_signals, 13, device='cuda')
    learner.attach(replay)
    return pe, dict(net=net, learner=learner, policy=policy, replay=replay)


def _loop_state(o):
    torch.cuda.synchronize()
    L, R = o['learner'], o['replay']
    out = {'par': L.flat, 'tgt': L.flat_target, 'm': L._m, 'v': L._v, 'ring.obs': R.obs, 'ring.act': R.act, 'ring.rew': R.rew, 'ring.done': R.done,
           'per.prio': L.prio, 'per.esum': L.esum, 'per.ssum': L.ssum, 'per.pmax': L.pmax}
    out = {k: t.detach().cpu().numpy().tobytes() for k, t in out.items()}
    out['scalars'] = (L.t, L.n_updates, R.head, R.count)
    return out


def _library_episode(pe, trainer, ep):
    pe.set_seed(1000 + ep)
    pe.reset()
    assert trainer.run(STEPS, None)


@pytest.mark.parametrize('pipes', [1, 2])
def test_library_loop_equals_the_python_loop_and_resumes(tmp_path, pipes):
    # the Python-driven loop of tools/train_pipes_ab.py: train_piped, two episodes
    pe, A = _loop_objects(pipes)
    L, P, R = A['learner'], A['policy'], A['replay']
    order = torch.as_tensor(P.order, dtype=torch.long, device='cuda')
    for ep in range(2):
        pe.set_seed(1000 + ep)
        pe.reset()
        for _ in range(STEPS):
            R.stage(pe.cat('mplight'))
            done = pe.step('mplight', P, linear_epsilon(L.t, 1.0, 0.0, DECAY), L.t)
            R.commit(pair_of_action(order, pe.cat('actions')), pe.cat('pressure').float(), done)
            L.observe_step(R)
        assert done
    want = _loop_state(A)
    prio = np.frombuffer(want['per.prio'], np.float32)
    assert want['scalars'][0] == 2 * STEPS and want['scalars'][1] > STEPS and want['scalars'][2:] == (2 * STEPS % CAPACITY, CAPACITY)
    assert (prio > 0).all() and len(np.unique(prio)) > 20 and np.frombuffer(want['per.pmax'], np.float32)[0] >= 1
    L.close()
    pe.close()

    # the same steps in one rs_group_train call per episode; a checkpoint with the ring between the episodes
    pe, B = _loop_objects(pipes)
    trainer = DeviceTrainer(pe, B['learner'], B['policy'], B['replay'], 1.0, 0.0, DECAY)
    _library_episode(pe, trainer, 0)
    path = str(tmp_path / 'a.pt')
    checkpoint.save(path, agent='MPLight', map_name='cologne1', objects=B, progress={})
    _library_episode(pe, trainer, 1)
    got = _loop_state(B)
    assert got['scalars'] == want['scalars']
    for k in want:
        assert got[k] == want[k], k

    # the checkpoint loaded into fresh objects and continued: the bits of the uninterrupted run
    ck = torch.load(path, weights_only=True)
    assert ck['signature']['fields']['learner.per_alpha'] == 0.6 and ck['signature']['fields']['learner.per_beta_steps'] == 16
    assert sorted(ck['objects']['learner']['state']['per']) == ['pmax', 'prio'], 'the sums are rebuilt, not stored'
    pe2, Cc = _loop_objects(pipes)
    checkpoint.load(path, agent='MPLight', map_name='cologne1', objects=Cc)
    _library_episode(pe2, DeviceTrainer(pe2, Cc['learner'], Cc['policy'], Cc['replay'], 1.0, 0.0, DECAY), 1)
    resumed = _loop_state(Cc)
    for k in want:
        assert resumed[k] == want[k], k
    if pipes == 1:
        # without the ring the priorities are not in the file; a learner without the option is refused, and the other way round
        checkpoint.save(path, agent='MPLight', map_name='cologne1', objects=B, progress={}, replay=False)
        assert 'per' not in torch.load(path, weights_only=True)['objects']['learner']['state']
        checkpoint.load(path, agent='MPLight', map_name='cologne1', objects=Cc)
        assert (Cc['learner'].prio == 1).all() and (Cc['learner'].pmax == 1).all() and len(Cc['replay']) == 0
        pe3, Dd = _loop_objects(pipes, per=None)
        with pytest.raises(ValueError, match=r'learner\.per_'):
            checkpoint.load(path, agent='MPLight', map_name='cologne1', objects=Dd)
        checkpoint.save(path, agent='MPLight', map_name='cologne1', objects=Dd, progress={}, replay=False)
        with pytest.raises(ValueError, match=r'learner\.per_'):
            checkpoint.load(path, agent='MPLight', map_name='cologne1', objects=Cc)
        Dd['learner'].close()
        pe3.close()
    for x in (B['learner'], Cc['learner']):
        x.close()
    for e in (pe, pe2):
        e.close()
