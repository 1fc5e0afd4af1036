"""GPU: prioritised experience replay in the fused DQN update (rs_dqn_set_priorities / rs_dqn_per_rebuild / rs_dqn_per_fill /
rs_dqn_per_commit of include/resco_sim.h; resco_amd/csrc/resco_dqn_per.h; FusedDQNLearner(per=...)).  The draw against float64
cumulative sums of the device's own priorities, every draw checked; the weighted minibatch gradient against float64 autograd
(tests/dqn_per_ref.py: truth = float64, e_ref = float32 against it, the device gets 4 e_ref per tensor and on the loss); what a commit
writes and what it leaves; the sums against a rebuild, bit for bit; rs_dqn_update against its pieces; off against a handle never
touched; the refusals; the library's training loop against the Python-driven one on one and two pipes, and a checkpoint of it.

The three-signal nets of tests/dqn_train_ref.py on rings of 6 and 8 slots x 5 environments (less than a wave, odd) and 130 (two full
strides of a wave and a ragged third), batches of 7 and of max_batch, before and after the wrap and not yet full."""
import ctypes as C

import numpy as np
import pytest
import torch

from dqn_nstep_ref import NAMES, ring_case, valid_slots
from dqn_per_ref import PER, committed, priorities, reference, uniforms
from dqn_train_ref import check_sample, predict_sample
from resco_amd import checkpoint
from resco_amd.agents.idqn_fused import FusedIDQN
from resco_amd.agents.idqn_learn import DeviceReplay, linear_epsilon
from resco_amd.agents.idqn_learn_fused import FusedDQNLearner
from resco_amd.agents.idqn_rollout import BatchedIDQN
from resco_amd.agents.train_fused import DeviceTrainer
from resco_amd.sim import DQNPer, load_library
from tools.train_pipes_ab import PipedEnvs
from train_ref import _device_net, _np, _ulp, check_4_e_ref, compare_gradients

pytestmark = pytest.mark.gpu

RS_EINVAL = -1
SEED = 0x5EED
MAX_BATCH = 33
#         T  N    head count
RINGS = [(6, 5, 4, 4),          # not full: slots 4 and 5 were never written
         (6, 5, 2, 6),          # full and wrapped
         (8, 130, 3, 8),
         (8, 130, 0, 8),        # full, head at 0: the newest slot is the last
         (6, 130, 3, 3)]
#          lmax T  N    B   head count n dq     done at
SHAPES = [(9, 8, 130, 96, 3, 8, 1, False, (5,)),
          (9, 8, 130, 96, 3, 8, 3, True, (5,)),
          (9, 8, 130, 96, 3, 8, 3, False, (5,)),
          (9, 8, 130, 96, 3, 8, 1, True, (5,)),
          (5, 6, 5, 7, 4, 4, 1, False, ()),         # not full, a batch of 7 below max_batch
          (5, 6, 5, 33, 2, 6, 3, True, (0,))]       # wrapped, fewer cells than rows: rows repeat


def _learner(c, B, per=PER, **kw):
    """a FusedDQNLearner on a device copy of the case's network, its target network the case's"""
    net = _device_net(c['net'])
    learner = FusedDQNLearner(net, batch_size=B, seed=SEED, per=per, **kw)
    with torch.no_grad():
        for k in NAMES:
            getattr(learner.target, k).copy_(getattr(c['target'], k))
    return net, learner


def _device_ring(c, head, count, sentinels=True):
    """the case's ring on the device at (head, count).  sentinels: NaN observations, NaN rewards and action -777 in every slot that
    was not written and in the reward and action of the newest slot -- one of them read, and a gradient is NaN"""
    T, N, S, lmax = c['obs'].shape[:4]
    rp = DeviceReplay(T, N, S, lmax, device='cuda')
    rp.obs.copy_(torch.from_numpy(c['obs']))
    rp.act.copy_(torch.from_numpy(c['act']))
    rp.rew.copy_(torch.from_numpy(c['rew']))
    rp.done.copy_(torch.from_numpy(c['done']))
    if sentinels:
        newest = (head - 1) % T
        lost = [t for t in range(T) if t not in valid_slots(T, head, count) + [newest]]
        rp.obs[lost] = float('nan')
        rp.act[lost + [newest]] = -777
        rp.rew[lost + [newest]] = float('nan')
    rp.head, rp.count = head, count
    return rp


def _set_priorities(learner, rp, prio):
    """the learner's priorities <- prio [T, N, S], its sums rebuilt"""
    learner.attach(rp)
    learner.prio.copy_(torch.from_numpy(np.array(prio)))
    learner.rebuild_priorities()
    torch.cuda.synchronize()


def _per_state(learner):
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy().copy() for x in (learner.prio, learner.ssum, learner.pmax))


# ---------------------------------------------------------------------------------------------------------------- 1. the draw
@pytest.mark.parametrize('B', [7, MAX_BATCH])
@pytest.mark.parametrize('T,N,head,count', RINGS)
def test_the_draw(T, N, head, count, B):
    c = ring_case(2, 3, 5, ())
    net, learner = _learner(c, MAX_BATCH)
    rp = DeviceReplay(T, N, 3, 2, device='cuda')            # (the draw reads nothing of the ring itself)
    rp.head, rp.count = head, count
    prio = priorities(T, N, head, count)
    _set_priorities(learner, rp, prio)
    got_prio, ssum, _ = _per_state(learner)
    assert got_prio.tobytes() == prio.tobytes()
    sums64 = prio.sum(1, dtype=np.float64)
    assert (np.abs(ssum - sums64) <= N * 2.0 ** -24 * sums64).all() and ((ssum == 0) == (sums64 == 0)).all()
    ok = valid_slots(T, head, count)
    n_checked, slots_seen = 0, set()
    for u in (0, 1, 77):
        idx = learner.sample(rp, batch_size=B, update_key=u).cpu().numpy()
        assert idx.shape == (B, 3, 2)
        check_sample(idx, T, N, head, count)                # in the ring; neither the newest nor an unwritten slot
        assert idx.tobytes() == learner.sample(rp, batch_size=B, update_key=u).cpu().numpy().tobytes(), 'two runs, the same bits'
        r0, r1 = uniforms(SEED, u, 3, B)
        for i in range(B):
            for s in range(3):
                t, e = int(idx[i, s, 0]), int(idx[i, s, 1])
                assert t in ok and ssum[t, s] > 0 and prio[t, e, s] > 0, 'an entry of weight 0 was drawn'
                for w, k, r in ((ssum[ok, s].astype(np.float64), ok.index(t), r0[i, s]), (prio[t, :, s].astype(np.float64), e, r1[i, s])):
                    Cm = np.concatenate([[0.0], np.cumsum(w)])
                    Z = Cm[-1]
                    tol = 2 * len(w) * 2.0 ** -24 * Z
                    assert Cm[k] - tol <= r * Z <= Cm[k + 1] + tol, (u, i, s, t, e, r, Cm[k], Cm[k + 1], Z)
                n_checked += 1
                slots_seen.add((s, t))
    assert n_checked == 3 * B * 3
    if B == MAX_BATCH:          # 99 draws per signal: a slot that holds a fifth of a signal's mass is missed with probability 0.8^99
        for s in range(3):
            for t in ok:
                assert sums64[t, s] < 0.2 * sums64[ok, s].sum() or (s, t) in slots_seen, (s, t)
    # priorities off on the same handle: the uniform draw again
    assert load_library().rs_dqn_set_priorities(learner._h, None) == 0
    learner.per = None
    assert np.array_equal(learner.sample(rp, batch_size=B, update_key=1).cpu().numpy(), predict_sample(SEED, 1, 3, T, N, head, count, B))
    learner.close()


# ------------------------------------------------------------------------------------------------------ 2. the gradient, 3. the commit
@pytest.mark.parametrize('lmax,T,N,B,head,count,n_step,double_q,done_slots', SHAPES)
def test_weighted_gradient_and_commit(lmax, T, N, B, head, count, n_step, double_q, done_slots):
    c = ring_case(lmax, T, N, done_slots)
    idx, prio, g64, g32, l64, l32, d64, d32 = reference(lmax, T, N, B, head, count, n_step, double_q, done_slots, beta=PER['beta0'])
    net, learner = _learner(c, max(B, MAX_BATCH), n_step=n_step, double_q=double_q)
    rp = _device_ring(c, head, count)
    _set_priorities(learner, rp, prio)
    idx_t = torch.from_numpy(idx).cuda()
    got = _np(learner.grad(rp, idx_t))
    loss = learner.loss_out.cpu().numpy().copy()
    print('lmax %d ring %d x %d at (%d, %d), B %d, n_step %d, double_q %d' % (lmax, T, N, head, count, B, n_step, double_q))
    worst = compare_gradients(NAMES, got, g64, g32)
    check_4_e_ref('loss', loss, l64, l32, worst)         # (l32: the float32 reference in several row orders, dqn_per_ref.reference)
    print('  loss: e_ref is %.2f float32 ulp of the largest loss' % (np.abs(l32 - l64).max() / _ulp(np.abs(l64).max())))
    assert not worst, worst
    assert all(np.abs(got[k]).max() > 0 for k in NAMES)
    again = _np(learner.grad(rp, idx_t))                    # the same bits again
    for k in NAMES:
        assert got[k].tobytes() == again[k].tobytes(), k
    before = _per_state(learner)
    assert before[0].tobytes() == prio.tobytes(), 'a gradient writes no priority'

    # ---- the commit of those rows
    learner.commit_priorities(rp, idx_t)
    after = _per_state(learner)
    eps, alpha = PER['eps'], PER['alpha']
    q64, q32 = committed(d64, eps, alpha, np.float64), committed(d32, eps, alpha, np.float32).astype(np.float64)
    e_ref = np.abs(q32 - q64).max()
    t, e, s = idx[..., 0], idx[..., 1], np.arange(3)[None, :]
    err = np.abs(after[0][t, e, s].astype(np.float64) - q64)
    print('  commit: |dev - truth| %.3e  e_ref %.3e  16 ulp %.3e' % (err.max(), e_ref, 16 * _ulp(q64).max()))
    assert (err <= 4 * e_ref + 16 * _ulp(q64)).all(), (err.max(), e_ref)
    touched = np.zeros(prio.shape, bool)
    touched[t, e, np.broadcast_to(s, t.shape)] = True
    assert after[0][~touched].tobytes() == before[0][~touched].tobytes(), 'a leaf no row names was written'
    want_pmax = np.maximum(before[2], np.where(touched, after[0], 0).max((0, 1)))
    assert after[2].tobytes() == want_pmax.astype(np.float32).tobytes(), 'pmax is the bitwise max of what was written'
    slot_touched = touched.any(1)
    assert after[1][~slot_touched].tobytes() == before[1][~slot_touched].tobytes()
    learner.rebuild_priorities()
    assert _per_state(learner)[1].tobytes() == after[1].tobytes(), 'commit and rebuild sum in the same order'
    # a commit needs the gradient of that batch
    L = load_library()
    if B > 1:
        ring = learner._ring(rp)
        assert L.rs_dqn_per_commit(learner._h, C.byref(ring), idx_t.data_ptr(), B - 1, None) == RS_EINVAL
        assert b'rs_dqn_per_commit' in L.rs_last_error(None) and b'rs_dqn_grad' in L.rs_last_error(None)
    learner.close()


def test_sums_after_updates_wraps_and_fills_equal_a_rebuild():
    """five env-steps on a full ring (fill of the slot written, the ring moves on, two updates): then ssum is what a rebuild writes,
    bit for bit, pmax bounds every leaf, and every slot that was filled or committed is positive"""
    lmax, T, N = 5, 6, 5
    c = ring_case(lmax, T, N, (0,))
    net, learner = _learner(c, MAX_BATCH, per=dict(PER, beta_steps=6), n_step=3, double_q=True)
    rp = _device_ring(c, 2, 6, sentinels=False)
    learner.attach(rp)
    first = _per_state(learner)
    assert (first[0] == 1).all() and (first[1] == N).all() and (first[2] == 1).all()
    for _ in range(5):
        learner.fill_priorities(rp.head)
        rp.head = (rp.head + 1) % T
        learner.update(rp, updates=2)
    assert learner.n_updates == 10
    prio, ssum, pmax = _per_state(learner)
    assert np.isfinite(prio).all() and (prio > 0).all() and (prio <= pmax[None, None, :]).all() and (pmax >= 1).all()
    assert len(np.unique(prio)) > 20, 'the commits wrote nothing'
    learner.rebuild_priorities()
    assert _per_state(learner)[1].tobytes() == ssum.tobytes()
    assert (np.abs(ssum - prio.sum(1, dtype=np.float64)) <= N * 2.0 ** -24 * prio.sum(1, dtype=np.float64)).all()
    learner.close()


# ------------------------------------------------------------------------------------------------- 4. the loop of single calls
def test_update_is_the_loop_of_single_calls():
    """rs_dqn_update(n_updates = 3) against sample (keyed by the steps so far), grad, step, commit, three times, from the same state;
    beta moves from 0.4 to 1 over the three (beta_steps 2)"""
    lmax, T, N, _, head, count, n_step, dq, done_slots = SHAPES[1]
    c = ring_case(lmax, T, N, done_slots)
    rp = _device_ring(c, head, count, sentinels=False)
    prio = priorities(T, N, head, count, zero_slot=False)

    def run(fused):
        net, learner = _learner(c, 40, per=dict(PER, beta_steps=2), n_step=n_step, double_q=dq)
        _set_priorities(learner, rp, prio)
        if fused:
            learner.update(rp, updates=3)
        else:
            for _ in range(3):
                idx = learner.sample(rp)
                learner.grad(rp, idx)
                learner.step()
                learner.commit_priorities(rp, idx)
        assert learner.n_updates == 3
        out = (_np(net), _np(learner.m), _np(learner.v), learner.loss_out.cpu().numpy().copy()) + _per_state(learner)
        learner.close()
        return out

    one, loop, again = run(True), run(False), run(True)
    for other in (loop, again):
        for a, b in zip(one[:3], other[:3]):
            for k in NAMES:
                assert a[k].tobytes() == b[k].tobytes(), k
        for a, b in zip(one[3:], other[3:]):
            assert a.tobytes() == b.tobytes()
    assert all(np.isfinite(one[0][k]).all() for k in NAMES) and np.isfinite(one[3]).all()
    assert np.abs(one[0]['fc2_w'] - c['net'].fc2_w.detach().numpy()).max() > 1e-4
    assert one[4].tobytes() != prio.tobytes(), 'the update committed no priority'


# ------------------------------------------------------------------------------------------------------------- 5. off is off
def test_off_gives_the_bytes_of_a_handle_never_touched():
    lmax, T, N, B, head, count, n_step, dq, done_slots = SHAPES[1]
    c = ring_case(lmax, T, N, done_slots)
    idx = torch.from_numpy(reference(lmax, T, N, B, head, count, n_step, dq, done_slots, beta=PER['beta0'])[0]).cuda()
    rp = _device_ring(c, head, count)
    L = load_library()
    prio = torch.from_numpy(np.array(priorities(T, N, head, count))).cuda()
    ssum, pmax = torch.zeros(T, 3, device='cuda'), torch.ones(3, device='cuda')
    per = DQNPer(prio.data_ptr(), ssum.data_ptr(), pmax.data_ptr(), T, N, 0.6, 0.4, 1e-6, 0)

    def run(calls):
        net, learner = _learner(c, B, per=None, n_step=n_step, double_q=dq)
        for on in calls:
            assert L.rs_dqn_set_priorities(learner._h, C.byref(per) if on else None) == 0
            if on:
                assert L.rs_dqn_per_rebuild(learner._h, None) == 0
        drawn = learner.sample(rp, update_key=5).cpu().numpy().copy()
        out = (_np(learner.grad(rp, idx)), learner.loss_out.cpu().numpy().copy(), drawn)
        learner.update(rp, updates=2)
        out += (_np(net),)
        learner.close()
        return out

    plain, back, on = run(()), run((True, False)), run((True,))
    for k in NAMES:
        assert plain[0][k].tobytes() == back[0][k].tobytes() and plain[3][k].tobytes() == back[3][k].tobytes(), k
    assert plain[1].tobytes() == back[1].tobytes() and plain[2].tobytes() == back[2].tobytes()
    assert np.array_equal(plain[2], predict_sample(SEED, 5, 3, T, N, head, count, B))
    assert any(plain[0][k].tobytes() != on[0][k].tobytes() for k in NAMES) and plain[2].tobytes() != on[2].tobytes()


# ------------------------------------------------------------------------------------------------------------ 6. the refusals
def test_refusals():
    T, N = 6, 5
    c = ring_case(2, 3, 5, ())
    net, learner = _learner(c, MAX_BATCH, per=None)
    L, h = load_library(), learner._h
    rp = DeviceReplay(T, N, 3, 2, device='cuda')
    rp.head, rp.count = 4, 4
    prio, ssum, pmax = torch.ones(T, N, 3, device='cuda'), torch.zeros(T, 3, device='cuda'), torch.ones(3, device='cuda')
    host = np.ones(3, np.float32)
    idx = torch.zeros(MAX_BATCH, 3, 2, dtype=torch.int32, device='cuda')
    out, on = DQNPer(), C.c_int32(-1)

    def state():
        assert L.rs_dqn_get_priorities(h, C.byref(out), C.byref(on)) == 0
        return on.value

    def per(**kw):
        d = dict(prio=prio.data_ptr(), ssum=ssum.data_ptr(), pmax=pmax.data_ptr(), capacity=T, n_envs=N, alpha=0.6, beta0=0.4, eps=1e-6, beta_steps=0)
        d.update(kw)
        return DQNPer(*[d[k] for k, _ in DQNPer._fields_])

    assert state() == 0
    ring = learner._ring(rp)
    # while off: nothing of prioritised replay runs
    for call, name in ((lambda: L.rs_dqn_per_rebuild(h, None), b'rs_dqn_per_rebuild'), (lambda: L.rs_dqn_per_fill(h, 0, None), b'rs_dqn_per_fill'),
                       (lambda: L.rs_dqn_per_commit(h, C.byref(ring), idx.data_ptr(), 7, None), b'rs_dqn_per_commit')):
        assert call() == RS_EINVAL and L.rs_last_error(None).startswith(name) and b'off' in L.rs_last_error(None)
    for bad, word in ((dict(prio=None), b'NULL'), (dict(ssum=None), b'NULL'), (dict(pmax=None), b'NULL'), (dict(pmax=host.ctypes.data), b'device'),
                      (dict(alpha=1.5), b'alpha'), (dict(alpha=-0.1), b'alpha'), (dict(beta0=1.01), b'beta0'), (dict(beta0=-1.0), b'beta0'),
                      (dict(eps=0.0), b'eps'), (dict(eps=-1e-6), b'eps'), (dict(beta_steps=-1), b'beta_steps'), (dict(capacity=1), b'capacity'),
                      (dict(n_envs=0), b'n_envs')):
        assert L.rs_dqn_set_priorities(h, C.byref(per(**bad))) == RS_EINVAL, bad
        assert L.rs_last_error(None).startswith(b'rs_dqn_set_priorities') and word in L.rs_last_error(None), (bad, L.rs_last_error(None))
        assert state() == 0, 'a refused call leaves the handle as it was'
    assert L.rs_dqn_set_priorities(None, C.byref(per())) == RS_EINVAL and L.rs_dqn_get_priorities(h, None, C.byref(on)) == RS_EINVAL
    assert L.rs_dqn_set_priorities(h, C.byref(per(alpha=1.0, beta0=0.0, beta_steps=9))) == 0 and state() == 1
    assert (out.capacity, out.n_envs, out.alpha, out.beta0, out.eps, out.beta_steps, out.prio) == (T, N, 1.0, 0.0, 1e-6, 9, prio.data_ptr())
    assert L.rs_dqn_set_priorities(h, C.byref(per(alpha=2.0))) == RS_EINVAL and state() == 1 and out.alpha == 1.0
    # a ring of other sizes than the priorities', at every call that takes one
    for T2, N2 in ((T + 1, N), (T, N + 1)):
        other = DeviceReplay(T2, N2, 3, 2, device='cuda')
        other.head, other.count = 3, 3
        r2 = FusedDQNLearner._ring(learner, other)
        for call in (lambda: L.rs_dqn_sample(h, C.byref(r2), 7, SEED, 0, idx.data_ptr(), None), lambda: L.rs_dqn_grad(h, C.byref(r2), idx.data_ptr(), 7, None, None),
                     lambda: L.rs_dqn_update(h, C.byref(r2), 7, SEED, 1, None, None), lambda: L.rs_dqn_per_commit(h, C.byref(r2), idx.data_ptr(), 7, None)):
            assert call() == RS_EINVAL and b'priorities' in L.rs_last_error(None), L.rs_last_error(None)
    assert learner.n_updates == 0
    for slot in (-1, T):
        assert L.rs_dqn_per_fill(h, slot, None) == RS_EINVAL and b'slot' in L.rs_last_error(None)
    # a commit without a gradient, and with another batch than the gradient's
    assert L.rs_dqn_per_commit(h, C.byref(ring), idx.data_ptr(), 7, None) == RS_EINVAL and b'rs_dqn_grad' in L.rs_last_error(None)
    assert L.rs_dqn_per_rebuild(h, None) == 0
    assert L.rs_dqn_grad(h, C.byref(ring), idx.data_ptr(), 7, None, None) == 0
    assert L.rs_dqn_per_commit(h, C.byref(ring), idx.data_ptr(), 8, None) == RS_EINVAL
    assert L.rs_dqn_per_commit(h, C.byref(ring), None, 7, None) == RS_EINVAL
    assert L.rs_dqn_per_commit(h, C.byref(ring), idx.data_ptr(), 7, None) == 0
    assert L.rs_dqn_set_priorities(h, None) == 0 and state() == 0
    torch.cuda.synchronize()
    learner.close()
    with pytest.raises(ValueError, match='alpha'):
        FusedDQNLearner(_device_net(c['net']), per=dict(alpha=2))
    # a checkpoint with the ring before the learner has seen its replay: told what to do, on the way out and on the way in
    fresh, seen = _learner(c, MAX_BATCH)[1], _learner(c, MAX_BATCH)[1]
    seen.attach(rp)
    with pytest.raises(RuntimeError, match=r'attach\(replay\)'):
        fresh.state_dict()
    with pytest.raises(RuntimeError, match=r'attach\(replay\)'):
        fresh.load_state_dict(seen.state_dict())
    assert 'per' not in fresh.state_dict(replay=False)['state']
    fresh.close()
    seen.close()


# ----------------------------------------------------------------------------------------------------------- 7. the library loop
# cologne1 x 8 environments, a ring of 8 slots (it wraps), batch 16, target_update 5, 12 env-steps
N_ENVS, CAPACITY, BATCH, TARGET_UPDATE, STEPS, DECAY = 8, 8, 16, 5, 12, 10
LOOP_PER = dict(alpha=0.6, beta0=0.4, beta_steps=8, eps=1e-6)


def _loop_objects(pipes):
    pe = PipedEnvs('cologne1', N_ENVS, pipes, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
    net = BatchedIDQN.from_scenario(pe.scenario, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=0)
    learner = FusedDQNLearner(net, gamma=0.99, lr=1e-3, target_update=TARGET_UPDATE, batch_size=BATCH, seed=0, n_step=3, double_q=True, per=LOOP_PER)
    policy = FusedIDQN(net, seed=7)
    replay = DeviceReplay(CAPACITY, N_ENVS, pe.n_signals, net.lmax, device='cuda')
    learner.attach(replay)
    return pe, dict(net=net, learner=learner, policy=policy, replay=replay)


def _loop_state(o):
    torch.cuda.synchronize()
    L = o['learner']
    out = {'par.' + k: getattr(o['net'], k) for k in NAMES}
    out.update({'tgt.' + k: getattr(L.target, k) for k in NAMES})
    out.update({'m.' + k: L.m[k] for k in NAMES})
    out.update({'v.' + k: L.v[k] for k in NAMES})
    out.update({'ring.obs': o['replay'].obs, 'ring.act': o['replay'].act, 'ring.rew': o['replay'].rew, 'ring.done': o['replay'].done})
    out.update({'per.prio': L.prio, 'per.ssum': L.ssum, 'per.pmax': L.pmax})
    out = {k: t.detach().cpu().numpy().tobytes() for k, t in out.items()}
    out['scalars'] = (L.t, L.n_updates, o['replay'].head, o['replay'].count)
    return out


@pytest.mark.parametrize('pipes', [1, 2])
def test_library_loop_equals_the_python_loop_and_resumes(tmp_path, pipes):
    # the Python-driven loop of tools/train_pipes_ab.py: train_piped
    pe, A = _loop_objects(pipes)
    L, P, R = A['learner'], A['policy'], A['replay']
    pe.set_seed(1000)
    pe.reset()
    for _ in range(STEPS):
        R.stage(pe.cat('drq_norm_f16'))
        done = pe.step('idqn', P, linear_epsilon(L.t, 1.0, 0.0, DECAY), L.t)
        R.commit(pe.cat('actions'), pe.cat('wait_norm').float(), done)
        if L.observe_step(R) is not None:
            P.refresh_on_device()
    want = _loop_state(A)
    prio = np.frombuffer(want['per.prio'], np.float32)
    assert want['scalars'] == (STEPS, STEPS - 2, STEPS % CAPACITY, CAPACITY)
    assert (prio > 0).all() and len(np.unique(prio)) > 20 and np.frombuffer(want['per.pmax'], np.float32).min() >= 1
    L.close()
    pe.close()

    # the same steps in one rs_group_train call
    pe, B = _loop_objects(pipes)
    trainer = DeviceTrainer(pe, B['learner'], B['policy'], B['replay'], 1.0, 0.0, DECAY)
    pe.set_seed(1000)
    pe.reset()
    trainer.run(STEPS, None)
    got = _loop_state(B)
    assert got['scalars'] == want['scalars']
    for k in want:
        assert got[k] == want[k], k

    if pipes == 1:
        # a checkpoint of it with the ring, loaded into fresh objects: the same bits, and the same bits after one more update
        path = str(tmp_path / 'a.pt')
        checkpoint.save(path, agent='IDQN', map_name='cologne1', objects=B, progress={})
        ck = torch.load(path, weights_only=True)
        assert ck['signature']['fields']['learner.per_alpha'] == 0.6 and ck['signature']['fields']['learner.per_beta_steps'] == 8
        assert sorted(ck['objects']['learner']['state']['per']) == ['pmax', 'prio'], 'ssum is rebuilt, not stored'
        pe2, Cc = _loop_objects(pipes)
        checkpoint.load(path, agent='IDQN', map_name='cologne1', objects=Cc)
        resumed = _loop_state(Cc)
        for k in want:
            assert resumed[k] == want[k], k
        B['learner'].update(B['replay'])
        Cc['learner'].update(Cc['replay'])
        one, two = _loop_state(B), _loop_state(Cc)
        for k in one:
            assert one[k] == two[k], k
        assert one['par.fc2_w'] != want['par.fc2_w'] and one['per.prio'] != want['per.prio']
        # without the ring the priorities are not in the file, and a learner without the option is refused
        checkpoint.save(path, agent='IDQN', map_name='cologne1', objects=B, progress={}, replay=False)
        assert 'per' not in torch.load(path, weights_only=True)['objects']['learner']['state']
        checkpoint.load(path, agent='IDQN', map_name='cologne1', objects=Cc)
        assert (Cc['learner'].prio == 0).all() and (Cc['learner'].pmax == 1).all() and len(Cc['replay']) == 0
        plain = FusedDQNLearner(Cc['net'], target_update=TARGET_UPDATE, batch_size=BATCH, n_step=3, double_q=True)
        with pytest.raises(ValueError, match=r'learner\.per_'):
            checkpoint.load(path, agent='IDQN', map_name='cologne1', objects=dict(Cc, learner=plain))
        for x in (Cc['learner'], plain):
            x.close()
        pe2.close()
    B['learner'].close()
    pe.close()
