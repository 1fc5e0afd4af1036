"""GPU: the target's options of the fused DQN update (rs_dqn_set_target: n-step returns, Double DQN; dqn_target_opt_kernel of
resco_amd/csrc/resco_dqn_train.h; FusedDQNLearner(n_step, double_q)).  A minibatch gradient against float64 autograd of the definition
(tests/dqn_nstep_ref.py: truth = float64, e_ref = float32 against it, the device gets 4 e_ref per tensor and on the loss); what the
walk may read of the ring; the options off against a handle never touched; rs_dqn_update against its pieces; the draw; the refusals;
the library's training loop against the Python-driven one, and a checkpoint of it.

Every ring is a DeviceReplay with three sentinel environments past the case's N; they, every unwritten slot, every slot a test
declares unreadable, and the reward and action of the newest slot hold NaN observations / NaN rewards / action -777: one of them
read, and a gradient is NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from dqn_nstep_ref import NAMES, reference, ring_case, valid_slots
from dqn_train_ref import predict_sample
from resco_amd import checkpoint
from resco_amd.agents.idqn_fused import FusedIDQN
from resco_amd.agents.idqn_learn import DeviceReplay, linear_epsilon
from resco_amd.agents.idqn_learn_fused import FusedDQNLearner
from resco_amd.agents.idqn_rollout import BatchedIDQN
from resco_amd.agents.train_fused import DeviceTrainer
from resco_amd.multi_signal import VecMultiSignal
from resco_amd.sim import load_library
from train_ref import _device_net, _np, check_4_e_ref, compare_gradients

pytestmark = pytest.mark.gpu

RS_EINVAL = -1
PAD_ENVS = 3
SEED = 0x5EED
#          lmax T  N   B  head count n dq     done at
SHAPES = [(2, 3, 5, 33, 0, 3, 2, True, ()),         # the smallest ring
          (9, 8, 9, 96, 3, 8, 3, False, (5,)),
          (9, 8, 9, 96, 3, 8, 3, True, (5,)),
          (9, 8, 9, 96, 3, 8, 1, True, (5,)),
          (17, 8, 11, 70, 6, 6, 5, True, ())]       # not full: slots 6 and 7 were never written


def _learner(c, B, **kw):
    """a FusedDQNLearner on a device copy of the case's network, its target network the case's"""
    net = _device_net(c['net'])
    learner = FusedDQNLearner(net, batch_size=B, seed=SEED, **kw)
    with torch.no_grad():
        for k in NAMES:
            getattr(learner.target, k).copy_(getattr(c['target'], k))
    return net, learner


def _device_ring(c, head, count, unreadable=(), pad=PAD_ENVS):
    """the case's ring on the device at (head, count): sentinels in the `pad` environments past N, in every slot that was not
    written, in the `unreadable` slots, and in the reward and action of the newest slot (its observations are intact)"""
    T, N, S, lmax = c['obs'].shape[:4]
    rp = DeviceReplay(T, N + pad, S, lmax, device='cuda')
    rp.obs.fill_(float('nan'))
    rp.act.fill_(-777)
    rp.rew.fill_(float('nan'))
    newest = (head - 1) % T
    keep = [t for t in valid_slots(T, head, count) + [newest] if t not in unreadable]
    rp.obs[keep, :N] = torch.from_numpy(c['obs'][keep]).cuda()
    keep.remove(newest)
    rp.act[keep, :N] = torch.from_numpy(c['act'][keep]).cuda()
    rp.rew[keep, :N] = torch.from_numpy(c['rew'][keep]).cuda()
    rp.done.copy_(torch.from_numpy(c['done']))
    rp.head, rp.count = head, count
    return rp


def _compare(got, loss, g64, g32, l64, l32):
    worst = compare_gradients(NAMES, got, g64, g32)
    check_4_e_ref('loss', loss, l64, l32, worst)
    assert not worst, worst


@pytest.mark.parametrize('lmax,T,N,B,head,count,n_step,double_q,done_slots', SHAPES)
def test_minibatch_gradient(lmax, T, N, B, head, count, n_step, double_q, done_slots):
    c = ring_case(lmax, T, N, done_slots)
    idx, g64, g32, l64, l32, info = reference(lmax, T, N, B, head, count, n_step, double_q, done_slots)
    net, learner = _learner(c, B, n_step=n_step, double_q=double_q)
    rp = _device_ring(c, head, count)
    idx_t = torch.from_numpy(idx).cuda()
    got = _np(learner.grad(rp, idx_t))
    loss = learner.loss_out.cpu().numpy().copy()
    print('lmax %d ring %d x %d at (%d, %d), B %d, n_step %d, double_q %d; walks of m = %s' % (lmax, T, N, head, count, B, n_step, double_q,
                                                                                            sorted(set(info['m'].ravel()))))
    _compare(got, loss, g64, g32, l64, l32)
    assert all(np.abs(got[k]).max() > 0 for k in NAMES)
    again = _np(learner.grad(rp, idx_t))                # the same bits again
    for k in NAMES:
        assert got[k].tobytes() == again[k].tobytes(), k
    assert loss.tobytes() == learner.loss_out.cpu().numpy().tobytes()
    learner.close()


def test_ring_semantics():
    """(9, 8, 9) at head 3, full, an episode end at slot 5, n_step 3 with double_q.  Rows of slots 3, 4, 5 (cut after 3 / 2 / 1
    rewards) and of slots 0, 1 (truncated at the newest slot, 2, after 2 / 1 rewards; slot 0 wraps nothing but bootstraps from the
    newest observation).  Slots 6 and 7, behind the cut, are unreadable in every environment, and so are reward and action of the
    newest slot: a bootstrap multiplied by zero instead of cut, or a walk past the newest slot, gives NaN."""
    lmax, T, N, B, head, count, n_step, dq, done_slots = SHAPES[2]
    c = ring_case(lmax, T, N, done_slots)
    idx, g64, g32, l64, l32, info = reference(lmax, T, N, B, head, count, n_step, dq, done_slots, slots=(3, 4, 5, 0, 1))
    assert info['read'] == {3, 4, 5, 0, 1} and set(info['u_m'][~info['cut']].ravel()) == {2}
    assert all((idx[..., 0] == t).sum() > 10 for t in (3, 4, 5, 0, 1))
    net, learner = _learner(c, B, n_step=n_step, double_q=dq)
    rp = _device_ring(c, head, count, unreadable=(6, 7))
    assert torch.isnan(rp.obs[[6, 7]]).all() and torch.isnan(rp.rew[2]).all() and not torch.isnan(rp.obs[2, :N]).any()
    got = _np(learner.grad(rp, torch.from_numpy(idx).cuda()))
    _compare(got, learner.loss_out.cpu().numpy(), g64, g32, l64, l32)
    learner.close()


def test_options_off_give_the_bytes_of_a_handle_never_touched():
    lmax, T, N, B, head, count, _, _, done_slots = SHAPES[1]
    c = ring_case(lmax, T, N, done_slots)
    idx = torch.from_numpy(reference(lmax, T, N, B, head, count, 3, True, done_slots)[0]).cuda()
    rp = _device_ring(c, head, count)
    L = load_library()

    def grads(set_to):
        net, learner = _learner(c, B)
        for pair in set_to:
            assert L.rs_dqn_set_target(learner._h, *pair) == 0
        out = (_np(learner.grad(rp, idx)), learner.loss_out.cpu().numpy().copy())
        learner.close()
        return out

    plain, back, on = grads(()), grads(((3, 1), (1, 0))), grads(((3, 1),))
    for k in NAMES:
        assert plain[0][k].tobytes() == back[0][k].tobytes(), k
    assert plain[1].tobytes() == back[1].tobytes()
    assert any(plain[0][k].tobytes() != on[0][k].tobytes() for k in NAMES)


def test_update_is_the_loop_of_single_calls():
    """rs_dqn_update(n_updates = 3) at (3, 1) against sample (keyed by the steps so far), grad, step, three times, from the same state:
    the online network of the second and third update's a* is the one the Adam step before it left"""
    lmax, T, N, B, head, count, n_step, dq, done_slots = SHAPES[2]
    c = ring_case(lmax, T, N, done_slots)
    rp = _device_ring(c, head, count, pad=0)        # (the draws cover every environment of the ring: none is a sentinel)

    def run(fused):
        net, learner = _learner(c, 40, n_step=n_step, double_q=dq)
        if fused:
            learner.update(rp, updates=3)
        else:
            for _ in range(3):
                learner.grad(rp, learner.sample(rp))
                learner.step()
        assert learner.n_updates == 3
        out = (_np(net), _np(learner.m), _np(learner.v), learner.loss_out.cpu().numpy().copy())
        learner.close()
        return out

    one, loop, again = run(True), run(False), run(True)
    for other in (loop, again):
        for a, b in zip(one[:3], other[:3]):
            for k in NAMES:
                assert a[k].tobytes() == b[k].tobytes(), k
        assert one[3].tobytes() == other[3].tobytes()
    assert all(np.isfinite(one[0][k]).all() for k in NAMES) and np.isfinite(one[3]).all()
    assert np.abs(one[0]['fc2_w'] - c['net'].fc2_w.detach().numpy()).max() > 1e-4


@pytest.mark.parametrize('n_step,double_q', [(3, True), (32, False), (1, True)])
def test_the_draw_does_not_depend_on_the_options(n_step, double_q):
    T, N, head, count = 5, 7, 1, 5
    c = ring_case(2, 3, 5, ())
    net, learner = _learner(c, 33, n_step=n_step, double_q=double_q)
    rp = DeviceReplay(T, N, 3, 2, device='cuda')        # (the draw reads nothing of it)
    rp.head, rp.count = head, count
    for u in (0, 1, 77):
        assert np.array_equal(learner.sample(rp, update_key=u).cpu().numpy(), predict_sample(SEED, u, 3, T, N, head, count, 33))
    learner.close()


def test_refusals():
    c = ring_case(2, 3, 5, ())
    net, learner = _learner(c, 33, n_step=3, double_q=True)
    L, h = load_library(), learner._h
    n, dq = C.c_int32(-1), C.c_int32(-1)

    def pair():
        assert L.rs_dqn_get_target(h, C.byref(n), C.byref(dq)) == 0
        return n.value, dq.value

    assert pair() == (3, 1)
    for bad, word in (((0, 0), b'n_step'), ((33, 1), b'n_step'), ((2, 2), b'double_q'), ((2, -1), b'double_q')):
        assert L.rs_dqn_set_target(h, *bad) == RS_EINVAL
        assert L.rs_last_error(None).startswith(b'rs_dqn_set_target') and word in L.rs_last_error(None)
        assert pair() == (3, 1), 'a refused call leaves the handle as it was'
    assert L.rs_dqn_set_target(None, 1, 0) == RS_EINVAL and b'NULL' in L.rs_last_error(None)
    assert L.rs_dqn_get_target(None, C.byref(n), C.byref(dq)) == RS_EINVAL and L.rs_dqn_get_target(h, None, C.byref(dq)) == RS_EINVAL
    assert L.rs_dqn_set_target(h, 32, 0) == 0 and pair() == (32, 0)
    learner.close()
    with pytest.raises(ValueError, match='n_step'):
        FusedDQNLearner(_device_net(c['net']), n_step=33)
    untouched = _learner(c, 33)[1]
    assert L.rs_dqn_get_target(untouched._h, C.byref(n), C.byref(dq)) == 0 and (n.value, dq.value) == (1, 0)
    untouched.close()


# ---- the loop: cologne1 x 8 environments, a ring of 8 slots (it wraps), batch 16, target_update 5, 12 env-steps
N_ENVS, CAPACITY, BATCH, TARGET_UPDATE, STEPS, DECAY = 8, 8, 16, 5, 12, 10


def _loop_objects():
    env = VecMultiSignal('cologne1', N_ENVS, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
    net = BatchedIDQN.from_scenario(env.scenario, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=0)
    learner = FusedDQNLearner(net, gamma=0.99, lr=1e-3, target_update=TARGET_UPDATE, batch_size=BATCH, seed=0, n_step=3, double_q=True)
    policy = FusedIDQN(net, seed=7)
    replay = DeviceReplay(CAPACITY, N_ENVS, env.n_signals, net.lmax, device='cuda')
    return env, dict(net=net, learner=learner, policy=policy, replay=replay)


def _loop_state(o):
    torch.cuda.synchronize()
    L = o['learner']
    out = {'par.' + k: getattr(o['net'], k) for k in NAMES}
    out.update({'tgt.' + k: getattr(L.target, k) for k in NAMES})
    out.update({'m.' + k: L.m[k] for k in NAMES})
    out.update({'v.' + k: L.v[k] for k in NAMES})
    out.update({'ring.obs': o['replay'].obs, 'ring.act': o['replay'].act, 'ring.rew': o['replay'].rew, 'ring.done': o['replay'].done})
    out = {k: t.detach().cpu().numpy().tobytes() for k, t in out.items()}
    out['scalars'] = (L.t, L.n_updates, o['replay'].head, o['replay'].count)
    return out


def test_library_loop_equals_the_python_loop_and_resumes(tmp_path):
    # the Python-driven loop of tools/idqn_train.py --device-update
    env, A = _loop_objects()
    L, P, R = A['learner'], A['policy'], A['replay']
    actions = env.tensor('actions')
    env.sim.set_seed(1000)
    obs = env.reset()['drq_norm_f16']
    for _ in range(STEPS):
        P.act(obs, epsilon=linear_epsilon(L.t, 1.0, 0.0, DECAY), step_key=L.t, out=actions)
        R.stage(obs)
        o, r, done, _ = env.step(None)
        R.commit(actions, r['wait_norm'], done)
        if L.observe_step(R) is not None:
            P.refresh_on_device()
        obs = o['drq_norm_f16']
    want = _loop_state(A)
    L.close()
    env.close()
    assert want['scalars'] == (STEPS, STEPS - 2, STEPS % CAPACITY, CAPACITY)

    # the same steps in one rs_group_train call
    env, B = _loop_objects()
    trainer = DeviceTrainer(env, B['learner'], B['policy'], B['replay'], 1.0, 0.0, DECAY)
    env.sim.set_seed(1000)
    env.reset()
    trainer.run(STEPS, None)
    got = _loop_state(B)
    assert got['scalars'] == want['scalars']
    for k in want:
        assert got[k] == want[k], k

    # a checkpoint of it, loaded into fresh objects: the same bits, and the same bits after one more update
    path = str(tmp_path / 'a.pt')
    checkpoint.save(path, agent='IDQN', map_name='cologne1', objects=B, progress={})
    assert torch.load(path, weights_only=True)['signature']['fields']['learner.n_step'] == 3
    env2, Cc = _loop_objects()
    checkpoint.load(path, agent='IDQN', map_name='cologne1', objects=Cc)
    resumed = _loop_state(Cc)
    for k in want:
        assert resumed[k] == want[k], k
    B['learner'].update(B['replay'])
    Cc['learner'].update(Cc['replay'])
    one, two = _loop_state(B), _loop_state(Cc)
    for k in one:
        assert one[k] == two[k], k
    assert one['par.fc2_w'] != want['par.fc2_w']
    plain = FusedDQNLearner(Cc['net'], target_update=TARGET_UPDATE, batch_size=BATCH)
    with pytest.raises(ValueError, match=r'learner\.n_step'):
        checkpoint.load(path, agent='IDQN', map_name='cologne1', objects=dict(Cc, learner=plain))
    for x in (B['learner'], Cc['learner'], plain):
        x.close()
    env.close()
    env2.close()
