"""GPU: the DQN training loop in the library (rs_group_train, agents/train_fused.py: DeviceTrainer) and the three entry points it is
made of.  rs_idqn_pack_weights against FusedIDQN.refresh_on_device, the two target syncs against the parameters, the loop against
the tools' --device-update loop in Python at the same seeds: the fused learners draw from a counter hash and the policies by the
global environment index, so every array and every figure must be EQUAL, no tolerance -- for IDQN, MPLight and MPLightFULL, on one,
two and three pipes (6 + 5 + 5 and 3 + 3 + 2 environments: slots that are not 16-byte aligned, the recorder's element path) and for
any split of an episode into calls.  Horizon 20 steps, batch 32, ring capacity 8 (wraps and saturates inside an episode),
target_update 7 (syncs inside it).  The refusals launch nothing."""
import ctypes as C
import types

import pytest
import torch

from resco_amd.agents.idqn_fused import FusedIDQN
from resco_amd.agents.idqn_learn import DeviceReplay, linear_epsilon
from resco_amd.agents.idqn_learn_fused import FusedDQNLearner
from resco_amd.agents.idqn_rollout import BatchedIDQN
from resco_amd.agents.mplight import FusedMPLight, MPLightReplay, frap_from_scenario
from resco_amd.agents.mplight_learn_fused import FusedMPLightLearner
from resco_amd.agents.train_fused import DeviceTrainer
from resco_amd.multi_signal import VecMultiSignal, load_scenario, map_configs
from resco_amd.sim import DQN_TENSORS, DQNTensors, SimGroup, load_library, torch_stream
from tools.train_pipes_ab import PipedEnvs, train_device_loop, train_one_handle

pytestmark = pytest.mark.gpu

STEPS, BATCH, CAPACITY, TARGET_UPDATE, EPISODES = 20, 32, 8, 7, 2
KEYS = ('episode', 'epsilon', 'mean_return', 'avg_delay_s', 'arrived_per_env', 'updates')
CASES = {'idqn-cologne1': ('idqn', 'cologne1', 16, False), 'idqn-ingolstadt21': ('idqn', 'ingolstadt21', 8, False),
         'mplight-cologne1': ('mplight', 'cologne1', 16, False), 'mplightfull-cologne1': ('mplight', 'cologne1', 16, True),
         'mplight-ingolstadt21': ('mplight', 'ingolstadt21', 8, False)}
SPLITS = {'whole': (20,), 'two': (7, 13), 'ones': (1,) * 20}


@pytest.fixture
def short_episode(monkeypatch):
    init = VecMultiSignal.__init__

    def short(self, *a, **kw):
        init(self, *a, **kw)
        self.horizon_steps = STEPS

    monkeypatch.setattr(VecMultiSignal, '__init__', short)


def scenario(map_name):
    return load_scenario(map_name, None, map_configs.get(map_name, {}).get('lights', ()), 3)


def setup(agent, map_name, n, full, pipes, seed=0):
    """the objects of tools/train_pipes_ab.py: train_piped with this file's ring capacity and target_update"""
    idqn = agent == 'idqn'
    state = 'drq_norm_f16' if idqn else ('mplight_full' if full else 'mplight')
    kw = dict(states=(state,), rewards=('wait_norm' if idqn else 'pressure',), seed=0)
    if not idqn:
        kw['outputs'] = (state,)
    pe = PipedEnvs(map_name, n, pipes, **kw)
    S = pe.n_signals
    if idqn:
        net = BatchedIDQN.from_scenario(pe.scenario, dtype=torch.float32, device='cuda')
        net.init_like_reference(seed=seed)
        learner = FusedDQNLearner(net, gamma=0.99, lr=1e-3, target_update=TARGET_UPDATE, batch_size=BATCH, seed=seed)
        policy = FusedIDQN(net, seed=7 + seed)
        replay = DeviceReplay(CAPACITY, n, S, net.lmax, device='cuda')
    else:
        net = frap_from_scenario(pe.scenario, 4 if full else 1).cuda()
        net.init_like_reference(seed)
        learner = FusedMPLightLearner(net, gamma=0.99, lr=1e-3, target_update=TARGET_UPDATE, batch_size=BATCH, seed=seed, n_signals=S)
        policy = FusedMPLight(net, pe.scenario, seed=7 + seed)
        policy.share_weights(learner.flat)
        replay = MPLightReplay(CAPACITY, n, S, 1 + 12 * net.demand_shape, device='cuda')
    return types.SimpleNamespace(idqn=idqn, state=state, reward='wait_norm' if idqn else 'pressure', pe=pe, net=net, learner=learner, policy=policy,
                                 replay=replay, n=n, S=S, decay=int(0.8 * EPISODES * STEPS), seed=seed)


def snapshot(X, ret, rows):
    """everything the two loops must agree on, as host copies"""
    torch.cuda.synchronize()
    L, R = X.learner, X.replay
    if X.idqn:
        tensors = {'par.' + k: getattr(X.net, k) for k in DQN_TENSORS}
        tensors.update({'tgt.' + k: getattr(L.target, k) for k in DQN_TENSORS})
        tensors.update({'m.' + k: L.m[k] for k in DQN_TENSORS})
        tensors.update({'v.' + k: L.v[k] for k in DQN_TENSORS})
    else:
        tensors = {'par': L.flat, 'tgt': L.flat_target, 'm': L._m, 'v': L._v}
    tensors.update({'ring.obs': R.obs, 'ring.act': R.act, 'ring.rew': R.rew, 'ring.done': R.done, 'actions': X.pe.cat('actions'), 'ret': ret,
                    'loss_out': L.loss_out})
    out = {k: t.detach().cpu().clone() for k, t in tensors.items()}
    out['scalars'] = dict(head=R.head, count=R.count, t=L.t, n_updates=L.n_updates, env_steps=[e.steps for e in X.pe.envs][0])
    out['rows'] = [{k: r[k] for k in KEYS} for r in rows]
    return out


def row(X, ep, eps, ret):
    d, arrived = X.pe.delay()
    return dict(episode=ep, epsilon=round(eps, 3), mean_return=float(ret.sum(1).mean()) / X.S, avg_delay_s=round(d, 2), arrived_per_env=round(arrived, 1),
                updates=X.learner.n_updates)


def python_training(agent, map_name, n, full):
    """the loop of tools/idqn_train.py / tools/mplight_train.py --device-update (what train_one_handle runs), on one handle"""
    X = setup(agent, map_name, n, full, 1)
    env, L, P, R = X.pe.envs[0], X.learner, X.policy, X.replay
    actions = env.tensor('actions')
    pair = torch.zeros(n, X.S, dtype=torch.int32, device='cuda')
    rows = []
    for ep in range(EPISODES):
        env.sim.set_seed(1000 + ep + 7919 * X.seed)
        obs = env.reset()[X.state]
        ret = torch.zeros(n, X.S, device='cuda')
        for k in range(STEPS):
            eps = linear_epsilon(L.t, 1.0, 0.0, X.decay)
            if X.idqn:
                P.act(obs, epsilon=eps, step_key=L.t, out=actions)
            else:
                P.act(obs, epsilon=eps, step_key=L.t, out=actions, pair_out=pair)
            R.stage(obs)
            o, r, done, _ = env.step(None)
            rew = r[X.reward].float()
            R.commit(actions if X.idqn else pair, rew, done)
            ret += rew
            if L.observe_step(R) is not None and X.idqn:
                P.refresh_on_device()
            obs = o[X.state]
        torch.cuda.synchronize()
        rows.append(row(X, ep, eps, ret))
    snap = snapshot(X, ret, rows)
    L.close()
    X.pe.close()
    return snap


def library_training(agent, map_name, n, full, pipes, split):
    X = setup(agent, map_name, n, full, pipes)
    trainer = DeviceTrainer(X.pe, X.learner, X.policy, X.replay, 1.0, 0.0, X.decay)
    rows = []
    for ep in range(EPISODES):
        X.pe.set_seed(1000 + ep + 7919 * X.seed)
        X.pe.reset()
        ret = torch.zeros(n, X.S, device='cuda')
        done = False
        for c in split:
            assert not done
            done = trainer.run(c, ret)
        assert done
        torch.cuda.synchronize()
        rows.append(row(X, ep, trainer.epsilon(X.learner.t - 1), ret))
    snap = snapshot(X, ret, rows)
    X.learner.close()
    X.pe.close()
    return snap


_reference = {}


def reference(case):
    """the Python loop's result, computed once per case and never changed"""
    if case not in _reference:
        _reference[case] = python_training(*CASES[case])
    return _reference[case]


# every case on one, two and three pipes and with every split (rotated), and the full cross on cologne1 for IDQN and MPLight
COMBOS = [(c, 1 + (i + j) % 3, s) for i, c in enumerate(CASES) for j, s in enumerate(SPLITS)]
COMBOS += [(c, p, s) for c in ('idqn-cologne1', 'mplight-cologne1') for p in (1, 2, 3) for s in SPLITS if (c, p, s) not in COMBOS]


@pytest.mark.parametrize('case,pipes,split', COMBOS)
def test_library_loop_equals_the_python_loop(short_episode, case, pipes, split):
    want = reference(case)
    got = library_training(*CASES[case], pipes, SPLITS[split])
    assert want['scalars']['n_updates'] > 0 and want['scalars']['count'] == CAPACITY and want['scalars']['t'] == EPISODES * STEPS
    assert want['ring.done'].sum() >= 1 and torch.isfinite(want['ret']).all()
    assert got['scalars'] == want['scalars']
    assert got['rows'] == want['rows']
    for k in want:
        if k not in ('scalars', 'rows'):
            assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize('agent,full', [('idqn', False), ('mplight', False)])
def test_device_loop_rows_equal_train_one_handle(short_episode, agent, full):
    """the A/B script's loop variants against its variant 1 (the tools' own loop, their ring and schedule): the same rows"""
    want = train_one_handle(agent, 'cologne1', 16, 2, batch=32, full=full)
    got = train_device_loop(agent, 'cologne1', 16, 2, batch=32, pipes=3, full=full, chunks=(7, 13))
    assert [{k: r[k] for k in KEYS} for r in got] == [{k: r[k] for k in KEYS} for r in want] and want[-1]['updates'] > 0


# ---------------------------------------------------------------------------------------------------------------- the entry points
@pytest.mark.parametrize('map_name', ['cologne1', 'ingolstadt21'])
def test_pack_weights_equals_refresh_on_device(map_name):
    lib = load_library()
    net = BatchedIDQN.from_scenario(scenario(map_name), dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=3)
    with torch.no_grad():
        net.fc3_b.copy_(torch.randn_like(net.fc3_b) * 0.2)
    policy = FusedIDQN(net, seed=5)
    S, N = len(net.lanes), 37
    params = DQNTensors(*[getattr(net, k).data_ptr() for k in DQN_TENSORS])
    assert lib.rs_idqn_pack_weights(policy._h, C.byref(params), torch_stream(0)) == -1        # RS_EINVAL: still on the create-time copy
    assert b'create-time' in lib.rs_last_error(None)
    gen = torch.Generator(device='cuda').manual_seed(1)
    obs = (torch.rand(N, S, net.lmax, 5, device='cuda', generator=gen) * 2).to(torch.float16)
    for round_ in range(2):
        policy.refresh_on_device()
        d = policy._dev
        want = {k: d[k].clone() for k in ('w1', 'w2', 'w3', 'b3')}
        a_want, q_want = [t.clone() for t in policy.act(obs, epsilon=0.3, step_key=9, want_q=True)]
        for k in want:
            d[k].fill_(7.0)
        assert lib.rs_idqn_pack_weights(policy._h, C.byref(params), torch_stream(0)) == 0
        a_got, q_got = policy.act(obs, epsilon=0.3, step_key=9, want_q=True)
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(d[k], want[k]), k
            assert not bool(policy._pad[k][S * d[k].shape[1]:].any()) if k != 'b3' else True, 'written behind ' + k
        assert torch.equal(a_got, a_want) and torch.equal(q_got, q_want)
        with torch.no_grad():       # other weights for the second round (padded fc1 rows stay zero: the masked learner keeps them so)
            for k in DQN_TENSORS:
                p = getattr(net, k)
                p.mul_(1.0 + 0.5 * torch.rand_like(p))
    policy.close()


def test_sync_target_calls():
    lib = load_library()
    sc = scenario('ingolstadt21')
    net = BatchedIDQN.from_scenario(sc, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=1)
    learner = FusedDQNLearner(net, batch_size=32)
    with torch.no_grad():
        for k in DQN_TENSORS:
            getattr(net, k).add_(torch.randn_like(getattr(net, k)))
    assert not torch.equal(learner.target.fc1_w, net.fc1_w)
    assert lib.rs_dqn_sync_target(learner._h, torch_stream(0)) == 0
    torch.cuda.synchronize()
    for k in DQN_TENSORS:
        assert torch.equal(getattr(learner.target, k), getattr(net, k)), k
    learner.close()
    for full in (False, True):
        frap = frap_from_scenario(sc, 4 if full else 1).cuda()
        frap.init_like_reference(2)
        ml = FusedMPLightLearner(frap, batch_size=32, n_signals=sc.n_signals)
        with torch.no_grad():
            ml.flat.add_(torch.randn_like(ml.flat))
        assert not torch.equal(ml.flat_target, ml.flat)
        assert lib.rs_mplight_dqn_sync_target(ml._h, torch_stream(0)) == 0
        torch.cuda.synchronize()
        assert torch.equal(ml.flat_target, ml.flat) and all(torch.equal(a, b) for a, b in zip(ml.target.parameters(), frap.parameters()))
        ml.close()
    assert lib.rs_dqn_sync_target(None, None) == -1 and lib.rs_mplight_dqn_sync_target(None, None) == -1


# ---------------------------------------------------------------------------------------------------------------- the refusals
def _state(X):
    torch.cuda.synchronize()
    t = [X.replay.obs, X.replay.act, X.replay.rew, X.replay.done] + ([getattr(X.net, k) for k in DQN_TENSORS] if X.idqn else [X.learner.flat])
    return [a.detach().clone() for a in t] + [X.pe.cat('actions').clone()]


def _train(X, group=None, n_steps=3, **kw):
    L = X.learner
    args = dict(done_step=-1, batch=L.batch_size, updates_per_step=1, target_update=L.target_update, eps_start=1.0, eps_end=0.0, decay_steps=X.decay,
                policy_seed=X.policy.seed, learner_seed=L.seed, loss_out=L.loss_out.data_ptr())
    policy, learner, ring = kw.pop('policy', X.policy.handle), kw.pop('learner', L._h), kw.pop('ring', None)
    args.update(kw)
    (group or X.trainer.group).train(n_steps, 'idqn' if X.idqn else 'mplight', policy, learner, ring if ring is not None else L._ring(X.replay), L.t, **args)


def test_refusals_launch_nothing(short_episode, monkeypatch):
    X = setup('idqn', 'cologne1', 16, False, 2)
    X.trainer = DeviceTrainer(X.pe, X.learner, X.policy, X.replay, 1.0, 0.0, X.decay)
    X.pe.reset()
    X.trainer.run(5)                    # a ring with something in it
    before, updates = _state(X), X.learner.n_updates
    other = BatchedIDQN.from_scenario(scenario('ingolstadt21'), dtype=torch.float32, device='cuda')
    other.init_like_reference(seed=0)
    other_policy, other_learner = FusedIDQN(other, seed=1), FusedDQNLearner(other, batch_size=BATCH)
    other_policy.refresh_on_device()
    fresh = FusedIDQN(X.net, seed=1)    # still on its create-time copy
    small = DeviceReplay(CAPACITY, 15, X.S, X.net.lmax, device='cuda')
    swapped = SimGroup([e.sim for e in reversed(X.pe.envs)])
    monkeypatch.setenv('RESCO_PLAIN_STREAMS', '1')
    plain = VecMultiSignal('cologne1', 16, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0, scenario=X.pe.scenario)
    monkeypatch.delenv('RESCO_PLAIN_STREAMS')
    refusals = [(dict(n_steps=0), 'n_steps >= 1'), (dict(n_steps=3, done_step=3), 'done_step'), (dict(done_step=-2), 'done_step'),
                (dict(updates_per_step=-1), 'updates_per_step >= 0'), (dict(target_update=0), 'target_update >= 1'),
                (dict(policy=other_policy.handle), 'built for this scenario'), (dict(learner=other_learner._h), 'learner does not fit'),
                (dict(policy=fresh.handle), 'create-time'), (dict(ring=X.learner._ring(small)), 'add up'), (dict(group=swapped), 'contiguous'),
                (dict(group=SimGroup([plain.sim])), 'non-blocking'), (dict(batch=BATCH + 1), 'max_batch')]
    for kw, text in refusals:
        with pytest.raises(RuntimeError, match=text):
            _train(X, **kw)
    X.pe.envs[1].sim.set_outputs(('mplight',))
    with pytest.raises(RuntimeError, match='switched off'):
        _train(X)
    X.pe.envs[1].sim.set_outputs(None)
    # the wrapper's own: a call across the horizon, a side stream
    with pytest.raises(ValueError, match='cross the horizon'):
        X.trainer.run(STEPS)
    with torch.cuda.stream(torch.cuda.Stream()), pytest.raises(RuntimeError, match='default stream'):
        X.trainer.run(1)
    after = _state(X)
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and X.learner.n_updates == updates and X.replay.head == 5 and X.learner.t == 5
    X.trainer.run(15)                   # and the loop still runs to the episode's end
    torch.cuda.synchronize()
    assert X.learner.n_updates > updates and X.pe.envs[0].steps == STEPS
    for o in (other_policy, fresh, other_learner, X.learner, plain, X.pe):
        o.close()


def test_mplight_refusals(short_episode):
    X = setup('mplight', 'cologne1', 16, False, 2)
    X.trainer = DeviceTrainer(X.pe, X.learner, X.policy, X.replay, 1.0, 0.0, X.decay)
    X.pe.reset()
    before = _state(X)
    full = frap_from_scenario(X.pe.scenario, 4).cuda()
    full.init_like_reference(0)
    full_learner = FusedMPLightLearner(full, batch_size=BATCH, n_signals=X.S)
    own = FusedMPLight(X.net, X.pe.scenario, seed=1)        # reads its own copy of the weights, not the learner's vector
    for kw, text in [(dict(learner=full_learner._h), 'learner does not fit'), (dict(policy=own.handle), 'parameter vector')]:
        with pytest.raises(RuntimeError, match=text):
            _train(X, **kw)
    X.pe.envs[0].sim.set_outputs(('drq_norm_f16',))
    with pytest.raises(RuntimeError, match='switched off'):
        _train(X)
    X.pe.envs[0].sim.set_outputs(('mplight',))
    assert all(torch.equal(a, b) for a, b in zip(before, _state(X))) and X.learner.n_updates == 0
    for o in (full_learner, own, X.learner, X.pe):
        o.close()
