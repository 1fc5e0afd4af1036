"""GPU: a training run that is saved at an episode boundary and continued by fresh objects computes, bit for bit, what the
uninterrupted run computes (resco_amd/checkpoint.py; the state_dict() / load_state_dict() of the learners, policies, rings and
trainers; rs_*_set_steps).  cologne1 x 16 environments, the horizon cut to 20 env-steps, 3 planned episodes; the DQN ring holds 8
slots (wraps and saturates inside an episode), target_update 7 (syncs inside an episode and across the checkpoint), segments of 8
steps (8 does not divide 20: IPPO's checkpoint holds a partly filled segment)."""
import types

import pytest
import torch

from resco_amd import checkpoint
from resco_amd.agents.fma2c import BatchedFMA2C, FMA2CLayout, FusedFMA2C
from resco_amd.agents.fma2c_learn_fused import FusedA2CLearner
from resco_amd.agents.idqn_fused import FusedIDQN
from resco_amd.agents.idqn_learn import DeviceReplay, linear_epsilon
from resco_amd.agents.idqn_learn_fused import FusedDQNLearner
from resco_amd.agents.idqn_rollout import BatchedIDQN
from resco_amd.agents.ippo import BatchedIPPO
from resco_amd.agents.ippo_fused import DeviceRollout, FusedIPPO
from resco_amd.agents.ippo_learn_fused import FusedPPOLearner
from resco_amd.agents.mplight import FusedMPLight, MPLightReplay, frap_from_scenario
from resco_amd.agents.mplight_learn_fused import FusedMPLightLearner
from resco_amd.agents.train_fused import DeviceA2CTrainer, DevicePPOTrainer, DeviceTrainer
from resco_amd.config.agent_config import agent_configs
from resco_amd.config.mdp_config import activate
from resco_amd.multi_signal import VecMultiSignal
from resco_amd.sim import DQN_TENSORS, PPO_TENSORS, load_library

pytestmark = pytest.mark.gpu

MAP, N, STEPS, EPISODES = 'cologne1', 16, 20, 3
BATCH, CAPACITY, TARGET_UPDATE, SEG = 32, 8, 7, 8
DECAY = int(0.8 * EPISODES * STEPS)
RS_EINVAL = -1


@pytest.fixture
def short_episode(monkeypatch):
    init = VecMultiSignal.__init__

    def short(self, *a, **kw):
        init(self, *a, **kw)
        self.horizon_steps = STEPS

    monkeypatch.setattr(VecMultiSignal, '__init__', short)


def same(a, b, path=''):
    """EVERY key of two loaded checkpoints: torch.equal for tensors, == for scalars"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            same(a[k], b[k], '%s/%s' % (path, k))
    elif isinstance(a, list):
        assert isinstance(b, list) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, '%s/%d' % (path, i))
    else:
        assert a == b, path


# ------------------------------------------------------------------------------------------------ the runs
def build(agent, seed):
    """the objects of the four training tools at this file's sizes -> (name, objects in load order, episode(ep) -> row, close)"""
    python_loop = agent == 'idqn-python'
    kind = agent.split('-')[0]
    if kind == 'idqn':
        env = VecMultiSignal(MAP, N, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
        net = BatchedIDQN.from_scenario(env.scenario, dtype=torch.float32, device='cuda')
        net.init_like_reference(seed=seed)
        learner = FusedDQNLearner(net, gamma=0.99, lr=1e-3, target_update=TARGET_UPDATE, batch_size=BATCH, seed=seed)
        policy = FusedIDQN(net, seed=7 + seed)
        replay = DeviceReplay(CAPACITY, N, env.n_signals, net.lmax, device='cuda')
    elif kind in ('mplight', 'mplightfull'):
        full = kind == 'mplightfull'
        state = 'mplight_full' if full else 'mplight'
        env = VecMultiSignal(MAP, N, states=(state,), rewards=('pressure',), seed=0, outputs=(state,))
        net = frap_from_scenario(env.scenario, 4 if full else 1).cuda()
        net.init_like_reference(seed)
        learner = FusedMPLightLearner(net, gamma=0.99, lr=1e-3, target_update=TARGET_UPDATE, batch_size=BATCH, seed=seed, n_signals=env.n_signals)
        policy = FusedMPLight(net, env.scenario, seed=7 + seed)
        policy.share_weights(learner.flat)
        replay = MPLightReplay(CAPACITY, N, env.n_signals, 1 + 12 * net.demand_shape, device='cuda')
    if kind in ('idqn', 'mplight', 'mplightfull'):
        S = env.n_signals
        objects = dict(env=env, net=net, learner=learner, policy=policy, replay=replay)
        if python_loop:
            actions = env.tensor('actions')

            def episode(ep):
                env.sim.set_seed(1000 + ep)
                obs = env.reset()['drq_norm_f16']
                ret = torch.zeros(N, S, device='cuda')
                for k in range(STEPS):
                    eps = linear_epsilon(learner.t, 1.0, 0.0, DECAY)
                    policy.act(obs, epsilon=eps, step_key=learner.t, out=actions)
                    replay.stage(obs)
                    o, r, done, _ = env.step(None)
                    replay.commit(actions, r['wait_norm'], done)
                    ret += r['wait_norm']
                    if learner.observe_step(replay) is not None:
                        policy.refresh_on_device()
                    obs = o['drq_norm_f16']
                return row(env, ep, float(ret.sum(1).mean()) / S, learner.n_updates)
        else:
            trainer = DeviceTrainer(env, learner, policy, replay, 1.0, 0.0, DECAY)
            objects['trainer'] = trainer

            def episode(ep):
                env.sim.set_seed(1000 + ep)
                env.reset()
                ret = torch.zeros(N, S, device='cuda')
                assert trainer.run(STEPS, ret)
                return row(env, ep, float(ret.sum(1).mean()) / S, learner.n_updates)

        def close():
            learner.close()
            env.close()
        return types.SimpleNamespace(objects=objects, episode=episode, close=close, before_save=lambda: None)
    if kind == 'ippo':
        env = VecMultiSignal(MAP, N, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
        net = BatchedIPPO.from_scenario(env.scenario, dtype=torch.float32, device='cuda')
        net.init_like_reference(seed=seed)
        learner = FusedPPOLearner(net, minibatch=48, epochs=2, seed=seed)         # 128 rows: two whole minibatches and a short one
        policy = FusedIPPO(net, seed=3 + seed)
        policy.refresh_on_device()
        rollout = DeviceRollout(SEG, [env.sim])
        trainer = DevicePPOTrainer(env, learner, policy, rollout)

        def episode(ep):
            env.sim.set_seed(1000 + ep)
            env.reset()
            torch.cuda.synchronize()
            assert trainer.run(STEPS)
            return row(env, ep, float(rollout.pipes[0]['rew'].sum()), learner.n_updates)

        def close():
            learner.close()
            env.close()
        return types.SimpleNamespace(objects=dict(env=env, net=net, learner=learner, policy=policy, rollout=rollout, trainer=trainer), episode=episode,
                                     close=close, before_save=lambda: None)
    assert kind == 'fma2c'
    cfg = agent_configs['FMA2C']
    activate('FMA2C', MAP)
    env = VecMultiSignal(MAP, N, states=(), rewards=(), seed=0, max_distance=cfg['max_distance'], outputs=('lane_agg', 'lane_arrivals'))
    layout = FMA2CLayout(env.scenario, False)
    net = BatchedFMA2C(layout).init_like_reference(seed).cuda()
    policy = FusedFMA2C(net, N, seed=7 + seed)
    learner = FusedA2CLearner(net, policy, N, batch_size=SEG, gamma=cfg['gamma'], lr=cfg['lr_init'], alpha=cfg['rmsp_alpha'], eps=cfg['rmsp_epsilon'],
                              max_grad_norm=cfg['max_grad_norm'], value_coef=cfg['value_coef'], entropy_coef=cfg['entropy_coef_init'],
                              reward_norm=cfg['reward_norm'], reward_clip=cfg['reward_clip'])
    trainer = DeviceA2CTrainer(env, learner, policy, False)

    def episode(ep):
        env.sim.set_seed(1000 + ep)
        env.reset()
        policy.reset()
        trainer.ret.zero_()
        assert trainer.run(STEPS)
        return row(env, ep, float(trainer.ret.mean()), learner.updates)

    def close():
        policy.close()          # (closes its learner first)
        env.close()
    # the network mirrors the learner's vector only after pull(): before a save, as tools/fma2c_train.py does
    return types.SimpleNamespace(objects=dict(env=env, net=net, learner=learner, policy=policy, trainer=trainer), episode=episode, close=close,
                                 before_save=learner.pull)


def row(env, ep, ret, updates):
    torch.cuda.synchronize()
    return dict(episode=ep, mean_return=ret, avg_delay_s=float(env.sim.trip_delay().mean()), arrived_per_env=float(env.sim.stats()['arrived'].mean()),
                updates=updates)


def run(agent, seed, first, last, path, load=None, replay=True):
    """episodes first .. last - 1 of the planned three, after loading `load`; the checkpoint goes to `path`; everything is closed"""
    X = build(agent, seed)
    rows = []
    if load:
        progress = checkpoint.load(load, agent=agent, map_name=MAP, objects=X.objects, hyper=dict(episodes=EPISODES))
        assert progress['episode'] == first
        rows = progress['rows']
    for ep in range(first, last):
        rows.append(X.episode(ep))
    X.before_save()
    checkpoint.save(path, agent=agent, map_name=MAP, objects=X.objects, hyper=dict(episodes=EPISODES), replay=replay, progress=dict(episode=last, rows=rows))
    X.close()
    return rows


# ------------------------------------------------------------------------------------------------ 5. and 6.
# (agent, episodes before the checkpoint).  After episode 2 IPPO's segment of 8 happens to be complete (40 = 5 x 8), so the partly
# filled segment -- slot 4 of 8 -- is the checkpoint after episode 1, a case of its own.
@pytest.mark.parametrize('agent,cut', [('idqn', 2), ('mplight', 2), ('mplightfull', 2), ('ippo', 2), ('ippo', 1), ('fma2c', 2), ('idqn-python', 2)])
def test_resume_is_bit_exact(short_episode, tmp_path, agent, cut):
    x, y, z, w = (str(tmp_path / ('%s.pt' % k)) for k in 'xyzw')
    rows_x = run(agent, 0, 0, 3, x)
    run(agent, 0, 0, cut, y)
    rows_z = run(agent, 5, cut, 3, z, load=y)          # fresh objects, another init seed: the load has to override all of it
    X, Z = torch.load(x, weights_only=True), torch.load(z, weights_only=True)
    same(X, Z)                                          # signature, every tensor and scalar of every object, progress
    assert rows_x[2] == rows_z[2] and rows_x == rows_z
    assert X['objects']['learner']['state'].get('steps', 1) > 0 and rows_x[2]['updates'] > rows_x[1]['updates'] > 0
    if agent == 'ippo':
        assert X['objects']['trainer']['state']['slot'] == (3 * STEPS) % SEG != 0
        assert torch.load(y, weights_only=True)['objects']['trainer']['state']['slot'] == (cut * STEPS) % SEG
        assert cut != 1 or (cut * STEPS) % SEG != 0
    if agent == 'fma2c':
        assert sorted(X['objects']['policy']['state']) == ['fingerprints', 'mgr_actions', 'parity', 'seed', 'state']
    if 'replay' in X['objects']:
        assert X['objects']['replay']['state']['count'] == CAPACITY
        # without the ring: loads and trains, a valid continuation (not compared)
        run(agent, 0, 0, cut, y, replay=False)
        assert len(run(agent, 5, cut, 3, w, load=y, replay=False)) == 3


# ------------------------------------------------------------------------------------------------ 7. rs_*_set_steps alone
def _filled_dqn_ring(net, gen):
    rp = DeviceReplay(CAPACITY, N, 1, net.lmax, device='cuda')
    rp.obs.copy_(torch.rand(rp.obs.shape, generator=gen).half())
    rp.act.copy_(torch.randint(0, net.actions[0], rp.act.shape, generator=gen))
    rp.rew.copy_(-torch.rand(rp.rew.shape, generator=gen))
    rp.done[3] = True
    rp.head, rp.count = 5, CAPACITY
    return rp


def _dqn(seed):
    from conftest import load_scenario
    net = BatchedIDQN.from_scenario(load_scenario(MAP), dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=seed)
    L = FusedDQNLearner(net, target_update=TARGET_UPDATE, batch_size=BATCH, seed=11)
    rp = _filled_dqn_ring(net, torch.Generator().manual_seed(1))
    tensors = lambda: [getattr(net, k) for k in DQN_TENSORS] + [getattr(L.target, k) for k in DQN_TENSORS] + [L.m[k] for k in DQN_TENSORS] + \
        [L.v[k] for k in DQN_TENSORS]
    return L, (lambda: L.update(rp)), tensors


def _mplight(seed):
    from conftest import load_scenario
    sc = load_scenario(MAP)
    net = frap_from_scenario(sc, 1).cuda()
    net.init_like_reference(seed)
    L = FusedMPLightLearner(net, target_update=TARGET_UPDATE, batch_size=BATCH, seed=11, n_signals=1)
    gen = torch.Generator().manual_seed(1)
    rp = MPLightReplay(CAPACITY, N, 1, 13, device='cuda')
    obs = torch.randint(0, 9, rp.obs.shape, generator=gen).float()
    obs[..., 0] = torch.randint(0, net.oshape, obs.shape[:-1], generator=gen).float()
    rp.obs.copy_(obs)
    rp.act.copy_(torch.randint(0, net.oshape, rp.act.shape, generator=gen))
    rp.rew.copy_(-torch.rand(rp.rew.shape, generator=gen))
    rp.done[3] = True
    rp.head, rp.count = 5, CAPACITY
    return L, (lambda: L.update(rp)), (lambda: [L.flat, L.flat_target, L._m, L._v])


def _ppo(seed):
    from conftest import load_scenario
    net = BatchedIPPO.from_scenario(load_scenario(MAP), dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=seed)
    n = 96
    L = FusedPPOLearner(net, minibatch=n, epochs=1)
    gen = torch.Generator().manual_seed(1)
    ds = dict(obs=torch.rand(n, 1, net.lmax, 5, generator=gen).half().cuda(), act=torch.randint(0, net.actions[0], (n, 1), generator=gen).cuda(),
              logp=(-torch.rand(n, 1, generator=gen) - 0.5).cuda(), adv=torch.randn(n, 1, generator=gen).cuda(), ret=-torch.rand(n, 1, generator=gen).cuda())
    perm = torch.randperm(n, generator=gen).reshape(1, n).cuda()
    return L, (lambda: L.fit(ds, perm)), (lambda: [getattr(net, k) for k in PPO_TENSORS] + [L.m[k] for k in PPO_TENSORS] + [L.v[k] for k in PPO_TENSORS])


@pytest.mark.parametrize('make,prefix', [(_dqn, 'rs_dqn'), (_mplight, 'rs_mplight_dqn'), (_ppo, 'rs_ppo')], ids=['dqn', 'mplight', 'ppo'])
def test_set_steps_alone(make, prefix):
    lib = load_library()
    set_steps, steps = getattr(lib, prefix + '_set_steps'), getattr(lib, prefix + '_steps')
    A, update_a, tensors_a = make(0)
    for _ in range(3):
        update_a()
    torch.cuda.synchronize()
    at3 = [t.detach().clone() for t in tensors_a()]
    for _ in range(2):
        update_a()
    B, update_b, tensors_b = make(4)
    with torch.no_grad():
        for dst, src in zip(tensors_b(), at3):
            dst.copy_(src)
    assert set_steps(B._h, 3) == 0 and steps(B._h) == 3 and B.n_updates == 3
    for _ in range(2):
        update_b()
    torch.cuda.synchronize()
    assert steps(A._h) == steps(B._h) == 5
    for i, (a, b) in enumerate(zip(tensors_a(), tensors_b())):
        assert torch.equal(a, b), i
    assert not torch.equal(tensors_a()[0], at3[0])          # (the last two updates did move the parameters)
    # refusals: nothing changes
    before = [t.detach().clone() for t in tensors_b()]
    assert set_steps(None, 3) == RS_EINVAL and b'NULL handle' in lib.rs_last_error(None)
    assert set_steps(B._h, -1) == RS_EINVAL and b't >= 0' in lib.rs_last_error(None)
    torch.cuda.synchronize()
    assert steps(B._h) == 5 and all(torch.equal(a, b) for a, b in zip(before, tensors_b()))
    A.close()
    B.close()


# ------------------------------------------------------------------------------------------------ 8. one tool end to end
def test_idqn_tool_saves_resumes_and_evaluates(short_episode, tmp_path):
    from tools.idqn_train import main
    path = str(tmp_path / 'tool.pt')
    rows, final = main(MAP, N, 3, device_loop=True, quiet=True)
    part, none = main(MAP, N, 3, device_loop=True, quiet=True, save=path, save_replay=True, stop_after=2)
    assert none is None and len(part) == 2
    rows_r, final_r = main(MAP, N, 3, device_loop=True, quiet=True, load=path, save=path, save_replay=True)
    assert final_r == final
    keys = ('episode', 'epsilon', 'mean_return', 'avg_delay_s', 'arrived_per_env', 'updates')
    assert [{k: r[k] for k in keys} for r in rows_r] == [{k: r[k] for k in keys} for r in rows]
    # --eval on the file the resumed run left: the weights alone, the greedy policy and the simulator are functions of weights and seed
    _, final_e = main(MAP, N, 3, device_loop=True, quiet=True, load=path, eval_only=True)
    assert final_e['greedy_avg_delay_s'] == final['greedy_avg_delay_s'] is not None
    assert final_e['greedy_on_last_training_seed_s'] == final['greedy_on_last_training_seed_s'] is not None
    assert final_e == final


# ------------------------------------------------------------------------------------------------ the flags of every tool and mode
def _tool(name):
    from tools import fma2c_train, idqn_train, ippo_train, mplight_train
    return {'idqn-update': (idqn_train.main, (32,), dict(device_update=True, quiet=True, evaluate=False)),
            'idqn-torch': (idqn_train.main, (32,), dict(use_graph=False, quiet=True, evaluate=False)),
            'idqn-graph': (idqn_train.main, (32,), dict(use_graph=True, quiet=True, evaluate=False)),
            'mplight-loop': (mplight_train.main, (32, CAPACITY), dict(device_loop=True, quiet=True)),
            'mplightfull-update': (mplight_train.main, (32, CAPACITY), dict(device_update=True, full=True, quiet=True)),
            'mplight-torch': (mplight_train.main, (32, CAPACITY), dict(quiet=True)),
            'ippo-loop': (ippo_train.main_device_loop, (SEG,), {}),
            'ippo-shuffle': (ippo_train.main_device_rollout, (SEG,), dict(device_update=True, device_shuffle=True)),
            'ippo-torch': (ippo_train.main, (SEG,), {}),
            'fma2c-loop': (fma2c_train.main, (), dict(device_loop=True, quiet=True)),
            'fma2c-update': (fma2c_train.main, (), dict(device_update=True, device_rewards=True, quiet=True)),
            'fma2c-torch': (fma2c_train.main, (), dict(quiet=True))}[name]


# the modes whose update is a fixed-order HIP kernel give the same bits twice; PyTorch's backward (atomics) does not promise that
EXACT = ('idqn-update', 'mplight-loop', 'mplightfull-update', 'ippo-loop', 'ippo-shuffle', 'fma2c-loop', 'fma2c-update')


@pytest.mark.parametrize('name', ['idqn-update', 'idqn-torch', 'idqn-graph', 'mplight-loop', 'mplightfull-update', 'mplight-torch', 'ippo-loop',
                                  'ippo-shuffle', 'ippo-torch', 'fma2c-loop', 'fma2c-update', 'fma2c-torch'])
def test_tool_flags_in_every_mode(short_episode, tmp_path, name):
    """two planned episodes: straight with --save; with --save --stop-after 1, then --load --save; then --load --eval.  The two
    final files hold the same state -- the same bits where the update is a HIP kernel."""
    main, args, kw = _tool(name)
    x, y = str(tmp_path / 'x.pt'), str(tmp_path / 'y.pt')
    main(MAP, N, 2, *args, **kw, save=x, save_replay=True)
    main(MAP, N, 2, *args, **kw, save=y, save_replay=True, stop_after=1)
    assert torch.load(y, weights_only=True)['progress']['episode'] == 1
    main(MAP, N, 2, *args, **kw, load=y, save=y, save_replay=True)
    X, Y = torch.load(x, weights_only=True), torch.load(y, weights_only=True)
    same(X['signature'], Y['signature'])
    assert X['progress']['episode'] == Y['progress']['episode'] == 2
    if name in EXACT:
        timing = ('env_steps_per_s', 'ms_per_step')
        rows = lambda ck: [{c: v for c, v in r.items() if c not in timing} for r in ck['progress'].get('rows', [])]
        same(rows(X), rows(Y))
        same(X['objects'], Y['objects'])
    else:
        scalars = lambda ck: {k: v for k, v in ck['objects']['learner']['state'].items() if k in ('t', 'n_updates', 'updates', 'steps_done', 'n')}
        assert scalars(X) == scalars(Y) and len(scalars(X)) >= 1
    out = main(MAP, N, 2, *args, **kw, load=y, eval_only=True)
    if not name.startswith('ippo'):         # (the IPPO tool prints its lines and returns none)
        final = out[1]
        assert final.get('greedy_avg_delay_s', final.get('eval_avg_delay_s')) is not None
