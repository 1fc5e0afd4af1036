"""GPU: the FMA2C training loop in the library (rs_group_fma2c_train, agents/train_fused.py: DeviceA2CTrainer) and the reward kernel it
adds (rs_fma2c_record).  The kernel against the host build of its body bit for bit on the buffers of a live simulator, and within the
two derived rounding bounds of VecMultiSignal.fma2c_rewards; the loop against the --device-update --device-rewards loop of
tools/fma2c_train.py in Python: the policy draws by the environment's index and the step key, the update has no floating-point
atomics, so every array and every figure must be EQUAL, no tolerance -- on cologne1 x 16 and ingolstadt21 x 8 (26 agents of unequal
widths), for any split of an episode into calls, and when calls and Python observe steps alternate.  Horizon 20 steps, segments of 6
(the fourth is cut by the episode's end after 2), 2 episodes.  The refusals launch nothing.

The reference ships no FMA2CFull hierarchy for cologne1 (resco_amd/config/mdp_configs.json: cologne8, ingolstadt7, ingolstadt21), so
the FMA2CFull case runs on cologne8, the smallest map that has one."""
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

from resco_amd.agents.fma2c import BatchedFMA2C, FMA2CLayout, FusedFMA2C
from resco_amd.agents.fma2c_learn_fused import FusedA2CLearner
from resco_amd.agents.train_fused import DeviceA2CTrainer
from resco_amd.config.agent_config import agent_configs
from resco_amd.config.mdp_config import activate
from resco_amd.multi_signal import VecMultiSignal
from resco_amd.sim import Fma2cRewardTable, Fma2cRewardTableStruct, SimGroup, load_library, torch_stream
from test_fma2c_loop_cpu import HOST_SIGNATURES, gamma
from tools import fma2c_train
from train_ref import build_host

pytestmark = pytest.mark.gpu

STEPS, T, EPISODES = 20, 6, 2
CASES = {'cologne1': ('cologne1', 16, False), 'ingolstadt21': ('ingolstadt21', 8, False)}
FULL_CASE = ('cologne8', 8, True)
SPLITS = {'whole': (20,), 'two': (7, 13), 'ones': (1,) * 20, 'mixed': (7, -13)}        # a negative entry: that many steps by the Python loop
POLICY_BUFFERS = ('state', 'fingerprints', 'mgr_actions', 'parity')
LEARNER_BUFFERS = ('weights', 'ms', 'states_bw', 'returns', 'advantages')


@pytest.fixture
def short_episode(monkeypatch):
    init = VecMultiSignal.__init__

    def short(self, *a, **kw):
        init(self, *a, **kw)
        self.horizon_steps = STEPS

    monkeypatch.setattr(VecMultiSignal, '__init__', short)


def setup(map_name, n, full, max_envs=None):
    """the objects of tools/fma2c_train.py --device-update, with this file's segment length"""
    cfg = agent_configs['FMA2CFULL' if full else 'FMA2C']
    activate('FMA2CFull' if full else 'FMA2C', map_name)
    env = VecMultiSignal(map_name, n, states=(), rewards=(), seed=0, max_distance=cfg['max_distance'], outputs=('lane_agg', 'lane_arrivals'))
    layout = FMA2CLayout(env.scenario, full)
    net = BatchedFMA2C(layout).init_like_reference(0).cuda()
    policy = FusedFMA2C(net, max_envs or n, seed=7)
    learner = FusedA2CLearner(net, policy, max_envs or n, batch_size=T, gamma=cfg['gamma'], lr=cfg['lr_init'], alpha=cfg['rmsp_alpha'], eps=cfg['rmsp_epsilon'],
                              max_grad_norm=cfg['max_grad_norm'], value_coef=cfg['value_coef'], entropy_coef=cfg['entropy_coef_init'],
                              reward_norm=cfg['reward_norm'], reward_clip=cfg['reward_clip'])
    return types.SimpleNamespace(env=env, layout=layout, net=net, policy=policy, learner=learner, n=n, full=full, K=layout.K, t=0,
                                 ret=torch.zeros(n, layout.K, device='cuda'), start=learner.buffer('weights').clone())


def close(X):
    X.policy.close()            # (closes its learner first)
    X.env.close()


def python_steps(X, n_steps):
    """n_steps iterations of the loop of tools/fma2c_train.py --device-update --device-rewards"""
    env, policy, learner = X.env, X.policy, X.learner
    lane_agg, actions = env.tensor('lane_agg'), env.tensor('actions')
    state, macts = policy.buffer('state'), policy.buffer('mgr_actions')
    done = False
    for _ in range(n_steps):
        out = policy.act(lane_agg, step_key=X.t, actions=actions, want=('value', 'rows'), out=learner.slot())
        acts = torch.cat([macts, out['actions']], dim=1).long()
        done = env.step(None)[2]
        rew = env.fma2c_rewards_device(X.full, policy=policy)
        X.ret += rew
        learner.observe(out['rows'], acts, rew, out['value'], done, state, lambda: policy.value(lane_agg))
        X.t += 1
    return done


def row(X, ep):
    torch.cuda.synchronize()
    return dict(episode=ep, avg_delay_s=round(float(X.env.sim.trip_delay().mean()), 2), arrived_per_env=round(float(X.env.sim.stats()['arrived'].mean()), 1),
                mean_return=float(X.ret.mean()), updates=X.learner.updates, loss=float(X.learner.last_loss.mean()))


def snapshot(X, rows):
    """everything the two loops must agree on, as host copies"""
    torch.cuda.synchronize()
    L = X.learner
    tensors = {'learner.' + k: L.buffer(k) for k in LEARNER_BUFFERS}
    tensors.update({'seg.' + k: getattr(L, k) for k in ('rows', 'acts', 'rews', 'vals', 'dones_dev')})
    tensors.update({'policy.' + k: X.policy.buffer(k) for k in POLICY_BUFFERS})
    tensors.update(actions=X.env.tensor('actions'), ret=X.ret, last_loss=L.last_loss)
    out = {k: t.detach().cpu().clone() for k, t in tensors.items()}
    out['scalars'] = dict(n=L.n, steps_done=L.steps_done, updates=L.updates, dones=list(L.dones), env_steps=X.env.steps, t=X.t)
    out['rows'] = rows
    out['start'] = X.start.cpu()
    return out


def training(map_name, n, full, split=None):
    """split None: the Python loop; else the library loop in calls of these lengths (a negative one: Python steps in between)"""
    X = setup(map_name, n, full)
    trainer = DeviceA2CTrainer(X.env, X.learner, X.policy, full) if split is not None else None
    if trainer is not None:
        X.ret = trainer.ret
    rows = []
    for ep in range(EPISODES):
        X.env.sim.set_seed(1000 + ep)
        X.env.reset()
        X.policy.reset()
        X.ret.zero_()
        done = False
        for c in (split if split is not None else (-STEPS,)):
            assert not done
            if c > 0:
                trainer.t = X.t
                done = trainer.run(c)
                X.t = trainer.t
            else:
                done = python_steps(X, -c)
        assert done
        rows.append(row(X, ep))
    snap = snapshot(X, rows)
    close(X)
    return snap


_reference = {}


def reference(case):
    """the Python loop's result, computed once per case and never changed"""
    if case not in _reference:
        _reference[case] = training(*(CASES[case] if case in CASES else FULL_CASE))
    return _reference[case]


def assert_equal_runs(got, want):
    assert want['scalars'] == dict(n=0, steps_done=0, updates=8, dones=[True], env_steps=STEPS, t=EPISODES * STEPS)
    w = want['learner.weights']
    assert bool(torch.isfinite(w).all()) and not torch.equal(w, want['start']) and float(want['last_loss'].abs().sum()) > 0
    assert float(want['ret'].abs().sum()) > 0 and float(want['seg.rews'].abs().sum()) > 0
    assert got['scalars'] == want['scalars']
    assert got['rows'] == want['rows']
    for k in want:
        if k not in ('scalars', 'rows'):
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


@pytest.mark.parametrize('split', SPLITS)
@pytest.mark.parametrize('case', CASES)
def test_library_loop_equals_the_python_loop(short_episode, case, split):
    assert_equal_runs(training(*CASES[case], SPLITS[split]), reference(case))


def test_library_loop_equals_the_python_loop_full_variant(short_episode):
    assert_equal_runs(training(*FULL_CASE, SPLITS['two']), reference('full'))


def test_the_tool(short_episode, capsys):
    """tools/fma2c_train.py --device-loop cologne1 16 2 against --device-update --device-rewards: the same lines but for the wall clock"""
    fma2c_train.main('cologne1', 16, 2, device_update=True, device_rewards=True)
    want = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    fma2c_train.main('cologne1', 16, 2, device_loop=True)
    got = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    clock = ('env_steps_per_s',)
    # (the tool's segment is the agent's batch_size, 120 steps: an episode of 20 ends in one update, on 20 slots)
    assert len(want) == 3 and want[1]['updates'] == 2 and want[1]['loss'] is not None and all(k in want[0] for k in clock)
    assert [{k: v for k, v in r.items() if k not in clock} for r in got] == [{k: v for k, v in r.items() if k not in clock} for r in want]


# ---------------------------------------------------------------------------------------------------------------- the reward kernel
@pytest.mark.parametrize('case', CASES)
def test_record_equals_the_host_body(case, tmp_path):
    map_name, n, full = CASES[case]
    X = setup(map_name, n, full)
    env, policy, K, M, S, O = X.env, X.policy, X.K, X.layout.M, X.layout.S, X.layout.O
    host = build_host('fma2c_loop', tmp_path, HOST_SIGNATURES)
    table = Fma2cRewardTable(env.scenario, X.layout.cfg, full)
    env.sim.set_seed(1000)
    env.reset()
    lane_agg, actions = env.tensor('lane_agg'), env.tensor('actions')
    for k in range(12):
        env.act_random(k)
        env.step(None)
    policy.act(lane_agg, step_key=3, actions=actions, want=())         # the managers' and the workers' actions of a step
    guard = lambda dtype, fill: torch.full((n * K + 1,), fill, dtype=dtype, device='cuda')
    rew, acts, ret = guard(torch.float32, -7.5), guard(torch.int32, -9), guard(torch.float32, 0.25)
    view = lambda t: t[:n * K].view(n, K)
    for _ in range(3):
        env.sim.fma2c_record(policy.handle, table, view(rew), view(acts), view(ret), stream=torch_stream(0))
    only = env.fma2c_rewards_device(full, policy=policy)                # neither actions nor a return
    dense = env.fma2c_rewards(full)
    torch.cuda.synchronize()
    assert float(rew[-1]) == -7.5 and int(acts[-1]) == -9 and float(ret[-1]) == 0.25, 'written behind an output'
    agg = lane_agg.cpu().numpy()
    assert agg[..., 0].sum() > 0, 'no vehicle queued in the window'
    f = lambda name: np.ascontiguousarray(env.tensor(name).cpu().numpy())
    larr, arr, dep = f('lane_arrivals'), f('arrivals'), f('departures')
    macts, wacts = np.ascontiguousarray(policy.buffer('mgr_actions').cpu().numpy()), f('actions')
    p = lambda a: a.ctypes.data
    off, idx, w = table.off.cpu().numpy(), table.idx.cpu().numpy(), table.w.cpu().numpy()
    want, want_acts = np.zeros((n, K), np.float32), np.zeros((n, K), np.int32)
    assert host.fl_host_record(K, M, O, S, n, p(off), p(idx), p(w), p(agg), p(larr), p(arr), p(dep), p(macts), p(wacts), p(want), p(want_acts), None, 1) == 0
    got = view(rew).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), 'the kernel and the host body differ'
    assert np.abs(got[:, :M]).max() > 0 and np.abs(got[:, M:]).max() > 0, 'a zero reward'
    assert np.array_equal(only.cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(view(acts).cpu().numpy(), want_acts) and np.array_equal(want_acts, np.concatenate([macts, wacts], axis=1))
    run = np.full((n, K), 0.25, np.float32)
    for _ in range(3):
        run = run + want
    assert np.array_equal(view(ret).cpu().numpy().view(np.int32), run.view(np.int32))
    # against the dense product of fma2c_rewards: each side within its own bound of the exact sum
    G = np.concatenate([agg[..., 0], agg[..., 3], larr, arr, dep], axis=1).astype(np.float64)
    Wd = np.zeros((3 * O + 2 * S, K))
    for k in range(K):
        Wd[idx[off[k]:off[k + 1]], k] = w[off[k]:off[k + 1]]
    mag = np.abs(G) @ np.abs(Wd)
    dense = np.stack([dense[a].cpu().numpy() for a in X.layout.agents], axis=1)
    err = np.abs(got.astype(np.float64) - dense.astype(np.float64))
    bound = (gamma(np.diff(off).astype(np.float64))[None] + gamma(3 * O + 2 * S)) * mag
    print('%s: max |record - dense| %.3e, bound %.3e at that element' % (case, err.max(), bound.reshape(-1)[err.argmax()]))
    assert (err <= bound).all()
    close(X)


# ---------------------------------------------------------------------------------------------------------------- the refusals
def _state(X):
    torch.cuda.synchronize()
    L = X.learner
    t = [L.buffer(k) for k in LEARNER_BUFFERS + ('grads',)] + [L.rows, L.acts, L.rews, L.vals, L.dones_dev, L._loss] + \
        [X.policy.buffer(k) for k in POLICY_BUFFERS] + [X.env.tensor('actions'), X.trainer.ret, X.trainer.R_boot, X.guard]
    return [a.detach().clone() for a in t], (L.n, L.steps_done, L.updates, list(L.dones), X.env.steps, X.trainer.t)


def _train(X, group=None, n_steps=3, table=None, **kw):
    L, tr = X.learner, X.trainer
    ptr = lambda t: t.data_ptr()
    args = dict(policy=X.policy.handle, learner=L.handle, table=table if table is not None else tr.table, rows=ptr(L.rows), acts=ptr(L.acts),
                rews=ptr(L.rews), vals=ptr(L.vals), dones=ptr(L.dones_dev), R_boot=ptr(tr.R_boot), T=L.T, t0=tr.t, slot0=L.n, done_step=-1,
                policy_seed=X.policy.seed, ret=ptr(tr.ret), loss_out=ptr(L._loss))
    args.update(kw)
    (group or tr.group).fma2c_train(n_steps, **args)


def test_refusals_launch_nothing(short_episode, monkeypatch):
    from resco_amd.agents.ippo import BatchedIPPO
    from resco_amd.agents.ippo_fused import FusedIPPO
    lib = load_library()
    X = setup('cologne1', 16, False)
    X.trainer = DeviceA2CTrainer(X.env, X.learner, X.policy)
    X.guard = torch.full((16 * X.K + 1,), -7.5, device='cuda')
    rew = X.guard[:16 * X.K].view(16, X.K)
    X.env.reset()
    X.policy.reset()
    X.trainer.run(8)                    # one update done, two slots of the second segment filled
    before = _state(X)
    assert before[1] == (2, 8, 1, [False, False, False], 8, 8)
    sim, tab = X.env.sim, X.trainer.table
    ippo_net = BatchedIPPO.from_scenario(X.env.scenario, dtype=torch.float32, device='cuda')
    ippo_net.init_like_reference(seed=0)
    ippo = FusedIPPO(ippo_net, seed=1)                                  # an rs_idqn_create policy
    Y = setup('cologne8', 16, False)                                     # an FMA2C policy of another scenario
    activate('FMA2C', 'cologne1')
    wide = FusedFMA2C(X.net, 32, seed=7)                                # max_envs is not the handle's n_envs
    twin = FusedFMA2C(X.net, 16, seed=7)
    twin_learner = FusedA2CLearner(X.net, twin, 16, batch_size=T)       # a learner created for another policy
    monkeypatch.setenv('RESCO_PLAIN_STREAMS', '1')
    plain = VecMultiSignal('cologne1', 16, states=(), rewards=(), seed=0, scenario=X.env.scenario, outputs=('lane_agg', 'lane_arrivals'))
    monkeypatch.delenv('RESCO_PLAIN_STREAMS')
    s = tab.struct
    table_cases = [(Fma2cRewardTableStruct(s.K + 1, s.n_rows, s.off, s.idx, s.w), "table's K"), (Fma2cRewardTableStruct(s.K, s.n_rows + 1, s.off, s.idx, s.w), 'n_rows'),
                   (Fma2cRewardTableStruct(s.K, s.n_rows, None, s.idx, s.w), 'NULL'), (Fma2cRewardTableStruct(s.K, s.n_rows, s.off, None, s.w), 'NULL'),
                   (Fma2cRewardTableStruct(s.K, s.n_rows, s.off, s.idx, None), 'NULL')]

    # rs_fma2c_record
    err = lambda: (lib.rs_last_error(None) or b'').decode()
    assert lib.rs_fma2c_record(None, X.policy.handle, C.byref(s), rew.data_ptr(), None, None, 1) == -1 and 'NULL handle' in err()
    record = [(dict(policy=None), 'policy handle is NULL'), (dict(table=None), 'NULL'), (dict(rew_out=None), 'rew_out is NULL'),
              (dict(policy=ippo.handle), 'not an rs_fma2c_create policy'), (dict(policy=Y.policy.handle), 'built for this scenario')]
    record += [(dict(table=t), text) for t, text in table_cases]
    for kw, text in record:
        a = dict(policy=X.policy.handle, table=tab, rew_out=rew)
        a.update(kw)
        with pytest.raises(RuntimeError, match=text):
            sim.fma2c_record(a['policy'], a['table'], a['rew_out'], stream=torch_stream(0))
    for outputs, text in ((('lane_arrivals',), 'RS_BUF_LANE_AGG, which rs_set_outputs has switched off'), (('lane_agg',), 'RS_BUF_LANE_ARRIVALS, which rs_set_outputs')):
        sim.set_outputs(outputs)
        with pytest.raises(RuntimeError, match=text):
            sim.fma2c_record(X.policy.handle, tab, rew, stream=torch_stream(0))
        with pytest.raises(RuntimeError, match=text):
            _train(X)
    sim.set_outputs(('lane_agg', 'lane_arrivals'))

    # rs_group_fma2c_train
    refusals = [(dict(group=SimGroup([sim, sim])), 'one handle only'), (dict(n_steps=0), 'n_steps >= 1'), (dict(slot0=-1), 'slot0'), (dict(slot0=T), 'slot0'),
                (dict(n_steps=3, done_step=3), 'done_step must be -1'), (dict(done_step=-2), 'done_step must be -1'),
                (dict(n_steps=3, done_step=1), 'does not run past a done'), (dict(T=0), 't_max'), (dict(T=T + 1), 't_max'), (dict(t0=-1), 't0 >= 0'),
                (dict(policy=ippo.handle), 'not an rs_fma2c_create policy'), (dict(policy=Y.policy.handle), 'built for this scenario'),
                (dict(policy=wide.handle), "max_envs must be the handle's n_envs"), (dict(learner=twin_learner.handle), 'created for another policy'),
                (dict(group=SimGroup([plain.sim])), 'non-blocking')]
    refusals += [({k: None}, 'NULL') for k in ('rows', 'acts', 'rews', 'vals', 'dones', 'R_boot', 'policy', 'learner')]
    refusals += [(dict(table=t), text) for t, text in table_cases]
    for kw, text in refusals:
        with pytest.raises(RuntimeError, match=text):
            _train(X, **kw)
    sim.timing(True)
    with pytest.raises(RuntimeError, match='rs_timing'):
        _train(X)
    sim.timing(False)
    # the wrapper's own: a call across the horizon, a side stream, other classes
    with pytest.raises(ValueError, match='cross the horizon'):
        X.trainer.run(STEPS)
    with torch.cuda.stream(torch.cuda.Stream()), pytest.raises(ValueError, match='default stream'):
        X.trainer.run(1)
    with pytest.raises(TypeError, match='FusedA2CLearner'):
        DeviceA2CTrainer(X.env, X.learner, ippo)
    with pytest.raises(ValueError, match='another policy'):
        DeviceA2CTrainer(X.env, twin_learner, X.policy)
    after = _state(X)
    assert after[1] == before[1] and all(torch.equal(a, b) for a, b in zip(before[0], after[0]))
    assert X.trainer.run(12)            # and the loop still runs to the episode's end
    torch.cuda.synchronize()
    L = X.learner
    assert (L.n, L.steps_done, L.updates, L.dones, X.env.steps, X.trainer.t) == (0, 0, 4, [True], STEPS, STEPS) and bool(torch.isfinite(L.last_loss).all())
    twin.close()
    wide.close()
    ippo.close()
    plain.close()
    close(Y)
    close(X)
