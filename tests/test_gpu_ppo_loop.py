"""GPU: the PPO training loop of IPPO in the library (rs_group_ppo_train, agents/train_fused.py: DevicePPOTrainer) and the two entry
points it adds.  rs_ppo_perm against the host build of its body, rs_ippo_pack_weights against FusedIPPO.refresh_on_device byte for
byte, the loop against the --device-update loop of tools/ippo_train.py in Python driven with the same shuffles
(perm=learner.device_perm(...)): the policy draws by the global environment index and the shuffle is a counter hash, so every array and
every figure must be EQUAL, no tolerance -- on cologne1 x 16 and ingolstadt21 x 8 (21 signals of unequal lanes and actions), for any
split of an episode into calls.  Horizon 20 steps, segments of 6 (the fourth spans the reset), 2 epochs, minibatch 40 on 96 rows (a
short last minibatch) and 20 on 48.  The refusals launch nothing."""
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

from resco_amd.agents.ippo import BatchedIPPO
from resco_amd.agents.ippo_fused import DeviceRollout, FusedIPPO
from resco_amd.agents.ippo_learn_fused import FusedPPOLearner
from resco_amd.agents.train_fused import DevicePPOTrainer
from resco_amd.multi_signal import VecMultiSignal, load_scenario, map_configs
from resco_amd.sim import PPO_TENSORS, PPOTensors, SimGroup, load_library, torch_stream
from tools import ippo_train
from train_ref import build_host

pytestmark = pytest.mark.gpu

STEPS, T, EPOCHS, EPISODES = 20, 6, 2, 2
CASES = {'cologne1': ('cologne1', 16, 40), 'ingolstadt21': ('ingolstadt21', 8, 20)}
SPLITS = {'whole': (20,), 'two': (7, 13), 'ones': (1,) * 20}
PACKED = ('w1', 'w2', 'w3', 'b3')


@pytest.fixture
def short_episode(monkeypatch):
    init = VecMultiSignal.__init__

    def short(self, *a, **kw):
        init(self, *a, **kw)
        self.horizon_steps = STEPS

    monkeypatch.setattr(VecMultiSignal, '__init__', short)


def scenario(map_name):
    return load_scenario(map_name, None, map_configs.get(map_name, {}).get('lights', ()), 3)


def setup(map_name, n, minibatch):
    """the objects of tools/ippo_train.py: main_device_rollout, with this file's segment, epochs and minibatch"""
    env = VecMultiSignal(map_name, n, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
    net = BatchedIPPO.from_scenario(env.scenario, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=0)
    learner = FusedPPOLearner(net, epochs=EPOCHS, minibatch=minibatch, seed=11)
    policy = FusedIPPO(net, seed=3)
    policy.refresh_on_device()
    return types.SimpleNamespace(env=env, net=net, learner=learner, policy=policy, rec=DeviceRollout(T, [env.sim]), n=n, S=env.n_signals)


def row(X, ep):
    return dict(episode=ep, avg_delay_s=round(float(X.env.sim.trip_delay().mean()), 2), arrived_per_env=round(float(X.env.sim.stats()['arrived'].mean()), 1),
                adam_steps=X.learner.n_updates)


def snapshot(X, adv, ret, done, rows):
    """everything the two loops must agree on, as host copies"""
    torch.cuda.synchronize()
    L = X.learner
    tensors = {'par.' + k: getattr(X.net, k) for k in PPO_TENSORS}
    tensors.update({'m.' + k: L.m[k] for k in PPO_TENSORS})
    tensors.update({'v.' + k: L.v[k] for k in PPO_TENSORS})
    tensors.update({'seg.' + k: X.rec.pipes[0][k] for k in DeviceRollout.FIELDS})
    tensors.update({'pack.' + k: X.policy._dev[k] for k in PACKED})
    tensors.update({'adv': adv.reshape(T, X.n, X.S), 'ret': ret.reshape(T, X.n, X.S), 'done': done, 'loss_out': L.loss_out, 'actions': X.env.tensor('actions')})
    out = {k: t.detach().cpu().clone() for k, t in tensors.items()}
    out['scalars'] = dict(rs_ppo_steps=L.n_updates, env_steps=X.env.steps)
    out['rows'] = rows
    return out


def python_training(map_name, n, minibatch):
    """the loop of tools/ippo_train.py: main_device_rollout(device_update=True), driven with the learner's own shuffles"""
    X = setup(map_name, n, minibatch)
    env, L, P, rec = X.env, X.learner, X.policy, X.rec
    grp = SimGroup([env.sim])
    obs = env.tensor('drq_norm_f16')
    done = [False] * T
    t_global, i, updates, rows = 0, 0, 0, []
    for ep in range(EPISODES):
        env.sim.set_seed(1000 + ep)
        env.reset()
        torch.cuda.synchronize()
        k = 0
        while k < STEPS:
            m = min(T - i, STEPS - k)
            grp.rollout(rec, P.handle, t0=i, n_steps=m, step_key=t_global, seed=P.seed)
            k, i, t_global = k + m, i + m, t_global + m
            done[i - 1] = env.advance(m)
            if i == T:
                grp.sync()
                L.update_from_rollout(rec, P.value(obs), torch.as_tensor(done, device='cuda'), perm=L.device_perm(T * n, updates))
                updates += 1
                P.refresh_on_device()
                torch.cuda.current_stream().synchronize()
                done, i = [False] * T, 0
        grp.sync()
        torch.cuda.synchronize()
        rows.append(row(X, ep))
    ds = L._keep[0]                 # the last update's dataset
    snap = snapshot(X, ds['adv'], ds['ret'], torch.as_tensor(done[:i], dtype=torch.uint8), rows)
    snap['scalars'].update(slot=i, t=t_global, updates=updates)
    L.close()
    env.close()
    return snap


def library_training(map_name, n, minibatch, split):
    X = setup(map_name, n, minibatch)
    trainer = DevicePPOTrainer(X.env, X.learner, X.policy, X.rec)
    rows = []
    for ep in range(EPISODES):
        X.env.sim.set_seed(1000 + ep)
        X.env.reset()
        done = False
        for c in split:
            assert not done
            done = trainer.run(c)
        assert done
        torch.cuda.synchronize()
        rows.append(row(X, ep))
    snap = snapshot(X, trainer.adv, trainer.ret, trainer.done[:trainer.slot], rows)
    snap['scalars'].update(slot=trainer.slot, t=trainer.t, updates=trainer.updates)
    X.learner.close()
    X.env.close()
    return snap


_reference = {}


def reference(case):
    """the Python loop's result, computed once per case and never changed"""
    if case not in _reference:
        _reference[case] = python_training(*CASES[case])
    return _reference[case]


@pytest.mark.parametrize('split', SPLITS)
@pytest.mark.parametrize('case', CASES)
def test_library_loop_equals_the_python_loop(short_episode, case, split):
    want = reference(case)
    got = library_training(*CASES[case], SPLITS[split])
    n_rows = T * CASES[case][1]
    per_update = EPOCHS * -(-n_rows // CASES[case][2])
    assert n_rows % CASES[case][2] != 0 or case != 'cologne1'              # cologne1: a short last minibatch
    assert want['scalars'] == dict(rs_ppo_steps=6 * per_update, env_steps=STEPS, slot=4, t=EPISODES * STEPS, updates=6)
    assert all(torch.isfinite(want[k]).all() for k in want if k.startswith('par.')) and want['loss_out'].abs().sum() > 0
    assert got['scalars'] == want['scalars']
    assert got['rows'] == want['rows']
    for k in want:
        if k not in ('scalars', 'rows'):
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def test_the_tool(short_episode, capsys):
    """tools/ippo_train.py --device-loop cologne1 16 2 6 2 against --device-update run through the same shuffle: the same two lines
    (but for the two figures of the wall clock)"""
    ippo_train.main_device_rollout('cologne1', 16, 2, 6, 2, device_update=True, device_shuffle=True)
    want = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    ippo_train.main_device_loop('cologne1', 16, 2, 6, 2)
    got = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    clock = ('env_steps_per_s', 'ms_per_step')
    assert len(want) == 2 and want[-1]['adam_steps'] == 6 * 4 and all(k in want[0] for k in clock)
    assert [{k: v for k, v in r.items() if k not in clock} for r in got] == [{k: v for k, v in r.items() if k not in clock} for r in want]


# ---------------------------------------------------------------------------------------------------------------- the entry points
def test_perm_equals_the_host_body(tmp_path):
    lib = load_library()
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    host = build_host('ppo_loop', tmp_path, dict(gp_host_perm=[i32, i32, u32, u32, vp, i32]))
    for n in (1, 65, 96, 1000):
        for seed, key in ((0, 0), (0xC0FFEE11, 7), (11, 2 ** 32 - 1)):
            got = torch.full((3 * n + 1,), -7, dtype=torch.int32, device='cuda')
            assert lib.rs_ppo_perm(n, 3, seed, key, got.data_ptr(), torch_stream(0)) == 0
            want = np.zeros((3, n), np.int32)
            assert host.gp_host_perm(n, 3, seed, key, want.ctypes.data, 1) == 0
            got = got.cpu().numpy()
            assert got[-1] == -7, 'written behind the rows'
            assert np.array_equal(got[:-1].reshape(3, n), want), (n, seed, key)
            assert np.array_equal(np.sort(want, axis=1), np.broadcast_to(np.arange(n, dtype=np.int32), (3, n)))
    buf = torch.zeros(8, dtype=torch.int32, device='cuda')
    for args, text in (((0, 1, 0, 0, buf.data_ptr()), b'1 <= n'), ((8, 0, 0, 0, buf.data_ptr()), b'epochs'), ((8, 1, 0, 0, None), b'NULL')):
        assert lib.rs_ppo_perm(*args, torch_stream(0)) == -1 and text in lib.rs_last_error(None)
    torch.cuda.synchronize()
    assert not bool(buf.any())


@pytest.mark.parametrize('map_name', ['cologne1', 'ingolstadt21'])
def test_ippo_pack_weights_equals_refresh_on_device(map_name):
    """byte for byte: w1, w2, w3 (with the value column) and b3.  Round 0: the initialised network, and the actor-critic kernel gives
    the same actions, log-probabilities and values on either pack.  Round 1: other weights, among them values that round to a
    denormal half, to zero at the tie below the smallest one, and to infinity.  (A padding element of refresh_on_device is source
    element 0 times zero, whose sign is that element's: the test keeps the three element 0 positive, so that +0 is what both write.)"""
    lib = load_library()
    net = BatchedIPPO.from_scenario(scenario(map_name), dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=3)
    with torch.no_grad():
        net.fc3_b.copy_(torch.randn_like(net.fc3_b) * 0.2)
        net.v_b.copy_(torch.randn_like(net.v_b) * 0.2)
        for k in ('fc1_w', 'fc2_w', 'fc3_w'):
            getattr(net, k)[:, 0, 0] = 0.125
    policy = FusedIPPO(net, seed=5)
    S, N = len(net.lanes), 37
    params = PPOTensors(*[getattr(net, k).data_ptr() for k in PPO_TENSORS])
    assert lib.rs_ippo_pack_weights(policy._h, C.byref(params), torch_stream(0)) == -1         # RS_EINVAL: still on the create-time copy
    assert b'create-time' in lib.rs_last_error(None)
    gen = torch.Generator(device='cuda').manual_seed(1)
    obs = (torch.rand(N, S, net.lmax, 5, device='cuda', generator=gen) * 2).to(torch.float16)
    for round_ in range(2):
        policy.refresh_on_device()
        d = policy._dev
        want = {k: d[k].clone() for k in PACKED}
        if round_ == 0:
            out_want = [t.clone() for t in policy.act(obs, step_key=9)]
        for k in PACKED:
            d[k].fill_(7.0)
        assert lib.rs_ippo_pack_weights(policy._h, C.byref(params), torch_stream(0)) == 0
        if round_ == 0:
            out_got = policy.act(obs, step_key=9)
        torch.cuda.synchronize()
        for k in PACKED:
            view = torch.int16 if k != 'b3' else torch.int32
            assert torch.equal(d[k].view(view), want[k].view(view)), k
            assert not bool(policy._pad[k][S * d[k].shape[1]:].any()) if k != 'b3' else True, 'written behind ' + k
        assert bool((want['b3'][:, 8] == net.v_b[:, 0]).all()) and bool((want['b3'][:, 9:] == 0).all())
        if round_ == 0:
            assert all(torch.equal(a, b) for a, b in zip(out_got, out_want)) and bool(out_want[2].abs().sum() > 0)
        else:
            w3 = want['w3'].view(S, 8, 64, 4)
            assert int(torch.isinf(want['w3']).sum()) == 2 and int(torch.isinf(w3[:, :, 8::32]).sum()) == 1        # one of them in the value column
            assert int(((want['w2'].view(torch.int16) & 0x7FFF) == 1).sum()) >= 1                                       # the smallest denormal half
        with torch.no_grad():       # other weights for the second round (padded fc1 rows stay zero: the masked learner keeps them so)
            for k in PPO_TENSORS:
                p = getattr(net, k)
                p.mul_(1.0 + 0.5 * torch.rand_like(p))
            net.fc2_w[0, 5, 7], net.fc2_w[0, 6, 7] = 2.0 ** -25 * 1.5, 2.0 ** -25          # -> 2^-24 (a denormal half); the tie -> 0
            net.fc3_w[S - 1, 9, 0], net.v_w[0, 4, 0], net.v_w[S - 1, 3, 0] = -70000.0, 70000.0, -2.0 ** -25 * 1.25
    policy.close()


# ---------------------------------------------------------------------------------------------------------------- the refusals
def _state(X):
    torch.cuda.synchronize()
    t = [getattr(X.net, k) for k in PPO_TENSORS] + [X.rec.pipes[0][k] for k in DeviceRollout.FIELDS] + [X.env.tensor('actions'), X.trainer.done, X.trainer.perm]
    return [a.detach().clone() for a in t]


def _train(X, group=None, n_steps=3, seg_T=None, **kw):
    L, tr = X.learner, X.trainer
    seg = X.rec.segments([X.env.sim])[0]
    if seg_T is not None:
        seg = type(seg)(seg.obs, seg.act, seg.logp, seg.value, seg.rew, seg_T)
    ptr = lambda t: t.data_ptr()
    args = dict(policy=X.policy.handle, learner=L._h, seg=seg, done=ptr(tr.done), last_value=ptr(tr.last_value), adv=ptr(tr.adv), ret=ptr(tr.ret),
                gae_scratch=ptr(tr._scratch), perm=ptr(tr.perm), t0=tr.t, update0=tr.updates, slot0=tr.slot, done_step=-1, epochs=L.epochs,
                minibatch=L.minibatch, gamma=L.gamma, lambd=L.lambd, policy_seed=X.policy.seed, learner_seed=L.seed, loss_out=ptr(L.loss_out))
    args.update(kw)
    (group or tr.group).ppo_train(n_steps, **args)


def test_refusals_launch_nothing(short_episode, monkeypatch):
    X = setup('cologne1', 16, 40)
    X.trainer = DevicePPOTrainer(X.env, X.learner, X.policy, X.rec)
    X.env.reset()
    X.trainer.run(8)                    # one update done, two slots of the second segment filled
    before, updates = _state(X), X.learner.n_updates
    assert updates == EPOCHS * 3 and X.trainer.slot == 2
    other = BatchedIPPO.from_scenario(scenario('ingolstadt21'), dtype=torch.float32, device='cuda')
    other.init_like_reference(seed=0)
    other_policy, other_learner = FusedIPPO(other, seed=1), FusedPPOLearner(other, minibatch=40)
    other_policy.refresh_on_device()
    fresh = FusedIPPO(X.net, seed=1)    # still on its create-time copy
    monkeypatch.setenv('RESCO_PLAIN_STREAMS', '1')
    plain = VecMultiSignal('cologne1', 16, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0, scenario=X.env.scenario)
    monkeypatch.delenv('RESCO_PLAIN_STREAMS')
    refusals = [(dict(group=SimGroup([X.env.sim, X.env.sim])), 'one handle only'), (dict(n_steps=0), 'n_steps >= 1'),
                (dict(slot0=-1), 'slot0'), (dict(slot0=T), 'slot0'), (dict(n_steps=3, done_step=3), 'done_step'), (dict(done_step=-2), 'done_step'),
                (dict(seg_T=0), 'T \\* n_envs'), (dict(minibatch=0), 'max_minibatch'), (dict(minibatch=41), 'max_minibatch'), (dict(epochs=0), 'epochs'),
                (dict(policy=other_policy.handle), 'built for this scenario'), (dict(learner=other_learner._h), 'learner does not fit'),
                (dict(policy=fresh.handle), 'create-time'), (dict(group=SimGroup([plain.sim])), 'non-blocking')]
    refusals += [({k: None}, 'NULL') for k in ('done', 'last_value', 'adv', 'ret', 'gae_scratch', 'perm', 'policy', 'learner')]
    for kw, text in refusals:
        with pytest.raises(RuntimeError, match=text):
            _train(X, **kw)
    seg = X.rec.segments([X.env.sim])[0]
    for k in DeviceRollout.FIELDS:
        broken = type(seg)(*[None if f == k else getattr(seg, f) for f in DeviceRollout.FIELDS], T)
        with pytest.raises(RuntimeError, match='NULL'):
            _train(X, seg=broken)
    X.env.sim.set_outputs(('mplight',))
    with pytest.raises(RuntimeError, match='switched off'):
        _train(X)
    X.env.sim.set_outputs(None)
    X.env.sim.timing(True)
    with pytest.raises(RuntimeError, match='rs_timing'):
        _train(X)
    X.env.sim.timing(False)
    # the wrapper's own: a call across the horizon, a side stream
    with pytest.raises(ValueError, match='cross the horizon'):
        X.trainer.run(STEPS)
    with torch.cuda.stream(torch.cuda.Stream()), pytest.raises(RuntimeError, match='default stream'):
        X.trainer.run(1)
    after = _state(X)
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and X.learner.n_updates == updates
    assert (X.trainer.slot, X.trainer.t, X.trainer.updates, X.env.steps) == (2, 8, 1, 8)
    assert X.trainer.run(12)            # and the loop still runs to the episode's end
    torch.cuda.synchronize()
    assert X.learner.n_updates == 3 * updates and X.trainer.slot == 2
    for o in (other_policy, fresh, other_learner, X.learner, plain, X.env):
        o.close()
