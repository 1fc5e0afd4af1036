#!/usr/bin/env python3
"""A/B: does splitting the environments over K pipes pay in TRAINING when the loop stays in Python?  (It does not:
profiles/r12_train_pipes.txt.)

    python tools/train_pipes_ab.py idqn|mplight [map] [n_envs] [episodes] [runs]

Variant 1 is the training loop of tools/idqn_train.py / tools/mplight_train.py with --device-update as it is (one handle).  Variants
2 and 4 are the same training on K handles of N / K environments with env_base offsets: per env-step the policy and step kernels of
all pipes are enqueued by ONE rs_group_step call, each pipe on its own stream; the replay ring and the fused learner see the
concatenation of the pipes (pipe i owns rows sum(n[:i]) ..), and MPLight's global pair index is looked up from the local action
taken.  That is the single handle's training bit for bit (tests/test_gpu_train_pipes.py), so the rates compare like with like.  The
variants alternate inside the process, `runs` rounds; the first episode of a run warms up.  Prints one line per run and a JSON
summary.  A measurement script: the tools themselves keep one handle.

Variants loop1, loop2 and loop4 are the same training again with the loop inside the library (agents/train_fused.py: DeviceTrainer,
rs_group_train: one call per episode) on 1, 2 and 4 pipes -- the same bits once more (tests/test_gpu_group_train.py); their ratios
are to variant 1, the Python-driven loop of the same process (profiles/r13_group_train.txt)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resco_amd.agents.idqn_fused import FusedIDQN                                           # noqa: E402
from resco_amd.agents.idqn_learn import DeviceReplay, linear_epsilon                        # noqa: E402
from resco_amd.agents.idqn_learn_fused import FusedDQNLearner                               # noqa: E402
from resco_amd.agents.idqn_rollout import BatchedIDQN                                       # noqa: E402
from resco_amd.agents.mplight import FusedMPLight, MPLightReplay, frap_from_scenario        # noqa: E402
from resco_amd.agents.mplight_learn_fused import FusedMPLightLearner                        # noqa: E402
from resco_amd.agents.train_fused import DeviceTrainer                                      # noqa: E402
from resco_amd.multi_signal import VecMultiSignal, load_scenario, map_configs               # noqa: E402
from resco_amd.sim import SimGroup, load_library                                            # noqa: E402
from tools import idqn_train, mplight_train                                                 # noqa: E402


def pipe_sizes(n_envs, pipes):
    """n_envs environments over `pipes` handles, as evenly as they go: the first n_envs % pipes get one more"""
    n, k = int(n_envs), int(pipes)
    if not 1 <= k <= n:
        raise ValueError('need 1 <= pipes <= n_envs')
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


def pair_of_action(order, actions):
    """MPLight: the global phase pair behind every local action.  order: int64 tensor [S, P] (sim.maxwave_tables: the valid pairs of
    a signal in dict order; a signal's local actions in that order are 0 .. n - 1, which rs_mplight_create enforces); actions int32
    [N, S] -> int32 [N, S]."""
    sig = torch.arange(order.shape[0], device=actions.device)
    return order[sig, actions.long()].to(torch.int32)


class PipedEnvs:
    """K VecMultiSignal that together hold n_envs environments, stepped under an on-device policy by one call per env-step.  The
    pipes' own streams are blocking streams, ordered with PyTorch's LEGACY default stream only: the ring copies and the learner must
    run there, which step() checks."""

    def __init__(self, map_name, n_envs, pipes, **kw):
        if os.environ.get('RESCO_PLAIN_STREAMS') is not None:
            raise RuntimeError('RESCO_PLAIN_STREAMS makes the handles\' streams non-blocking: nothing would order them with the ring copies')
        sizes = pipe_sizes(n_envs, pipes)
        sc = load_scenario(map_name, None, map_configs.get(map_name, {}).get('lights', ()), 3)
        if len(sizes) > 1:      # the workgroup shape for the device's whole load, not for one pipe's share
            kw = dict(kw, block_threads=load_library().rs_default_block(int(sc.capacity), int(n_envs), 0))
        self.envs, base = [], 0
        for n in sizes:
            self.envs.append(VecMultiSignal(map_name, n, env_base=base, scenario=sc, **kw))
            base += n
        self.group = SimGroup([e.sim for e in self.envs])
        self.scenario, self.n_signals, self.horizon_steps = sc, self.envs[0].n_signals, self.envs[0].horizon_steps

    def set_seed(self, seed):
        for e in self.envs:
            e.sim.set_seed(seed)

    def reset(self):
        for e in self.envs:
            e.reset()

    def cat(self, name):
        """buffer `name` of all pipes, rows in group order"""
        return torch.cat([e.tensor(name) for e in self.envs])

    def step(self, agent, policy=None, epsilon=0.0, step_key=0):
        """act and step, every pipe on its own stream: rs_group_step.  Returns done."""
        if torch.cuda.current_stream().cuda_stream != 0:
            raise RuntimeError('PipedEnvs needs PyTorch\'s default stream current: only that one is ordered with the pipes\' streams')
        if policy is None:
            self.group.step(agent, step_key=step_key)
        else:
            self.group.step(agent, step_key=step_key, policy=policy.handle, epsilon=epsilon, seed=policy.seed)
        return [e.advance(1) for e in self.envs][0]

    def delay(self):
        """mean over all environments of utils/readXML.py's episode figure, and of the arrived vehicles"""
        return (float(np.concatenate([e.sim.trip_delay() for e in self.envs]).mean()),
                float(np.concatenate([e.sim.stats()['arrived'] for e in self.envs]).mean()))

    def close(self):
        for e in self.envs:
            e.close()


def train_piped(agent, map_name='cologne1', n=256, episodes=4, batch=256, pipes=2, seed=0, full=False):
    """The training of tools/idqn_train.py (agent 'idqn') or tools/mplight_train.py ('mplight'; full: MPLightFULL) with
    device_update=True -- same seeds, ring, schedule and rows -- on `pipes` handles.  Returns the rows."""
    idqn = agent == 'idqn'
    state = 'drq_norm_f16' if idqn else ('mplight_full' if full else 'mplight')
    reward = 'wait_norm' if idqn else 'pressure'
    kw = dict(states=(state,), rewards=(reward,), seed=0)
    if not idqn:
        kw['outputs'] = (state,)
    pe = PipedEnvs(map_name, n, pipes, **kw)
    S, steps = pe.n_signals, pe.horizon_steps
    if idqn:
        net = BatchedIDQN.from_scenario(pe.scenario, dtype=torch.float32, device='cuda')
        net.init_like_reference(seed=seed)
        learner = FusedDQNLearner(net, gamma=0.99, lr=1e-3, target_update=500, batch_size=batch, seed=seed)
        policy = FusedIDQN(net, seed=7 + seed)
        replay = DeviceReplay(min(2048, 4 * steps), n, S, net.lmax, device='cuda')
    else:
        net = frap_from_scenario(pe.scenario, 4 if full else 1).cuda()
        net.init_like_reference(seed)
        learner = FusedMPLightLearner(net, gamma=0.99, lr=1e-3, target_update=500, batch_size=batch, seed=seed, n_signals=S)
        policy = FusedMPLight(net, pe.scenario, seed=7 + seed)
        policy.share_weights(learner.flat)
        replay = MPLightReplay(2048, n, S, 1 + 12 * net.demand_shape, device='cuda')
        order = torch.as_tensor(policy.order, dtype=torch.long, device='cuda')
    decay = int(0.8 * episodes * steps)
    rows = []
    for ep in range(episodes):
        pe.set_seed(1000 + ep + 7919 * seed)
        pe.reset()
        ret = torch.zeros(n, S, device='cuda')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            eps = linear_epsilon(learner.t, 1.0, 0.0, decay)
            replay.stage(pe.cat(state))
            done = pe.step(agent, policy, eps, learner.t)       # RS_BUF_ACTIONS keeps what was taken
            rew = pe.cat(reward).float()
            taken = pe.cat('actions')
            replay.commit(taken if idqn else pair_of_action(order, taken), rew, done)
            ret += rew
            if learner.observe_step(replay) is not None and idqn:
                policy.refresh_on_device()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        d, arrived = pe.delay()
        rows.append(dict(episode=ep, epsilon=round(eps, 3), mean_return=float(ret.sum(1).mean()) / S, avg_delay_s=round(d, 2),
                         arrived_per_env=round(arrived, 1), updates=learner.n_updates, env_steps_per_s=round(n * steps / dt)))
    learner.close()
    pe.close()
    return rows


def train_device_loop(agent, map_name='cologne1', n=256, episodes=4, batch=256, pipes=1, seed=0, full=False, chunks=None):
    """train_piped's training with the loop in the library: DeviceTrainer.run, one call per episode, or one per entry of `chunks`
    (step counts that add up to the horizon).  Returns the rows."""
    idqn = agent == 'idqn'
    state = 'drq_norm_f16' if idqn else ('mplight_full' if full else 'mplight')
    kw = dict(states=(state,), rewards=('wait_norm' if idqn else 'pressure',), seed=0)
    if not idqn:
        kw['outputs'] = (state,)
    pe = PipedEnvs(map_name, n, pipes, **kw)
    S, steps = pe.n_signals, pe.horizon_steps
    if idqn:
        net = BatchedIDQN.from_scenario(pe.scenario, dtype=torch.float32, device='cuda')
        net.init_like_reference(seed=seed)
        learner = FusedDQNLearner(net, gamma=0.99, lr=1e-3, target_update=500, batch_size=batch, seed=seed)
        policy = FusedIDQN(net, seed=7 + seed)
        replay = DeviceReplay(min(2048, 4 * steps), n, S, net.lmax, device='cuda')
    else:
        net = frap_from_scenario(pe.scenario, 4 if full else 1).cuda()
        net.init_like_reference(seed)
        learner = FusedMPLightLearner(net, gamma=0.99, lr=1e-3, target_update=500, batch_size=batch, seed=seed, n_signals=S)
        policy = FusedMPLight(net, pe.scenario, seed=7 + seed)
        policy.share_weights(learner.flat)
        replay = MPLightReplay(2048, n, S, 1 + 12 * net.demand_shape, device='cuda')
    trainer = DeviceTrainer(pe, learner, policy, replay, 1.0, 0.0, int(0.8 * episodes * steps))
    rows = []
    for ep in range(episodes):
        pe.set_seed(1000 + ep + 7919 * seed)
        pe.reset()
        ret = torch.zeros(n, S, device='cuda')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in (chunks or (steps,)):
            trainer.run(c, ret)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        d, arrived = pe.delay()
        rows.append(dict(episode=ep, epsilon=round(trainer.epsilon(learner.t - 1), 3), mean_return=float(ret.sum(1).mean()) / S, avg_delay_s=round(d, 2),
                         arrived_per_env=round(arrived, 1), updates=learner.n_updates, env_steps_per_s=round(n * steps / dt)))
    learner.close()
    pe.close()
    return rows


def train_one_handle(agent, map_name, n, episodes, batch=256, seed=0, full=False):
    """the tools' own loop with --device-update: the rows"""
    if agent == 'idqn':
        return idqn_train.main(map_name, n, episodes, batch, 1, evaluate=False, quiet=True, seed=seed, device_update=True)[0]
    return mplight_train.main(map_name, n, episodes, batch, seed=seed, full=full, quiet=True, device_update=True)[0]


def main(agent='idqn', map_name='ingolstadt21', n=1024, episodes=4, runs=2):
    res = {}
    for run in range(runs):
        for pipes in (1, 2, 4, 'loop1', 'loop2', 'loop4'):
            if isinstance(pipes, str):
                rows = train_device_loop(agent, map_name, n, episodes, pipes=int(pipes[4:]))
            else:
                rows = train_one_handle(agent, map_name, n, episodes) if pipes == 1 else train_piped(agent, map_name, n, episodes, pipes=pipes)
            rates = [r['env_steps_per_s'] for r in rows[1:]]
            res.setdefault(pipes, []).append(rates)
            print('%s %s x %d pipes %s run %d: %s env-steps/s, last delay %.2f s' % (agent, map_name, n, pipes, run, rates, rows[-1]['avg_delay_s']),
                  flush=True)
    base = np.mean(res[1])
    print(json.dumps(dict(agent=agent, map=map_name, envs=n, episodes=episodes, runs=runs, env_steps_per_s={str(k): v for k, v in res.items()},
                          ratio_to_one_handle={str(k): round(float(np.mean(v) / base), 3) for k, v in res.items()})))


if __name__ == '__main__':
    a = sys.argv[1:]
    main(a[0] if len(a) > 0 else 'idqn', a[1] if len(a) > 1 else 'ingolstadt21', int(a[2]) if len(a) > 2 else 1024,
         int(a[3]) if len(a) > 3 else 4, int(a[4]) if len(a) > 4 else 2)
