#!/usr/bin/env python3
"""A/B in ONE process: the PPO training loop in the library (tools/ippo_train.py --device-loop: one rs_group_ppo_train per episode)
against the Python-driven --device-update loop, alternating, `rounds` times each.

    python tools/ippo_loop_ab.py [map] [n_envs] [episodes] [rounds] [segment_steps] [minibatches_per_epoch]

Every round of a variant is a fresh run of the tool's own function (new environment, network, learner); its first episode warms up and
is dropped.  Prints per round and variant the env-steps/s with learning of the remaining episodes, and at the end one JSON line with
the medians, the ratio loop / python, the spread between the rounds of a variant, and ms per update = (episode time - the time of the
same episode's rollout without any update) / updates per episode, for both.  The two variants shuffle differently (torch.randperm
against the counter hash), so their trainings are not the same numbers; tests/test_gpu_ppo_loop.py holds them equal under one shuffle."""
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resco_amd.agents.ippo import BatchedIPPO                          # noqa: E402
from resco_amd.agents.ippo_fused import DeviceRollout, FusedIPPO      # noqa: E402
from resco_amd.multi_signal import VecMultiSignal                     # noqa: E402
from resco_amd.sim import SimGroup                                    # noqa: E402
from tools import ippo_train                                          # noqa: E402


def rows_of(fn, *a, **kw):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        fn(*a, **kw)
    return [json.loads(line) for line in out.getvalue().strip().splitlines()]


def rollout_only(map_name, n, episodes, seg):
    """seconds per episode of the recorded rollout alone (rs_group_rollout, `seg` steps per call), first episode dropped"""
    env = VecMultiSignal(map_name, n, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
    net = BatchedIPPO.from_scenario(env.scenario, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=0)
    policy = FusedIPPO(net, seed=3)
    policy.refresh_on_device()
    grp, rec = SimGroup([env.sim]), DeviceRollout(seg, [env.sim])
    steps, out, t_global = env.horizon_steps, [], 0
    for ep in range(episodes):
        env.sim.set_seed(1000 + ep)
        env.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(0, steps, seg):
            m = min(seg, steps - k)
            grp.rollout(rec, policy.handle, t0=0, n_steps=m, step_key=t_global, seed=policy.seed)
            env.advance(m)
            t_global += m
        grp.sync()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    env.close()
    return out[1:], steps


def main(map_name='cologne1', n=256, episodes=4, rounds=3, seg=30, mbs=4):
    variants = {'python': lambda: rows_of(ippo_train.main_device_rollout, map_name, n, episodes, seg, mbs, device_update=True),
                'loop': lambda: rows_of(ippo_train.main_device_loop, map_name, n, episodes, seg, mbs)}
    rates = {k: [] for k in variants}
    for r in range(rounds):
        for k, run in variants.items():
            rows = run()[1:]
            rates[k].append([row['env_steps_per_s'] for row in rows])
            print('ippo %s x %d seg %d %s round %d: %s env-steps/s, adam steps %d' % (map_name, n, seg, k, r, rates[k][-1], rows[-1]['adam_steps']), flush=True)
    base, steps = rollout_only(map_name, n, episodes, seg)
    t_roll = statistics.median(base)
    med = {k: statistics.median(x for rnd in v for x in rnd) for k, v in rates.items()}
    spread = {k: round(max(statistics.median(rnd) for rnd in v) / min(statistics.median(rnd) for rnd in v) - 1.0, 4) for k, v in rates.items()}
    ms = {k: round((n * steps / med[k] - t_roll) / (steps // seg) * 1e3, 2) for k in variants}
    print(json.dumps(dict(agent='ippo', map=map_name, envs=n, segment=seg, episodes=episodes, rounds=rounds, env_steps_per_s=rates, median=med,
                          ratio_loop_to_python=round(med['loop'] / med['python'], 3), spread_between_rounds=spread,
                          rollout_only_env_steps_per_s=round(n * steps / t_roll), ms_per_update=ms)), flush=True)


if __name__ == '__main__':
    a = sys.argv[1:]
    main(a[0] if len(a) > 0 else 'cologne1', *[int(x) for x in a[1:6]])
