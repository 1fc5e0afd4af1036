#!/usr/bin/env python3
"""MPLight training loop entirely on the GPU: HIP simulator -> states.mplight rows -> fused FRAP kernel (rs_mplight_act, global pair
indices out) -> device replay ring -> shared-DQN update (PyTorch, or with --device-update the fused HIP update of
resco_amd/agents/mplight_learn_fused.py on the policy's own weight vector) -> weights re-packed on the device.  The analogue of
tools/idqn_train.py for the reference's MPLight (agents/mplight.py, config/agent_config.py:101-113; batching:
resco_amd/agents/mplight.py).

    python tools/mplight_train.py [--device-update | --device-loop] [map] [n_envs] [episodes] [batch] [replay_steps] [seed] [full]

Prints one JSON line per episode (mean episode return of rewards.pressure per signal, average trip delay as utils/readXML.py
computes it, epsilon, env-steps/s including learning) and a final line with the best training episode and the on-device random
policy on the same demand.  --device-loop (implies --device-update): the loop itself in the library as well
(agents/train_fused.py: DeviceTrainer, rs_group_train), one call per episode; the same rows.  `full`: MPLightFULL (states.mplight_full, demand_shape 4)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resco_amd.agents.idqn_learn import linear_epsilon                                      # noqa: E402
from resco_amd.agents.mplight import FusedMPLight, MPLightLearner, MPLightReplay, frap_from_scenario      # noqa: E402
from resco_amd.agents.mplight_learn_fused import FusedMPLightLearner                        # noqa: E402
from resco_amd.agents.train_fused import DeviceTrainer                                      # noqa: E402
from resco_amd.multi_signal import VecMultiSignal                                           # noqa: E402


def delay(env):
    return float(env.sim.trip_delay().mean()), float(env.sim.stats()['arrived'].mean())


def main(map_name='cologne1', n=256, episodes=30, batch=256, replay_steps=2048, seed=0, full=False, quiet=False, device_update=False, device_loop=False, chunk=0):
    """device_loop: the episodes' steps through DeviceTrainer.run, `chunk` steps per call (0: the whole episode in one)"""
    device_update = device_update or device_loop
    state = 'mplight_full' if full else 'mplight'
    env = VecMultiSignal(map_name, n, states=(state,), rewards=('pressure',), seed=0, outputs=(state,))
    S, steps = env.n_signals, env.horizon_steps
    net = frap_from_scenario(env.scenario, 4 if full else 1).cuda()
    net.init_like_reference(seed)
    if device_update:
        learner = FusedMPLightLearner(net, gamma=0.99, lr=1e-3, target_update=500, batch_size=batch, seed=seed, n_signals=S)
    else:
        learner = MPLightLearner(net, gamma=0.99, lr=1e-3, target_update=500, batch_size=batch)
    policy = FusedMPLight(net, env.scenario, seed=7 + seed)
    if device_update:
        policy.share_weights(learner.flat)      # the policy reads the vector the update writes: no re-pack per step
    replay = MPLightReplay(replay_steps, n, S, 1 + 12 * net.demand_shape, device='cuda')
    actions = env.tensor('actions')
    pair = torch.zeros(n, S, dtype=torch.int32, device='cuda')
    gen = torch.Generator(device='cuda').manual_seed(seed)
    decay = int(0.8 * episodes * steps)     # the reference decays over config['steps'] env-steps
    trainer = DeviceTrainer(env, learner, policy, replay, 1.0, 0.0, decay) if device_loop else None

    env.sim.set_seed(12345)
    env.reset()
    for k in range(steps):
        env.act_random(k)
        env.step(None)
    rnd_delay, _ = delay(env)

    rows = []
    for ep in range(episodes):
        env.sim.set_seed(1000 + ep + 7919 * seed)
        obs = env.reset()[state]
        ret = torch.zeros(n, S, device='cuda')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while trainer is not None and env.steps < steps:
            trainer.run(min(chunk, steps - env.steps) if chunk > 0 else steps - env.steps, ret)
            eps = trainer.epsilon(learner.t - 1)
        for k in range(steps if trainer is None else 0):
            eps = linear_epsilon(learner.t, 1.0, 0.0, decay)
            policy.act(obs, epsilon=eps, step_key=learner.t, out=actions, pair_out=pair)
            replay.stage(obs)
            o, r, done, _ = env.step(None)
            rew = r['pressure'].float()
            replay.commit(pair, rew, done)
            ret += rew
            if learner.observe_step(replay, gen) is not None and not device_update:
                policy.refresh_on_device()
            obs = o[state]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        d, arrived = delay(env)
        rows.append(dict(episode=ep, epsilon=round(eps, 3), mean_return=float(ret.sum(1).mean()) / S, avg_delay_s=round(d, 2),
                         arrived_per_env=round(arrived, 1), updates=learner.n_updates, env_steps_per_s=round(n * steps / dt)))
        if not quiet:
            print(json.dumps(rows[-1]), flush=True)
    final = dict(map=map_name, agent='MPLightFULL' if full else 'MPLight', envs=n, episodes=episodes, batch=batch, replay_steps=replay.T,
                 seed=seed, best_training_episode_delay_s=min(r['avg_delay_s'] for r in rows), random_avg_delay_s=round(rnd_delay, 2))
    if not quiet:
        print(json.dumps(final), flush=True)
    if device_update:
        learner.close()
    env.close()
    return rows, final


if __name__ == '__main__':
    a = sys.argv[1:]
    device_loop = bool(a) and a[0] == '--device-loop'
    device_update = device_loop or (bool(a) and a[0] == '--device-update')
    a = a[1:] if device_update else a
    main(a[0] if len(a) > 0 else 'cologne1', int(a[1]) if len(a) > 1 else 256, int(a[2]) if len(a) > 2 else 30,
         int(a[3]) if len(a) > 3 else 256, int(a[4]) if len(a) > 4 else 2048, int(a[5]) if len(a) > 5 else 0,
         full=len(a) > 6 and a[6] == 'full', device_update=device_update, device_loop=device_loop)
