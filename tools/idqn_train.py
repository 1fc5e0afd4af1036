#!/usr/bin/env python3
"""IDQN training loop entirely on the GPU: HIP simulator -> fp16 observations -> fused HIP policy kernel
(rs_idqn_act) -> device replay ring -> batched DQN update (PyTorch, or HIP with --device-update) -> weights re-packed on the device.  Nothing crosses PCIe per step except the launch calls.

    python tools/idqn_train.py [--n-step K] [--double-q] [--per [alpha,beta0,beta_steps]] [--device-update | --device-loop] [map] [n_envs] [episodes] [batch] [updates_per_step] [graph|nograph] [replay_steps] [eps_end] [seed]

--device-update: the update itself in HIP kernels as well (FusedDQNLearner, rs_dqn_update: sampling, target, backward and Adam of all
updates of a step in one call; no HIP graph is captured).  --device-loop (implies --device-update): the loop itself in the library
as well (agents/train_fused.py: DeviceTrainer, rs_group_train), one call per episode; the same rows.  Without either: the batched PyTorch learner, graph-captured unless `nograph`.

--n-step K (1 .. 32) and --double-q, in every mode: n-step returns (truncated at the newest slot of the ring, cut at an episode end) and
Double DQN's bootstrap; both are part of a checkpoint's signature.  Without them: PFRL's plain one-step DQN.

--per [alpha,beta0,beta_steps] (with --device-update or --device-loop only): prioritised experience replay in the fused update -- the
minibatches are drawn by priority (|TD error| + 1e-6)^alpha, the loss carries importance weights whose exponent goes from beta0 to 1
over beta_steps updates (0: constant).  Without a value: 0.6,0.4 and the run's planned number of updates.  Part of a checkpoint's
signature; the priorities are saved with the ring (--save-replay) and start again without it.  The default beta_steps follows the
planned episodes, which are part of the signature themselves (a --load with another total is refused either way): give beta_steps
explicitly to pin the schedule to something else than the run's length.

Prints one JSON line per episode (mean episode return of rewards.wait_norm per signal, average trip delay as
utils/readXML.py computes it, epsilon, env-steps/s including learning) and a final line comparing with the
on-device random policy on the same demand.  Random-init weights, synthetic (rou.xml) demand.

Checkpoints (resco_amd/checkpoint.py), in every mode: --save PATH [--save-freq K] [--save-replay] writes the training state after every
K-th episode and after the last (the replay ring only with --save-replay: it is the large part); --load PATH continues at the stored
episode (`episodes` stays the planned total, so the epsilon schedule and the demand seeds go on where they stopped; bit-exact with the
ring, a valid continuation without); --load PATH --eval loads the weights alone and runs the greedy evaluation; --stop-after K leaves
after K episodes of the planned total, as a job that ran out of time would."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resco_amd.agents.idqn_learn import BatchedDQNLearner, DeviceReplay, linear_epsilon      # noqa: E402
from resco_amd.agents.idqn_learn_fused import FusedDQNLearner                               # noqa: E402
from resco_amd.agents.idqn_fused import FusedIDQN                                           # noqa: E402
from resco_amd.agents.idqn_rollout import BatchedIDQN                                       # noqa: E402
from resco_amd.agents.train_fused import DeviceTrainer                                      # noqa: E402
from resco_amd.multi_signal import VecMultiSignal                                           # noqa: E402
from resco_amd import checkpoint                                                            # noqa: E402


def delay(env):
    """Mean over the environments of utils/readXML.py's episode figure (timeLoss + departDelay per trip)."""
    return float(env.sim.trip_delay().mean()), float(env.sim.stats()['arrived'].mean())


def greedy_evaluation(env, policy, actions, steps, seeds):
    """greedy episodes with the policy's present weights (no learning) -> {demand seed: average trip delay}"""
    out = {}
    for seed in seeds:
        env.sim.set_seed(seed)
        obs = env.reset()['drq_norm_f16']
        for k in range(steps):
            policy.act(obs, out=actions)
            o, _, _, _ = env.step(None)
            obs = o['drq_norm_f16']
        out[seed] = round(delay(env)[0], 2)
    return out


def main(map_name='cologne1', n=256, episodes=12, batch=256, updates=1, use_graph=True, replay_steps=0, eps_end=0.0, evaluate=True, quiet=False, seed=0, tls_expiry=True,
         device_update=False, device_loop=False, chunk=0, save=None, save_freq=0, save_replay=False, load=None, eval_only=False, stop_after=0, n_step=1, double_q=False, per=None):
    """n_step / double_q: the learners' options of the same names.  per: None, True (the defaults) or (alpha, beta0[, beta_steps]):
    prioritised replay, with the fused learner only.  device_loop: the episodes' steps through DeviceTrainer.run, `chunk` steps per call (0: the whole episode in one).
    save / save_freq / save_replay / load / eval_only / stop_after: the checkpoint flags of the module docstring; a run that leaves
    at stop_after returns (rows, None)."""
    device_update = device_update or device_loop
    if per is not None and per is not False and not device_update:
        raise SystemExit('--per needs --device-update or --device-loop: prioritised replay is built into the fused update only')
    rows = []
    env = VecMultiSignal(map_name, n, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0, tls_expiry=tls_expiry)
    S, steps = env.n_signals, env.horizon_steps
    net = BatchedIDQN.from_scenario(env.scenario, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=seed)
    if device_update:
        if per is True:
            per = (0.6, 0.4)
        if per:             # beta reaches 1 with the last planned update unless told otherwise
            per = dict(alpha=per[0], beta0=per[1], beta_steps=int(per[2]) if len(per) > 2 else episodes * steps * updates)
        learner = FusedDQNLearner(net, gamma=0.99, lr=1e-3, target_update=500, batch_size=batch, seed=seed, n_step=n_step, double_q=double_q, per=per or None)
        use_graph = False                               # one call enqueues the update's few launches: nothing to capture
    else:
        learner = BatchedDQNLearner(net, gamma=0.99, lr=1e-3, target_update=500, batch_size=batch, n_step=n_step, double_q=double_q)
    policy = FusedIDQN(net, seed=7 + seed)             # acting: one HIP kernel; weights re-packed on the device after each update
    actions = env.tensor('actions')
    # the reference keeps the last 10 000 transitions of its ONE environment = 27.8 episodes of history (pfrl_dqn.py:55); a ring of
    # `replay_steps` env-steps over all N environments (0: the last four episodes -- a small ring forgets exploratory data within
    # four episodes of epsilon reaching 0)
    replay = DeviceReplay(replay_steps if replay_steps > 0 else min(2048, 4 * steps), n, S, net.lmax, device='cuda')
    if device_update:
        learner.attach(replay)                          # (the priorities, if any, are sized from the ring: before a checkpoint is loaded)
    gen = torch.Generator(device='cuda').manual_seed(seed)
    decay = int(0.8 * episodes * steps)                 # the reference decays over config['steps'] agent steps
    trainer = DeviceTrainer(env, learner, policy, replay, 1.0, eps_end, decay, updates) if device_loop else None
    # what a checkpoint holds (the network before the learner and the policy that read it) and what else shapes the trajectory
    objects = dict(env=env, net=net, learner=learner, policy=policy, replay=replay)
    if not device_update:
        objects.update(gen=gen, default_gen=torch.cuda.default_generators[env.sim.device])     # (the graph-captured update draws from the default one)
    hyper = dict(episodes=episodes, decay_steps=decay, updates_per_step=updates, eps_end=float(eps_end), seed=seed)
    first_ep = 0
    if load and eval_only:
        rows = checkpoint.load(load, agent='IDQN', map_name=map_name, objects=dict(net=net, policy=policy), strict=False)['rows']
        first_ep = episodes
    elif load:
        progress = checkpoint.load(load, agent='IDQN', map_name=map_name, objects=objects, hyper=hyper)
        first_ep, rows = int(progress['episode']), list(progress['rows'])

    env.sim.set_seed(12345)                             # baseline: random policy on an evaluation demand seed
    env.reset()
    for k in range(steps):
        env.act_random(k)
        env.step(None)
    rnd_delay, _ = delay(env)

    for ep in range(first_ep, episodes):
        env.sim.set_seed(1000 + ep + 7919 * seed)
        obs = env.reset()['drq_norm_f16']
        ret = torch.zeros(n, S, device='cuda')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while trainer is not None and env.steps < steps:
            trainer.run(min(chunk, steps - env.steps) if chunk > 0 else steps - env.steps, ret)
            eps = trainer.epsilon(learner.t - 1)
        for k in range(steps if trainer is None else 0):
            eps = linear_epsilon(learner.t, 1.0, eps_end, decay)
            policy.act(obs, epsilon=eps, step_key=learner.t, out=actions)
            replay.stage(obs)
            o, r, done, _ = env.step(None)
            rew = r['wait_norm']
            replay.commit(actions, rew, done)
            ret += rew
            if use_graph and (learner.n_updates == 0 or first_ep > 0) and getattr(learner, '_graph', None) is None and len(replay) >= batch:
                learner.capture_update(replay)      # [sample -> loss -> backward -> Adam] as one HIP graph
            if learner.observe_step(replay, gen, updates) is not None:
                policy.refresh_on_device()
            obs = o['drq_norm_f16']
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        d, arrived = delay(env)
        rows.append(dict(episode=ep, epsilon=round(eps, 3), mean_return=float(ret.sum(1).mean()) / S,
                         avg_delay_s=round(d, 2), arrived_per_env=round(arrived, 1), updates=learner.n_updates,
                         env_steps_per_s=round(n * steps / dt), ms_per_step=round(dt / steps * 1e3, 3)))
        if not quiet:
            print(json.dumps(rows[-1]), flush=True)
        write, stop = checkpoint.due(ep + 1, episodes, save, save_freq, stop_after)
        if write:
            checkpoint.save(save, agent='IDQN', map_name=map_name, objects=objects, hyper=hyper, replay=save_replay,
                            progress=dict(episode=ep + 1, seed=seed, rows=rows))
        if stop:
            if device_update:
                learner.close()
            env.close()
            return rows, None

    # greedy evaluation with the final weights (no further learning): on the baseline's seed and on the seed the last
    # training episode used - DQN keeps adapting within an episode, so a frozen copy can do worse than the last
    # training episodes did
    evals = {12345: None, 1000 + episodes - 1: None}
    evals.update(greedy_evaluation(env, policy, actions, steps, (12345, 1000 + episodes - 1) if evaluate or eval_only else ()))
    final = dict(map=map_name, envs=n, episodes=episodes, batch=batch, updates_per_step=updates, replay_steps=replay.T,
                 best_training_episode_delay_s=min(r['avg_delay_s'] for r in rows),
                 greedy_avg_delay_s=evals[12345], greedy_on_last_training_seed_s=evals[1000 + episodes - 1],
                 random_avg_delay_s=round(rnd_delay, 2))
    if not quiet:
        print(json.dumps(final))
    if device_update:
        learner.close()
    env.close()
    return rows, final


def _per_value(text):
    """'alpha,beta0[,beta_steps]' -> the tuple, or None where the text is not one (it is then the next positional argument)"""
    parts = text.split(',')
    try:
        v = (float(parts[0]), float(parts[1])) + ((int(parts[2]),) if len(parts) > 2 else ())
    except (ValueError, IndexError):
        return None
    return v if len(parts) in (2, 3) else None


def target_flags(argv):
    """--n-step K, --double-q and --per [alpha,beta0[,beta_steps]] taken out of an argument list -> (keyword arguments for main(), the
    remaining arguments)"""
    kw, rest, i = {}, [], 0
    while i < len(argv):
        if argv[i] == '--per':
            v = _per_value(argv[i + 1]) if i + 1 < len(argv) else None
            kw['per'] = True if v is None else v
            if v is not None and not (0.0 <= v[0] <= 1.0 and 0.0 <= v[1] <= 1.0 and (len(v) < 3 or v[2] >= 0)):
                raise SystemExit('--per: alpha and beta0 in [0, 1], beta_steps >= 0')
            i += 1 if v is None else 2
            continue
        if argv[i] == '--n-step':
            if i + 1 >= len(argv):
                raise SystemExit('--n-step needs a value')
            kw['n_step'] = int(argv[i + 1])
            if not 1 <= kw['n_step'] <= 32:
                raise SystemExit('--n-step: 1 .. 32')
            i += 2
            continue
        if argv[i] == '--double-q':
            kw['double_q'] = True
        else:
            rest.append(argv[i])
        i += 1
    return kw, rest


if __name__ == '__main__':
    ckpt, a = checkpoint.tool_flags(sys.argv[1:])
    opts, a = target_flags(a)
    ckpt.update(opts)
    loop = a[:1] == ['--device-loop']
    dev = loop or a[:1] == ['--device-update']
    a = a[1:] if dev else a
    if 'per' in ckpt and not dev:
        raise SystemExit('--per needs --device-update or --device-loop: prioritised replay is built into the fused update only')
    main(a[0] if len(a) > 0 else 'cologne1', int(a[1]) if len(a) > 1 else 256, int(a[2]) if len(a) > 2 else 12,
         int(a[3]) if len(a) > 3 else 256, int(a[4]) if len(a) > 4 else 1, (a[5] != 'nograph') if len(a) > 5 else True,
         int(a[6]) if len(a) > 6 else 0, float(a[7]) if len(a) > 7 else 0.0, seed=int(a[8]) if len(a) > 8 else 0, device_update=dev, device_loop=loop, **ckpt)
