#!/usr/bin/env python3
"""MPLight training loop entirely on the GPU: HIP simulator -> states.mplight rows -> fused FRAP kernel (rs_mplight_act, global pair
indices out) -> device replay ring -> shared-DQN update (PyTorch, or with --device-update the fused HIP update of
resco_amd/agents/mplight_learn_fused.py on the policy's own weight vector) -> weights re-packed on the device.  The analogue of
tools/idqn_train.py for the reference's MPLight (agents/mplight.py, config/agent_config.py:101-113; batching:
resco_amd/agents/mplight.py).

    python tools/mplight_train.py [--n-step K] [--double-q] [--per [alpha,beta0,beta_steps]] [--device-update | --device-loop] [map] [n_envs] [episodes] [batch] [replay_steps] [seed] [full]

Prints one JSON line per episode (mean episode return of rewards.pressure per signal, average trip delay as utils/readXML.py
computes it, epsilon, env-steps/s including learning) and a final line with the best training episode and the on-device random
policy on the same demand.  --device-loop (implies --device-update): the loop itself in the library as well
(agents/train_fused.py: DeviceTrainer, rs_group_train), one call per episode; the same rows.  `full`: MPLightFULL (states.mplight_full, demand_shape 4).

--n-step K (1 .. 32) and --double-q, in every mode (the flags of tools/idqn_train.py): n-step returns (truncated at the newest slot of
the ring, cut at an episode end) and Double DQN's bootstrap (the online network's best of ALL pairs, valued by the target network);
both are part of a checkpoint's signature.  Without them: PFRL's plain one-step DQN.

--per [alpha,beta0,beta_steps] (with --device-update or --device-loop only): prioritised experience replay in the fused update -- the
minibatch is drawn by priority over the pooled rows (slot, environment, signal), the loss carries the importance weights and every
update writes the rows' new priorities back (FusedMPLightLearner(per=...), rs_mplight_dqn_set_priorities).  Defaults 0.6, 0.4 and a
beta that reaches 1 with the last planned update.  Part of a checkpoint's signature; --save-replay saves the priorities with the ring.

Checkpoints (resco_amd/checkpoint.py), in every mode: --save PATH [--save-freq K] [--save-replay] (the replay ring only with --save-replay: it is the large part; without it a resumed run is a valid continuation, not the same one) writes the training state after every K-th
episode and after the last; --load PATH continues at the stored episode (`episodes` stays the planned total, so the schedules and the
demand seeds go on where they stopped); --load PATH --eval loads the weights alone and runs one evaluation episode without learning on
the baseline's demand seed; --stop-after K leaves after K episodes of the planned total, as a job that ran out of time would.

Demand variants (resco_amd/demand.py), in every mode: --demand-variants K[,jitter_s[,keep_lo,keep_hi]] gives the environments of the batch
K variants of the map's demand (environment e runs variant e % K), drawn anew for every episode from (seed, episode); the spec is part of a
checkpoint's signature, and a resumed run draws the same sets.  --eval-demand K[,jitter_s[,keep_lo,keep_hi]]: after training, one greedy
episode on the map's own demand and one on K held-out variants (K alone: the training spec's jitter and keep; seeds no training episode
uses); the final line reports both, per variant."""
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
from resco_amd import checkpoint, demand                                                    # noqa: E402
from tools.idqn_train import target_flags                                                   # noqa: E402


def delay(env):
    return float(env.sim.trip_delay().mean()), float(env.sim.stats()['arrived'].mean())


def greedy_evaluation(env, policy, state, actions, steps, seed):
    """one greedy episode with the policy's present weights (no learning) -> average trip delay"""
    env.sim.set_seed(seed)
    obs = env.reset()[state]
    for k in range(steps):
        policy.act(obs, out=actions)
        obs = env.step(None)[0][state]
    return round(delay(env)[0], 2)


def greedy_on_variants(env, policy, state, actions, steps, seed, variants):
    """the greedy episode on held-out demand variants -> the mean delay of the environments of every variant"""
    env.set_demand(variants)
    greedy_evaluation(env, policy, state, actions, steps, seed)
    per = demand.per_variant_mean(env.sim.trip_delay(), demand.env_variants(env.n_envs, env.sim.env_base, len(variants)), len(variants))
    env.set_demand(None)
    return [round(float(x), 2) for x in per]


def main(map_name='cologne1', n=256, episodes=30, batch=256, replay_steps=2048, seed=0, full=False, quiet=False, device_update=False, device_loop=False, chunk=0,
         save=None, save_freq=0, save_replay=False, load=None, eval_only=False, stop_after=0, demand_variants=None, eval_demand=0, n_step=1, double_q=False, per=None):
    """n_step / double_q: the learners' options of the same names.  per: None, True (the defaults) or (alpha, beta0[, beta_steps]):
    prioritised replay, with the fused learner only.  device_loop: the episodes' steps through DeviceTrainer.run, `chunk` steps per call (0: the whole episode in one).
    save / save_freq / save_replay / load / eval_only / stop_after: the checkpoint flags of the module docstring; a run that leaves
    at stop_after returns (rows, None).  demand_variants / eval_demand: the demand flags of the module docstring."""
    device_update = device_update or device_loop
    if per is not None and per is not False and not device_update:
        raise SystemExit('--per needs --device-update or --device-loop: prioritised replay is built into the fused update only')
    n_var, var_kw = demand.parse_spec(demand_variants)
    n_eval, eval_kw = demand.parse_spec(eval_demand)
    eval_kw = eval_kw or var_kw
    state = 'mplight_full' if full else 'mplight'
    env = VecMultiSignal(map_name, n, states=(state,), rewards=('pressure',), seed=0, outputs=(state,))
    S, steps = env.n_signals, env.horizon_steps
    net = frap_from_scenario(env.scenario, 4 if full else 1).cuda()
    net.init_like_reference(seed)
    if device_update:
        if per is True:
            per = (0.6, 0.4)
        if per:             # beta reaches 1 with the last planned update unless told otherwise (one update per env-step)
            per = dict(alpha=per[0], beta0=per[1], beta_steps=int(per[2]) if len(per) > 2 else episodes * steps)
        learner = FusedMPLightLearner(net, gamma=0.99, lr=1e-3, target_update=500, batch_size=batch, seed=seed, n_signals=S, n_step=n_step, double_q=double_q,
                                      per=per or None)
    else:
        learner = MPLightLearner(net, gamma=0.99, lr=1e-3, target_update=500, batch_size=batch, n_step=n_step, double_q=double_q)
    policy = FusedMPLight(net, env.scenario, seed=7 + seed)
    if device_update:
        policy.share_weights(learner.flat)      # the policy reads the vector the update writes: no re-pack per step
    replay = MPLightReplay(replay_steps, n, S, 1 + 12 * net.demand_shape, device='cuda')
    actions = env.tensor('actions')
    pair = torch.zeros(n, S, dtype=torch.int32, device='cuda')
    gen = torch.Generator(device='cuda').manual_seed(seed)
    decay = int(0.8 * episodes * steps)     # the reference decays over config['steps'] env-steps
    trainer = DeviceTrainer(env, learner, policy, replay, 1.0, 0.0, decay) if device_loop else None
    if device_update:
        learner.attach(replay)      # (prioritised replay: the priorities are sized from this ring, before a checkpoint is loaded)
    # what a checkpoint holds (the network before the learner and the policy that read it) and what else shapes the trajectory
    agent = 'MPLightFULL' if full else 'MPLight'
    objects = dict(env=env, net=net, learner=learner, policy=policy, replay=replay)
    if not device_update:
        objects['gen'] = gen
    hyper = dict(episodes=episodes, decay_steps=decay, seed=seed)
    if n_var:
        hyper['demand_variants'] = str(demand_variants)     # (a resume under another spec is another run: refused)
    first_ep, rows = 0, []
    if load and eval_only:
        rows = checkpoint.load(load, agent=agent, map_name=map_name, objects=dict(net=net, policy=policy), strict=False)['rows']
        first_ep = episodes
    elif load:
        progress = checkpoint.load(load, agent=agent, map_name=map_name, objects=objects, hyper=hyper)
        first_ep, rows = int(progress['episode']), list(progress['rows'])

    env.sim.set_seed(12345)
    env.reset()
    for k in range(steps):
        env.act_random(k)
        env.step(None)
    rnd_delay, _ = delay(env)

    for ep in range(first_ep, episodes):
        env.sim.set_seed(1000 + ep + 7919 * seed)
        if n_var:
            env.set_demand(demand.episode_set(env.scenario, n_var, seed, ep, **var_kw))
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
        write, stop = checkpoint.due(ep + 1, episodes, save, save_freq, stop_after)
        if write:
            checkpoint.save(save, agent=agent, map_name=map_name, objects=objects, hyper=hyper, replay=save_replay,
                            progress=dict(episode=ep + 1, seed=seed, rows=rows))
        if stop:
            if device_update:
                learner.close()
            env.close()
            return rows, None
    final = dict(map=map_name, agent='MPLightFULL' if full else 'MPLight', envs=n, episodes=episodes, batch=batch, replay_steps=replay.T,
                 seed=seed, best_training_episode_delay_s=min(r['avg_delay_s'] for r in rows), random_avg_delay_s=round(rnd_delay, 2))
    env.set_demand(None)        # the evaluations below start from the map's own demand
    if n_var:
        final['demand_variants'] = str(demand_variants)
    if eval_only or n_eval > 0:
        final['greedy_avg_delay_s'] = greedy_evaluation(env, policy, state, actions, steps, 12345)
    if n_eval > 0:              # reported, not judged: held-out variants (the spec of --eval-demand, or the training spec's jitter and keep)
        held_out = demand.eval_set(env.scenario, n_eval, seed, **eval_kw)
        final['greedy_variant_delay_s'] = greedy_on_variants(env, policy, state, actions, steps, 12345, held_out)
        final['greedy_variants_mean_delay_s'] = round(sum(final['greedy_variant_delay_s']) / len(final['greedy_variant_delay_s']), 2)
    if not quiet:
        print(json.dumps(final), flush=True)
    if device_update:
        learner.close()
    env.close()
    return rows, final


if __name__ == '__main__':
    ckpt, a = checkpoint.tool_flags(sys.argv[1:])
    dem, a = demand.tool_flags(a)
    opts, a = target_flags(a)
    ckpt.update(opts)
    device_loop = bool(a) and a[0] == '--device-loop'
    device_update = device_loop or (bool(a) and a[0] == '--device-update')
    a = a[1:] if device_update else a
    if 'per' in ckpt and not device_update:
        raise SystemExit('--per needs --device-update or --device-loop: prioritised replay is built into the fused update only')
    main(a[0] if len(a) > 0 else 'cologne1', int(a[1]) if len(a) > 1 else 256, int(a[2]) if len(a) > 2 else 30,
         int(a[3]) if len(a) > 3 else 256, int(a[4]) if len(a) > 4 else 2048, int(a[5]) if len(a) > 5 else 0,
         full=len(a) > 6 and a[6] == 'full', device_update=device_update, device_loop=device_loop, **ckpt, **dem)
