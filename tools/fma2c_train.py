#!/usr/bin/env python3
"""FMA2C training loop on the GPU: HIP simulator -> fused FMA2C acting kernel on RS_BUF_LANE_AGG (rs_fma2c_act: input rows, both
LSTM actor-critic nets of every manager and worker, the draw; state and fingerprints stay on the device) -> rs_step -> rewards.fma2c
for all agents (VecMultiSignal.fma2c_rewards) -> the A2C learner in PyTorch (resco_amd/agents/fma2c.py: A2CLearner, an update every
120 steps or at the episode's end) -> weights re-packed on the device.  The reference's FMA2C (agents/fma2c.py, agents/ma2c.py,
config/agent_config.py:114-138) batched over N environments.

    python tools/fma2c_train.py [--full] [--device-update [--device-rewards] | --device-loop] [--steps-per-episode n] [map] [n_envs] [episodes] [seed]

--device-update: the fused A2C update (rs_fma2c_learn_*; resco_amd/agents/fma2c_learn_fused.py: FusedA2CLearner) instead of the PyTorch
learner: rows and values land in the learner's segment buffers, the policy acts with the learner's own weight vector (no re-pack).
--device-rewards (with --device-update): the rewards come from the reward kernel (rs_fma2c_record; VecMultiSignal.fma2c_rewards_device)
instead of the dense product of fma2c_rewards; the summation order differs, so the figures differ in the last bits.
--device-loop: the whole loop in the library, one call per episode (rs_group_fma2c_train; resco_amd/agents/train_fused.py:
DeviceA2CTrainer): the same bits as --device-update --device-rewards, and the same JSON lines.

Prints one JSON line per episode (mean episode return per agent, average trip delay as utils/readXML.py computes it, the last
update's mean loss, env-steps/s including learning) and a final line with the best training episode and the on-device random policy
on the same demand.  --full: FMA2CFULL (states.fma2c_full / rewards.fma2c_full).  --steps-per-episode cuts every episode short (smoke runs).

Checkpoints (resco_amd/checkpoint.py), in every mode: --save PATH [--save-freq K] writes the training state -- weights, RMSProp's ms,
and what the reference carries from one episode into the next: fingerprints, parity, the managers' last actions -- after every K-th
episode and after the last; --load PATH continues at the stored episode (`episodes` stays the planned total, the demand seeds go on
where they stopped); --load PATH --eval loads the weights alone and runs one episode without learning on demand seed 12345, adding
eval_avg_delay_s to the final line; --stop-after K leaves after K episodes of the planned total, as a job that ran out of time would."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resco_amd.agents.fma2c import A2CLearner, BatchedFMA2C, FMA2CLayout, FusedFMA2C      # noqa: E402
from resco_amd.config.agent_config import agent_configs                                 # noqa: E402
from resco_amd.config.mdp_config import activate                                        # noqa: E402
from resco_amd.multi_signal import VecMultiSignal                                       # noqa: E402
from resco_amd import checkpoint                                                        # noqa: E402


def delay(env):
    return float(env.sim.trip_delay().mean()), float(env.sim.stats()['arrived'].mean())


def main(map_name='cologne1', n=256, episodes=30, seed=0, full=False, steps_per_episode=0, quiet=False, keep=None, device_update=False,
         device_rewards=False, device_loop=False, save=None, save_freq=0, save_replay=False, load=None, eval_only=False, stop_after=0):
    """keep: a dict that receives net, policy, learner and env instead of having them closed (tests).
    save / save_freq / load / eval_only / stop_after: the checkpoint flags of the module docstring (save_replay is accepted and has
    nothing to leave out: FMA2C keeps no ring); a run that leaves at stop_after returns (rows, None)."""
    if device_loop:
        device_update = True
    elif device_rewards and not device_update:
        raise ValueError('--device-rewards goes with --device-update')
    cfg = agent_configs['FMA2CFULL' if full else 'FMA2C']
    activate('FMA2CFull' if full else 'FMA2C', map_name)
    env = VecMultiSignal(map_name, n, states=(), rewards=(), seed=0, max_distance=cfg['max_distance'], outputs=('lane_agg', 'lane_arrivals'))
    steps = min(env.horizon_steps, steps_per_episode) if steps_per_episode else env.horizon_steps
    layout = FMA2CLayout(env.scenario, full)
    net = BatchedFMA2C(layout).init_like_reference(seed).cuda()
    policy = FusedFMA2C(net, n, seed=7 + seed)
    hyper = dict(batch_size=cfg['batch_size'], gamma=cfg['gamma'], lr=cfg['lr_init'], alpha=cfg['rmsp_alpha'],
                 eps=cfg['rmsp_epsilon'], max_grad_norm=cfg['max_grad_norm'], value_coef=cfg['value_coef'],
                 entropy_coef=cfg['entropy_coef_init'], reward_norm=cfg['reward_norm'], reward_clip=cfg['reward_clip'])
    if device_update:
        from resco_amd.agents.fma2c_learn_fused import FusedA2CLearner
        learner = FusedA2CLearner(net, policy, n, **hyper)
    else:
        learner = A2CLearner(net, n, **hyper)
        policy.refresh_on_device()
    lane_agg, actions = env.tensor('lane_agg'), env.tensor('actions')
    state, macts = policy.buffer('state'), policy.buffer('mgr_actions')

    env.sim.set_seed(12345)
    env.reset()
    for k in range(steps):
        env.act_random(k)
        env.step(None)
    rnd_delay, _ = delay(env)

    trainer = None
    if device_loop:
        from resco_amd.agents.train_fused import DeviceA2CTrainer
        trainer = DeviceA2CTrainer(env, learner, policy, full)
        if steps != env.horizon_steps:
            env.horizon_steps = steps       # (--steps-per-episode: the trainer reads the episode's end off the environment)
    # what a checkpoint holds.  With the fused learner the weights ARE the learner's vector (the network mirrors it after pull());
    # the Python loops' act key t is the loop's own state
    agent = 'FMA2CFULL' if full else 'FMA2C'
    c = checkpoint.Counters(t=0)
    objects = dict(env=env, net=net, learner=learner, policy=policy, loop=c)
    if trainer is not None:
        objects['trainer'] = trainer
    hyper = dict(episodes=episodes, steps_per_episode=steps, seed=seed)
    first_ep, rows = 0, []
    if load and eval_only:
        weights = dict(net=net, learner=learner, policy=policy) if device_update else dict(net=net, policy=policy)
        rows = checkpoint.load(load, agent=agent, map_name=map_name, objects=weights, strict=False)['rows']
        first_ep = episodes
    elif load:
        progress = checkpoint.load(load, agent=agent, map_name=map_name, objects=objects, hyper=hyper)
        first_ep, rows = int(progress['episode']), list(progress['rows'])
    loss = None
    for ep in range(first_ep, episodes):
        env.sim.set_seed(1000 + ep + 7919 * seed)
        env.reset()
        policy.reset()                      # model.reset() at the episode's end (ma2c.py:144-146); the fingerprints stay, as there
        ret = torch.zeros(n, layout.K, device='cuda')
        loss = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if trainer is not None:
            trainer.ret.zero_()
            updates = learner.updates
            trainer.run(steps)              # (returns done: `steps` steps from a reset reach the horizon)
            ret = trainer.ret
            if learner.updates > updates:
                loss = learner.last_loss
        for k in range(steps if trainer is None else 0):
            out = policy.act(lane_agg, step_key=c.t, actions=actions, want=('value', 'rows'), out=learner.slot()) if device_update else \
                policy.act(lane_agg, step_key=c.t, actions=actions)
            acts = torch.cat([macts, out['actions']], dim=1).long()
            env.step(None)
            done = k == steps - 1
            if device_rewards:
                rew = env.fma2c_rewards_device(full, policy=policy)
            else:
                r = env.fma2c_rewards(full)
                rew = torch.stack([r[a] for a in layout.agents], dim=1)
            ret += rew
            res = learner.observe(out['rows'], acts, rew, out['value'], done, state, lambda: policy.value(lane_agg))
            if res is not None:
                loss = res
                if not device_update:
                    policy.refresh_on_device()
            c.t += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        d, arrived = delay(env)
        rows.append(dict(episode=ep, mean_return=float(ret.mean()), avg_delay_s=round(d, 2), arrived_per_env=round(arrived, 1),
                         updates=learner.updates, loss=float(loss.mean()) if loss is not None else None, env_steps_per_s=round(n * steps / dt)))
        if not quiet:
            print(json.dumps(rows[-1]), flush=True)
        write, stop = checkpoint.due(ep + 1, episodes, save, save_freq, stop_after)
        if write:
            if device_update:
                learner.pull()
            checkpoint.save(save, agent=agent, map_name=map_name, objects=objects, hyper=hyper, progress=dict(episode=ep + 1, seed=seed, rows=rows))
        if stop:
            policy.close()
            env.close()
            return rows, None
    final = dict(map=map_name, agent='FMA2CFULL' if full else 'FMA2C', envs=n, episodes=episodes, steps_per_episode=steps, seed=seed,
                 best_training_episode_delay_s=min(r['avg_delay_s'] for r in rows), random_avg_delay_s=round(rnd_delay, 2))
    if eval_only:           # one episode on the baseline's demand seed, actions drawn by the loaded policy, no learning
        env.sim.set_seed(12345)
        env.reset()
        policy.reset()
        for k in range(steps):
            policy.act(lane_agg, step_key=k, actions=actions, want=())
            env.step(None)
        final['eval_avg_delay_s'] = round(delay(env)[0], 2)
    if not quiet:
        print(json.dumps(final), flush=True)
    if device_update:
        learner.pull()
    if keep is not None:
        keep.update(net=net, policy=policy, learner=learner, env=env, layout=layout, loss=loss)
    else:
        policy.close()
        env.close()
    return rows, final


if __name__ == '__main__':
    ckpt, a = checkpoint.tool_flags(sys.argv[1:])
    full, dev_up, dev_rew, dev_loop = '--full' in a, '--device-update' in a, '--device-rewards' in a, '--device-loop' in a
    a = [x for x in a if x not in ('--full', '--device-update', '--device-rewards', '--device-loop')]
    spe = 0
    if '--steps-per-episode' in a:
        i = a.index('--steps-per-episode')
        spe = int(a[i + 1])
        del a[i:i + 2]
    main(a[0] if len(a) > 0 else 'cologne1', int(a[1]) if len(a) > 1 else 256, int(a[2]) if len(a) > 2 else 30,
         int(a[3]) if len(a) > 3 else 0, full=full, steps_per_episode=spe, device_update=dev_up, device_rewards=dev_rew, device_loop=dev_loop, **ckpt)
