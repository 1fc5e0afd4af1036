#!/usr/bin/env python3
"""IPPO training loop on the GPU: HIP simulator -> fp16 observations -> fused HIP policy kernel in sampling mode
(rs_idqn_act, mode 1) -> rollout segment in HBM -> batched PPO update (PyTorch) -> weights re-packed on the device.

    python tools/ippo_train.py [--device-rollout] [--device-update] [--device-shuffle] [--device-loop] [map] [n_envs] [episodes] [segment_steps] [minibatches_per_epoch]

--device-rollout: the segment is recorded on the device by the group path (rs_group_rollout: actor-critic kernel, step kernel and
recorder, `segment_steps` env-steps per call through the ABI), the update takes logp / value from the recording and GAE from the
fused kernel (BatchedPPOLearner.update_from_rollout) -- no Python work per env-step, no second forward over the segment.

--device-update (implies --device-rollout): the PPO update itself runs on the device too (FusedPPOLearner: loss, backward,
per-signal clipping and Adam in HIP kernels, rs_ppo_fit -- one call through the ABI per update instead of ~200 launches per Adam
step).

--device-loop: the loop itself runs in the library (agents/train_fused.py: DevicePPOTrainer, rs_group_ppo_train): rollout, bootstrap
value, GAE, shuffle, update and re-pack of a whole episode are ONE call through the ABI; the shuffles are the learner's counter-hash
permutations (FusedPPOLearner.device_perm) instead of torch.randperm's.  --device-shuffle (implies --device-update) is the same loop
driven from Python, shuffle included, and gives the same bits.  Opt-in.

Prints one JSON line per episode (average trip delay as utils/readXML.py computes it, env-steps/s including
learning).  The reference's IPPO learns far more slowly than its IDQN (1400 published episodes); this tool shows the
machinery end to end, not a converged policy.  Random-init weights, synthetic (rou.xml) demand.

Checkpoints (resco_amd/checkpoint.py), in every mode: --save PATH [--save-freq K] writes the training state -- the partly filled
segment included, it spans episodes -- after every K-th episode and after the last; --load PATH continues at the stored episode
(`episodes` stays the planned total, the demand seeds go on where they stopped); --load PATH --eval loads the weights alone and runs
one episode without learning on demand seed 12345, printing its line; --stop-after K leaves after K episodes of the planned total, as
a job that ran out of time would."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resco_amd.agents.idqn_fused import FusedIDQN                   # noqa: E402
from resco_amd.agents.ippo import BatchedIPPO, BatchedPPOLearner      # noqa: E402
from resco_amd.agents.ippo_fused import DeviceRollout, FusedIPPO      # noqa: E402
from resco_amd.agents.ippo_learn_fused import FusedPPOLearner         # noqa: E402
from resco_amd.agents.train_fused import DevicePPOTrainer             # noqa: E402
from resco_amd.multi_signal import VecMultiSignal                     # noqa: E402
from resco_amd.sim import SimGroup                                    # noqa: E402
from resco_amd import checkpoint                                      # noqa: E402


def report(env, learner, ep, n, steps, dt):
    print(json.dumps(dict(episode=ep, avg_delay_s=round(float(env.sim.trip_delay().mean()), 2),
                          arrived_per_env=round(float(env.sim.stats()['arrived'].mean()), 1), adam_steps=learner.n_updates,
                          env_steps_per_s=round(n * steps / dt), ms_per_step=round(dt / steps * 1e3, 3))), flush=True)


class Checkpoints:
    """the checkpoint flags of one run: load() before the first episode -> the episode to start at (`episodes` for --eval), after(ep)
    behind every episode -> leave now"""

    def __init__(self, map_name, episodes, seg, objects, weights, save=None, save_freq=0, save_replay=False, load=None, eval_only=False, stop_after=0):
        self.map_name, self.episodes, self.objects, self.weights = map_name, episodes, objects, weights
        self.hyper = dict(episodes=episodes, segment_steps=seg)
        self.save, self.save_freq, self.path, self.eval_only, self.stop_after = save, save_freq, load, eval_only, stop_after

    def load(self):
        if self.path and self.eval_only:
            checkpoint.load(self.path, agent='IPPO', map_name=self.map_name, objects=self.weights, strict=False)
            return self.episodes
        if self.path:
            return int(checkpoint.load(self.path, agent='IPPO', map_name=self.map_name, objects=self.objects, hyper=self.hyper)['episode'])
        return 0

    def after(self, ep):
        write, stop = checkpoint.due(ep + 1, self.episodes, self.save, self.save_freq, self.stop_after)
        if write:
            checkpoint.save(self.save, agent='IPPO', map_name=self.map_name, objects=self.objects, hyper=self.hyper, progress=dict(episode=ep + 1))
        return stop


def evaluation(env, act, map_name):
    """--eval: one episode on demand seed 12345, actions drawn by the loaded policy, no learning; prints and returns its line"""
    env.sim.set_seed(12345)
    obs = env.reset()['drq_norm_f16']
    for k in range(env.horizon_steps):
        act(obs, k)
        obs = env.step(None)[0]['drq_norm_f16']
    torch.cuda.synchronize()
    line = dict(map=map_name, agent='IPPO', eval_avg_delay_s=round(float(env.sim.trip_delay().mean()), 2),
                arrived_per_env=round(float(env.sim.stats()['arrived'].mean()), 1))
    print(json.dumps(line), flush=True)
    return line


def main_device_rollout(map_name='cologne1', n=256, episodes=20, seg=30, mbs=4, device_update=False, device_shuffle=False, **ckpt):
    env = VecMultiSignal(map_name, n, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
    steps = env.horizon_steps
    net = BatchedIPPO.from_scenario(env.scenario, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=0)
    learner = (FusedPPOLearner if device_update else BatchedPPOLearner)(net, minibatch=max(256, seg * n // mbs))
    policy = FusedIPPO(net, seed=3)
    policy.refresh_on_device()
    grp, rec = SimGroup([env.sim]), DeviceRollout(seg, [env.sim])
    obs = env.tensor('drq_norm_f16')
    gen = torch.Generator(device='cuda').manual_seed(0)
    c = checkpoint.Counters(done=[False] * seg, t_global=0, i=0, updates=0)     # the loop's own state: where the segment stands
    ck = Checkpoints(map_name, episodes, seg, dict(env=env, net=net, learner=learner, policy=policy, rollout=rec, loop=c, gen=gen),
                     dict(net=net, policy=policy), **ckpt)
    for ep in range(ck.load(), episodes):
        env.sim.set_seed(1000 + ep)
        env.reset()
        torch.cuda.synchronize()                # (the rollout runs on the handle's own stream, the reset ran on torch's)
        t0 = time.perf_counter()
        k = 0
        while k < steps:
            m = min(seg - c.i, steps - k)
            grp.rollout(rec, policy.handle, t0=c.i, n_steps=m, step_key=c.t_global, seed=policy.seed)
            k, c.i, c.t_global = k + m, c.i + m, c.t_global + m
            c.done[c.i - 1] = env.advance(m)
            if c.i == seg:
                grp.sync()
                kw = dict(perm=learner.device_perm(seg * n, c.updates)) if device_shuffle else dict(generator=gen)
                learner.update_from_rollout(rec, policy.value(obs), torch.as_tensor(c.done, device='cuda'), **kw)
                c.updates += 1
                policy.refresh_on_device()
                torch.cuda.current_stream().synchronize()       # the next rollout reads the re-packed weights on another stream
                c.done, c.i = [False] * seg, 0
        grp.sync()
        torch.cuda.synchronize()
        report(env, learner, ep, n, steps, time.perf_counter() - t0)
        if ck.after(ep):
            break
    if ck.eval_only:
        evaluation(env, lambda o, k: policy.act(o, step_key=k, out=env.tensor('actions')), map_name)
    env.close()


def main_device_loop(map_name='cologne1', n=256, episodes=20, seg=30, mbs=4, **ckpt):
    env = VecMultiSignal(map_name, n, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
    steps = env.horizon_steps
    net = BatchedIPPO.from_scenario(env.scenario, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=0)
    learner = FusedPPOLearner(net, minibatch=max(256, seg * n // mbs))
    policy = FusedIPPO(net, seed=3)
    policy.refresh_on_device()
    rollout = DeviceRollout(seg, [env.sim])
    trainer = DevicePPOTrainer(env, learner, policy, rollout)
    ck = Checkpoints(map_name, episodes, seg, dict(env=env, net=net, learner=learner, policy=policy, rollout=rollout, trainer=trainer),
                     dict(net=net, policy=policy), **ckpt)
    for ep in range(ck.load(), episodes):
        env.sim.set_seed(1000 + ep)
        env.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert trainer.run(steps)               # the whole episode; a segment may span the reset
        torch.cuda.synchronize()
        report(env, learner, ep, n, steps, time.perf_counter() - t0)
        if ck.after(ep):
            break
    if ck.eval_only:
        evaluation(env, lambda o, k: policy.act(o, step_key=k, out=env.tensor('actions')), map_name)
    env.close()
    return trainer


def main(map_name='cologne1', n=256, episodes=20, seg=30, mbs=4, **ckpt):
    env = VecMultiSignal(map_name, n, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
    S, steps = env.n_signals, env.horizon_steps
    net = BatchedIPPO.from_scenario(env.scenario, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=0)
    learner = BatchedPPOLearner(net, minibatch=max(256, seg * n // mbs))
    policy = FusedIDQN(net, seed=3)
    policy.refresh_on_device()
    actions = env.tensor('actions')
    obs_buf = torch.zeros(seg, n, S, net.lmax, 5, dtype=torch.float16, device='cuda')
    act_buf = torch.zeros(seg, n, S, dtype=torch.int32, device='cuda')
    rew_buf = torch.zeros(seg, n, S, dtype=torch.float32, device='cuda')
    done_buf = torch.zeros(seg, dtype=torch.bool, device='cuda')
    gen = torch.Generator(device='cuda').manual_seed(0)
    c = checkpoint.Counters(t_global=0, i=0, obs=obs_buf, act=act_buf, rew=rew_buf, done=done_buf)      # the loop's own state: the segment
    ck = Checkpoints(map_name, episodes, seg, dict(env=env, net=net, learner=learner, policy=policy, loop=c, gen=gen), dict(net=net, policy=policy), **ckpt)
    for ep in range(ck.load(), episodes):
        env.sim.set_seed(1000 + ep)
        obs = env.reset()['drq_norm_f16']
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            obs_buf[c.i].copy_(obs)
            policy.act(obs, step_key=c.t_global, out=actions, sample=True)
            o, r, done, _ = env.step(None)
            act_buf[c.i].copy_(actions)
            rew_buf[c.i].copy_(r['wait_norm'])
            done_buf[c.i] = bool(done)
            obs = o['drq_norm_f16']
            c.t_global += 1
            c.i += 1
            if c.i == seg:
                learner.update(obs_buf, act_buf, rew_buf, done_buf, obs, generator=gen)
                policy.refresh_on_device()
                c.i = 0
        torch.cuda.synchronize()
        report(env, learner, ep, n, steps, time.perf_counter() - t0)
        if ck.after(ep):
            break
    if ck.eval_only:
        evaluation(env, lambda o, k: policy.act(o, step_key=k, out=actions, sample=True), map_name)
    env.close()


if __name__ == '__main__':
    flags = ('--device-rollout', '--device-update', '--device-shuffle', '--device-loop')
    ckpt, rest = checkpoint.tool_flags(sys.argv[1:])
    a = [x for x in rest if x not in flags]
    run = main_device_loop if '--device-loop' in sys.argv[1:] else (main_device_rollout if any(f in sys.argv[1:] for f in flags) else main)
    kw = dict(device_update=True) if '--device-update' in sys.argv[1:] and run is main_device_rollout else {}
    if '--device-shuffle' in sys.argv[1:] and run is main_device_rollout:       # (--device-update with the library loop's shuffles)
        kw = dict(device_update=True, device_shuffle=True)
    run(a[0] if len(a) > 0 else 'cologne1', int(a[1]) if len(a) > 1 else 256, int(a[2]) if len(a) > 2 else 20,
        int(a[3]) if len(a) > 3 else 30, int(a[4]) if len(a) > 4 else 4, **kw, **ckpt)
