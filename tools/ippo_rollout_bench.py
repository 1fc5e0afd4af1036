#!/usr/bin/env python3
"""What the IPPO device rollout costs and saves (GPU box; the figures of profiles/r08_ippo_device_rollout.txt).

    python tools/ippo_rollout_bench.py ratio   [map] [envs_per_pipe] [pipes] [steps] [reps]
        env-steps/s of the group path: sim only (rs_group_step 'none'), sim + policy (rs_group_step 'idqn' mode 1) and
        sim + actor-critic + recorder (rs_group_rollout), alternating, median and range over `reps` windows of `steps` steps.
        RESCO_SIM_LIB=variants/<name>.so measures another build of the library (tools/ab.py build), e.g. the recorder variants.
    python tools/ippo_rollout_bench.py update  [map] [envs] [segment_steps] [reps]
        one BatchedPPOLearner.update against one update_from_rollout and one FusedPPOLearner.update_from_rollout (the update on the
        device, rs_ppo_fit) on the same recorded segment (median ms and range), and the
        largest |logp_kernel - logp_fp32net| and |value_kernel - value_fp32net| of that segment.
    python tools/ippo_rollout_bench.py kernels [map] [envs ...]
        launches rs_idqn_act mode 1 and rs_ippo_act 50 times each per batch size: run it under
        `rocprofv3 --kernel-trace --stats -d DIR -- python tools/ippo_rollout_bench.py kernels ...` and read the kernel stats.
"""
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resco_amd.agents.idqn_fused import FusedIDQN                    # noqa: E402
from resco_amd.agents.ippo import BatchedIPPO, BatchedPPOLearner      # noqa: E402
from resco_amd.agents.ippo_fused import DeviceRollout, FusedIPPO      # noqa: E402
from resco_amd.agents.ippo_learn_fused import FusedPPOLearner         # noqa: E402
from resco_amd.multi_signal import load_scenario                      # noqa: E402
from resco_amd.sim import BatchedSim, SimGroup                        # noqa: E402


def _scenario(map_name):
    from resco_amd.config.map_config import map_configs
    return load_scenario(map_name, None, map_configs.get(map_name, {}).get('lights', ()), 3)


def _policy(sc):
    net = BatchedIPPO.from_scenario(sc, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=0)
    pol = FusedIPPO(net, seed=3)
    pol.refresh_on_device()
    torch.cuda.synchronize()
    return net, pol


def _med(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3), n=len(xs))


def ratio(map_name='ingolstadt21', n=1024, pipes=2, steps=60, reps=5):
    sc = _scenario(map_name)
    sims = [BatchedSim(sc, n, seed=1, env_base=i * n, device_envs=n * pipes) for i in range(pipes)]
    grp = SimGroup(sims)
    net, pol = _policy(sc)
    rec = DeviceRollout(steps, sims)
    grp.step('random', step_key=0, n_steps=90)          # a loaded network
    grp.sync()
    modes = {'sim_only': lambda k: grp.step('none', n_steps=steps),
             'group_step_mode1': lambda k: grp.step('idqn', step_key=k, n_steps=steps, policy=pol.handle, mode=1, seed=3),
             'group_rollout': lambda k: grp.rollout(rec, pol.handle, t0=0, n_steps=steps, step_key=k, seed=3)}
    rate = {m: [] for m in modes}
    snaps = [s.snapshot() for s in sims]                # every window steps the same traffic
    for rep in range(reps + 1):                         # (the first round is the warm-up)
        for m, fn in modes.items():
            for s, sn in zip(sims, snaps):
                s.restore(sn)
            grp.sync()
            t0 = time.perf_counter()
            fn(1000 + rep * steps)
            grp.sync()
            if rep:
                rate[m].append(n * pipes * steps / (time.perf_counter() - t0))
    out = dict(map=map_name, envs_per_pipe=n, pipes=pipes, steps=steps, lib=os.environ.get('RESCO_SIM_LIB', 'default'),
               env_steps_per_s={m: _med(v) for m, v in rate.items()})
    med = {m: statistics.median(v) for m, v in rate.items()}
    out['rollout_over_group_step'] = round(med['group_rollout'] / med['group_step_mode1'], 4)
    out['rollout_over_sim_only'] = round(med['group_rollout'] / med['sim_only'], 4)
    out['group_step_over_sim_only'] = round(med['group_step_mode1'] / med['sim_only'], 4)
    print(json.dumps(out), flush=True)


def update(map_name='cologne1', n=256, seg=30, reps=5):
    sc = _scenario(map_name)
    sim = BatchedSim(sc, n, seed=1)
    grp = SimGroup([sim])
    net, pol = _policy(sc)
    rec = DeviceRollout(seg, [sim])
    grp.step('random', step_key=0, n_steps=90)
    grp.rollout(rec, pol.handle, t0=0, n_steps=seg, step_key=0, seed=3)
    grp.sync()
    p = rec.pipes[0]
    last_obs = sim.tensor('drq_norm_f16')
    done = torch.zeros(seg, dtype=torch.bool, device='cuda')
    with torch.no_grad():
        lg, v = net(p['obs'].reshape(seg * n, *p['obs'].shape[2:]))
        lp = torch.log_softmax(lg.float(), -1).gather(-1, p['act'].reshape(seg * n, -1, 1).long()).squeeze(-1).reshape(seg, n, -1)
        gap_lp = (lp - p['logp']).abs().max().item()
        gap_v = (v.float().reshape(seg, n, -1) - p['value']).abs().max().item()
        vmax = p['value'].abs().max().item()
    ms = {'update': [], 'update_from_rollout': [], 'fused update_from_rollout': []}
    for rep in range(reps + 1):
        for name in ms:
            cls = FusedPPOLearner if name.startswith('fused') else BatchedPPOLearner
            learner = cls(copy.deepcopy(net), minibatch=max(256, seg * n // 4))
            gen = torch.Generator(device='cuda').manual_seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == 'update':
                learner.update(p['obs'], p['act'], p['rew'], done, last_obs, generator=gen)
            else:
                learner.update_from_rollout(rec, pol.value(last_obs), done, generator=gen)
            torch.cuda.synchronize()
            if rep:
                ms[name].append((time.perf_counter() - t0) * 1e3)
            if name.startswith('fused'):
                learner.close()
    # the dataset alone (what the two paths differ in; the Adam loop is the same code)
    learner = BatchedPPOLearner(copy.deepcopy(net))
    ds = {'make_dataset': [], 'dataset_from_rollout': []}
    for rep in range(reps + 1):
        for name in ds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == 'make_dataset':
                learner.make_dataset(p['obs'], p['act'], p['rew'], done, last_obs)
            else:
                learner.dataset_from_rollout(rec, pol.value(last_obs), done)
            torch.cuda.synchronize()
            if rep:
                ds[name].append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(map=map_name, envs=n, seg=seg, ms={k: _med(v) for k, v in ms.items()}, dataset_ms={k: _med(v) for k, v in ds.items()},
                          max_abs_logp_kernel_minus_fp32net=gap_lp, max_abs_value_kernel_minus_fp32net=gap_v, max_abs_value=vmax)), flush=True)


def kernels(map_name='ingolstadt21', sizes=(1024, 4096)):
    sc = _scenario(map_name)
    net, pol = _policy(sc)
    for n in sizes:
        sim = BatchedSim(sc, n, seed=1)
        sim.act_random(0)
        for k in range(30):
            sim.act_random(k)
            sim.step(None)
        sim.sync()
        obs = sim.tensor('drq_norm_f16')
        for k in range(50):
            pol.act(obs, step_key=k)
            FusedIDQN.act(pol, obs, step_key=k, sample=True)        # the same handle through rs_idqn_act, mode 1
        torch.cuda.synchronize()
        sim.close()


if __name__ == '__main__':
    a = sys.argv[1:]
    if a[0] == 'ratio':
        ratio(*([a[1]] if len(a) > 1 else []), *[int(x) for x in a[2:]])
    elif a[0] == 'update':
        update(*([a[1]] if len(a) > 1 else []), *[int(x) for x in a[2:]])
    else:
        kernels(a[1] if len(a) > 1 else 'ingolstadt21', [int(x) for x in a[2:]] or (1024, 4096))
