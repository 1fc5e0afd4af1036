#!/usr/bin/env python3
"""MPLight rollout timings: the fused FRAP kernel (rs_mplight_act) against the simulator it runs beside.

    python tools/mplight_rollout.py kernel <map> <n_envs> [launches]     # FRAP launches on the simulator's own mplight buffer
                                                                          #   (greedy: the pruned Q of every row); run it under
                                                                          #   rocprofv3 --kernel-trace --stats for us per launch
    python tools/mplight_rollout.py ratio <map> <n_envs> <pipes> [steps]  # env-steps/s through rs_group_step: sim-only (the on-device
                                                                          #   random agent) and sim + MPLight (greedy), alternated 3x
    python tools/mplight_rollout.py torch <map> <n_envs> [reps]           # the batched PyTorch FRAP forward on the same tensor

Prints one JSON line per measurement.  Random-init network (init_like_reference(0)); the buffers come from 170 random steps of the
map's demand (a loaded network)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resco_amd.agents.mplight import FusedMPLight, frap_from_scenario      # noqa: E402
from resco_amd.multi_signal import load_scenario                          # noqa: E402
from resco_amd.config.map_config import map_configs                       # noqa: E402
from resco_amd.sim import BatchedSim, SimGroup                            # noqa: E402

START = 170


def scenario(name):
    return load_scenario(name, None, map_configs.get(name, {}).get('lights', ()), 3)


def sync_all(sims):
    for s in sims:
        s.sync()
    torch.cuda.synchronize()


def loaded_sim(sc, n):
    sim = BatchedSim(sc, n, seed=0, sigma=-1.0, speed_dev=1)
    sim.reset()
    SimGroup([sim]).step('random', step_key=0, n_steps=START)
    sim.sync()
    return sim


def kernel(name, n, launches=200):
    sc = scenario(name)
    sim = loaded_sim(sc, n)
    net = frap_from_scenario(sc, 1).cuda().init_like_reference(0)
    pol = FusedMPLight(net, sc, seed=7)
    obs, out = sim.tensor('mplight'), sim.tensor('actions')
    for _ in range(10):
        pol.act(obs, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(launches):
        pol.act(obs, out=out, step_key=k)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / launches
    valid = sum(int((pol.valid[s] >= 0).sum()) for s in range(sc.n_signals)) / sc.n_signals
    flop = n * sc.n_signals * (valid * (net.oshape - 1) * 2 * (20 * 20 + 20 + 20) + net.oshape * 2 * (2 * 20 * 16 + 2 * 16 * 4 + 8))
    print(json.dumps(dict(mode='frap_kernel_greedy', map=name, envs=n, launches=launches, us_per_launch_events=round(us, 2),
                          valid_pairs_per_signal=round(valid, 2), gflop_per_launch=round(flop / 1e9, 3),
                          tflops=round(flop / (us * 1e-6) / 1e12, 2))), flush=True)
    sim.close()


def group_rate(sc, n, k, steps, agent, pol=None):
    per = n // k
    sims = [BatchedSim(sc, per, seed=0, sigma=-1.0, speed_dev=1, env_base=i * per, device_envs=n) for i in range(k)]
    for s in sims:
        s.set_outputs(('mplight',))
        s.reset()
    grp = SimGroup(sims)
    kw = dict(policy=pol.handle, epsilon=0.0, seed=7) if agent == 'mplight' else {}
    grp.step('random', step_key=0, n_steps=START)
    grp.step(agent, step_key=START, n_steps=5, **kw)
    sync_all(sims)
    t0 = time.perf_counter()
    for j in range(steps):
        grp.step(agent, step_key=START + 5 + j, **kw)
    sync_all(sims)
    dt = time.perf_counter() - t0
    for s in sims:
        s.close()
    return n * steps / dt


def ratio(name, n, k, steps=150):
    sc = scenario(name)
    net = frap_from_scenario(sc, 1).cuda().init_like_reference(0)
    pol = FusedMPLight(net, sc, seed=7)
    rows = []
    for rep in range(3):
        a = group_rate(sc, n, k, steps, 'random')
        b = group_rate(sc, n, k, steps, 'mplight', pol)
        rows.append((a, b))
        print(json.dumps(dict(mode='group_rep', map=name, envs=n, pipes=k, steps=steps, rep=rep, sim_only_env_steps_per_s=round(a),
                              sim_plus_mplight_env_steps_per_s=round(b), ratio=round(b / a, 3))), flush=True)
    a = sorted(r[0] for r in rows)[1]
    b = sorted(r[1] for r in rows)[1]
    print(json.dumps(dict(mode='group_median', map=name, envs=n, pipes=k, steps=steps, sim_only_env_steps_per_s=round(a),
                          sim_plus_mplight_env_steps_per_s=round(b), ratio=round(b / a, 3), target=0.90)), flush=True)


def torch_forward(name, n, reps=20):
    sc = scenario(name)
    sim = loaded_sim(sc, n)
    net = frap_from_scenario(sc, 1).cuda().init_like_reference(0)
    pol = FusedMPLight(net, sc, seed=7)
    obs = sim.tensor('mplight')
    with torch.no_grad():
        for _ in range(3):
            net(obs.float())
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            q = net(obs.float()).reshape(n, sc.n_signals, -1)
        e1.record()
        torch.cuda.synchronize()
        us_torch = e0.elapsed_time(e1) * 1e3 / reps
        _, qk = pol.act(obs, want_q=True)
        for _ in range(3):
            pol.act(obs, want_q=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            pol.act(obs, want_q=True)
        e1.record()
        torch.cuda.synchronize()
        us_full = e0.elapsed_time(e1) * 1e3 / reps
        e0.record()
        for _ in range(reps):
            pol.act(obs)
        e1.record()
        torch.cuda.synchronize()
        us_greedy = e0.elapsed_time(e1) * 1e3 / reps
    err = float((qk[..., :net.oshape] - q).abs().max())
    print(json.dumps(dict(mode='torch_vs_kernel', map=name, envs=n, torch_frap_forward_us=round(us_torch, 1),
                          kernel_all_q_us=round(us_full, 1), kernel_greedy_us=round(us_greedy, 1),
                          speedup_greedy=round(us_torch / us_greedy, 1), speedup_all_q=round(us_torch / us_full, 1),
                          max_abs_q_diff=err, peak_torch_mem_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20))), flush=True)
    sim.close()


if __name__ == '__main__':
    a = sys.argv[1:]
    if a[0] == 'kernel':
        kernel(a[1], int(a[2]), int(a[3]) if len(a) > 3 else 200)
    elif a[0] == 'ratio':
        ratio(a[1], int(a[2]), int(a[3]), int(a[4]) if len(a) > 4 else 150)
    elif a[0] == 'torch':
        torch_forward(a[1], int(a[2]), int(a[3]) if len(a) > 3 else 20)
    else:
        raise SystemExit(__doc__)
