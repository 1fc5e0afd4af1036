#!/usr/bin/env python3
"""MPLight trained on SEVERAL maps at once: one shared FRAP, one simulator, policy and replay ring per map, one fused update over all
rings (resco_amd/agents/mplight_multi.py: MultiMapMPLightLearner, rs_mplight_multi_*), then evaluated on maps it never saw.  FRAP's
weights do not depend on a map's signals or phase pairs, so one vector serves every map; with a single-instance simulator nobody can
afford this, here the maps step in lock-step on one GPU.

    python tools/mplight_multimap_train.py maps=cologne3,ingolstadt7 [n_envs per map: comma list or one value] [episodes] [batch]
                                           [replay_steps] [seed] [full] [--eval-on cologne8,...] [--n-step K] [--double-q]

Per env-step and map: policy_m.act -> replay_m.stage -> env_m.step -> replay_m.commit; then ONE learner.observe_step over all rings
(a Python-driven loop: the library loop and pipes per map are not built for this learner).  Every policy reads learner.flat
(share_weights); policy m draws with seed 7 + seed + 101 m; epsilon and the step key come from the one learner.t.  The maps must have
one episode length (horizon_steps).  Prints one JSON line per episode with the average trip delay per map, and a final line that adds,
for every --eval-on map, the greedy delay of the shared weights (zero-shot) beside that map's on-device random policy on the same demand.
`full`: MPLightFULL (states.mplight_full, demand_shape 4).  --n-step K (1 .. 32) and --double-q (the flags of tools/idqn_train.py): the
target's options of the shared update (rs_mplight_maps_set_target), every row walking its own map's ring; part of a checkpoint's signature.

Checkpoints (resco_amd/checkpoint.py, the flags of tools/mplight_train.py): --save PATH [--save-freq K] [--save-replay], --load PATH,
--stop-after K; the checkpoint's map is '+'.join(maps).  --load PATH --eval loads the weights alone -- from a multi-map checkpoint or
from a SINGLE-map one of tools/mplight_train.py, whatever its map was (checkpoint.load_frap_weights) -- and evaluates greedily on
the maps given and on the --eval-on maps.

Demand variants (the flags of tools/mplight_train.py): --demand-variants K[,jitter_s[,keep_lo,keep_hi]] gives the environments of every
training map K variants of that map's demand, drawn anew per episode from (seed, episode, map); the spec is part of the checkpoint's
signature.  --eval-demand K[,...]: the greedy evaluation of every training map (and of every --eval-on map) also runs on K held-out
variants and reports the mean delay per variant beside the figure of the map's own demand."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resco_amd.agents.idqn_learn import linear_epsilon                                      # noqa: E402
from resco_amd.agents.mplight import FusedMPLight, MPLightReplay, frap_from_scenario        # noqa: E402
from resco_amd.agents.mplight_multi import MultiMapMPLightLearner                           # noqa: E402
from resco_amd.multi_signal import VecMultiSignal                                           # noqa: E402
from resco_amd import checkpoint, demand                                                    # noqa: E402
from tools.idqn_train import target_flags                                                   # noqa: E402
from tools.mplight_train import delay, greedy_evaluation, greedy_on_variants                # noqa: E402


def random_delay(env, steps):
    """the on-device random policy on the baseline's demand seed -> average trip delay"""
    env.sim.set_seed(12345)
    env.reset()
    for k in range(steps):
        env.act_random(k)
        env.step(None)
    return round(delay(env)[0], 2)


def main(maps=('cologne3', 'ingolstadt7'), n_envs=(256,), episodes=30, batch=256, replay_steps=2048, seed=0, full=False, eval_on=(), quiet=False, made=None,
         save=None, save_freq=0, save_replay=False, load=None, eval_only=False, stop_after=0, demand_variants=None, eval_demand=0, n_step=1, double_q=False, per=None):
    """n_step / double_q: the learner's options of the same names.  per: refused (--per; prioritised replay is the single-map learner's).  -> (rows, final); a run that leaves at stop_after returns (rows, None).  made: a dict that receives the learner (closed when
    the call returns; its vectors stay readable).  demand_variants / eval_demand: the demand flags of the module docstring."""
    if per is not None and per is not False:
        raise SystemExit('--per is not available on several maps: prioritised replay is built into the single-map fused update only (tools/mplight_train.py)')
    n_var, var_kw = demand.parse_spec(demand_variants)
    n_eval, eval_kw = demand.parse_spec(eval_demand)
    eval_kw = eval_kw or var_kw
    maps, eval_on = [str(m) for m in maps], [str(m) for m in eval_on]
    n_envs = [int(n) for n in n_envs]
    n_envs = n_envs * len(maps) if len(n_envs) == 1 else n_envs
    if len(n_envs) != len(maps):
        raise ValueError('%d environment counts for %d maps' % (len(n_envs), len(maps)))
    state, D = ('mplight_full', 4) if full else ('mplight', 1)
    make_env = lambda name, n: VecMultiSignal(name, n, states=(state,), rewards=('pressure',), seed=0, outputs=(state,))
    envs = [make_env(name, n) for name, n in zip(maps, n_envs)]
    steps = envs[0].horizon_steps
    if any(e.horizon_steps != steps for e in envs):
        for e in envs:
            e.close()
        raise ValueError('the maps step in lock-step and must have one horizon_steps, got %s' % {m: e.horizon_steps for m, e in zip(maps, envs)})
    nets = [frap_from_scenario(e.scenario, D).cuda() for e in envs]
    nets[0].init_like_reference(seed)
    learner = MultiMapMPLightLearner(nets, [e.n_signals for e in envs], gamma=0.99, lr=1e-3, target_update=500, batch_size=batch, seed=seed, n_step=n_step,
                                     double_q=double_q)
    if made is not None:
        made['learner'] = learner
    policies = [FusedMPLight(net, e.scenario, seed=7 + seed + 101 * m) for m, (net, e) in enumerate(zip(nets, envs))]
    for p in policies:
        p.share_weights(learner.flat)           # every map's policy reads the vector the update writes
    replays = [MPLightReplay(replay_steps, n, e.n_signals, 1 + 12 * D, device='cuda') for n, e in zip(n_envs, envs)]
    actions = [e.tensor('actions') for e in envs]
    pairs = [torch.zeros(n, e.n_signals, dtype=torch.int32, device='cuda') for n, e in zip(n_envs, envs)]
    decay = int(0.8 * episodes * steps)
    agent = 'MPLightFULLMulti' if full else 'MPLightMulti'
    # every net's parameters are views of learner.flat: net0 stands for all of them (and is what load_frap_weights reads)
    objects = {'env%d' % m: e for m, e in enumerate(envs)}
    objects.update(net0=nets[0], learner=learner)
    for kind, seq in (('policy', policies), ('replay', replays)):
        objects.update({'%s%d' % (kind, m): o for m, o in enumerate(seq)})
    hyper = dict(episodes=episodes, decay_steps=decay, seed=seed)
    if n_var:
        hyper['demand_variants'] = str(demand_variants)     # (a resume under another spec is another run: refused)
    map_name = '+'.join(maps)
    first_ep, rows = 0, []
    if load and eval_only:
        rows = list(checkpoint.load_frap_weights(load, nets[0]).get('rows', []))        # (nets[0]'s parameters ARE learner.flat)
        first_ep = episodes
    elif load:
        progress = checkpoint.load(load, agent=agent, map_name=map_name, objects=objects, hyper=hyper)
        first_ep, rows = int(progress['episode']), list(progress['rows'])

    def leave():
        learner.close()
        for o in policies + envs:
            o.close()

    rnd = {name: random_delay(e, steps) for name, e in zip(maps, envs)}
    for ep in range(first_ep, episodes):
        obs = []
        for m, e in enumerate(envs):
            e.sim.set_seed(1000 + ep + 7919 * seed)
            if n_var:
                e.set_demand(demand.demand_set(e.scenario, n_var, (demand.TRAIN_STREAM, seed, ep, m), **var_kw))
            obs.append(e.reset()[state])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            eps = linear_epsilon(learner.t, 1.0, 0.0, decay)
            for m, e in enumerate(envs):
                policies[m].act(obs[m], epsilon=eps, step_key=learner.t, out=actions[m], pair_out=pairs[m])
                replays[m].stage(obs[m])
                o, r, done, _ = e.step(None)
                replays[m].commit(pairs[m], r['pressure'].float(), done)
                obs[m] = o[state]
            learner.observe_step(replays)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rows.append(dict(episode=ep, epsilon=round(eps, 3), avg_delay_s={name: round(delay(e)[0], 2) for name, e in zip(maps, envs)},
                         updates=learner.n_updates, env_steps_per_s=round(sum(n_envs) * steps / dt)))
        if not quiet:
            print(json.dumps(rows[-1]), flush=True)
        write, stop = checkpoint.due(ep + 1, episodes, save, save_freq, stop_after)
        if write:
            checkpoint.save(save, agent=agent, map_name=map_name, objects=objects, hyper=hyper, replay=save_replay,
                            progress=dict(episode=ep + 1, seed=seed, rows=rows))
        if stop:
            leave()
            return rows, None
    final = dict(maps=maps, agent=agent, envs=n_envs, episodes=episodes, batch=batch, replay_steps=replay_steps, seed=seed, random_avg_delay_s=rnd)
    if not eval_only:       # (the rows of a checkpoint loaded for evaluation may be another tool's)
        final['best_training_episode_delay_s'] = {name: min(r['avg_delay_s'][name] for r in rows) for name in maps}
    for e in envs:
        e.set_demand(None)      # the evaluations below start from every map's own demand
    if n_var:
        final['demand_variants'] = str(demand_variants)
    held_out = lambda e, m: demand.demand_set(e.scenario, n_eval, (demand.EVAL_STREAM, seed, m), **eval_kw)
    if eval_only or n_eval > 0:
        final['greedy_avg_delay_s'] = {name: greedy_evaluation(e, p, state, a, steps, 12345) for name, e, p, a in zip(maps, envs, policies, actions)}
    if n_eval > 0:              # reported, not judged
        final['greedy_variant_delay_s'] = {name: greedy_on_variants(e, p, state, a, steps, 12345, held_out(e, m))
                                           for m, (name, e, p, a) in enumerate(zip(maps, envs, policies, actions))}
    zero = {}
    for m, name in enumerate(eval_on):          # a map the weights never saw: its own pairs, the shared vector
        e = make_env(name, n_envs[0])
        if e.horizon_steps != steps:
            e.close()
            raise ValueError('%s has horizon_steps %d, the training maps %d' % (name, e.horizon_steps, steps))
        p = FusedMPLight(frap_from_scenario(e.scenario, D).cuda(), e.scenario, seed=7 + seed + 101 * (len(maps) + m))
        p.share_weights(learner.flat)
        zero[name] = dict(random_avg_delay_s=random_delay(e, steps), greedy_avg_delay_s=greedy_evaluation(e, p, state, e.tensor('actions'), steps, 12345))
        if n_eval > 0:
            zero[name]['greedy_variant_delay_s'] = greedy_on_variants(e, p, state, e.tensor('actions'), steps, 12345, held_out(e, len(maps) + m))
        p.close()
        e.close()
    if eval_on:
        final['zero_shot'] = zero
    if not quiet:
        print(json.dumps(final), flush=True)
    leave()
    return rows, final


if __name__ == '__main__':
    ckpt, a = checkpoint.tool_flags(sys.argv[1:])
    dem, a = demand.tool_flags(a)
    opts, a = target_flags(a)
    ckpt.update(opts)
    eval_on = ()
    if '--eval-on' in a:
        i = a.index('--eval-on')
        if i + 1 >= len(a):
            raise SystemExit('--eval-on needs a comma list of maps')
        eval_on = tuple(x for x in a[i + 1].split(',') if x)
        a = a[:i] + a[i + 2:]
    if not a or not a[0].startswith('maps='):
        raise SystemExit(__doc__)
    main(tuple(x for x in a[0][len('maps='):].split(',') if x), tuple(int(x) for x in a[1].split(',')) if len(a) > 1 else (256,),
         int(a[2]) if len(a) > 2 else 30, int(a[3]) if len(a) > 3 else 256, int(a[4]) if len(a) > 4 else 2048, int(a[5]) if len(a) > 5 else 0,
         full=len(a) > 6 and a[6] == 'full', eval_on=eval_on, **ckpt, **dem)
