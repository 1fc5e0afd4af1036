#!/usr/bin/env python3
"""Generate the MPLight fixtures from the reference (BUILD CONTAINER ONLY: imports the reference at generation time, as
make_golden.py does; the fixtures are data).

  tests/golden/mplight_frap.npz   per map: a seeded state_dict of the reference's FRAP (torch.manual_seed(SEED) before
                                   MPLight(...) is built), observation batches -- the states.mplight rows of the existing golden
                                   case of the map plus random rows with large pressures and every phase index --, the reference's
                                   Q-values (FRAP.forward) and greedy actions (SharedDQN.batch_act with training off, through
                                   SharedAgent.act); the same for demand_shape 4 (MPLightFULL) on the states.mplight_full rows
  tests/golden/ref_mplight.json   per map with data: best episode and mean of the last ten episodes of the reference's MPLight
                                   delay curve (resco_benchmark/utils/avg_timeLoss.py rows 'MPLight <map> ...')

PFRL is not installed: a minimal stub `pfrl` holds what agents/mplight.py and agents/pfrl_dqn.py import and what FRAP.forward /
SharedDQN.batch_act call (the greedy path only; the stub's DQN evaluates the model on phi(batch_obs)).

  python tests/golden/make_mplight_golden.py
"""
import contextlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('RESCO_REFERENCE', '/root/reference')
MAPS = {'cologne1': 'cologne1_d200', 'cologne3': 'cologne3_d200', 'cologne8': 'cologne8_d200', 'ingolstadt1': 'ingolstadt1_d200',
        'ingolstadt7': 'ingolstadt7_d200', 'ingolstadt21': 'ingolstadt21_d200'}
SEED = 5
N_RANDOM = 24


def install_pfrl_stub():
    pfrl = types.ModuleType('pfrl')
    mods = {n: types.ModuleType('pfrl.' + n) for n in ('explorers', 'replay_buffers', 'explorer', 'agents', 'q_functions', 'utils',
                                                        'replay_buffer')}
    contexts = types.ModuleType('pfrl.utils.contexts')

    class Explorer:
        pass

    class LinearDecayEpsilonGreedy(Explorer):
        def __init__(self, start_epsilon, end_epsilon, decay_steps, random_action_func, logger=None):
            self.start_epsilon, self.end_epsilon, self.decay_steps = start_epsilon, end_epsilon, decay_steps
            self.random_action_func, self.epsilon = random_action_func, start_epsilon

    class ReplayBuffer:
        def __init__(self, capacity):
            self.capacity = capacity

    class _AV:
        def __init__(self, q):
            self.params = (q,)

        @property
        def greedy_actions(self):
            return self.params[0].argmax(axis=1)

    class DiscreteActionValueHead(torch.nn.Module):
        def forward(self, q):
            return _AV(q)

    class DQN:
        def __init__(self, q_function, optimizer, replay_buffer, gamma, explorer, gpu=None, minibatch_size=32, replay_start_size=32,
                     phi=lambda x: x, target_update_interval=1, update_interval=1):
            self.model, self.phi, self.training = q_function, phi, False

        def _evaluate_model_and_update_recurrent_states(self, batch_obs):
            return self.model(torch.as_tensor(np.stack([self.phi(o) for o in batch_obs])))

        def batch_act(self, batch_obs):
            with torch.no_grad():
                return self._evaluate_model_and_update_recurrent_states(batch_obs).greedy_actions.numpy()

    @contextlib.contextmanager
    def evaluating(model):
        was = model.training
        model.eval()
        try:
            yield
        finally:
            model.train(was)

    mods['explorers'].LinearDecayEpsilonGreedy = LinearDecayEpsilonGreedy
    mods['explorer'].Explorer = Explorer
    mods['replay_buffers'].ReplayBuffer = ReplayBuffer
    mods['replay_buffer'].AbstractReplayBuffer = ReplayBuffer
    mods['agents'].DQN = DQN
    mods['q_functions'].DiscreteActionValueHead = DiscreteActionValueHead
    contexts.evaluating = evaluating
    mods['utils'].contexts = contexts
    for n, m in mods.items():
        setattr(pfrl, n, m)
    sys.modules['pfrl'] = pfrl
    sys.modules.update({'pfrl.' + n: m for n, m in mods.items()})
    sys.modules['pfrl.utils.contexts'] = contexts


def reference_agent(map_name, demand_shape, signal_ids):
    from resco_benchmark.agents.mplight import MPLight
    config = {'demand_shape': demand_shape, 'EPS_START': 1.0, 'EPS_END': 0.0, 'steps': 1000, 'GAMMA': 0.99, 'BATCH_SIZE': 32,
              'TARGET_UPDATE': 500, 'num_lights': len(signal_ids), 'load': False}
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(open(os.devnull, 'w')):
        ag = MPLight(config, None, map_name, 0)
    ag.agent.agent.training = False
    return ag


def batches(sc, rows_golden, width, rng, full):
    """[R, S, width] observation batches: the golden case's rows, then random rows whose phase runs through every green index"""
    S = sc.n_signals
    g = rows_golden.reshape(rows_golden.shape[0], S, width).astype(np.float32 if full else np.int32)
    R = N_RANDOM
    if full:
        r = rng.normal(0.0, 6.0, (R, S, width)).astype(np.float32)
    else:
        r = rng.integers(-80, 81, (R, S, width)).astype(np.int32)
    for s in range(S):
        r[:, s, 0] = np.arange(R) % int(sc.tls_ngreen[s])
    return np.concatenate([g, r])


def main():
    sys.path.insert(0, ROOT)
    os.environ.setdefault('SUMO_HOME', tempfile.mkdtemp())
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from oracle import ref_harness
    ref_harness.install_stubs(None)         # traci / sumolib / gym stand-ins: the reference package imports them at import time
    install_pfrl_stub()
    from resco_amd.multi_signal import load_scenario
    from resco_amd.config.map_config import map_configs
    out = {}
    rng = np.random.default_rng(2024)
    for mp, case in MAPS.items():
        sc = load_scenario(mp, None, map_configs.get(mp, {}).get('lights', ()), 3)
        gold = np.load(os.path.join(HERE, case + '.npz'))
        ids = list(sc.signal_ids)
        for D, key, full in ((1, 'mplight', False), (4, 'mplight_full', True)):
            ag = reference_agent(mp, D, ids)
            model = ag.agent.model
            obs = batches(sc, gold[key], 1 + 12 * D, rng, full)
            q = np.zeros(obs.shape[:2] + (model.oshape,), np.float32)
            act = np.zeros(obs.shape[:2], np.int32)
            with torch.no_grad():
                for t in range(obs.shape[0]):
                    q[t] = model(torch.as_tensor(obs[t].astype(np.float32))).params[0].numpy()
                    a = ag.act({sid: obs[t, s] for s, sid in enumerate(ids)})
                    act[t] = [a[sid] for sid in ids]
            tag = '%s_d%d' % (mp, D)
            out[tag + '_obs'] = obs
            out[tag + '_q'] = q
            out[tag + '_act'] = act
            for k, v in model.state_dict().items():
                out['%s_sd_%s' % (tag, k)] = v.numpy()
        print(mp, {k: v.shape for k, v in out.items() if k.startswith(mp + '_d1_') and '_sd_' not in k})
    np.savez_compressed(os.path.join(HERE, 'mplight_frap.npz'), seed=np.int64(SEED), **out)

    ns = {}
    with open(os.path.join(REF, 'resco_benchmark', 'utils', 'avg_timeLoss.py')) as f:
        exec(f.read(), {'np': np, 'array': np.array, '__name__': 'ref'}, ns)
    ref = {}
    for mp in MAPS:
        for k, v in ns['delays'].items():
            if k.startswith('MPLight %s ' % mp) and not k.endswith('_yerr') and len(v):
                a = np.asarray(v, float)
                ref[mp] = dict(best=round(float(a.min()), 2), last10_mean=round(float(a[-10:].mean()), 2), episodes=int(a.size), row=k)
    with open(os.path.join(HERE, 'ref_mplight.json'), 'w') as f:
        json.dump(ref, f, indent=1, sort_keys=True)
    print(json.dumps(ref, indent=1))


if __name__ == '__main__':
    main()
