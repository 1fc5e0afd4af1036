"""MultiSignal: the gym-style multi-agent traffic-signal environment, backed by the HIP simulator.

Drop-in for the reference's resco_benchmark/multi_signal.py:9-234 — same constructor arguments
(multi_signal.py:10-12, as main.py:81-89 passes them), reset() / step(act) / close() / render(), and the
attributes callers read (obs_shape, phases, all_ts_ids, ts_order, signals, signal_ids, observation_space,
action_space, n_agents, connection_name, run).  The `self.sumo` TraCI connection does not exist: every
sumo.* call of the reference (simulationStep, trafficlight.setPhase/getPhase, lane/vehicle getters) happens
inside one HIP kernel launch per step (resco_amd/csrc/resco_sim.hip) through the C ABI of
include/resco_sim.h.

MultiSignal is the single-environment dict API existing agents plug into unchanged;
VecMultiSignal is the batched tensor API (N lock-step environments on one GPU).
"""
import os

import numpy as np

from . import rewards as _rewards
from . import states as _states
from .config.map_config import map_configs
from .config.signal_config import signal_configs
from .scenario import Scenario, compile_from_sumocfg, compile_scenario, parse_net, parse_routes
from .sim import BatchedSim, speed_factor, torch_stream
from .traffic_signal import Phase, Signal

try:  # gym is optional: only observation_space / action_space use it
    import gym as _gym
    _Box, _Discrete = _gym.spaces.Box, _gym.spaces.Discrete
    _EnvBase = _gym.Env
except Exception:  # pragma: no cover - gym is not installed in the build image
    _EnvBase = object

    class _Box:
        def __init__(self, low, high, shape, dtype=np.float32):
            self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), dtype

    class _Discrete:
        def __init__(self, n):
            self.n = int(n)

_SCEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'scenarios')


def tripinfo_records(sc, log, now, lane, trip, depart, tloss, wtot, seed, env_index, speed_dev):
    """tripinfo entries from the trip log ([n_trips][4] depart tick, arrival tick, timeLoss / 1024, waiting) and the
    per-slot arrays of the vehicles still on the network: finished trips in arrival order, then the running ones."""
    sched = sc.trip_depart

    def rec(k, depart_tick, arrival_tick, tl, waiting):
        dep = depart_tick - 1               # inserted at the end of the previous simulation second
        # (the speed factor is a function of seed, environment and trip)
        sf = speed_factor(seed, env_index, k, sc.vtype_params[int(sc.trip_vtype[k])], speed_dev)
        return {'id': sc.trip_ids[k], 'depart': float(sc.begin + dep), 'departDelay': float(dep - int(sched[k])),
                'arrival': float(sc.begin + arrival_tick) if arrival_tick > 0 else -1.0,
                'duration': float((arrival_tick if arrival_tick > 0 else now) - depart_tick),
                'waitingTime': float(waiting), 'timeLoss': float(tl),
                'vType': sc.vtype_ids[int(sc.trip_vtype[k])], 'speedFactor': float(sf)}

    done = np.nonzero(log[:, 1] > 0)[0]
    recs = [rec(int(k), int(log[k, 0]), int(log[k, 1]), log[k, 2] / 1024.0, int(log[k, 3]))
            for k in done[np.argsort(log[done, 1], kind='stable')]]
    for s_ in np.nonzero(np.asarray(lane) < 0xFFFE)[0]:
        recs.append(rec(int(trip[s_]), int(depart[s_]), 0, float(tloss[s_]), int(wtot[s_])))
    return recs


def write_tripinfo(path, recs):
    """tripinfo_<run>.xml with the attributes the reference's post-processing reads (utils/readXML.py:36-47)"""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        f.write('<?xml version="1.0" encoding="UTF-8"?>\n<tripinfos>\n')
        for r in recs:
            f.write('    <tripinfo id="%s" depart="%.2f" departDelay="%.2f" arrival="%.2f" duration="%.2f" '
                    'waitingTime="%.2f" timeLoss="%.2f" vType="%s" speedFactor="%.2f"/>\n'
                    % (r['id'], r['depart'], r['departDelay'], r['arrival'], r['duration'], r['waitingTime'],
                       r['timeLoss'], r['vType'], r['speedFactor']))
        f.write('</tripinfos>\n')


def load_scenario(map_name, net=None, lights=(), yellow_length=3):
    """Scenario tables for a map: compiled from the SUMO files when `net` names an existing .sumocfg,
    otherwise the pre-compiled tables shipped in resco_amd/scenarios/."""
    if net is not None and os.path.isfile(net) and net.endswith('.sumocfg'):
        return compile_from_sumocfg(map_name, net, signal_configs[map_name], lights=lights,
                                    yellow_length=yellow_length)
    path = os.path.join(_SCEN_DIR, map_name + '.npz')
    if not os.path.exists(path):
        raise EnvironmentError('no scenario for map %r: %r is not a .sumocfg and %s does not exist'
                               % (map_name, net, path))
    sc = Scenario.load(path)
    if sc.yellow_length != yellow_length:
        raise EnvironmentError('packaged scenario %s was compiled with yellow_length=%d (asked %d); pass the '
                               '.sumocfg path to recompile' % (map_name, sc.yellow_length, yellow_length))
    if len(lights) > 0 and list(lights) != list(sc.signal_ids):
        raise EnvironmentError('packaged scenario %s controls %s' % (map_name, sc.signal_ids))
    return sc


class MultiSignal(_EnvBase):
    """The reference's MultiSignal (resco_benchmark/multi_signal.py:10-216: same constructor, reset / step / close, attributes) on the
    HIP simulator; the keyword-only arguments after `gymma` are this package's.

    **tls_expiry** -- what `trafficlight.setPhase` (Signal.prep_phase / set_phase, traffic_signal.py:176-187) leaves behind is a
    parameter of this simulator (rs_params.tls_hold, inverted).  `tls_expiry=True` (default) is SUMO's documented setPhase: the phase
    runs for its programme duration and the programme then continues with the next phase of the list (the switch is re-scheduled
    `duration` seconds ahead, MSSimpleTrafficLightLogic::changeStepAndDuration), so a 6 s green chosen for a 10 s step hands its 7th
    second to the next index.  `tls_expiry=False` keeps the selected phase until the next action: round 5's default, a calibration
    of this build's own traffic model that reproduces the reference-held random-policy figures better (36 of 42 result cells inside
    +-35 % against 29, profiles/r06_reference_bands_both_modes.txt) while trained agents reach the same delays either way
    (profiles/r06_heldout_both_modes.txt).  Neither is pinned against a SUMO binary (`tools/sumo_runner.py diff` decides it on a box
    that has SUMO); results, bench figures and the held-out IDQN check are reported for BOTH values (README).
    """

    def __init__(self, run_name, map_name, net, state_fn, reward_fn, route=None, gui=False, end_time=3600,
                 step_length=10, yellow_length=4, step_ratio=1, max_distance=200, lights=(), log_dir='/',
                 libsumo=False, warmup=0, gymma=False, *, device=0, seed=None, sigma=-1.0, speed_dev=1,
                 fixed_program=False, scenario=None, use_fast_path=True, tripinfo=True, tls_expiry=True):
        if int(step_ratio) < 1:
            raise ValueError('step_ratio must be a positive integer')
        if int(step_ratio) > 1:
            # the reference uses step_ratio for SUB-SECOND SUMO steps (its .sumocfg sets the step length; e.g. four 0.25 s steps per
            # step_sim()).  A tick here is always 1 s: step_ratio = k means k one-second ticks per step_sim(), so an env-step advances
            # step_length x k simulated seconds and `done` comes after 1 / k of the env-steps.  The loop structure is the reference's
            # (pinned by tests/golden/cologne8_d200_sr2), the time semantics of a sub-second configuration are not.
            import warnings
            warnings.warn('step_ratio=%d: ticks stay 1 s long here (a sub-second SUMO step length is not modelled); one env-step '
                          'covers %d simulated seconds' % (int(step_ratio), int(step_length) * int(step_ratio)))
        self.libsumo, self.gymma, self.gui = libsumo, gymma, gui
        self.log_dir, self.net, self.route = log_dir, net, route
        self.state_fn, self.reward_fn = state_fn, reward_fn
        self.max_distance, self.warmup = max_distance, warmup
        self.end_time, self.step_length = end_time, step_length
        self.yellow_length, self.step_ratio = yellow_length, step_ratio
        self.map_name = map_name
        self.use_fast_path = use_fast_path
        self.connection_name = run_name + '-' + map_name + '---' + state_fn.__name__ + '-' + reward_fn.__name__

        # multi_signal.py:33-38, 123-124: with `route` the demand comes from one route file PER RUN, `<route>_<run>.rou.xml` next to
        # the net file `net` (the two grid maps; their archives unpack into a directory of the map's name)
        self._lights, self._net_parsed, self._sc_run = tuple(lights), None, None
        if route is not None and scenario is None:
            for grid in ('grid4x4', 'arterial4x4'):
                if grid in self.route:
                    self.route += '/' + grid
                    break
            scenario = self._compile_run(1)
            self._sc_run = 1
        self.scenario = scenario if scenario is not None else load_scenario(map_name, net, lights, yellow_length)
        sc = self.scenario
        if sc.yellow_length != yellow_length:       # the yellow phases are compiled into the scenario's programmes
            raise EnvironmentError('scenario %s was compiled with yellow_length=%d (asked %d)' % (map_name, sc.yellow_length, yellow_length))
        self._base_seed = int.from_bytes(os.urandom(4), 'little') if seed is None else int(seed)
        self._sim_kw = dict(device=device, max_distance=max_distance, sigma=sigma, speed_dev=speed_dev,
                            fixed_program=1 if fixed_program else 0, step_length=step_length, yellow_length=yellow_length,
                            trip_log=1 if tripinfo else 0,
                            step_ratio=step_ratio,      # multi_signal.py:102-105: step_sim() = step_ratio simulation steps
                            tls_expiry=1 if tls_expiry else 0)       # include/resco_sim.h: what setPhase leaves behind
        self.sim = BatchedSim(sc, 1, seed=self._base_seed, **self._sim_kw)
        self.tripinfo = tripinfo
        self.view_env = 0
        self._version = 0
        self._cache = {}

        # multi_signal.py:48-59: all TLS ids, green phases per signal
        self.signal_ids = list(sc.signal_ids)
        self.phases = {sid: [Phase(d, s) for d, s in sc.signal_meta[sid]['phases'][:sc.signal_meta[sid]['n_green']]]
                       for sid in sc.signal_ids}
        self.all_ts_ids = list(lights) if len(lights) > 0 else list(sc.signal_ids)
        self.ts_starter = len(self.all_ts_ids)
        self.signals = {}
        for i, ts in enumerate(self.all_ts_ids):
            self.signals[ts] = Signal(self, i, ts)
        for ts in self.all_ts_ids:
            self.signals[ts].signals = self.signals

        # multi_signal.py:67-86: observation shapes from one evaluation of the state function
        self.obs_shape, self.observation_space, self.action_space, self.ts_order = {}, [], [], []
        observations = self._evaluate(self.state_fn)
        for ts in observations:
            shape = observations[ts].shape
            self.obs_shape[ts] = shape
            self.ts_order.append(ts)
            self.observation_space.append(_Box(low=-np.inf, high=np.inf, shape=shape))
            if ts not in self.phases:       # FMA2C manager keys are not traffic signals (the reference tests only
                continue                    # 'top_mgr' / 'bot_mgr' and raises KeyError on ingolstadt21's managers)
            self.action_space.append(_Discrete(len(self.phases[ts])))
        self.n_agents = self.ts_starter
        self.run = 0
        self.metrics = []
        self.wait_metric = {}
        self.connection_name = (run_name + '-' + map_name + '-' + str(len(lights)) + '-' + state_fn.__name__ + '-' +
                                reward_fn.__name__)
        try:
            os.makedirs(log_dir + self.connection_name, exist_ok=True)
        except OSError:
            pass

    def _compile_run(self, run):
        """scenario tables for the demand of episode `run`: `<route>_<run>.rou.xml` over the net file (SUMO's `-n net -r routes`,
        begin 0: multi_signal.py:123-124)"""
        path = self.route + '_' + str(run) + '.rou.xml'
        if not os.path.isfile(path) or not (self.net and os.path.isfile(self.net)):
            raise EnvironmentError('route file %s (or net file %s) does not exist' % (path, self.net))
        if self._net_parsed is None:
            self._net_parsed = parse_net(self.net)
        vtypes, trips = parse_routes(path)
        return compile_scenario(self.map_name, self._net_parsed, vtypes, trips, 0, int(self.end_time), signal_configs[self.map_name],
                                lights=self._lights, yellow_length=self.yellow_length)

    # ------------------------------------------------------------------ device buffer access
    def _host(self, name):
        hit = self._cache.get(name)
        if hit is None or hit[0] != self._version:
            hit = (self._version, self.sim.read(name))
            self._cache[name] = hit
        return hit[1]

    def _is_fast(self, fn):
        fast = getattr(fn, 'fast_buffer', None) if self.use_fast_path else None
        registry = _states.REGISTRY.get(fn.__name__) is fn or _rewards.REGISTRY.get(fn.__name__) is fn
        return bool(fast) and registry

    def _observe_all(self):
        """Signal.observe() runs for every signal in every step of the reference (multi_signal.py:183-186): when a plugin
        function reads the Signal views, every view is decoded once per step, so that `arrivals` / `departures` are relative
        to the previous STEP also for a signal the function did not look at last time."""
        if not (self._is_fast(self.state_fn) and self._is_fast(self.reward_fn)):
            for sg in self.signals.values():
                sg.full_observation

    def _evaluate(self, fn):
        """fn(signals) through the kernel-produced buffer when the registry knows one, else on the host."""
        if not self._is_fast(fn):
            return fn(self.signals)
        sc, e = self.scenario, self.view_env
        out = {}
        name = fn.__name__
        for i, ts in enumerate(self.all_ts_ids):
            o0, o1 = int(sc.sig_obs_start[i]), int(sc.sig_obs_start[i + 1])
            if name == 'drq_norm':
                out[ts] = np.expand_dims(self._host('drq_norm')[e, o0:o1].astype(np.float64), axis=0)
            elif name == 'drq':
                agg = self._host('lane_agg')[e, o0:o1].astype(np.float64)
                ph = int(self._host('phase')[e, i])
                rows = np.stack([(np.arange(o1 - o0) == ph).astype(np.float64), agg[:, 1], agg[:, 2], agg[:, 0],
                                 agg[:, 4]], axis=1)
                out[ts] = np.expand_dims(rows, axis=0)
            elif name == 'mplight':
                out[ts] = self._host('mplight')[e, i].astype(np.int64)
            elif name == 'wave':
                out[ts] = self._host('wave')[e, i].astype(np.int64)
            elif name == 'wait':
                w = float(self._host('wait')[e, i])      # -sum(float waiting times); the empty sum is the int 0
                out[ts] = w if w != 0 else 0
            elif name == 'wait_norm':
                out[ts] = np.float32(self._host('wait_norm')[e, i])
            elif name == 'pressure':
                out[ts] = int(self._host('pressure')[e, i])
            else:  # pragma: no cover
                return fn(self.signals)
        return out

    # ------------------------------------------------------------------ gym API
    def step_sim(self):
        """step_ratio x sumo.simulationStep() (multi_signal.py:102-105) and nothing else -- the Signal objects are not observed,
        their waiting times and arrival / departure sets stay as they are; MultiSignal.step() fuses its ticks into one launch"""
        self.sim.step_sim(int(self.step_ratio))
        self._version += 1

    def reinit_signals(self):
        """Fresh Signal objects on the RUNNING simulation (what reset() does after restarting SUMO,
        multi_signal.py:141-147): returns the first observation, like reset()."""
        self.sim.reinit_signals()
        self._version += 1
        for ts in self.signal_ids:
            self.signals[ts].last_step_vehicles = None
        states = self._evaluate(self.state_fn)
        return [states[ts] for ts in self.ts_order] if self.gymma else states

    def reset(self):
        if self.run != 0:
            self.save_metrics()
            self.save_tripinfo()
        self.metrics = []
        self.run += 1
        if self.route is not None and self._sc_run is not None and self._sc_run != self.run:
            # a new SUMO with this run's route file (multi_signal.py:123-124): the tables are compiled from it, the net stays
            self.sim.close()
            self.scenario = self._compile_run(self.run)
            self._sc_run = self.run
            self.sim = BatchedSim(self.scenario, 1, seed=self._base_seed, **self._sim_kw)
            self._cache = {}
        # the reference restarts SUMO with --random (multi_signal.py:127): a new seed per episode
        self.sim.set_seed((self._base_seed + 0x9E3779B1 * self.run) & 0xFFFFFFFF)
        self.sim.reset()
        if self.warmup > 0:             # multi_signal.py:139-140: warm-up ticks before the Signal objects exist
            self.sim.ticks(self.warmup * int(self.step_ratio))      # `warmup` x step_sim() (multi_signal.py:139-140)
            self.sim.reinit_signals()
        self._version += 1
        self.signal_ids = [self.all_ts_ids[i] for i in range(self.ts_starter)]
        for ts in self.signal_ids:
            self.signals[ts].last_step_vehicles = None
            self.wait_metric[ts] = 0.0
        self._observe_all()
        states = self._evaluate(self.state_fn)
        if self.gymma:
            return [states[ts] for ts in self.ts_order]
        return states

    def step(self, act):
        if self.gymma:
            act = {ts: act[i] for i, ts in enumerate(self.ts_order)}
        a = np.asarray([[int(act[ts]) for ts in self.all_ts_ids]], dtype=np.int32)
        self.sim.step(a)
        self._version += 1
        self._observe_all()
        observations = self._evaluate(self.state_fn)
        rewards = self._evaluate(self.reward_fn)
        self.calc_metrics(rewards)
        done = self.sim_time() >= self.end_time
        if self.gymma:
            return ([observations[ts] for ts in self.ts_order], [rewards[ts] for ts in self.ts_order], [done],
                    {'eps': self.run})
        return observations, rewards, done, {'eps': self.run}

    def sim_time(self):
        """simulation.getTime(): absolute seconds (sumocfg begin + ticks)."""
        return float(self.scenario.begin + int(self._host('env')[self.view_env, 0]))

    def calc_metrics(self, rewards):
        qs, qm = self._host('queue_sum')[self.view_env], self._host('queue_max')[self.view_env]
        queue_lengths = {ts: int(qs[i]) for i, ts in enumerate(self.all_ts_ids)}
        max_queues = {ts: int(qm[i]) for i, ts in enumerate(self.all_ts_ids)}
        self.metrics.append({'step': self.sim_time(), 'reward': rewards, 'max_queues': max_queues,
                             'queue_lengths': queue_lengths})

    def save_metrics(self):
        log = os.path.join(self.log_dir, self.connection_name + os.sep + 'metrics_' + str(self.run) + '.csv')
        try:
            os.makedirs(os.path.dirname(log), exist_ok=True)
            with open(log, 'w+') as output_file:
                for line in self.metrics:
                    csv_line = ''
                    for metric in ['step', 'reward', 'max_queues', 'queue_lengths']:
                        csv_line = csv_line + str(line[metric]) + ', '
                    output_file.write(csv_line + '\n')
        except OSError:
            pass

    def tripinfo_records(self):
        """Per-trip records of the running episode, finished trips first then the ones still in the network
        (SUMO's --tripinfo-output with --tripinfo-output.write-unfinished, multi_signal.py:127-129)."""
        if not self.tripinfo:
            return []
        e = self.view_env
        rd = self.sim.read
        # (the trips of the viewed environment's own demand variant, if the handle has variants: BatchedSim.set_demand)
        return tripinfo_records(self.sim.env_scenarios()[e], rd('trip_log')[e], int(rd('env')[e, 0]), rd('veh_lane')[e], rd('veh_trip')[e],
                                rd('veh_depart')[e], rd('veh_tloss')[e], rd('veh_wtot')[e], self.sim.seed,
                                self.sim.env_base + e, self.sim.speed_dev)

    def save_tripinfo(self):
        if not self.tripinfo:
            return
        try:
            write_tripinfo(os.path.join(self.log_dir, self.connection_name, 'tripinfo_' + str(self.run) + '.xml'), self.tripinfo_records())
        except OSError:
            pass

    def trip_stats(self):
        """tripinfo-style episode aggregates of this environment (avg duration / timeLoss / departDelay)."""
        st = {k: int(v[self.view_env]) for k, v in self.sim.stats().items()}
        n = max(1, st['arrived'])
        st.update(avg_duration=st['sum_duration'] / n, avg_time_loss=st['sum_time_loss_q10'] / 1024.0 / n,
                  avg_depart_delay=st['sum_depart_delay'] / max(1, st['inserted']),
                  mean_active=st['active_ticks'] / max(1, st['ticks']))
        return st

    def render(self, mode='human'):
        pass

    def close(self):
        self.save_metrics()
        self.save_tripinfo()
        self.sim.close()


def fma2c_state_tables(sc, cfg, full=False):
    """The index tables of states.fma2c / fma2c_full (reference states.py:162-305) over the feature vector F of
    VecMultiSignal.fma2c_states: per key (signals in all_ts_ids order, then managers) the gather (index, scale) lists, and the
    lane / fringe / same-region maps the reward tables are built from.  Shared with agents/fma2c.py: FMA2CLayout."""
    sup, alpha = cfg['supervisors'], float(cfg['alpha'])
    ids = list(sc.signal_ids)
    O = sc.n_obs
    lane_pos = {l: i for i, l in enumerate(sc.obs_lane_ids)}
    lanes = {sid: list(sc.obs_lane_ids[int(sc.sig_obs_start[i]):int(sc.sig_obs_start[i + 1])]) for i, sid in enumerate(ids)}
    meta = sc.signal_meta
    fringes = {mgr: [] for mgr in cfg['management']}           # states._fma2c_regions
    for sid in ids:
        for direction, nb in meta[sid]['downstream'].items():
            if nb is None or sup[nb] != sup[sid]:
                inbound = meta[sid]['inbounds_fr_direction'].get(direction)
                if inbound is not None:
                    fringes[sup[sid]] += inbound
    same_region = {sid: [nb for nb in meta[sid]['downstream'].values() if nb is not None and sup[nb] == sup[sid]] for sid in ids}
    keys = list(ids) + list(cfg['management'].keys())
    # states: feature vector F = [clip(wave / norm_wave), clip(max_wait / norm_wait)] per observed lane
    s_idx, s_scale = {}, {}
    mgr_terms = {mgr: ([lane_pos[l] for l in fl], [1.0] * len(fl)) for mgr, fl in fringes.items()}
    # feature blocks of F: wave (0), [full: total_wait / 28 (1), speed term (2)], max_wait (last)
    nb_blocks = 3 if full else 1

    def own_idx(sid_):      # fma2c_full interleaves wave, total_wait / 28 and the drq_norm speed term per lane (states.py:232-305)
        out_ = []
        for l in lanes[sid_]:
            out_ += [b * O + lane_pos[l] for b in range(nb_blocks)]
        return out_
    for sid in ids:
        idx = own_idx(sid)
        sc_ = [1.0] * len(idx)
        for nb in same_region[sid]:
            ni = own_idx(nb)
            idx += ni
            sc_ += [alpha] * len(ni)
        idx += [nb_blocks * O + lane_pos[l] for l in lanes[sid]]
        sc_ += [1.0] * len(lanes[sid])
        s_idx[sid], s_scale[sid] = idx, sc_
    for mgr in cfg['management']:
        idx, sc_ = list(mgr_terms[mgr][0]), list(mgr_terms[mgr][1])
        for n in cfg['management_neighbors'][mgr]:
            idx += mgr_terms[n][0]
            sc_ += [alpha] * len(mgr_terms[n][0])
        s_idx[mgr], s_scale[mgr] = idx, sc_
    return keys, s_idx, s_scale, lanes, lane_pos, fringes, same_region


def fma2c_reward_matrix(sc, cfg, full=False):
    """The matrix W float32 [3 O + 2 S, S + M] of rewards.fma2c / fma2c_full (reference rewards.py:72-136): every reward is the linear
    form G @ W of G = [queue (O), max_wait (O), lane arrivals (O), signal arrivals (S), signal departures (S)] per environment.
    Columns in the key order of fma2c_state_tables: signals in all_ts_ids order, then managers.  cfg: the ACTIVE mdp_configs['FMA2C' |
    'FMA2CFull'] of the map.  No GPU is needed."""
    sup, alpha = cfg['supervisors'], float(cfg['alpha'])
    ids = list(sc.signal_ids)
    O, S = sc.n_obs, len(ids)
    keys, _, _, lanes, lane_pos, fringes, same_region = fma2c_state_tables(sc, cfg, full)
    W = np.zeros((3 * O + 2 * S, len(keys)), np.float32)
    own = np.zeros((3 * O + 2 * S, S), np.float32)
    for i, sid in enumerate(ids):
        for l in lanes[sid]:
            own[lane_pos[l], i] -= 1.0
            own[O + lane_pos[l], i] -= float(cfg['coef'])
    pos = {sid: i for i, sid in enumerate(ids)}
    for i, sid in enumerate(ids):
        W[:, i] = own[:, i]
        for nb in same_region[sid]:
            W[:, i] += alpha * own[:, pos[nb]]
    mg = {mgr: np.zeros(3 * O + 2 * S, np.float32) for mgr in cfg['management']}
    for i, sid in enumerate(ids):
        m = mg[sup[sid]]
        m[3 * O + S + i] += 1.0         # departures
        m[3 * O + i] -= 1.0             # arrivals
        for l in lanes[sid]:
            if l in fringes[sup[sid]]:
                m[2 * O + lane_pos[l]] += 1.0
    for j, mgr in enumerate(cfg['management']):
        W[:, S + j] = mg[mgr]
        for n in cfg['management_neighbors'][mgr]:
            W[:, S + j] += alpha * mg[n]
    return W


def fma2c_reward_csr(W, columns=None):
    """The non-zeros of W [R, K] column by column, rows ascending, as the three arrays of rs_fma2c_reward_table (include/resco_sim.h):
    off int32 [K + 1], idx int32 [nnz], w float32 [nnz].  columns: the order the columns are stored in (default: W's own)."""
    W = np.asarray(W, np.float32)
    cols = range(W.shape[1]) if columns is None else columns
    off, idx, w = [0], [], []
    for j in cols:
        nz = np.flatnonzero(W[:, j])
        idx.append(nz.astype(np.int32))
        w.append(W[nz, j])
        off.append(off[-1] + len(nz))
    return np.asarray(off, np.int32), np.concatenate(idx).astype(np.int32), np.concatenate(w).astype(np.float32)


def fma2c_reward_table(sc, cfg, full=False):
    """(off, idx, w, n_rows) of the reward matrix with its columns in the order of the learner's agents -- FMA2CLayout.agents:
    managers in `management` order, then the signals -- which is what rs_fma2c_record and rs_group_fma2c_train read"""
    W = fma2c_reward_matrix(sc, cfg, full)
    S, M = len(sc.signal_ids), len(cfg['management'])
    return fma2c_reward_csr(W, list(range(S, S + M)) + list(range(S))) + (W.shape[0],)


class VecMultiSignal:
    """N lock-step environments on one GPU; observations / rewards are zero-copy torch tensors over the
    library-owned device buffers (the agent boundary), actions are an int32 [N, S] tensor or None (actions
    already written on device by act_random / act_maxwave).

    **tls_expiry** -- what `trafficlight.setPhase` (Signal.prep_phase / set_phase, traffic_signal.py:176-187) leaves behind is a
    parameter of this simulator (rs_params.tls_hold, inverted).  `tls_expiry=True` (default) is SUMO's documented setPhase: the phase
    runs for its programme duration and the programme then continues with the next phase of the list (the switch is re-scheduled
    `duration` seconds ahead, MSSimpleTrafficLightLogic::changeStepAndDuration), so a 6 s green chosen for a 10 s step hands its 7th
    second to the next index.  `tls_expiry=False` keeps the selected phase until the next action: round 5's default, a calibration
    of this build's own traffic model that reproduces the reference-held random-policy figures better (36 of 42 result cells inside
    +-35 % against 29, profiles/r06_reference_bands_both_modes.txt) while trained agents reach the same delays either way
    (profiles/r06_heldout_both_modes.txt).  Neither is pinned against a SUMO binary (`tools/sumo_runner.py diff` decides it on a box
    that has SUMO); results, bench figures and the held-out IDQN check are reported for BOTH values (README).
    """

    def __init__(self, map_name, n_envs, states=('drq_norm',), rewards=('wait',), net=None, device=0, seed=0,
                 max_distance=200, step_length=10, yellow_length=3, sigma=-1.0, speed_dev=1, fixed_program=False,
                 env_base=0, block_threads=0, scenario=None, outputs=None, step_ratio=1, tls_expiry=True, demand=None):
        mc = map_configs.get(map_name, {})
        self.scenario = scenario if scenario is not None else load_scenario(map_name, net, mc.get('lights', ()),
                                                                            yellow_length)
        self.sim = BatchedSim(self.scenario, n_envs, device=device, seed=seed, max_distance=max_distance,
                              sigma=sigma, speed_dev=speed_dev, fixed_program=1 if fixed_program else 0,
                              env_base=env_base, step_length=step_length, yellow_length=yellow_length,
                              block_threads=block_threads, step_ratio=step_ratio, tls_expiry=1 if tls_expiry else 0)
        self.n_envs, self.n_signals = n_envs, self.scenario.n_signals
        self.state_names, self.reward_names = tuple(states), tuple(rewards)
        self.step_length = step_length
        self.horizon_steps = self.scenario.horizon // (step_length * max(1, int(step_ratio)))
        self.steps = 0
        self.all_ts_ids = list(self.scenario.signal_ids)
        self.n_actions = [int(g) for g in self.scenario.tls_ngreen]
        self._tensors = {}
        if outputs is not None:         # only these per-lane / per-movement buffers are written (BatchedSim.set_outputs)
            self.sim.set_outputs(outputs)
        if demand:                      # demand variants, one per environment ((env_base + e) % K): in force from the first reset()
            self.set_demand(demand)
            self.sim.reset()

    def set_demand(self, scenarios, env_variant=None):
        """Every environment runs the trips of its own demand variant from the next reset() on (BatchedSim.set_demand; resco_amd/demand.py
        builds variants); an empty list or None returns to the scenario's own trips."""
        if scenarios:
            self.sim.set_demand(scenarios, env_variant)
        else:
            self.sim.clear_demand()

    # registry names that are not a device buffer of their own but a cheap arrangement of buffers (torch ops on the stream)
    DERIVED = ('drq', 'fma2c', 'fma2c_full')

    def tensor(self, name):
        self.sim.require_output(name)           # a buffer switched off with set_outputs holds stale rows: refuse, loudly
        t = self._tensors.get(name)
        if t is None:
            t = self._tensors[name] = self.sim.tensor(name)
        return t

    def derived(self, name):
        """states.drq (reference states.py:9-28) for all environments: [N, n_obs, 5] rows (lane position == phase, approach,
        total_wait, queue, speed sum) from the lane aggregates (queue, approach, total_wait, max_wait, speed_sum) and the
        one-hot column the kernel writes into drq_norm"""
        import torch
        if name == 'drq':
            agg, onehot = self.tensor('lane_agg'), self.tensor('drq_norm')[..., 0]
            return torch.stack((onehot, agg[..., 1], agg[..., 2], agg[..., 0], agg[..., 4]), dim=-1)
        raise KeyError(name)

    # ---- FMA2C (states.py:162-229, rewards.py:72-136) for all environments: every worker / manager observation is a gather
    # of normalised per-lane waves and waits, every reward a linear form of per-lane queues, waits, arrivals and the
    # per-signal arrival / departure counters -- index tables built once from mdp_configs['FMA2C'] (activate() it first)
    def _fma2c_tables(self, full=False):
        import torch
        cache = getattr(self, '_fma2c', None)
        if cache is None:
            cache = self._fma2c = {}
        if full in cache:
            return cache[full]
        from .config.mdp_config import mdp_configs
        cfg, sc = mdp_configs['FMA2CFull' if full else 'FMA2C'], self.scenario
        keys, s_idx, s_scale = fma2c_state_tables(sc, cfg, full)[:3]
        dev = self.tensor('lane_agg').device
        st = {k: (torch.as_tensor(s_idx[k], dtype=torch.long, device=dev), torch.as_tensor(s_scale[k], dtype=torch.float32, device=dev))
              for k in keys}
        # rewards: G = [queue (O), max_wait (O), lane arrivals (O), signal arrivals (S), signal departures (S)] @ W
        W = fma2c_reward_matrix(sc, cfg, full)
        cache[full] = dict(cfg=cfg, keys=keys, states=st, W=torch.as_tensor(W, device=dev), full=full)
        return cache[full]

    def fma2c_states(self, full=False):
        """dict key -> f32 [N, dim] for every signal and manager (states.fma2c / states.fma2c_full)"""
        import torch
        t = self._fma2c_tables(full)
        cfg, agg = t['cfg'], self.tensor('lane_agg')
        nw, cw = cfg['norm_wave'], cfg['clip_wave']
        blocks = [torch.clamp((agg[..., 0] + agg[..., 1]) / nw, 0, cw)]
        if full:
            blocks += [torch.clamp(agg[..., 2] / 28 / nw, 0, cw), torch.clamp(agg[..., 4] / 20 / 28 / nw, 0, cw)]
        blocks.append(torch.clamp(agg[..., 3] / cfg['norm_wait'], 0, cfg['clip_wait']))
        F = torch.cat(blocks, dim=1)
        # (the managers' observations use the wave block only, in both variants)
        return {k: F[:, idx] * scale for k, (idx, scale) in t['states'].items()}

    def fma2c_rewards(self, full=False):
        """dict key -> f32 [N] for every signal and manager (rewards.fma2c / rewards.fma2c_full)"""
        import torch
        t = self._fma2c_tables(full)
        agg = self.tensor('lane_agg')
        G = torch.cat((agg[..., 0], agg[..., 3], self.tensor('lane_arrivals').float(), self.tensor('arrivals').float(),
                       self.tensor('departures').float()), dim=1)
        R = G @ t['W']
        return {k: R[:, j] for j, k in enumerate(t['keys'])}

    def fma2c_rewards_device(self, full=False, out=None, policy=None):
        """The rewards of fma2c_rewards for all K agents as ONE f32 tensor [N, K] in the order of the learner's agents (managers
        first), by one HIP kernel on the library's buffers (rs_fma2c_record: neither actions nor a return are recorded) instead of
        the casts, the cat and the dense product.  The summation order is the kernel's (a column's non-zeros, rows ascending), so the
        values differ from fma2c_rewards' in the last bits.  policy: the FusedFMA2C of these environments -- the entry point takes
        its agent counts from it; needed on the first call, remembered afterwards.  out: an f32 [N, K] device tensor to write."""
        import torch
        from .sim import Fma2cRewardTable, torch_stream
        if policy is not None:
            self._fma2c_policy = policy
        policy = getattr(self, '_fma2c_policy', None)
        if policy is None:
            raise ValueError('fma2c_rewards_device needs the FusedFMA2C policy of these environments on its first call (policy=...)')
        t = self._fma2c_tables(full)
        if 'table' not in t:
            t['table'] = Fma2cRewardTable(self.scenario, t['cfg'], full, self.sim.device)
        K = t['table'].K
        if out is None:
            out = torch.empty(self.n_envs, K, dtype=torch.float32, device=self.tensor('lane_agg').device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (self.n_envs, K)
        self.sim.fma2c_record(policy.handle, t['table'], out, stream=torch_stream(self.sim.device))
        return out

    def _pack(self):
        obs = {}
        for n in self.state_names:
            obs[n] = self.fma2c_states(n == 'fma2c_full') if n in ('fma2c', 'fma2c_full') else (
                self.derived(n) if n in self.DERIVED else self.tensor(n))
        rew = {n: (self.fma2c_rewards(n == 'fma2c_full') if n in ('fma2c', 'fma2c_full') else self.tensor(n))
               for n in self.reward_names}
        return obs, rew

    def _stream(self, stream):
        # the tensors handed out are consumed by torch kernels: launch on torch's current stream unless told otherwise
        return torch_stream(self.sim.device) if stream is None else stream

    def reset(self, stream=None):
        self.sim.reset(self._stream(stream))
        self.steps = 0
        return self._pack()[0]

    def act_random(self, step_key, stream=None):
        self.sim.act_random(step_key, self._stream(stream))

    def act_maxwave(self, use_pressure, stream=None):
        self.sim.act_maxwave(use_pressure, self._stream(stream))

    def step(self, actions=None, stream=None):
        self.sim.step(actions, self._stream(stream))
        self.steps += 1
        obs, rew = self._pack()
        return obs, rew, self.steps >= self.horizon_steps, {'steps': self.steps}

    def advance(self, n_steps):
        """n_steps env-steps were taken on the simulator behind this wrapper's back (SimGroup.step / SimGroup.rollout on self.sim):
        keep the episode's step counter -- and with it `done` -- right.  Returns done."""
        self.steps += int(n_steps)
        return self.steps >= self.horizon_steps

    def sync(self):
        self.sim.sync()

    def close(self):
        self.sim.close()
