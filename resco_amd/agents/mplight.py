"""MPLight on the device: the shared FRAP network, its fused HIP forward (rs_mplight_*), a batched shared-DQN learner and the
reference's agent interface.

The reference (resco_benchmark/agents/mplight.py:13-130, agents/pfrl_dqn.py:49-188, agents/agent.py:39-79,
config/agent_config.py:101-113, 141-153) trains ONE FRAP network shared by every signal of the map with PFRL's DQN as
``DQNAgent(num_agents=S)`` configures it:

    Adam() (lr 1e-3) - ReplayBuffer(10000) - minibatch 32, replay_start_size 32 - gamma 0.99 - Huber loss (delta 1) on
    Q(s)[g] against r + gamma (1 - done) max_{all P} Q_target(s') - update_interval S and target_update_interval 500 S agent
    steps (= one update per env-step, a hard target copy every 500 env-steps) - SharedEpsGreedy decaying linearly from 1 to 0
    over S * steps agent steps (= `steps` env-steps); the reward is rewards.pressure.

Acting (SharedDQN.batch_act): on maps with valid_acts the greedy pair is the first maximum of Q over the signal's valid_acts
keys in dict order (strict >) and the simulator receives valid_acts[s][g], a LOCAL index; without valid_acts a plain argmax over
all P.  With probability epsilon the k-th valid entry, k uniform.  The replay stores the GLOBAL pair index g.  On every shipped
map a signal's local actions in dict order are 0 .. n-1, so "the k-th entry" is the reference's reverse_valid[k]
(rs_mplight_create refuses tables where that is not so; ``mplight_tables`` refuses a valid_acts map that lacks a signal -- the
reference would crash there).

Batching over N lock-step environments (what differs by design).  The reference steps ONE environment: S transitions per
env-step enter a ring of 10 000 transitions (10 000 / S env-steps) and one minibatch of 32 is drawn per env-step.  Here the S x N
transitions of an env-step enter ONE device ring (MPLightReplay: the last ``capacity_steps`` env-steps of all N environments, no
host copy), and ONE update per env-step draws ``batch_size`` transitions uniformly over (slot, environment, signal) -- a single
shared network, so the signals are pooled exactly as the reference pools them.  The target copy every 500 env-steps and the
epsilon schedule over env-steps are the reference's.  PFRL is not installed here, so the update is a restatement of the
published DQN update, checked against an unbatched plain-PyTorch restatement (tests/test_mplight_cpu.py).

PFRL's own exploration draws np.random; the fused kernel draws the model's counter hash over (seed; global environment,
signal, step key) instead, so that pipes and GPUs draw what the single batch draws.
"""
import copy
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..sim import load_library, maxwave_tables, torch_stream
from . import _state
from .idqn_learn import linear_epsilon, nstep_walk, target_options_signature

N_MOVEMENTS = 12
Q_WIDTH = 16            # the q output of rs_mplight_act: [N][S][16], -inf beyond P


class FRAP(nn.Module):
    """FRAP (mplight.py:48-130), vectorised: every (environment, signal) row, phase pair and ordered pair of pairs in one tensor
    op each, no Python loop over rows.  Parameter names are the reference's, so the model_state_dict of an agent.pt the
    reference's MPLight saved loads unchanged.  Input: [B, 1 + 12 D] rows (obs[0] = the signal's current LOCAL green index,
    used as a global pair index as the reference does; clamped to [0, P) where the reference would raise)."""

    def __init__(self, n_pairs, phase_pairs, demand_shape=1):
        super().__init__()
        pairs = [list(map(int, p)) for p in phase_pairs]
        assert len(pairs) == int(n_pairs) and 2 <= len(pairs) <= Q_WIDTH
        self.oshape, self.demand_shape, self.phase_pairs = len(pairs), int(demand_shape), pairs
        # the reference's construction order (mplight.py:60-72): init_like_reference relies on it
        self.p = nn.Embedding(2, 4)
        self.d = nn.Linear(self.demand_shape, 4)
        self.lane_embedding = nn.Linear(8, 16)
        self.lane_conv = nn.Conv2d(32, 20, kernel_size=(1, 1))
        self.relation_embedding = nn.Embedding(2, 4)
        self.relation_conv = nn.Conv2d(4, 20, kernel_size=(1, 1))
        self.hidden_layer = nn.Conv2d(20, 20, kernel_size=(1, 1))
        self.before_merge = nn.Conv2d(20, 1, kernel_size=(1, 1))
        P = self.oshape
        ii, jj = zip(*[(i, j) for i in range(P) for j in range(P) if i != j])       # the reference's rotated order, i-major
        comp = [int(len(set(pairs[i] + pairs[j])) == 3) for i, j in zip(ii, jj)]
        self.register_buffer('_pairs', torch.tensor(pairs, dtype=torch.long), persistent=False)
        self.register_buffer('_ii', torch.tensor(ii, dtype=torch.long), persistent=False)
        self.register_buffer('_jj', torch.tensor(jj, dtype=torch.long), persistent=False)
        self.register_buffer('_comp', torch.tensor(comp, dtype=torch.long), persistent=False)
        win = torch.arange(N_MOVEMENTS)[:, None] + torch.arange(self.demand_shape)[None, :]    # states[:, i:i+D]: overlapping windows
        self.register_buffer('_win', win, persistent=False)

    def init_like_reference(self, seed):
        """The weights the reference's FRAP(...) constructor draws after torch.manual_seed(seed) (PyTorch's default init, same
        module order, CPU generator)."""
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(seed))
            fresh = FRAP(self.oshape, self.phase_pairs, self.demand_shape)
        self.load_state_dict(fresh.state_dict())
        return self

    def forward(self, states):
        states = states.reshape(-1, states.shape[-1])
        P, D = self.oshape, self.demand_shape
        acts = states[:, 0].to(torch.int64).clamp(0, P - 1)
        x = states[:, 1:].float()
        pp = self._pairs[acts]                                                  # [B, 2]
        mv = torch.arange(N_MOVEMENTS, device=states.device)
        bits = ((mv[None, :] == pp[:, :1]) | (mv[None, :] == pp[:, 1:])).long()  # [B, 12]
        phase = torch.sigmoid(self.p(bits))                                     # [B, 12, 4]
        demand = torch.sigmoid(self.d(x[:, self._win]))                         # [B, 12, 4]
        e = F.relu(self.lane_embedding(torch.cat((phase, demand), -1)))         # [B, 12, 16]
        pair = e[:, self._pairs[:, 0]] + e[:, self._pairs[:, 1]]                # [B, P, 16]
        rot = torch.cat((pair[:, self._ii], pair[:, self._jj]), -1)             # [B, P(P-1), 32]
        lc = F.relu(F.linear(rot, self.lane_conv.weight.reshape(20, 32), self.lane_conv.bias))
        rel = F.relu(self.relation_embedding(self._comp))                       # [P(P-1), 4]
        rel = F.relu(F.linear(rel, self.relation_conv.weight.reshape(20, 4), self.relation_conv.bias))
        h = F.relu(F.linear(lc * rel, self.hidden_layer.weight.reshape(20, 20), self.hidden_layer.bias))
        y = F.linear(h, self.before_merge.weight.reshape(1, 20), self.before_merge.bias)
        return y.reshape(-1, P, P - 1).sum(-1)                                  # [B, P]


def frap_from_scenario(sc, demand_shape=1):
    return FRAP(len(sc.phase_pairs), sc.phase_pairs, demand_shape)


def pack_mplight_weights(net):
    """The packed f32 weight vector of rs_mplight_create (include/resco_sim.h): FRAP's parameters in state_dict order, each
    row-major.  Same device / dtype as the network, float32."""
    return torch.cat([t.detach().reshape(-1).float() for t in net.state_dict().values()])


def unpack_mplight_weights(flat, net):
    """Inverse of pack_mplight_weights: load a packed vector into `net`."""
    sd, off = {}, 0
    for k, t in net.state_dict().items():
        n = t.numel()
        sd[k] = torch.as_tensor(flat[off:off + n]).reshape(t.shape).to(t.dtype)
        off += n
    assert off == len(flat), (off, len(flat))
    net.load_state_dict(sd)
    return net


def mplight_tables(sc):
    """pairs [P][2], valid [S][P], order [S][P] (sim.maxwave_tables) for rs_mplight_create.  A valid_acts map that lacks one
    of the scenario's signals is refused: the reference's batch_act would crash on it (valid_acts[i] is None)."""
    if sc.valid_acts is not None:
        missing = [sid for sid in sc.signal_ids if sid not in sc.valid_acts]
        if missing:
            raise ValueError('valid_acts has no entry for signal(s) %s: the reference cannot act there' % ', '.join(map(str, missing)))
    return maxwave_tables(sc)


class FusedMPLight:
    """The fused HIP forward (rs_mplight_act): epsilon-greedy actions of all N x S rows in one launch on the simulator's
    mplight (demand_shape 1, int32 [N, S, 13]) or mplight_full (4, f32 [N, S, 49]) buffer."""

    def __init__(self, net, scenario, seed=0, device=0):
        self.net, self.sc, self.device, self.seed = net, scenario, int(device), int(seed) & 0xFFFFFFFF
        self.S, self.P, self.D = scenario.n_signals, net.oshape, net.demand_shape
        self.width = 1 + N_MOVEMENTS * self.D
        if [list(map(int, p)) for p in scenario.phase_pairs] != net.phase_pairs:
            raise ValueError('the network was built for other phase pairs than the scenario has')
        self.pairs, self.valid, self.order = mplight_tables(scenario)
        self._lib = load_library()
        self._h = None
        self._actions = {}
        self._wdev = None
        self.refresh()

    @property
    def handle(self):
        """the rs_policy_handle (SimGroup.step('mplight', policy=...))"""
        return self._h.value if self._h is not None else None

    def refresh(self):
        """(Re)create the policy with the network's current weights (host copy)."""
        w = np.ascontiguousarray(pack_mplight_weights(self.net).cpu().numpy(), np.float32)
        h = C.c_void_p()
        rc = self._lib.rs_mplight_create(self.device, self.D, self.P, self.pairs.ctypes.data, self.S, self.valid.ctypes.data,
                                         self.order.ctypes.data, w.ctypes.data, C.byref(h))
        if rc != 0:
            msg = self._lib.rs_last_error(None)
            raise RuntimeError('rs_mplight_create failed (%d): %s' % (rc, msg.decode() if msg else '?'))
        self.close()
        self._h = h
        self._wdev = None

    @torch.no_grad()
    def refresh_on_device(self):
        """Re-pack the network's current weights on the GPU into a persistent buffer and point the kernel at it (no host copy):
        what a learner calls after every update."""
        flat = pack_mplight_weights(self.net)
        if self._wdev is None or self._wdev.numel() != flat.numel() or self._wdev.device != flat.device:
            self._wdev = torch.empty_like(flat)
        self._wdev.copy_(flat)
        rc = self._lib.rs_mplight_set_device_weights(self._h, self._wdev.data_ptr())
        if rc != 0:
            raise RuntimeError('rs_mplight_set_device_weights failed (%d)' % rc)

    def share_weights(self, flat):
        """Point the kernel at a caller-owned packed float32 device vector (pack_mplight_weights' layout; e.g. the parameter vector
        of mplight_learn_fused.FusedMPLightLearner) and keep a reference to it: whoever updates that vector in stream order updates
        the policy, with no re-pack.  refresh() ends the sharing (a new policy over a host copy); refresh_on_device() does not: it
        packs the network into this same vector -- a copy onto itself where the network's parameters are views of it -- and points
        the kernel at it again."""
        n = sum(p.numel() for p in self.net.parameters())
        if not (flat.is_cuda and flat.dtype == torch.float32 and flat.is_contiguous() and flat.dim() == 1 and flat.numel() == n):
            raise ValueError('share_weights needs a contiguous float32 device vector of %d elements' % n)
        rc = self._lib.rs_mplight_set_device_weights(self._h, flat.data_ptr())
        if rc != 0:
            raise RuntimeError('rs_mplight_set_device_weights failed (%d)' % rc)
        self._wdev = flat

    # ---- checkpoints (resco_amd/checkpoint.py)
    def state_dict(self):
        return {'state': {'seed': int(self.seed)}}

    def load_state_dict(self, sd, weights_only=False):
        """list the network (and a fused learner) before the policy.  A policy that shares a learner's vector keeps sharing it --
        the load wrote into that vector --; one on a create-time or re-packed copy re-packs the network on the device."""
        if not weights_only:
            self.seed = int(sd['state']['seed']) & 0xFFFFFFFF
        self.refresh_on_device()

    def close(self):
        if getattr(self, '_h', None) is not None:
            self._lib.rs_mplight_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def act(self, obs, epsilon=0.0, step_key=0, out=None, pair_out=None, want_q=False, env_base=0, dyn=None, stream=None):
        """obs: CUDA tensor [N, S, 13] int32 (demand_shape 1) or [N, S, 49] float32 (4).  Returns the int32 local actions [N, S]
        (`out`, e.g. the simulator's RS_BUF_ACTIONS tensor), and -- with `pair_out` given -- writes the global pair indices there;
        with want_q returns (actions, q [N, S, 16], -inf beyond P).  dyn: optional CUDA tensor {epsilon as float32 bits, step key}
        read by the kernel instead of the scalars (graph replay).  env_base: global index of obs[0]'s environment."""
        want = torch.int32 if self.D == 1 else torch.float32
        assert obs.is_cuda and obs.dtype == want and obs.is_contiguous(), (obs.dtype, want)
        N = obs.shape[0]
        assert tuple(obs.shape[1:]) == (self.S, self.width), obs.shape
        if out is not None:
            assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (N, self.S)
            actions = out
        else:
            if N not in self._actions:
                self._actions[N] = torch.empty(N, self.S, dtype=torch.int32, device=obs.device)
            actions = self._actions[N]
        if pair_out is not None:
            assert pair_out.is_cuda and pair_out.dtype == torch.int32 and pair_out.is_contiguous() and tuple(pair_out.shape) == (N, self.S)
        q = torch.empty(N, self.S, Q_WIDTH, dtype=torch.float32, device=obs.device) if want_q else None
        st = torch_stream(self.device) if stream is None else stream
        rc = self._lib.rs_mplight_act(self._h, obs.data_ptr(), N, int(env_base), float(epsilon), self.seed, int(step_key) & 0xFFFFFFFF,
                                      dyn.data_ptr() if dyn is not None else None, actions.data_ptr(),
                                      pair_out.data_ptr() if pair_out is not None else None, q.data_ptr() if want_q else None, st)
        if rc != 0:
            raise RuntimeError('rs_mplight_act failed (%d)' % rc)
        return (actions, q) if want_q else actions


class MPLightReplay:
    """Device ring over the last ``capacity_steps`` env-steps of all N environments: the observation rows the agents acted on
    ([T, N, S, 1 + 12 D] float32; the int32 mplight rows are exact in it), the global pair index taken, the pressure reward and
    the episode-end flag.  The successor of slot t is slot t + 1 (done cuts the bootstrap, as in idqn_learn.DeviceReplay)."""

    def __init__(self, capacity_steps, n_envs, n_signals, width, device='cuda'):
        T, N, S = int(capacity_steps), int(n_envs), int(n_signals)
        assert T >= 2
        self.T, self.N, self.S = T, N, S
        self.obs = torch.zeros(T, N, S, width, dtype=torch.float32, device=device)
        self.act = torch.zeros(T, N, S, dtype=torch.int16, device=device)
        self.rew = torch.zeros(T, N, S, dtype=torch.float32, device=device)
        self.done = torch.zeros(T, dtype=torch.bool, device=device)
        self.head = 0
        self.count = 0

    def __len__(self):
        """transitions that can be sampled (all signals of all environments pooled)"""
        return max(0, self.count - 1) * self.N * self.S

    def stage(self, obs):
        self.obs[self.head].copy_(obs)

    def commit(self, pair_index, rew, done):
        i = self.head
        self.act[i].copy_(pair_index)
        self.rew[i].copy_(rew)
        self.done[i] = bool(done)
        self.head = (i + 1) % self.T
        self.count = min(self.count + 1, self.T)

    def push(self, obs, pair_index, rew, done):
        self.stage(obs)
        self.commit(pair_index, rew, done)

    def signature(self):
        return dict(_state.ring_signature(self), width=int(self.obs.shape[-1]))

    def state_dict(self, replay=True):
        return _state.ring_state(self, replay)

    def load_state_dict(self, sd, weights_only=False):
        if not weights_only:
            _state.load_ring_state(self, sd, 'MPLightReplay')

    def sample(self, batch_size, generator=None, n_step=1, gamma=None):
        """B transitions uniform over (slot with a successor, environment, signal): o [B, W], g [B] long, r [B], o2 [B, W], d [B].
        n_step > 1 (needs gamma): the same rows from the same draws, with r the discounted sum of the walk's rewards, o2 the
        observation the walk ends at, d the cut flag, and a sixth element disc = gamma^m (idqn_learn.nstep_walk)."""
        n_ok = self.count - 1
        assert n_ok >= 1, 'need two pushes before sampling'
        dev, B = self.obs.device, int(batch_size)
        k = torch.randint(0, n_ok, (B,), device=dev, generator=generator)
        t = (self.head - self.count + k) % self.T
        e = torch.randint(0, self.N, (B,), device=dev, generator=generator)
        s = torch.randint(0, self.S, (B,), device=dev, generator=generator)
        if int(n_step) == 1:
            t2 = (t + 1) % self.T
            return self.obs[t, e, s], self.act[t, e, s].long(), self.rew[t, e, s], self.obs[t2, e, s], self.done[t].to(torch.float32)
        assert 1 < int(n_step) <= 32 and gamma is not None, 'n-step rows need 1 <= n_step <= 32 and gamma'
        R, u_m, cut, disc = nstep_walk(self, t, e, self.head, n_step, gamma, s)
        return self.obs[t, e, s], self.act[t, e, s].long(), R, self.obs[u_m, e, s], cut.to(torch.float32), disc


class MPLightLearner:
    """PFRL's DQN update on the shared FRAP network (see the module docstring for the batching)."""

    def __init__(self, net, gamma=0.99, lr=1e-3, target_update=500, batch_size=32, n_step=1, double_q=False, per=None):
        """n_step (1 .. 32): n-step returns (idqn_learn.nstep_walk); double_q: Double DQN's bootstrap.  The defaults are PFRL's plain DQN.
        per: refused -- prioritised replay exists in the fused learner only."""
        if per is not None:
            raise ValueError('MPLightLearner: prioritised replay is implemented in the device update only '
                             '(FusedMPLightLearner(per=...), tools/mplight_train.py --device-update or --device-loop)')
        self.n_step, self.double_q = int(n_step), bool(double_q)
        if not 1 <= self.n_step <= 32:
            raise ValueError('MPLightLearner: n_step must be in 1 .. 32, got %d' % self.n_step)
        self.q = net
        self.target = copy.deepcopy(net)
        for p in self.target.parameters():
            p.requires_grad_(False)
        self.gamma, self.batch_size, self.target_update = float(gamma), int(batch_size), int(target_update)
        self.opt = torch.optim.Adam(self.q.parameters(), lr=lr)
        self.t = 0              # env-steps seen
        self.n_updates = 0

    def loss(self, o, g, r, o2, d, disc=None):
        """disc: the discount of the bootstrap per row (gamma^m of an n-step row); None: gamma"""
        y = self.q(o).gather(-1, g.unsqueeze(-1)).squeeze(-1)
        with torch.no_grad():
            if self.double_q:                                                   # the online network's best of ALL P outputs (the first of
                best = self.q(o2).argmax(dim=-1, keepdim=True)                  # equal maxima), valued by the target network
                nxt = self.target(o2).gather(-1, best).squeeze(-1)
            else:
                nxt = self.target(o2).max(dim=-1).values                        # over ALL P outputs: not masked by valid_acts
            tgt = r + (self.gamma if disc is None else disc) * (1.0 - d) * nxt
        return F.smooth_l1_loss(y, tgt, reduction='mean')                      # Huber, delta 1, mean over the minibatch

    def update(self, batch):
        self.opt.zero_grad(set_to_none=True)
        loss = self.loss(*batch)
        loss.backward()
        self.opt.step()
        self.n_updates += 1
        return loss.detach()

    def sync_target(self):
        self.target.load_state_dict(self.q.state_dict())

    # ---- checkpoints (resco_amd/checkpoint.py): loaded in place
    def signature(self):
        return target_options_signature({'batch': self.batch_size, 'target_update': self.target_update, 'gamma': self.gamma}, self.n_step, self.double_q)

    def state_dict(self):
        return {'weights': {'target': _state.module_tensors(self.target)},
                'state': {'opt': _state.adam_state(self.opt), 't': int(self.t), 'n_updates': int(self.n_updates)}}

    def load_state_dict(self, sd, weights_only=False):
        _state.load_module(self.target, sd['weights']['target'], 'MPLightLearner.target')
        if not weights_only:
            _state.load_adam_state(self.opt, sd['state']['opt'], 'MPLightLearner.opt')
            self.t, self.n_updates = int(sd['state']['t']), int(sd['state']['n_updates'])

    def observe_step(self, replay, generator=None):
        """One env-step of SharedDQN.batch_observe: the target copy every `target_update` env-steps (before the update, as PFRL
        orders them), then one update once the ring holds a minibatch."""
        self.t += 1
        if self.t % self.target_update == 0:
            self.sync_target()
        if len(replay) >= self.batch_size:
            return self.update(replay.sample(self.batch_size, generator, self.n_step, self.gamma))
        return None


class MPLight:
    """The reference's agent interface (agents/mplight.py:13-45 + agents/agent.py:57-79): act(observation dict) -> dict of local
    actions, observe(observation, reward, done, info), for a MultiSignal loop written for the reference.  Acting runs the fused
    kernel on the signals' rows (one environment), learning the shared-DQN learner above; config: agent_configs['MPLight'] or
    ['MPLightFULL'] plus the keys main.py adds ('steps', and optionally 'load' / 'log_dir' / 'save_freq')."""

    def __init__(self, config, obs_act, map_name, thread_number, scenario=None, device=0, seed=0):
        from ..multi_signal import load_scenario
        from ..config.map_config import map_configs
        self.config = config
        self.sc = scenario if scenario is not None else load_scenario(map_name, None, map_configs.get(map_name, {}).get('lights', ()), 3)
        self.ids = list(self.sc.signal_ids)
        D = int(config['demand_shape'])
        self.net = frap_from_scenario(self.sc, D).to('cuda:%d' % device)
        self.net.init_like_reference(seed)
        if config.get('load'):
            self.net.load_state_dict(torch.load(os.path.join(config['log_dir'], 'agent.pt'), map_location='cpu')['model_state_dict'])
        self.policy = FusedMPLight(self.net, self.sc, seed=seed, device=device)
        self.learner = MPLightLearner(self.net, gamma=config['GAMMA'], target_update=config['TARGET_UPDATE'],
                                      batch_size=config['BATCH_SIZE'])
        self.replay = MPLightReplay(max(2, 10000 // len(self.ids)), 1, len(self.ids), 1 + N_MOVEMENTS * D, device='cuda:%d' % device)
        self.training = not config.get('load')
        self.steps = int(config.get('steps', 1))
        self._dt = torch.int32 if D == 1 else torch.float32
        self._pair = torch.zeros(1, len(self.ids), dtype=torch.int32, device='cuda:%d' % device)
        self._staged = False

    def _rows(self, observation):
        rows = np.stack([np.asarray(observation[sid], np.float64) for sid in self.ids])
        return torch.as_tensor(rows[None], dtype=self._dt).cuda(self.policy.device).contiguous()

    def act(self, observation):
        obs = self._rows(observation)
        eps = linear_epsilon(self.learner.t, 1.0, 0.0, self.steps) if self.training else 0.0
        a = self.policy.act(obs, epsilon=eps, step_key=self.learner.t, pair_out=self._pair)
        if self.training:
            self.replay.stage(obs.float())
            self._staged = True
        acts = a.cpu().numpy()[0]
        return {sid: int(acts[i]) for i, sid in enumerate(self.ids) if sid in observation}

    def observe(self, observation, reward, done, info):
        if self.training and self._staged:
            rew = torch.tensor([[float(reward[sid]) for sid in self.ids]], device=self.replay.obs.device)
            self.replay.commit(self._pair, rew, done)
            self._staged = False
            if self.learner.observe_step(self.replay) is not None:
                self.policy.refresh_on_device()
        if done and info and self.config.get('log_dir') and info.get('eps', 1) % self.config.get('save_freq', 100) == 0:
            self.save(os.path.join(self.config['log_dir'], 'agent'))

    def save(self, path):
        torch.save({'model_state_dict': self.net.state_dict(), 'optimizer_state_dict': self.learner.opt.state_dict()}, path + '.pt')
