"""Device-resident replay ring and batched DQN learner for the IDQN rollout path ("+ replay write").

The reference wraps one ``pfrl.agents.DQN`` per signal (resco_benchmark/agents/pfrl_dqn.py:49-80):

    Adam() (lr 1e-3) - ReplayBuffer(10000) - LinearDecayEpsilonGreedy(EPS_START, EPS_END, steps)
    - minibatch BATCH_SIZE (32), replay_start_size BATCH_SIZE, target_update_interval TARGET_UPDATE (500),
    gamma GAMMA (0.99)                                       (resco_benchmark/config/agent_config.py:83-94)

and PFRL's DQN update is the published one:  y = Q(s)[a],  t = r + gamma (1 - done) max_a' Q_target(s')[a'],
loss = mean Huber(y - t, delta 1), hard target copy every ``target_update_interval`` agent steps.
PFRL is a third-party dependency that is not vendored in the reference tree and is not installed in this image,
so this module restates that published update and is checked against an unbatched PyTorch fp32 restatement of it
built from ``reference_q_network`` (tests/test_idqn_learn.py) - not against PFRL itself.

What is different by design: the S per-signal agents are ONE set of stacked parameters (BatchedIDQN) trained
with one Adam over the sum of the per-signal losses.  Adam is element-wise and the per-signal parameters are
disjoint, so this equals S independent Adam optimisers step for step.  Transitions of all N lock-step
environments are written to one ring in HBM (no host copy); every signal draws its own minibatch.
"""
import copy

import torch

from . import _state
from .idqn_rollout import BatchedIDQN
from .trunk import fc1_row_mask


class DeviceReplay:
    """Ring over the last ``capacity_steps`` env-steps of all N environments, resident on the GPU.

    Slot i holds (obs_i, act_i, rew_i, done_i): the observation the agents saw, what they did, and the reward /
    episode end that followed.  The successor observation of slot i is the obs of slot i+1, so a transition is
    sampled as (slot i, slot i+1) with i+1 already written; ``done_i`` cuts the bootstrap at episode ends (the
    post-reset observation stored in slot i+1 is then never used as a successor).

    Sizes for ingolstadt21 (S=21, Lmax=17): obs fp16 3 570 B per env-step -> N=4096 is 14.6 MB per slot,
    512 slots = 7.5 GB of the 288 GB HBM."""

    def __init__(self, capacity_steps, n_envs, n_signals, lmax, device='cuda', obs_dtype=torch.float16):
        T, N, S = int(capacity_steps), int(n_envs), int(n_signals)
        assert T >= 2
        self.T, self.N, self.S = T, N, S
        self.obs = torch.zeros(T, N, S, lmax, 5, dtype=obs_dtype, device=device)
        self.act = torch.zeros(T, N, S, dtype=torch.int16, device=device)
        self.rew = torch.zeros(T, N, S, dtype=torch.float32, device=device)
        self.done = torch.zeros(T, dtype=torch.bool, device=device)
        self.head = 0           # next slot to write
        self.count = 0          # slots written so far (saturates at T)
        self._sig = torch.arange(S, device=device)
        self._pos = torch.zeros(2, dtype=torch.int64, device=device)     # [head, count] mirrored on the device (graph replay)

    def __len__(self):
        """Number of complete transitions that can be sampled (per signal)."""
        return max(0, self.count - 1) * self.N

    def stage(self, obs):
        """Copy the observation the agents are about to act on (the simulator's zero-copy output tensor is
        overwritten by the next step, so this must happen before env.step)."""
        self.obs[self.head].copy_(obs)

    def commit(self, act, rew, done):
        """Complete the staged slot with the action taken and the reward / episode end that followed."""
        i = self.head
        self.act[i].copy_(act)
        self.rew[i].copy_(rew)
        self.done[i] = bool(done)
        self.head = (i + 1) % self.T
        self.count = min(self.count + 1, self.T)
        self._pos[0] = self.head
        self._pos[1] = self.count

    def push(self, obs, act, rew, done):
        """obs [N,S,L,5], act [N,S] int, rew [N,S] float, done bool (lock-step: one flag for all envs)."""
        self.stage(obs)
        self.commit(act, rew, done)

    # ---- checkpoints (resco_amd/checkpoint.py): the ring IS training state; loaded in place, the library reads these arrays
    def signature(self):
        return _state.ring_signature(self)

    def state_dict(self, replay=True):
        return _state.ring_state(self, replay)

    def load_state_dict(self, sd, weights_only=False):
        if not weights_only:
            _state.load_ring_state(self, sd, 'DeviceReplay')

    def sample(self, batch_size, generator=None, n_step=1, gamma=None):
        """Independent minibatch per signal: returns o [B,S,L,5], a [B,S] long, r [B,S], o2 [B,S,L,5], d [B,S] float.
        n_step > 1 (needs gamma): the same rows from the same draws, with r the discounted sum of the walk's rewards, o2 the
        observation the walk ends at, d the cut flag, and a sixth element disc = gamma^m (nstep_walk)."""
        n_ok = self.count - 1                       # slots with a written successor
        assert n_ok >= 1, 'need two pushes before sampling'
        dev = self.obs.device
        B, S = int(batch_size), self.S
        # the oldest valid slot is head - count; the newest slot (head - 1) has no successor yet
        k = torch.randint(0, n_ok, (B, S), device=dev, generator=generator)
        t = (self.head - self.count + k) % self.T
        e = torch.randint(0, self.N, (B, S), device=dev, generator=generator)
        return _rows(self, t, e, self.head, n_step, gamma)


def nstep_walk(rp, t, e, head, n_step, gamma, s=None):
    """The n-step walk of rows (t, e) [B, S] of the ring rp (s None: column j is signal j, a DeviceReplay's rows), or of rows (t, e, s)
    of any one shape (an MPLightReplay's [B]), vectorised: n_step masked steps, no data-dependent control flow, `head`
    a Python int or a device scalar (so it can be captured in a HIP graph).  newest = (head - 1) mod T is the one written slot
    without a successor.  u_0 = t; step j takes rew[u_j] and the walk stops after it where done[u_j] (cut), where j + 1 == n_step, or
    where (u_j + 1) mod T == newest; m = j + 1.  In the ring's float32 and in this order: R = rew_0, g = gamma; for j = 1 .. m - 1:
    R = R + g rew_j, g = g gamma.  -> (R [B, S], u_m = (t + m) mod T [B, S], cut [B, S] bool, g = gamma^m [B, S]).
    Truncated at the newest slot (PFRL's n-step buffer would wait for n successors); rs_dqn_set_target of include/resco_sim.h is the
    same definition for the fused update."""
    T, sig = rp.T, (rp._sig if s is None else s)
    newest = (head - 1) % T
    u = t
    R = rp.rew[t, e, sig]
    g = torch.full_like(R, float(gamma))
    cut = rp.done[t]
    stopped = cut | ((u + 1) % T == newest)
    for _ in range(1, int(n_step)):
        alive = ~stopped
        u = torch.where(alive, (u + 1) % T, u)
        R = torch.where(alive, R + g * rp.rew[u, e, sig], R)
        g = torch.where(alive, g * float(gamma), g)
        ended = rp.done[u] & alive
        cut = cut | ended
        stopped = stopped | ended | ((u + 1) % T == newest)
    return R, (u + 1) % T, cut, g


def _rows(rp, t, e, head, n_step, gamma):
    """what sample returns for the rows (t, e): five tensors at n_step 1, six beyond"""
    sig = rp._sig
    if int(n_step) == 1:
        return (rp.obs[t, e, sig], rp.act[t, e, sig].long(), rp.rew[t, e, sig], rp.obs[(t + 1) % rp.T, e, sig], rp.done[t].to(torch.float32))
    assert 1 < int(n_step) <= 32 and gamma is not None, 'n-step rows need 1 <= n_step <= 32 and gamma'
    R, u_m, cut, disc = nstep_walk(rp, t, e, head, n_step, gamma)
    return (rp.obs[t, e, sig], rp.act[t, e, sig].long(), R, rp.obs[u_m, e, sig], cut.to(torch.float32), disc)


def target_options_signature(fields, n_step, double_q):
    """the learners' signature rule for the target's options: a key only where it differs from the default, so that a checkpoint
    written before the options existed loads into a default learner and any other mix is refused by the field comparison"""
    if int(n_step) != 1:
        fields['n_step'] = int(n_step)
    if double_q:
        fields['double_q'] = True
    return fields


PER_DEFAULTS = dict(alpha=0.6, beta0=0.4, beta_steps=0, eps=1e-6)


def per_options(per, name):
    """the options of prioritised replay as a learner takes them: None (off), or a dict of any of PER_DEFAULTS' keys -> the full
    dict, checked (rs_dqn_set_priorities of include/resco_sim.h refuses the same values)"""
    if per is None:
        return None
    unknown = sorted(set(per) - set(PER_DEFAULTS))
    if unknown:
        raise ValueError('%s: unknown prioritised-replay options %s (known: %s)' % (name, unknown, sorted(PER_DEFAULTS)))
    o = dict(PER_DEFAULTS, **per)
    o = dict(alpha=float(o['alpha']), beta0=float(o['beta0']), beta_steps=int(o['beta_steps']), eps=float(o['eps']))
    if not 0.0 <= o['alpha'] <= 1.0:
        raise ValueError('%s: per alpha must lie in [0, 1], got %r' % (name, o['alpha']))
    if not 0.0 <= o['beta0'] <= 1.0:
        raise ValueError('%s: per beta0 must lie in [0, 1], got %r' % (name, o['beta0']))
    if not o['eps'] > 0.0:
        raise ValueError('%s: per eps must be positive, got %r' % (name, o['eps']))
    if o['beta_steps'] < 0:
        raise ValueError('%s: per beta_steps must not be negative, got %r' % (name, o['beta_steps']))
    return o


def per_options_signature(fields, per):
    """target_options_signature's rule for prioritised replay: the keys are there only when it is on"""
    if per is not None:
        fields.update({'per_' + k: per[k] for k in sorted(per)})
    return fields


def _sample_from_device_position(rp, batch_size, n_step=1, gamma=None):
    """DeviceReplay.sample with the ring position read from device memory and PyTorch's default generator: every value
    that changes between calls lives on the device, so the call can be captured in a HIP graph and replayed."""
    dev = rp.obs.device
    B, S = int(batch_size), rp.S
    head, count = rp._pos[0], rp._pos[1]
    n_ok = torch.clamp(count - 1, min=1)
    k = (torch.rand(B, S, device=dev) * n_ok).long().clamp_(max=rp.T - 2)
    k = torch.minimum(k, n_ok - 1)
    t = torch.remainder(head - count + k, rp.T)
    e = torch.randint(0, rp.N, (B, S), device=dev)
    return _rows(rp, t, e, head, n_step, gamma)


def linear_epsilon(t, start, end, decay_steps):
    """pfrl.explorers.LinearDecayEpsilonGreedy.compute_epsilon (pfrl_dqn.py:62-67 passes config['steps'])."""
    if t >= decay_steps:
        return float(end)
    return float(start + (end - start) * (t / float(decay_steps)))


class BatchedDQNLearner:
    """DQN update for the S stacked per-signal networks of a BatchedIDQN."""

    def __init__(self, qnet, gamma=0.99, lr=1e-3, target_update=500, batch_size=32, n_step=1, double_q=False, per=None):
        """n_step (1 .. 32): n-step returns (nstep_walk); double_q: Double DQN's bootstrap.  The defaults are PFRL's plain DQN.
        per: refused -- prioritised replay exists in the fused learner only."""
        assert isinstance(qnet, BatchedIDQN)
        if per is not None:
            raise ValueError('BatchedDQNLearner has no prioritised replay: it is built into the fused update only '
                             '(FusedDQNLearner(per=...), tools/idqn_train.py --device-update or --device-loop)')
        self.n_step, self.double_q = int(n_step), bool(double_q)
        if not 1 <= self.n_step <= 32:
            raise ValueError('BatchedDQNLearner: n_step must be in 1 .. 32, got %d' % self.n_step)
        self.q = qnet
        self.target = copy.deepcopy(qnet)
        for p in self.target.parameters():
            p.requires_grad_(False)
        self.gamma, self.batch_size, self.target_update = float(gamma), int(batch_size), int(target_update)
        self.opt = torch.optim.Adam(self.q.parameters(), lr=lr)
        self.t = 0              # agent steps seen (PFRL's self.t)
        self.n_updates = 0
        # padded lanes feed relu(conv bias) into fc1: their rows are zero at load and must stay zero
        self._fc1_mask = fc1_row_mask(qnet.lanes, qnet.lmax, qnet.fc1_w.dtype, qnet.fc1_w.device)
        qnet.fc1_w.register_hook(lambda g: g * self._fc1_mask)

    def loss(self, o, a, r, o2, d, disc=None):
        """Sum over signals of the mean Huber loss of each signal's minibatch.  Inputs as DeviceReplay.sample()
        returns them, but signal-major batches ([B,S,...]) are read as 'B independent draws per signal'.
        disc: the discount of the bootstrap per row (gamma^m of an n-step row); None: gamma."""
        q = self.q(o)                                               # [B, S, Amax]
        y = q.gather(-1, a.unsqueeze(-1)).squeeze(-1)               # [B, S]
        with torch.no_grad():
            if self.double_q:                                       # the online network's best action (the first of equal maxima),
                best = self.q(o2).argmax(dim=-1, keepdim=True)      # valued by the target network
                nxt = self.target(o2).gather(-1, best).squeeze(-1)
            else:
                nxt = self.target(o2).max(dim=-1).values            # padded actions are -inf: never the max
            tgt = r + (self.gamma if disc is None else disc) * (1.0 - d) * nxt
        per = torch.nn.functional.smooth_l1_loss(y.float(), tgt.float(), reduction='none')   # Huber, delta 1
        return per.mean(dim=0).sum()

    def update(self, batch):
        self.opt.zero_grad(set_to_none=True)
        loss = self.loss(*batch)
        loss.backward()
        self.opt.step()
        self.n_updates += 1
        return loss.detach()

    def capture_update(self, replay, warmup=3):
        """Capture [sample a minibatch per signal -> loss -> backward -> Adam step] as ONE HIP graph.  The ~150 small
        kernels of an update are launch-bound (S = 21 networks x batch 256 is little work each); replaying the graph
        removes the launch gaps.  Needs >= 2 slots in the ring and an Adam created with capturable=True (done here,
        optimiser state is carried over by re-creating it before any update has run)."""
        assert len(replay) >= 1
        carried = _state.adam_state(self.opt)           # empty before the first update; a loaded checkpoint's otherwise
        carried = dict(carried, exp_avg=[t.clone() for t in carried['exp_avg']], exp_avg_sq=[t.clone() for t in carried['exp_avg_sq']])
        done_before = self.n_updates
        self.opt = torch.optim.Adam(self.q.parameters(), lr=self.opt.param_groups[0]['lr'], capturable=True)
        self._graph_replay = replay

        def one():
            self.opt.zero_grad(set_to_none=False)
            loss = self.loss(*_sample_from_device_position(replay, self.batch_size, self.n_step, self.gamma))
            loss.backward()
            self.opt.step()
            return loss.detach()

        state = {k: v.detach().clone() for k, v in self.q.state_dict().items()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for p_ in self.q.parameters():
                p_.grad = torch.zeros_like(p_)
            for _ in range(warmup):
                one()
        torch.cuda.current_stream().wait_stream(side)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self._graph_loss = one()
        # the warm-up / capture iterations were real updates: rewind weights and optimiser to where they started
        self.q.load_state_dict(state)
        for st_ in self.opt.state.values():
            for v in st_.values():
                if torch.is_tensor(v):
                    v.zero_()
        _state.load_adam_state(self.opt, carried, 'BatchedDQNLearner.opt')      # in place: the graph reads these tensors
        self.n_updates = done_before
        return self

    def sync_target(self):
        self.target.load_state_dict(self.q.state_dict())

    # ---- checkpoints (resco_amd/checkpoint.py).  Everything is loaded IN PLACE, so a learner whose update has been graph-captured
    # (capture_update) keeps its graph: the graph reads the parameters, the gradients and the optimizer's state tensors by address.
    def signature(self):
        return target_options_signature({'batch': self.batch_size, 'target_update': self.target_update, 'gamma': self.gamma}, self.n_step, self.double_q)

    def state_dict(self):
        return {'weights': {'target': _state.module_tensors(self.target)},
                'state': {'opt': _state.adam_state(self.opt), 't': int(self.t), 'n_updates': int(self.n_updates)}}

    def load_state_dict(self, sd, weights_only=False):
        _state.load_module(self.target, sd['weights']['target'], 'BatchedDQNLearner.target')
        if not weights_only:
            _state.load_adam_state(self.opt, sd['state']['opt'], 'BatchedDQNLearner.opt')
            self.t, self.n_updates = int(sd['state']['t']), int(sd['state']['n_updates'])

    def observe_step(self, replay, generator=None, updates=1):
        """One agent step of PFRL's DQN.observe(): count it, update once the buffer holds a minibatch, and copy
        the target network every ``target_update`` steps."""
        self.t += 1
        out = None
        if self.t % self.target_update == 0:        # PFRL's DQN.batch_observe_train syncs the target BEFORE the replay update
            self.sync_target()
        if len(replay) >= self.batch_size:
            for _ in range(updates):
                if getattr(self, '_graph', None) is not None and replay is self._graph_replay:
                    self._graph.replay()
                    self.n_updates += 1
                    out = self._graph_loss
                else:
                    out = self.update(replay.sample(self.batch_size, generator, self.n_step, self.gamma))
        return out
