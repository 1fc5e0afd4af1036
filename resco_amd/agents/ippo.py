"""Batched IPPO: the S per-signal actor-critic networks of the reference and their PPO update, for N lock-step envs.

The reference wraps one `pfrl.agents.PPO` per signal (resco_benchmark/agents/pfrl_ppo.py:38-75):

    Conv2d(1, 64, (2,2)) - ReLU - Flatten - Linear(h*w*64, 64) - ReLU - Linear(64, 64) - ReLU -
    Branched( Linear(64, A) [LeCun-normal, gain 1e-2] + SoftmaxCategoricalHead ,  Linear(64, 1) )
    Adam(lr 2.5e-4, eps 1e-5); clip_eps 0.1, no value clipping, update_interval 1024, minibatch 256, epochs 4,
    standardize_advantages, entropy_coef 0.001, max_grad_norm 0.5     (PFRL defaults: gamma 0.99, lambda 0.95,
    value_func_coef 1.0)

PFRL is not vendored in the reference tree and not installed here, so - as for DQN (idqn_learn.py) - this module
restates the published PPO update with those settings and is checked against an unbatched PyTorch fp32 restatement
built from `reference_ppo_network` (tests/test_ippo.py), not against PFRL itself.

The trunk -- stacked parameters, weight import, forward up to fc2 -- is trunk.BatchedTrunk's, shared with IDQN; BatchedIPPO adds the
value head and the gradient hooks that keep the weights of padded lanes and actions zero.

What is different by design: the S agents are one set of stacked parameters under one Adam (element-wise, disjoint
parameters: equal to S optimisers); the loss is the sum of the per-signal losses; gradient clipping and advantage
standardisation are done per signal as S separate agents would.  A rollout segment holds T env-steps of all N
environments (T*N samples per signal per update instead of 1024 consecutive steps of one environment).
Acting can go through the fused HIP kernel (`FusedIDQN(net).act(obs, sample=True)`: same trunk, softmax sampling), or through its
actor-critic mode, which also returns the log-probability and the value (ippo_fused.py: FusedIPPO; update_from_rollout below).
"""
import math

import torch
import torch.nn as nn

from . import _state
from .trunk import BatchedTrunk, fc1_row_mask


class ReferencePPONet(nn.Module):
    """The per-signal model of pfrl_ppo.py:49-64 (SoftmaxCategoricalHead = softmax over the returned logits)."""

    def __init__(self, n_lanes, n_actions):
        super().__init__()
        h, w = n_lanes - 1, 4
        self.trunk = nn.Sequential(nn.Conv2d(1, 64, kernel_size=(2, 2)), nn.ReLU(), nn.Flatten(), nn.Linear(h * w * 64, 64),
                                   nn.ReLU(), nn.Linear(64, 64), nn.ReLU())
        self.pi = nn.Linear(64, n_actions)
        self.v = nn.Linear(64, 1)
        for layer, gain in ((self.trunk[0], 1.0), (self.trunk[3], 1.0), (self.trunk[5], 1.0), (self.pi, 1e-2), (self.v, 1.0)):
            fan_in = layer.weight[0].numel()                     # init_lecun_normal: N(0, gain / sqrt(fan_in)), zero bias
            nn.init.normal_(layer.weight, 0.0, gain / math.sqrt(fan_in))
            nn.init.zeros_(layer.bias)

    def forward(self, x):
        z = self.trunk(x)
        return self.pi(z), self.v(z).squeeze(-1)


class BatchedIPPO(BatchedTrunk):
    """The trunk with fc3 as the policy head, plus a value head."""
    reference_module = ReferencePPONet

    def __init__(self, lanes_per_signal, actions_per_signal, dtype=torch.float32, device='cpu'):
        super().__init__(lanes_per_signal, actions_per_signal, dtype=dtype, device=device)
        S = len(self.lanes)
        self.v_w = nn.Parameter(torch.zeros(S, 64, 1, dtype=dtype, device=device))
        self.v_b = nn.Parameter(torch.zeros(S, 1, dtype=dtype, device=device))
        self.register_buffer('fc1_mask', fc1_row_mask(self.lanes, self.lmax, dtype, device))
        # padded lanes feed relu(conv bias) into fc1 and padded actions are masked: their weights stay zero
        self.fc1_w.register_hook(lambda g: g * self.fc1_mask)
        self.fc3_w.register_hook(lambda g: g * self.action_mask.unsqueeze(1))
        self.fc3_b.register_hook(lambda g: g * self.action_mask)

    @torch.no_grad()
    def load_reference_modules(self, modules):
        """modules[s]: a ReferencePPONet(L_s, A_s) (or any module with the same .trunk / .pi / .v)."""
        for s, m in enumerate(modules):
            self.load_trunk(s, m.trunk[0], m.trunk[3], m.trunk[5])
            self.load_head(s, m.pi.weight, m.pi.bias)
            self.v_w[s] = m.v.weight.t().to(self.v_w)
            self.v_b[s] = m.v.bias.to(self.v_b)
        return self

    def forward(self, obs):
        """obs [B, S, Lmax, 5] -> logits [B, S, Amax] (-inf beyond a signal's actions), value [B, S]."""
        y = self.features(obs)
        return self.head(y), torch.baddbmm(self.v_b.unsqueeze(1), y, self.v_w).squeeze(-1).transpose(0, 1)

    @torch.no_grad()
    def act(self, obs, generator=None):
        logits, _ = self.forward(obs)
        p = torch.softmax(logits.float(), dim=-1)
        return torch.multinomial(p.reshape(-1, p.shape[-1]), 1, generator=generator).reshape(p.shape[:-1]).to(torch.int32)


def gae(rew, val, next_val, done, gamma=0.99, lambd=0.95):
    """Generalised advantage estimates over a segment.  rew, val [T, ...]; next_val [...] = value of the state after
    the last step; done [T] bool: the episode ended after step t (no bootstrap across it)."""
    T = rew.shape[0]
    adv = torch.zeros_like(rew)
    last = torch.zeros_like(rew[0])
    for t in range(T - 1, -1, -1):
        nv = next_val if t == T - 1 else val[t + 1]
        nd = 1.0 - done[t].to(rew.dtype)
        delta = rew[t] + gamma * nd * nv - val[t]
        last = delta + gamma * lambd * nd * last
        adv[t] = last
    return adv, adv + val


class BatchedPPOLearner:
    """PPO update of the S stacked actor-critics of a BatchedIPPO from one rollout segment."""

    def __init__(self, net, lr=2.5e-4, adam_eps=1e-5, gamma=0.99, lambd=0.95, clip_eps=0.1, epochs=4, minibatch=256,
                 entropy_coef=0.001, value_coef=1.0, max_grad_norm=0.5):
        assert isinstance(net, BatchedIPPO)
        self.net = net
        self.opt = torch.optim.Adam(net.parameters(), lr=lr, eps=adam_eps)
        self.gamma, self.lambd, self.clip_eps, self.epochs, self.minibatch = gamma, lambd, clip_eps, int(epochs), int(minibatch)
        self.entropy_coef, self.value_coef, self.max_grad_norm = entropy_coef, value_coef, max_grad_norm
        self.n_updates = 0

    # ---- pieces the test compares one by one with the per-signal restatement
    @torch.no_grad()
    def make_dataset(self, obs, act, rew, done, last_obs, chunk=4096):
        """obs [T, N, S, L, 5], act [T, N, S] int, rew [T, N, S], done [T] bool, last_obs [N, S, L, 5]: old log-probs and
        values from the current parameters, GAE, per-signal standardised advantages; flattened to [T*N, S, ...]."""
        T, N, S = act.shape
        flat = torch.cat([obs.reshape(T * N, *obs.shape[2:]), last_obs], 0)
        lg, vs = [], []
        for i in range(0, flat.shape[0], chunk):
            l_, v_ = self.net(flat[i:i + chunk])
            lg.append(torch.log_softmax(l_.float(), -1))
            vs.append(v_.float())
        logp_all, v_all = torch.cat(lg, 0), torch.cat(vs, 0)
        logp = logp_all[:T * N].gather(-1, act.reshape(T * N, S, 1).long()).squeeze(-1)
        val = v_all[:T * N].reshape(T, N, S)
        adv, ret = gae(rew.float(), val, v_all[T * N:], done, self.gamma, self.lambd)
        adv = adv.reshape(T * N, S)
        adv = (adv - adv.mean(0, keepdim=True)) / (adv.std(0, unbiased=False, keepdim=True) + 1e-8)
        return dict(obs=flat[:T * N], act=act.reshape(T * N, S).long(), logp=logp, adv=adv, ret=ret.reshape(T * N, S))

    def loss(self, mb):
        logits, v = self.net(mb['obs'])
        lp_all = torch.log_softmax(logits.float(), -1)
        lp = lp_all.gather(-1, mb['act'].unsqueeze(-1)).squeeze(-1)
        ratio = torch.exp(lp - mb['logp'])
        a = mb['adv']
        pg = -torch.minimum(ratio * a, torch.clamp(ratio, 1.0 - self.clip_eps, 1.0 + self.clip_eps) * a).mean(0)
        vf = ((v.float() - mb['ret']) ** 2).mean(0)
        # entropy over a signal's own actions: the -inf log-probabilities of padded actions are replaced BEFORE the
        # product (0 * -inf would put NaN into the gradient even behind a torch.where)
        ent = -(torch.exp(lp_all) * lp_all.masked_fill(~self.net.action_mask, 0.0)).sum(-1).mean(0)
        return (pg + self.value_coef * vf - self.entropy_coef * ent).sum()          # sum over signals

    def clip_grad_per_signal(self):
        """torch.nn.utils.clip_grad_norm_(agent parameters, max_grad_norm) for each of the S agents."""
        S = len(self.net.lanes)
        sq = torch.zeros(S, device=self.net.fc1_w.device)
        views = []
        for p_ in self.net.parameters():
            if p_.grad is None:
                continue
            g = p_.grad.reshape(S, -1)
            views.append(g)
            sq += (g.float() ** 2).sum(1)
        scale = torch.clamp(self.max_grad_norm / (sq.sqrt() + 1e-6), max=1.0)
        for g in views:
            g.mul_(scale.unsqueeze(1).to(g.dtype))

    def update(self, obs, act, rew, done, last_obs, generator=None):
        return self._fit(self.make_dataset(obs, act, rew, done, last_obs), generator)

    @torch.no_grad()
    def dataset_from_rollout(self, rollout, last_value, done):
        """The dataset of make_dataset from a recorded segment (agents/ippo_fused.py: DeviceRollout, filled by rs_group_rollout)
        WITHOUT a second forward: logp and value are the ones the actor-critic kernel wrote when it drew the actions, GAE and the
        per-signal standardisation are ONE call of the fused kernels (rs_ppo_gae).  last_value float32 [N, S] = the value of the
        state after the last step (FusedIPPO.value), done [T] bool / uint8."""
        from ..sim import load_library, torch_stream
        obs, act, logp, val, rew = (rollout.cat(k) for k in ('obs', 'act', 'logp', 'value', 'rew'))
        for t in (obs, act, logp, val, rew, last_value, done):
            if not t.is_cuda:
                raise RuntimeError('update_from_rollout needs device tensors: rs_ppo_gae is a HIP kernel (there is no CPU fallback)')
        T, N, S = act.shape
        assert tuple(last_value.shape) == (N, S) and last_value.dtype == torch.float32 and tuple(done.shape) == (T,)
        val, rew, last_value = val.contiguous(), rew.contiguous(), last_value.contiguous()
        done8 = done.to(torch.uint8).contiguous()
        adv, ret = torch.empty_like(val), torch.empty_like(val)
        scratch = torch.empty(N, S, dtype=torch.float32, device=val.device)
        rc = load_library().rs_ppo_gae(rew.data_ptr(), val.data_ptr(), last_value.data_ptr(), done8.data_ptr(), T, N, S, float(self.gamma),
                                       float(self.lambd), adv.data_ptr(), ret.data_ptr(), scratch.data_ptr(), torch_stream(val.device.index))
        if rc != 0:
            raise RuntimeError('rs_ppo_gae failed (%d)' % rc)
        return dict(obs=obs.reshape(T * N, *obs.shape[2:]), act=act.reshape(T * N, S).long(), logp=logp.reshape(T * N, S),
                    adv=adv.reshape(T * N, S), ret=ret.reshape(T * N, S))

    def update_from_rollout(self, rollout, last_value, done, generator=None):
        """update() on a segment the device recorded: dataset_from_rollout, then the unchanged loss / clip_grad_per_signal / Adam
        loop.  CPU tensors raise.  logp_old here is the BEHAVIOUR policy's own log-probability -- that of the fp16 kernel which drew
        the action -- where make_dataset re-evaluates the fp32 network: the ratio of the first minibatch is
        exp(logp_fp32 - logp_kernel) instead of exactly 1 (largest |difference| measured on a recorded segment: 1.4e-4 on cologne1,
        5.4e-4 on ingolstadt21, profiles/r08_ippo_device_rollout.txt); likewise V in the advantages is the kernel's value."""
        return self._fit(self.dataset_from_rollout(rollout, last_value, done), generator)

    # ---- checkpoints (resco_amd/checkpoint.py): the optimizer's state is loaded in place
    def signature(self):
        return {'epochs': self.epochs, 'minibatch': self.minibatch, 'gamma': float(self.gamma), 'lambd': float(self.lambd)}

    def state_dict(self):
        return {'state': {'opt': _state.adam_state(self.opt), 'n_updates': int(self.n_updates)}}

    def load_state_dict(self, sd, weights_only=False):
        if not weights_only:
            _state.load_adam_state(self.opt, sd['state']['opt'], 'BatchedPPOLearner.opt')
            self.n_updates = int(sd['state']['n_updates'])

    def _fit(self, ds, generator=None):
        n = ds['act'].shape[0]
        last = None
        for _ in range(self.epochs):
            perm = torch.randperm(n, device=ds['act'].device, generator=generator)
            for i in range(0, n, self.minibatch):
                idx = perm[i:i + self.minibatch]
                mb = {k: v[idx] for k, v in ds.items()}
                self.opt.zero_grad(set_to_none=True)
                last = self.loss(mb)
                last.backward()
                self.clip_grad_per_signal()
                self.opt.step()
                self.n_updates += 1
        return last.detach()
