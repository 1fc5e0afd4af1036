"""Batched IDQN rollout policy (BASELINE config 5).

The reference gives every signal its own Q-network (resco_benchmark/agents/pfrl_dqn.py:24-40):

    Conv2d(1, 64, kernel_size=(2, 2)) - ReLU - Flatten - Linear(h*w*64, 64) - ReLU - Linear(64, 64) - ReLU
    - Linear(64, n_actions)                       with (h, w) = (L - 1, 4) for an observation (1, L, 5)

evaluated one observation at a time on the host.  Here the S networks (different L and n_actions per
signal) are evaluated for all N environments at once from the kernel-produced fp16 tensor
``drq_norm_f16 [N, S, Lmax, 5]``: the stacked parameters, the forward up to the last layer and the import of weights
from the per-signal reference-architecture modules (so a trained IDQN plugs in) are trunk.BatchedTrunk's, shared with IPPO.
Epsilon-greedy action selection is included; the replay ring and the DQN update live in idqn_learn.py.
"""
import torch
import torch.nn as nn

from .trunk import BatchedTrunk


def reference_q_network(n_lanes, n_actions):
    """The per-signal model of pfrl_dqn.py:30-39 (DiscreteActionValueHead is an output wrapper, omitted)."""
    h, w = n_lanes - 1, 4
    return nn.Sequential(nn.Conv2d(1, 64, kernel_size=(2, 2)), nn.ReLU(), nn.Flatten(), nn.Linear(h * w * 64, 64),
                         nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, n_actions))


class BatchedIDQN(BatchedTrunk):
    """The trunk with fc3 as the Q head.  No gradient hook: BatchedDQNLearner masks the padded fc1 rows of the net it trains."""
    reference_module = staticmethod(reference_q_network)

    @torch.no_grad()
    def load_reference_modules(self, modules):
        """modules[s] = the nn.Sequential of reference_q_network(L_s, A_s) (e.g. a loaded IDQN checkpoint)."""
        for s, m in enumerate(modules):
            self.load_trunk(s, m[0], m[3], m[5])
            self.load_head(s, m[7].weight, m[7].bias)
        return self

    @torch.no_grad()
    def to_reference_modules(self):
        """The inverse of load_reference_modules: one reference_q_network(L_s, A_s) per signal (float32, on the CPU) holding signal
        s's weights un-padded, e.g. for checkpoint.save_reference_idqn."""
        with torch.random.fork_rng(devices=[]):         # (the constructors' initial draws are overwritten: the caller's generator stays)
            mods = [reference_q_network(l, a) for l, a in zip(self.lanes, self.actions)]
        for s, m in enumerate(mods):
            self.export_trunk(s, m[0], m[3], m[5])
            self.export_head(s, m[7])
        return mods

    def forward(self, obs):
        """obs [N, S, Lmax, 5] (zero padded) -> Q [N, S, Amax] (padded actions = -inf)."""
        return self.head(self.features(obs))

    @torch.no_grad()
    def act(self, obs, epsilon=0.0, generator=None):
        """epsilon-greedy actions, int32 [N, S] on obs.device."""
        q = self.forward(obs)
        greedy = q.argmax(dim=-1)
        if epsilon <= 0.0:
            return greedy.to(torch.int32)
        if not hasattr(self, '_n_act') or self._n_act.device != q.device:
            self._n_act = torch.as_tensor(self.actions, device=q.device, dtype=torch.float32)
        u = torch.rand((2,) + tuple(greedy.shape), device=q.device, generator=generator)
        rnd = torch.minimum((u[1] * self._n_act).long(), (self._n_act - 1).long())
        return torch.where(u[0] < epsilon, rnd, greedy).to(torch.int32)

