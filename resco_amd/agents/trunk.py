"""The trunk the per-signal networks of IDQN and IPPO share, stacked over the S signals for N lock-step environments.

Both references give every signal its own network (resco_benchmark/agents/pfrl_dqn.py:24-40, pfrl_ppo.py:49-64) with one trunk

    Conv2d(1, 64, kernel_size=(2, 2)) - ReLU - Flatten - Linear(h*w*64, 64) - ReLU - Linear(64, 64) - ReLU
                                                  with (h, w) = (L - 1, 4) for an observation (1, L, 5)

followed by Linear(64, n_actions) -- the Q head of IDQN, the policy head of IPPO, which adds a value head next to it.  Here the S
trunks (different L and n_actions per signal) are evaluated at once from the kernel-produced fp16 tensor ``drq_norm_f16
[N, S, Lmax, 5]``: the 2x2 convolution is one grouped conv2d, the linear layers are batched matmuls over the signal axis, padded
lanes / actions are masked.  `BatchedTrunk` owns the eight stacked parameters ``conv_w .. fc3_b``, the exchange of weights with the
per-signal reference-architecture modules, and `features`; idqn_rollout.BatchedIDQN and ippo.BatchedIPPO add their heads.
"""
import torch
import torch.nn as nn


def fc1_row_mask(lanes, lmax, dtype=torch.float32, device='cpu'):
    """float [S, 64 H 4, 1]: 1 on the fc1_w rows of conv rows a signal really has.  Padded lanes feed relu(conv bias) into fc1:
    their rows are zero at load and must stay zero, so the learners multiply the gradient of fc1_w by this."""
    H = lmax - 1
    mask = torch.zeros(len(lanes), 64, H, 4, dtype=dtype, device=device)
    for s, l in enumerate(lanes):
        mask[s, :, :l - 1] = 1.0
    return mask.reshape(len(lanes), 64 * H * 4, 1)


class BatchedTrunk(nn.Module):
    reference_module = None         # (n_lanes, n_actions) -> the per-signal module of the reference that a subclass loads

    def __init__(self, lanes_per_signal, actions_per_signal, dtype=torch.float32, device='cpu'):
        super().__init__()
        self.lanes = [int(x) for x in lanes_per_signal]
        self.actions = [int(x) for x in actions_per_signal]
        S, self.lmax, self.amax = len(self.lanes), max(self.lanes), max(self.actions)
        H = self.lmax - 1
        kw = dict(dtype=dtype, device=device)
        self.conv_w = nn.Parameter(torch.zeros(S * 64, 1, 2, 2, **kw))     # grouped conv2d: one group per signal
        self.conv_b = nn.Parameter(torch.zeros(S * 64, **kw))
        self.fc1_w = nn.Parameter(torch.zeros(S, 64 * H * 4, 64, **kw))    # rows in the reference's Flatten order (c, h, w)
        self.fc1_b = nn.Parameter(torch.zeros(S, 64, **kw))
        self.fc2_w = nn.Parameter(torch.zeros(S, 64, 64, **kw))
        self.fc2_b = nn.Parameter(torch.zeros(S, 64, **kw))
        self.fc3_w = nn.Parameter(torch.zeros(S, 64, self.amax, **kw))     # Q head / policy head (named as FusedIDQN packs it)
        self.fc3_b = nn.Parameter(torch.zeros(S, self.amax, **kw))
        amask = torch.zeros(S, self.amax, dtype=torch.bool)
        for s, a in enumerate(self.actions):
            amask[s, :a] = True
        self.register_buffer('action_mask', amask.to(device))

    @classmethod
    def from_scenario(cls, sc, **kw):
        lanes = (sc.sig_obs_start[1:] - sc.sig_obs_start[:-1]).tolist()
        return cls(lanes, sc.tls_ngreen.tolist(), **kw)

    # ------------------------------------------------------------------ weight exchange with the reference layout
    @torch.no_grad()
    def load_trunk(self, s, conv, fc1, fc2):
        """signal s <- the Conv2d and the two Linear modules of its reference network"""
        H, hs = self.lmax - 1, self.lanes[s] - 1
        self.conv_w[s * 64:(s + 1) * 64] = conv.weight.to(self.conv_w)
        self.conv_b[s * 64:(s + 1) * 64] = conv.bias.to(self.conv_b)
        w1 = fc1.weight.reshape(64, 64, hs, 4)                       # out, c, h, w (Flatten order c, h, w)
        full = torch.zeros(64, 64, H, 4, dtype=w1.dtype)
        full[:, :, :hs] = w1                                          # rows of padded lanes stay zero
        self.fc1_w[s] = full.reshape(64, 64 * H * 4).t().to(self.fc1_w)
        self.fc1_b[s] = fc1.bias.to(self.fc1_b)
        self.fc2_w[s] = fc2.weight.t().to(self.fc2_w)
        self.fc2_b[s] = fc2.bias.to(self.fc2_b)

    @torch.no_grad()
    def load_head(self, s, weight, bias):
        """fc3 of signal s <- weight [A_s, 64], bias [A_s] of its reference head; padded actions are zero"""
        A = self.actions[s]
        self.fc3_w[s].zero_()
        self.fc3_b[s].zero_()
        self.fc3_w[s, :, :A] = weight.t().to(self.fc3_w)
        self.fc3_b[s, :A] = bias.to(self.fc3_b)

    @torch.no_grad()
    def export_trunk(self, s, conv, fc1, fc2):
        """the inverse of load_trunk: the Conv2d and the two Linear modules of signal s's reference network <- signal s, un-padded"""
        H, hs = self.lmax - 1, self.lanes[s] - 1
        conv.weight.copy_(self.conv_w[s * 64:(s + 1) * 64])
        conv.bias.copy_(self.conv_b[s * 64:(s + 1) * 64])
        full = self.fc1_w[s].t().reshape(64, 64, H, 4)                # out, c, h, w
        fc1.weight.copy_(full[:, :, :hs].reshape(64, 64 * hs * 4))
        fc1.bias.copy_(self.fc1_b[s])
        fc2.weight.copy_(self.fc2_w[s].t())
        fc2.bias.copy_(self.fc2_b[s])

    @torch.no_grad()
    def export_head(self, s, linear):
        """the inverse of load_head: weight [A_s, 64] and bias [A_s] of signal s's reference head <- fc3 of signal s"""
        A = self.actions[s]
        linear.weight.copy_(self.fc3_w[s, :, :A].t())
        linear.bias.copy_(self.fc3_b[s, :A])

    @torch.no_grad()
    def init_like_reference(self, seed=0):
        """PyTorch / PFRL default initialisation of every per-signal network (what an untrained agent starts from)."""
        g = torch.random.get_rng_state()
        torch.manual_seed(seed)
        mods = [self.reference_module(l, a) for l, a in zip(self.lanes, self.actions)]
        torch.random.set_rng_state(g)
        self.load_reference_modules(mods)
        return mods

    # ------------------------------------------------------------------ forward
    def features(self, obs):
        """obs [N, S, Lmax, 5] (zero padded) -> the activations after fc2, [S, N, 64].

        The S 2x2 convolutions are ONE grouped conv2d (signals = groups, MIOpen); the linear layers are signal-major
        strided-batched GEMMs (rocBLAS): [S] x ([N, F] @ [F, O]).  The ReLUs are in place: autograd reads only their results."""
        N, S = obs.shape[0], obs.shape[1]
        y = torch.nn.functional.conv2d(obs.to(self.conv_w.dtype), self.conv_w, self.conv_b, groups=S)   # [N, S*64, H, 4]
        y = torch.relu_(y).reshape(N, S, -1).transpose(0, 1)                # [S, N, 64*H*4] in (c, h, w) order
        y = torch.relu_(torch.baddbmm(self.fc1_b.unsqueeze(1), y, self.fc1_w))
        return torch.relu_(torch.baddbmm(self.fc2_b.unsqueeze(1), y, self.fc2_w))

    def head(self, y):
        """features -> fc3 outputs [N, S, Amax], -inf beyond a signal's actions"""
        out = torch.baddbmm(self.fc3_b.unsqueeze(1), y, self.fc3_w).transpose(0, 1)
        return out.masked_fill(~self.action_mask, float('-inf'))
