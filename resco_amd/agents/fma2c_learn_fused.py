"""The fused A2C learner of FMA2C (rs_fma2c_learn_*; resco_amd/csrc/resco_fma2c_train.h): A2CLearner's interface and bookkeeping
(resco_amd/agents/fma2c.py) over HIP kernels -- returns and advantages, the re-run of the segment, the loss, BPTT through both LSTM
nets, the per-agent clip and TF1's RMSProp.  The segment buffers, the weights, ms and the segment's start state live on the device;
the policy (FusedFMA2C) acts with the learner's own weight vector, so nothing is re-packed after an update."""
import ctypes as C
import weakref

import torch

from .fma2c import N_LSTM, PARAMS


class FusedA2CLearner:
    BUF = {'weights': 0, 'ms': 1, 'grads': 2, 'states_bw': 3, 'returns': 4, 'advantages': 5, 'norms': 6, 'scales': 7}

    def __init__(self, net, policy, n_envs, batch_size=120, gamma=0.96, lr=2.5e-4, alpha=0.99, eps=1e-5, max_grad_norm=40.0, value_coef=0.5,
                 entropy_coef=0.001, reward_norm=2000.0, reward_clip=2.0, workspace_bytes=0):
        from ..sim import Fma2cLearnConfig, load_library
        self.net, self.policy, self.N, self.T = net, policy, int(n_envs), int(batch_size)
        self.gamma, self.lr, self.alpha, self.eps, self.max_grad_norm = gamma, lr, alpha, eps, max_grad_norm
        self.value_coef, self.entropy_coef, self.reward_norm, self.reward_clip = value_coef, entropy_coef, reward_norm, reward_clip
        self._lib, L = load_library(), net.layout
        if not hasattr(self._lib, 'rs_fma2c_learn_create'):
            raise RuntimeError('the loaded library has no rs_fma2c_learn_*: rebuild it (there is no CPU fallback)')
        self.device = policy.device
        dev, K, W = torch.device('cuda:%d' % self.device), L.K, L.W
        self.rows = torch.zeros(self.T, self.N, K, W, device=dev)
        self.acts = torch.zeros(self.T, self.N, K, dtype=torch.int32, device=dev)
        self.rews, self.vals = torch.zeros(self.T, self.N, K, device=dev), torch.zeros(self.T, self.N, K, device=dev)   # rewards RAW: the kernel clips
        self.dones = [False]                # as A2CLearner.dones, mirrored into dones_dev [T + 1]
        self.dones_dev = torch.zeros(self.T + 1, dtype=torch.int32, device=dev)
        self.n, self.steps_done, self.updates = 0, 0, 0
        self.last_loss = None
        self._loss = torch.zeros(K, device=dev)
        cfg = Fma2cLearnConfig(float(gamma), float(lr), float(alpha), float(eps), float(max_grad_norm or 0.0), float(value_coef), float(entropy_coef),
                               float(reward_norm or 0.0), float(reward_clip or 0.0), int(workspace_bytes))
        h = C.c_void_p()
        self._check(self._lib.rs_fma2c_learn_create(policy._h, C.byref(cfg), self.N, self.T, C.byref(h)), 'rs_fma2c_learn_create')
        self._h = h
        policy._learner = weakref.ref(self)
        self.grad_norm = self.buffer('norms')

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError('%s failed (%d): %s' % (what, rc, (self._lib.rs_last_error(None) or b'?').decode()))

    @property
    def handle(self):
        return self._h.value if self._h is not None else None

    def close(self):
        """the weights go back into the policy's own vector, which it acts with from here on; close the learner BEFORE its policy"""
        if getattr(self, '_h', None) is not None:
            self._lib.rs_fma2c_learn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            if getattr(self.policy, '_h', None) is not None:        # a closed policy has closed this learner first
                self.close()
        except Exception:
            pass

    def buffer(self, name):
        """zero-copy tensor over the learner's weights / ms / grads [n] (the packed layout), states_bw [N, K, 4, 64], returns /
        advantages [T, N, K] or the per-agent norms / scales [K] of the last step"""
        from ..sim import _DevArray
        p = C.c_void_p()
        self._check(self._lib.rs_fma2c_learn_buffer(self._h, self.BUF[name], C.byref(p)), 'rs_fma2c_learn_buffer')
        K = self.net.layout.K
        n = sum(getattr(self.net, t).numel() for t in PARAMS)
        shape = {'weights': (n,), 'ms': (n,), 'grads': (n,), 'states_bw': (self.N, K, 4, N_LSTM), 'returns': (self.T, self.N, K),
                 'advantages': (self.T, self.N, K), 'norms': (K,), 'scales': (K,)}[name]
        return torch.as_tensor(_DevArray(p.value, shape, 0, self), device='cuda:%d' % self.device)

    @property
    def states_bw(self):
        return self.buffer('states_bw')

    def slot(self):
        """the views of the next step's segment slot: pass them to FusedFMA2C.act(out=...) so that rows and values land there without
        a copy (add() skips the copy of a tensor that already is the slot)"""
        return {'rows': self.rows[self.n], 'value': self.vals[self.n]}

    def unpack(self, flat):
        """the packed vector as the dict of BatchedFMA2C's parameter tensors (views)"""
        out, off = {}, 0
        for name in PARAMS:
            p = getattr(self.net, name)
            out[name] = flat[off:off + p.numel()].view(p.shape)
            off += p.numel()
        return out

    @torch.no_grad()
    def pull(self):
        """copy the learner's weights into net's parameters (for save and for the PyTorch path)"""
        for name, w in self.unpack(self.buffer('weights')).items():
            getattr(self.net, name).copy_(w)
        return self.net

    def add(self, rows, actions, rewards, values, done):
        t = self.n
        for dst, src in ((self.rows[t], rows), (self.acts[t], actions), (self.rews[t], rewards), (self.vals[t], values)):
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src)
        self.dones.append(bool(done))
        self.dones_dev[t + 1] = int(bool(done))
        self.n += 1

    def _segment(self, R):
        R = R.detach().float().contiguous()
        return R, [self.rows.data_ptr(), self.acts.data_ptr(), self.rews.data_ptr(), self.vals.data_ptr(), self.dones_dev.data_ptr(), R.data_ptr(), self.n]

    def grad(self, R):
        """returns, advantages and the un-clipped gradients of the stored steps (buffer('grads')); -> the per-agent losses [K]"""
        from ..sim import torch_stream
        R, seg = self._segment(R)
        self._check(self._lib.rs_fma2c_learn_grad(self._h, *seg, self._loss.data_ptr(), torch_stream(self.device)), 'rs_fma2c_learn_grad')
        return self._loss

    def step(self):
        from ..sim import torch_stream
        self._check(self._lib.rs_fma2c_learn_step(self._h, torch_stream(self.device)), 'rs_fma2c_learn_step')

    def update(self, R, states_fw):
        """A2CLearner.update: R [N, K] = the bootstrap value (zeros at done); states_fw = the acting state now"""
        from ..sim import torch_stream
        assert states_fw.is_cuda and states_fw.dtype == torch.float32 and states_fw.is_contiguous()
        R, seg = self._segment(R)
        self._check(self._lib.rs_fma2c_learn_update(self._h, *seg, self._loss.data_ptr(), states_fw.data_ptr(), torch_stream(self.device)),
                    'rs_fma2c_learn_update')
        self.dones, self.n = [self.dones[-1]], 0
        self.dones_dev[0] = int(self.dones[0])
        self.updates += 1
        self.last_loss = self._loss.clone()
        return self.last_loss

    # ---- checkpoints (resco_amd/checkpoint.py), at an episode boundary (the segment is empty there): the library-owned weights, ms
    # and states_bw are written in place through their zero-copy tensors.  The learner has no hidden counter: TF1's RMSProp has
    # no bias correction and the rate is constant.
    def signature(self):
        return {'T': self.T, 'n_envs': self.N, 'K': int(self.net.layout.K)}

    def state_dict(self):
        return {'weights': {'weights': self.buffer('weights')},
                'state': {'ms': self.buffer('ms'), 'states_bw': self.buffer('states_bw'), 'dones': [bool(d) for d in self.dones],
                          'dones_dev0': int(self.dones_dev[0]), 'n': int(self.n), 'steps_done': int(self.steps_done), 'updates': int(self.updates)}}

    @torch.no_grad()
    def load_state_dict(self, sd, weights_only=False):
        from . import _state
        _state.copy_into(self.buffer('weights'), sd['weights']['weights'], 'FusedA2CLearner.weights')
        self.pull()                             # the network mirrors the vector the policy acts with
        if weights_only:
            return
        st = sd['state']
        if int(st['n']) != 0:
            raise ValueError('FusedA2CLearner: the checkpoint was taken inside a segment (n = %d)' % int(st['n']))
        _state.copy_into(self.buffer('ms'), st['ms'], 'FusedA2CLearner.ms')
        _state.copy_into(self.buffer('states_bw'), st['states_bw'], 'FusedA2CLearner.states_bw')
        self.dones, self.n = [bool(d) for d in st['dones']], 0
        self.dones_dev[0] = int(st['dones_dev0'])
        self.steps_done, self.updates = int(st['steps_done']), int(st['updates'])

    def observe(self, rows, actions, rewards, values, done, states_fw, bootstrap):
        """A2CLearner.observe: store, and every batch_size steps or at done update with R = 0 (done) or bootstrap()"""
        from ..sim import torch_stream
        self.add(rows, actions, rewards, values, done)
        self.steps_done += 1
        out = None
        if self.steps_done % self.T == 0 or done:
            R = torch.zeros_like(values) if done else bootstrap()
            out = self.update(R, states_fw)
        if done:
            self.steps_done = 0
            self._check(self._lib.rs_fma2c_learn_reset(self._h, torch_stream(self.device)), 'rs_fma2c_learn_reset')
        return out
