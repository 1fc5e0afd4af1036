"""The PPO update of a BatchedIPPO on the device (include/resco_sim.h: rs_ppo_create / rs_ppo_grad / rs_ppo_step / rs_ppo_fit;
resco_amd/csrc/resco_ppo_train.h).

`FusedPPOLearner(net)` does what `BatchedPPOLearner._fit` does -- loss(), its backward through the S stacked actor-critics,
clip_grad_per_signal, torch.optim.Adam -- in HIP kernels, all in fp32, every signal at its own lane and action count, the minibatch
rows gathered through an index array.  One update (all epochs and minibatches) is ONE call through the ABI.  The network's own
parameter storages are updated in place: `net` stays the source of truth, `FusedIPPO.refresh_on_device()` and `state_dict()` work
unchanged.  Gradients and Adam moments are torch tensors this object owns (`.grads`, `.m`, `.v`: name -> tensor); the library owns
only its workspace and the step counter (the handle's life cycle, .n_updates and .step() -- per-signal clipping and one Adam step
on what .grads holds -- are learn_fused.FusedLearnerBase's).  There is no CPU fallback.
"""
import torch

from ..sim import PPO_TENSORS, PPOConfig, PPOTensors, torch_stream
from . import _state
from .ippo import BatchedIPPO, BatchedPPOLearner
from .learn_fused import FusedLearnerBase


class FusedPPOLearner(FusedLearnerBase):
    NAME, PREFIX, TENSORS, TENSOR_SET, LOSS_SHAPE = 'FusedPPOLearner', 'rs_ppo', PPO_TENSORS, PPOTensors, (3,)

    def __init__(self, net, lr=2.5e-4, adam_eps=1e-5, gamma=0.99, lambd=0.95, clip_eps=0.1, epochs=4, minibatch=256,
                 entropy_coef=0.001, value_coef=1.0, max_grad_norm=0.5, seed=0):
        assert isinstance(net, BatchedIPPO)
        super().__init__(net)
        self.seed = int(seed) & 0xFFFFFFFF      # of device_perm's shuffles (torch.randperm draws from its own generator)
        self.lr, self.adam_eps = lr, adam_eps
        self.gamma, self.lambd, self.clip_eps, self.epochs, self.minibatch = gamma, lambd, clip_eps, int(epochs), int(minibatch)
        self.entropy_coef, self.value_coef, self.max_grad_norm = entropy_coef, value_coef, max_grad_norm
        if net.fc1_w.is_cuda:
            self._need_handle()

    def _need_handle(self):
        """the handle is created as soon as the network is on the device: at construction, else at the first use (a CPU net raises)"""
        if self._h is None:
            if self.net.fc1_w.is_cuda:
                self._create(PPOConfig(self.lr, self.adam_eps, 0.9, 0.999, self.clip_eps, self.entropy_coef, self.value_coef, self.max_grad_norm),
                             self.minibatch)
            else:
                raise RuntimeError('FusedPPOLearner needs the network on the device: the update is a HIP kernel (there is no CPU fallback)')

    # ---- the dataset as the kernels read it
    def _device_dataset(self, ds):
        S, lmax = len(self.net.lanes), self.net.lmax
        for k in ('obs', 'act', 'logp', 'adv', 'ret'):
            if not ds[k].is_cuda:
                raise RuntimeError('FusedPPOLearner needs device tensors: the update is a HIP kernel (there is no CPU fallback)')
        n = ds['act'].shape[0]
        obs = ds['obs'].contiguous()
        assert obs.dtype == torch.float16 and tuple(obs.shape) == (n, S, lmax, 5), 'obs must be the recorded f16 [n, S, lmax, 5]'
        out = dict(obs=obs, act=ds['act'].to(torch.int32).contiguous())
        for k in ('logp', 'adv', 'ret'):
            out[k] = ds[k].to(torch.float32).contiguous()
        for k in ('act', 'logp', 'adv', 'ret'):
            assert tuple(out[k].shape) == (n, S), k
        return out, n

    _dataset_from_rollout = BatchedPPOLearner.dataset_from_rollout      # reused: needs only .gamma and .lambd of self

    # ---- the pieces (what the tests compare one by one) and the update
    def grad(self, dataset, idx):
        """The gradient of the minibatch `dataset rows idx` into .grads and its three loss terms per signal into .loss_out [S, 3]
        (policy term, (value - ret)^2, entropy; un-weighted means).  dataset: obs f16 [n, S, lmax, 5], act, logp, adv, ret [n, S]."""
        self._need_handle()
        d, n = self._device_dataset(dataset)
        if not idx.is_cuda:
            raise RuntimeError('FusedPPOLearner.grad needs a device index tensor (there is no CPU fallback)')
        idx32 = idx.to(torch.int32).contiguous()
        self._keep = (d, idx32)
        rc = self._lib.rs_ppo_grad(self._h, d['obs'].data_ptr(), d['act'].data_ptr(), d['logp'].data_ptr(), d['adv'].data_ptr(), d['ret'].data_ptr(),
                                   idx32.data_ptr(), idx32.numel(), self.loss_out.data_ptr(), torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_ppo_grad', rc)
        return self.grads

    def fit(self, dataset, perm):
        """All Adam steps of an update in one call: minibatches perm[e][i : i + minibatch] as BatchedPPOLearner._fit takes them.
        perm: integer device tensor [epochs, n]."""
        self._need_handle()
        d, n = self._device_dataset(dataset)
        assert perm.is_cuda and perm.dim() == 2 and perm.shape[1] == n
        perm32 = perm.to(torch.int32).contiguous()
        self._keep = (d, perm32)
        rc = self._lib.rs_ppo_fit(self._h, d['obs'].data_ptr(), d['act'].data_ptr(), d['logp'].data_ptr(), d['adv'].data_ptr(), d['ret'].data_ptr(), n,
                                  perm32.data_ptr(), perm32.shape[0], self.minibatch, self.loss_out.data_ptr(), torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_ppo_fit', rc)
        return self.loss_out

    def device_perm(self, n, update_key, out=None):
        """The shuffles of update `update_key` over n rows, int32 [epochs, n] on the device (rs_ppo_perm): row e is a permutation of
        0 .. n - 1 that is a function of (self.seed, update_key, e, n) alone -- what the library's own loop (rs_group_ppo_train)
        draws, where torch.randperm's generator cannot be restated.  out: a tensor of that shape to write into."""
        self._need_handle()
        if not hasattr(self._lib, 'rs_ppo_perm'):
            raise RuntimeError('the loaded library has no rs_ppo_perm: rebuild it (there is no CPU fallback)')
        perm = out if out is not None else torch.empty(self.epochs, int(n), dtype=torch.int32, device=self.device)
        assert perm.is_cuda and perm.dtype == torch.int32 and perm.is_contiguous() and tuple(perm.shape) == (self.epochs, int(n))
        rc = self._lib.rs_ppo_perm(int(n), self.epochs, self.seed, int(update_key) & 0xFFFFFFFF, perm.data_ptr(), torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_ppo_perm', rc)
        return perm

    # ---- checkpoints (resco_amd/checkpoint.py): m and v in place (the library has borrowed them), the step count through
    # rs_ppo_set_steps
    def signature(self):
        return {'epochs': self.epochs, 'minibatch': self.minibatch, 'gamma': float(self.gamma), 'lambd': float(self.lambd)}

    def state_dict(self):
        self._need_handle()
        return {'state': {'m': dict(self.m), 'v': dict(self.v), 'steps': _state.fused_counter_state(self), 'seed': int(self.seed)}}

    def load_state_dict(self, sd, weights_only=False):
        if not weights_only:
            self._need_handle()
            st = sd['state']
            _state.copy_dict_into(self.m, st['m'], 'FusedPPOLearner.m')
            _state.copy_dict_into(self.v, st['v'], 'FusedPPOLearner.v')
            _state.set_fused_counter(self, st['steps'], 'FusedPPOLearner')
            self.seed = int(st['seed']) & 0xFFFFFFFF

    def update_from_rollout(self, rollout, last_value, done, generator=None, perm=None):
        """BatchedPPOLearner.update_from_rollout with the fused update: the same dataset (dataset_from_rollout: the recording and
        rs_ppo_gae), one torch.randperm per epoch on the device, one rs_ppo_fit.  perm: None, or the shuffles to use as they are
        (an integer device tensor [epochs, n], e.g. device_perm's); the generator is then not drawn from.  CPU tensors raise.
        Returns the last minibatch's loss as .loss() forms it (a device scalar)."""
        ds = self._dataset_from_rollout(rollout, last_value, done)
        n, dev = ds['act'].shape[0], ds['act'].device
        ds['act'] = rollout.cat('act').reshape(n, -1)       # the recorded int32 itself (the dataset's copy is int64 for torch's gather)
        if perm is None:
            perm = torch.stack([torch.randperm(n, device=dev, generator=generator) for _ in range(self.epochs)])
        lo = self.fit(ds, perm)
        return (lo[:, 0] + self.value_coef * lo[:, 1] - self.entropy_coef * lo[:, 2]).sum()
