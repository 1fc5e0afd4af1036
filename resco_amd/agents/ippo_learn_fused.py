"""The PPO update of a BatchedIPPO on the device (include/resco_sim.h: rs_ppo_create / rs_ppo_grad / rs_ppo_step / rs_ppo_fit;
resco_amd/csrc/resco_ppo_train.h).

`FusedPPOLearner(net)` does what `BatchedPPOLearner._fit` does -- loss(), its backward through the S stacked actor-critics,
clip_grad_per_signal, torch.optim.Adam -- in HIP kernels, all in fp32, every signal at its own lane and action count, the minibatch
rows gathered through an index array.  One update (all epochs and minibatches) is ONE call through the ABI.  The network's own
parameter storages are updated in place: `net` stays the source of truth, `FusedIPPO.refresh_on_device()` and `state_dict()` work
unchanged.  Gradients and Adam moments are torch tensors this object owns (`.grads`, `.m`, `.v`: name -> tensor); the library owns
only its workspace and the step counter.  There is no CPU fallback.
"""
import ctypes as C

import torch

from ..sim import PPO_TENSORS, PPOConfig, PPOTensors, load_library, torch_stream
from .ippo import BatchedIPPO, BatchedPPOLearner


class FusedPPOLearner:
    def __init__(self, net, lr=2.5e-4, adam_eps=1e-5, gamma=0.99, lambd=0.95, clip_eps=0.1, epochs=4, minibatch=256,
                 entropy_coef=0.001, value_coef=1.0, max_grad_norm=0.5):
        assert isinstance(net, BatchedIPPO)
        self.net = net
        self.lr, self.adam_eps = lr, adam_eps
        self.gamma, self.lambd, self.clip_eps, self.epochs, self.minibatch = gamma, lambd, clip_eps, int(epochs), int(minibatch)
        self.entropy_coef, self.value_coef, self.max_grad_norm = entropy_coef, value_coef, max_grad_norm
        self._lib, self._h, self._keep = None, None, None
        self.grads = self.m = self.v = self.loss_out = None
        if net.fc1_w.is_cuda:
            self._create()

    # ---- the handle
    def _create(self):
        net = self.net
        for k in PPO_TENSORS:
            p = getattr(net, k)
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError('FusedPPOLearner needs contiguous float32 device parameters: the update is a HIP kernel (there is no CPU fallback)')
        self._lib = load_library()
        if not hasattr(self._lib, 'rs_ppo_create'):
            raise RuntimeError('the loaded library has no rs_ppo_create: rebuild it (there is no CPU fallback)')
        self.device = net.fc1_w.device
        S = len(net.lanes)
        zeros = lambda: {k: torch.zeros_like(getattr(net, k).detach()) for k in PPO_TENSORS}
        self.grads, self.m, self.v = zeros(), zeros(), zeros()
        self.loss_out = torch.zeros(S, 3, dtype=torch.float32, device=self.device)
        sets = [PPOTensors(*[getattr(net, k).data_ptr() for k in PPO_TENSORS])]
        sets += [PPOTensors(*[d[k].data_ptr() for k in PPO_TENSORS]) for d in (self.grads, self.m, self.v)]
        cfg = PPOConfig(self.lr, self.adam_eps, 0.9, 0.999, self.clip_eps, self.entropy_coef, self.value_coef, self.max_grad_norm)
        lanes, acts = (C.c_int32 * S)(*net.lanes), (C.c_int32 * S)(*net.actions)
        h = C.c_void_p()
        torch.cuda.synchronize(self.device)
        rc = self._lib.rs_ppo_create(self.device.index or 0, S, net.lmax, lanes, acts, net.amax, C.byref(cfg), *[C.byref(t) for t in sets],
                                     self.minibatch, C.byref(h))
        if rc != 0:
            raise RuntimeError('rs_ppo_create failed (%d): %s' % (rc, (self._lib.rs_last_error(None) or b'').decode()))
        self._h = h

    def _need_handle(self):
        if self._h is None:
            if self.net.fc1_w.is_cuda:
                self._create()
            else:
                raise RuntimeError('FusedPPOLearner needs the network on the device: the update is a HIP kernel (there is no CPU fallback)')

    def close(self):
        if self._h is not None:
            self._lib.rs_ppo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_updates(self):
        """Adam steps taken so far"""
        return 0 if self._h is None else int(self._lib.rs_ppo_steps(self._h))

    def _fail(self, name, rc):
        raise RuntimeError('%s failed (%d): %s' % (name, rc, (self._lib.rs_last_error(None) or b'').decode()))

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

    def step(self):
        """Per-signal clipping and one Adam step on what .grads holds (.grads itself stays un-scaled)."""
        self._need_handle()
        rc = self._lib.rs_ppo_step(self._h, torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_ppo_step', rc)

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

    def update_from_rollout(self, rollout, last_value, done, generator=None):
        """BatchedPPOLearner.update_from_rollout with the fused update: the same dataset (dataset_from_rollout: the recording and
        rs_ppo_gae), one torch.randperm per epoch on the device, one rs_ppo_fit.  CPU tensors raise.  Returns the last minibatch's
        loss as .loss() forms it (a device scalar)."""
        ds = self._dataset_from_rollout(rollout, last_value, done)
        n, dev = ds['act'].shape[0], ds['act'].device
        ds['act'] = rollout.cat('act').reshape(n, -1)       # the recorded int32 itself (the dataset's copy is int64 for torch's gather)
        perm = torch.stack([torch.randperm(n, device=dev, generator=generator) for _ in range(self.epochs)])
        lo = self.fit(ds, perm)
        return (lo[:, 0] + self.value_coef * lo[:, 1] - self.entropy_coef * lo[:, 2]).sum()
