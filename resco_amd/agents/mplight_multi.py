"""MPLight trained on several maps at once: ONE shared FRAP, one replay ring per map, the update on the device (include/resco_sim.h:
rs_mplight_multi_create / _sample / _grad / _step / _update; resco_amd/csrc/resco_frap_multi.h).

FRAP's parameters (1365 + 4 D floats) do not depend on a map's signal count or its number of phase pairs P: a network sees its map
only through its phase pairs.  `MultiMapMPLightLearner(nets)` takes one FRAP per map -- same demand_shape, any P -- and makes the
parameters of EVERY one of them views of the one packed vector `.flat` (in state_dict order, as FusedMPLightLearner does for its
single network): nets[0]'s weights at construction are the shared weights, every net's state_dict() is then the same tensors, and a
FusedMPLight per map bound by share_weights(learner.flat) acts on the updated weights with no re-pack.  `.target` is a FRAP of
nets[0]'s shape whose parameters view `.flat_target`; `.grads`, `.m`, `.v` are name -> view dicts.

A minibatch is drawn uniformly over all stored transitions of all rings that have a successor (one replay buffer shared by the maps
would give the same) by the library's counter hash from (seed, Adam steps so far); its rows come grouped by map, and the group sizes
are known to the host without a synchronisation.  There is no CPU fallback and no PyTorch twin.
"""
import ctypes as C

import torch

from ..sim import DQNConfig, MPLightMap, MPLightRing, load_library, torch_stream
from . import _state
from .idqn_learn import target_options_signature
from .learn_fused import FusedLearnerBase
from .mplight import FRAP
from .mplight_learn_fused import _views

MAX_MAPS = 8        # FPM_MAPS of resco_frap_multi.h


class MultiMapMPLightLearner(FusedLearnerBase):
    NAME, PREFIX, SET_TARGET = 'MultiMapMPLightLearner', 'rs_mplight_multi', 'rs_mplight_maps_set_target'

    def __init__(self, nets, n_signals, gamma=0.99, lr=1e-3, target_update=500, batch_size=32, seed=0, n_step=1, double_q=False):
        """nets: one FRAP per map; n_signals: the maps' signal counts (their rings' S); n_step (1 .. 32) and double_q: the target's
        options, as FusedMPLightLearner's (rs_mplight_maps_set_target): every row walks its own map's ring."""
        nets, n_signals = list(nets), [int(s) for s in n_signals]
        if not 1 <= len(nets) <= MAX_MAPS or len(n_signals) != len(nets):
            raise ValueError('MultiMapMPLightLearner takes 1 .. %d networks and as many signal counts' % MAX_MAPS)
        assert all(isinstance(n, FRAP) for n in nets)
        super().__init__(nets[0])
        self._take_target_options(n_step, double_q)
        self.nets, self.n_signals = nets, n_signals
        D = nets[0].demand_shape
        if any(n.demand_shape != D for n in nets):
            raise ValueError('the maps of one shared FRAP must have one demand_shape, got %s' % [n.demand_shape for n in nets])
        self.gamma, self.lr, self.adam_eps = float(gamma), float(lr), 1e-8
        self.batch_size, self.target_update, self.seed = int(batch_size), int(target_update), int(seed) & 0xFFFFFFFF
        self.t = 0              # env-steps seen (one per lock-step of all maps)
        shapes = [tuple(p.shape) for p in nets[0].parameters()]
        for n in nets:
            assert [k for k, _ in n.named_parameters()] == list(n.state_dict().keys()), 'the packed layout is the state_dict order'
            assert [tuple(p.shape) for p in n.parameters()] == shapes
            for p in n.parameters():
                if not (p.is_cuda and p.dtype == torch.float32):
                    raise RuntimeError('MultiMapMPLightLearner needs float32 device parameters: the update is a HIP kernel (there is no CPU fallback)')
        self.device = next(nets[0].parameters()).device
        n_par = sum(p.numel() for p in nets[0].parameters())
        self.flat, self.flat_target, self._g, self._m, self._v = (torch.zeros(n_par, dtype=torch.float32, device=self.device) for _ in range(5))
        with torch.no_grad():
            self.flat.copy_(torch.cat([p.detach().reshape(-1) for p in nets[0].parameters()]))
            for n in nets:
                for p, view in zip(n.parameters(), _views(self.flat, n).values()):
                    p.data = view                   # every map's parameter now IS its slice of the one packed vector
            self.flat_target.copy_(self.flat)
        with torch.random.fork_rng(devices=[]):     # (the constructor's initial draws are overwritten: they must not move the caller's generator)
            self.target = FRAP(nets[0].oshape, nets[0].phase_pairs, D).to(self.device)
        for p, view in zip(self.target.parameters(), _views(self.flat_target, self.target).values()):
            p.data = view
            p.requires_grad_(False)
        self.grads, self.m, self.v = _views(self._g, nets[0]), _views(self._m, nets[0]), _views(self._v, nets[0])
        self.loss_out = torch.zeros((), dtype=torch.float32, device=self.device)
        self.counts = (C.c_int32 * len(nets))()     # the group sizes of the last sample()
        self._create()

    def _create(self):
        """The handle: rs_mplight_multi_create(device, D, n_maps, maps, cfg, the five flat vectors, batch_size, &handle)."""
        self._lib = load_library()
        if not hasattr(self._lib, 'rs_mplight_multi_create'):
            raise RuntimeError('the loaded library has no rs_mplight_multi_create: rebuild it (there is no CPU fallback)')
        tables = [(C.c_int32 * (2 * n.oshape))(*[m for p in n.phase_pairs for m in p]) for n in self.nets]
        maps = (MPLightMap * len(self.nets))(*[MPLightMap(n.oshape, C.addressof(t), s) for n, t, s in zip(self.nets, tables, self.n_signals)])
        cfg = DQNConfig(self.lr, self.adam_eps, 0.9, 0.999, self.gamma)
        h = C.c_void_p()
        torch.cuda.synchronize(self.device)
        rc = self._lib.rs_mplight_multi_create(self.device.index or 0, self.nets[0].demand_shape, len(self.nets), maps, C.byref(cfg), self.flat.data_ptr(),
                                               self.flat_target.data_ptr(), self._g.data_ptr(), self._m.data_ptr(), self._v.data_ptr(), self.batch_size,
                                               C.byref(h))
        if rc != 0:
            self._fail('rs_mplight_multi_create', rc)
        self._h = h
        self._set_target_options()

    def _rings(self, replays):
        """rs_mplight_ring [n_maps] over the MPLightReplays' own arrays (no copies) at their present positions"""
        replays = list(replays)
        if len(replays) != len(self.nets):
            raise ValueError('%d replay rings for %d maps' % (len(replays), len(self.nets)))
        if self._h is None:
            raise RuntimeError('MultiMapMPLightLearner is closed')
        W = 1 + 12 * self.nets[0].demand_shape
        rings = (MPLightRing * len(replays))()
        for k, rp in enumerate(replays):
            for a in (rp.obs, rp.act, rp.rew, rp.done):
                if not a.is_cuda:
                    raise RuntimeError('MultiMapMPLightLearner needs the replay rings on the device: the update is a HIP kernel (there is no CPU fallback)')
                assert a.is_contiguous()
            assert rp.obs.dtype == torch.float32 and tuple(rp.obs.shape) == (rp.T, rp.N, rp.S, W), 'obs must be f32 [T, N, S, 1 + 12 D]'
            assert rp.act.dtype == torch.int16 and rp.rew.dtype == torch.float32 and rp.done.dtype == torch.bool
            rings[k] = MPLightRing(rp.obs.data_ptr(), rp.act.data_ptr(), rp.rew.data_ptr(), rp.done.data_ptr(), rp.T, rp.N, rp.S, W, rp.head, rp.count)
        self._keep = (replays, rings)
        return rings

    # ---- the pieces (what the tests compare one by one) and the update
    def sample(self, replays, batch_size=None, update_key=None):
        """The minibatch the next update would draw -> (idx: int32 device tensor [B, 4] of (map, slot, environment, signal), grouped by
        map, and the group sizes: a list of n_maps ints, computed on the host).  update_key: the Adam steps so far unless given."""
        B = self.batch_size if batch_size is None else int(batch_size)
        rings = self._rings(replays)
        idx = torch.empty(max(B, 0), 4, dtype=torch.int32, device=self.device)
        key = self.n_updates if update_key is None else int(update_key)
        rc = self._lib.rs_mplight_multi_sample(self._h, rings, B, self.seed, key & 0xFFFFFFFF, idx.data_ptr(), self.counts, torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_mplight_multi_sample', rc)
        return idx, list(self.counts)

    def grad(self, replays, idx, counts):
        """The gradient of the grouped minibatch idx (device tensor [B, 4]; counts: the group sizes, sum B) into .grads and the mean
        Huber loss over all B rows into .loss_out."""
        if not idx.is_cuda:
            raise RuntimeError('MultiMapMPLightLearner.grad needs a device index tensor (there is no CPU fallback)')
        assert idx.dim() == 2 and idx.shape[1] == 4
        idx32 = idx.to(torch.int32).contiguous()
        rings = self._rings(replays)
        self._keep += (idx32,)
        cnt = (C.c_int32 * len(self.nets))(*[int(c) for c in counts])
        rc = self._lib.rs_mplight_multi_grad(self._h, rings, idx32.data_ptr(), cnt, idx32.shape[0], self.loss_out.data_ptr(), torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_mplight_multi_grad', rc)
        return self.grads

    def update(self, replays, updates=1):
        """`updates` times [sample -> gradient -> Adam step], enqueued by one call.  Returns .loss_out (the last update's)."""
        rings = self._rings(replays)
        rc = self._lib.rs_mplight_multi_update(self._h, rings, self.batch_size, self.seed, int(updates), self.loss_out.data_ptr(),
                                               torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_mplight_multi_update', rc)
        return self.loss_out

    def sync_target(self):
        """target <- parameters: one copy kernel on the vector the library reads"""
        rc = self._lib.rs_mplight_multi_sync_target(self._h, torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_mplight_multi_sync_target', rc)

    # ---- checkpoints (resco_amd/checkpoint.py): the vectors are loaded in place, the step count through rs_mplight_multi_set_steps
    def signature(self):
        fields = {'batch': self.batch_size, 'target_update': self.target_update, 'gamma': self.gamma, 'demand_shape': int(self.nets[0].demand_shape),
                  'n_pairs': [int(n.oshape) for n in self.nets], 'n_signals': list(self.n_signals)}
        return target_options_signature(fields, self.n_step, self.double_q)

    def state_dict(self):
        return {'weights': {'flat': self.flat, 'flat_target': self.flat_target},
                'state': {'m': self._m, 'v': self._v, 't': int(self.t), 'steps': _state.fused_counter_state(self), 'seed': int(self.seed)}}

    def load_state_dict(self, sd, weights_only=False):
        _state.copy_into(self.flat, sd['weights']['flat'], 'MultiMapMPLightLearner.flat')
        _state.copy_into(self.flat_target, sd['weights']['flat_target'], 'MultiMapMPLightLearner.flat_target')
        if not weights_only:
            st = sd['state']
            _state.copy_into(self._m, st['m'], 'MultiMapMPLightLearner.m')
            _state.copy_into(self._v, st['v'], 'MultiMapMPLightLearner.v')
            _state.set_fused_counter(self, st['steps'], 'MultiMapMPLightLearner')
            self.t, self.seed = int(st['t']), int(st['seed']) & 0xFFFFFFFF

    def observe_step(self, replays):
        """One lock-step of all maps: count it, copy the target every ``target_update`` steps, then one update once the rings together
        hold a minibatch.  len(ring) counts transitions, (count - 1) N S, not slots: the sum is the library's `total`, so a sum of at
        least batch_size >= 1 means some ring has count >= 2 and the update is never refused for total == 0.  Returns .loss_out after
        an update, else None."""
        self.t += 1
        if self.t % self.target_update == 0:
            self.sync_target()
        if sum(len(rp) for rp in replays) >= self.batch_size:
            return self.update(replays)
        return None
