"""The DQN update of a BatchedIDQN on the device (include/resco_sim.h: rs_dqn_create / rs_dqn_sample / rs_dqn_grad / rs_dqn_step /
rs_dqn_update; resco_amd/csrc/resco_dqn_train.h).

`FusedDQNLearner(net)` does what `BatchedDQNLearner` does per update -- DeviceReplay.sample, loss(), its backward through the S
stacked Q-networks, torch.optim.Adam -- in HIP kernels, all in fp32, every signal at its own lane and action count, the replay ring
read in place.  All updates of an agent step are ONE call through the ABI.  The network's own parameter storages are updated in
place: `net` stays the source of truth, `FusedIDQN.refresh_on_device()` and `state_dict()` work unchanged.  Gradients, Adam moments
and the target network are torch tensors this object owns (`.grads`, `.m`, `.v`: name -> tensor; `.target`: a BatchedIDQN); the
library owns only its workspace and the step counter (the handle's life cycle, .n_updates and .step() are
learn_fused.FusedLearnerBase's).  The minibatches come from the library's counter hash, not from a torch generator: the distribution
is DeviceReplay.sample's, the draws are not.  There is no CPU fallback.

`per=dict(alpha, beta0, beta_steps, eps)` turns prioritised experience replay on (rs_dqn_set_priorities; resco_amd/csrc/resco_dqn_per.h):
the draw is by priority, the loss carries the importance weights, and every update writes the rows' new priorities back.  The
priorities (`.prio` [T, N, S], `.ssum` [T, S], `.pmax` [S]) are torch tensors this object owns, sized from the replay ring at first
use (`attach`).
"""
import copy
import ctypes as C

import torch

from ..sim import DQN_TENSORS, DQNConfig, DQNPer, DQNRing, DQNTensors, torch_stream
from . import _state
from .idqn_learn import per_options, per_options_signature, target_options_signature
from .idqn_rollout import BatchedIDQN
from .learn_fused import FusedLearnerBase


class FusedDQNLearner(FusedLearnerBase):
    NAME, PREFIX, TENSORS, TENSOR_SET = 'FusedDQNLearner', 'rs_dqn', DQN_TENSORS, DQNTensors
    STATE_FOLLOWS_REPLAY = True         # resco_amd/checkpoint.py: state_dict(replay=...) -- the priorities are saved with the ring only

    def __init__(self, net, gamma=0.99, lr=1e-3, target_update=500, batch_size=32, seed=0, n_step=1, double_q=False, per=None):
        """n_step (1 .. 32): n-step returns, truncated at the newest slot of the ring and cut at an episode end; double_q: the
        bootstrap is the target network's value of the online network's best action (rs_dqn_set_target has the definition).  per:
        None, or the options of prioritised replay, any of dict(alpha=0.6, beta0=0.4, beta_steps=0, eps=1e-6) (rs_dqn_set_priorities
        has the definition).  The defaults are PFRL's plain one-step DQN with uniform replay."""
        assert isinstance(net, BatchedIDQN)
        super().__init__(net)
        self._take_target_options(n_step, double_q)
        self.per = per_options(per, self.NAME)
        self.prio = self.ssum = self.pmax = None
        self.gamma, self.lr, self.adam_eps = float(gamma), float(lr), 1e-8
        self.batch_size, self.target_update, self.seed = int(batch_size), int(target_update), int(seed) & 0xFFFFFFFF
        self.t = 0              # agent steps seen (PFRL's self.t)
        self.target = copy.deepcopy(net)
        for p in self.target.parameters():
            p.requires_grad_(False)
        self._create(DQNConfig(self.lr, self.adam_eps, 0.9, 0.999, self.gamma), self.batch_size, more_nets=(self.target,))     # (a CPU net raises)
        self._set_target_options()

    def _ring(self, replay):
        """rs_dqn_ring over a DeviceReplay's own arrays (no copies) at its present position"""
        S, lmax = len(self.net.lanes), self.net.lmax
        for a in (replay.obs, replay.act, replay.rew, replay.done):
            if not a.is_cuda:
                raise RuntimeError('FusedDQNLearner needs the replay ring on the device: the update is a HIP kernel (there is no CPU fallback)')
            assert a.is_contiguous()
        assert replay.obs.dtype == torch.float16 and tuple(replay.obs.shape) == (replay.T, replay.N, S, lmax, 5), 'obs must be f16 [T, N, S, lmax, 5]'
        assert replay.act.dtype == torch.int16 and replay.rew.dtype == torch.float32 and replay.done.dtype == torch.bool
        ring = DQNRing(replay.obs.data_ptr(), replay.act.data_ptr(), replay.rew.data_ptr(), replay.done.data_ptr(), replay.T, replay.N,
                       replay.head, replay.count)
        self._keep = (replay, ring)
        if self.per is not None:
            self.attach(replay)
        return ring

    # ---- prioritised replay
    def attach(self, replay):
        """The priorities of `replay`, at first use: prio = 1 in the slots written so far and 0 elsewhere, pmax = 1, the sums rebuilt;
        the handle borrows the three tensors.  Every call that takes the replay comes through here; call it yourself before a
        checkpoint is loaded into a learner that has not seen its replay yet."""
        if self.per is None:
            return
        if self.prio is not None:
            if tuple(self.prio.shape[:2]) != (replay.T, replay.N):
                raise ValueError('FusedDQNLearner: the priorities were sized for a ring of %s, not %s' % (tuple(self.prio.shape[:2]), (replay.T, replay.N)))
            return
        if not hasattr(self._lib, 'rs_dqn_set_priorities'):
            raise RuntimeError('the loaded library has no rs_dqn_set_priorities: rebuild it (there is no CPU fallback)')
        T, N, S = replay.T, replay.N, len(self.net.lanes)
        self.prio = torch.zeros(T, N, S, dtype=torch.float32, device=self.device)
        self.ssum = torch.zeros(T, S, dtype=torch.float32, device=self.device)
        self.pmax = torch.ones(S, dtype=torch.float32, device=self.device)
        written = [(replay.head - replay.count + k) % T for k in range(replay.count)]
        if written:
            self.prio[written] = 1.0
        o = self.per
        per = DQNPer(self.prio.data_ptr(), self.ssum.data_ptr(), self.pmax.data_ptr(), T, N, o['alpha'], o['beta0'], o['eps'], o['beta_steps'])
        rc = self._lib.rs_dqn_set_priorities(self._h, C.byref(per))
        if rc != 0:
            self.prio = self.ssum = self.pmax = None
            self._fail('rs_dqn_set_priorities', rc)
        self.rebuild_priorities()

    def _per_call(self, name, *args):
        rc = getattr(self._lib, name)(self._h, *args, torch_stream(self.device.index))
        if rc != 0:
            self._fail(name, rc)

    def rebuild_priorities(self):
        """ssum <- the sums of prio (rs_dqn_per_rebuild)"""
        self._per_call('rs_dqn_per_rebuild')

    def fill_priorities(self, slot):
        """the transitions of `slot` enter at the maximum priority (rs_dqn_per_fill)"""
        self._per_call('rs_dqn_per_fill', int(slot))

    def commit_priorities(self, replay, idx):
        """the priorities of the rows idx of the last grad() <- their |delta| (rs_dqn_per_commit)"""
        idx32 = idx.to(torch.int32).contiguous()
        ring = self._ring(replay)
        self._keep += (idx32,)
        self._per_call('rs_dqn_per_commit', C.byref(ring), idx32.data_ptr(), idx32.shape[0])

    # ---- the pieces (what the tests compare one by one) and the update
    def sample(self, replay, batch_size=None, update_key=None):
        """The minibatch the next update would draw: int32 device tensor [B, S, 2] of (slot, environment) per signal.
        update_key: the number of Adam steps taken so far unless given."""
        B = self.batch_size if batch_size is None else int(batch_size)
        idx = torch.empty(max(B, 0), len(self.net.lanes), 2, dtype=torch.int32, device=self.device)
        key = self.n_updates if update_key is None else int(update_key)
        rc = self._lib.rs_dqn_sample(self._h, C.byref(self._ring(replay)), B, self.seed, key & 0xFFFFFFFF, idx.data_ptr(), torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_dqn_sample', rc)
        return idx

    def grad(self, replay, idx):
        """The gradient of the minibatch idx (integer device tensor [B, S, 2]: slot, environment) into .grads and the mean Huber loss
        of every signal into .loss_out [S]."""
        if not idx.is_cuda:
            raise RuntimeError('FusedDQNLearner.grad needs a device index tensor (there is no CPU fallback)')
        assert idx.dim() == 3 and idx.shape[1] == len(self.net.lanes) and idx.shape[2] == 2
        idx32 = idx.to(torch.int32).contiguous()
        ring = self._ring(replay)
        self._keep += (idx32,)
        rc = self._lib.rs_dqn_grad(self._h, C.byref(ring), idx32.data_ptr(), idx32.shape[0], self.loss_out.data_ptr(), torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_dqn_grad', rc)
        return self.grads

    def update(self, replay, updates=1):
        """`updates` times [sample -> gradient -> Adam step (-> commit of the priorities)], enqueued by one call.  Returns .loss_out
        (the last update's)."""
        rc = self._lib.rs_dqn_update(self._h, C.byref(self._ring(replay)), self.batch_size, self.seed, int(updates), self.loss_out.data_ptr(),
                                     torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_dqn_update', rc)
        return self.loss_out

    @torch.no_grad()
    def sync_target(self):
        """target <- parameters: device-to-device copies into the storages the library reads"""
        for k in DQN_TENSORS:
            getattr(self.target, k).copy_(getattr(self.net, k))

    # ---- checkpoints (resco_amd/checkpoint.py): in place, the library has borrowed target, m and v; its step count goes back
    # through rs_dqn_set_steps (the bias correction's t and the key of the next minibatch draw)
    def signature(self):
        fields = target_options_signature({'batch': self.batch_size, 'target_update': self.target_update, 'gamma': self.gamma}, self.n_step, self.double_q)
        return per_options_signature(fields, self.per)

    def state_dict(self, replay=True):
        """replay: the checkpoint holds the ring, and with it prio and pmax (ssum is rebuilt from them on load)"""
        sd = {'weights': {'target': _state.module_tensors(self.target)},
              'state': {'m': dict(self.m), 'v': dict(self.v), 't': int(self.t), 'steps': _state.fused_counter_state(self), 'seed': int(self.seed)}}
        if self.per is not None and replay:
            if self.prio is None:
                raise RuntimeError('FusedDQNLearner: the priorities are sized from the replay ring at first use: call attach(replay) before '
                                   'a checkpoint with the ring is written or loaded')
            sd['state']['per'] = {'prio': self.prio, 'pmax': self.pmax}
        return sd

    def load_state_dict(self, sd, weights_only=False):
        _state.load_module(self.target, sd['weights']['target'], 'FusedDQNLearner.target')
        if not weights_only:
            st = sd['state']
            _state.copy_dict_into(self.m, st['m'], 'FusedDQNLearner.m')
            _state.copy_dict_into(self.v, st['v'], 'FusedDQNLearner.v')
            _state.set_fused_counter(self, st['steps'], 'FusedDQNLearner')
            self.t, self.seed = int(st['t']), int(st['seed']) & 0xFFFFFFFF
            if self.per is not None and 'per' in st:
                if self.prio is None:
                    raise RuntimeError('FusedDQNLearner: the priorities are sized from the replay ring at first use: call attach(replay) before '
                                       'a checkpoint with the ring is written or loaded')
                _state.copy_into(self.prio, st['per']['prio'], 'FusedDQNLearner.prio')
                _state.copy_into(self.pmax, st['per']['pmax'], 'FusedDQNLearner.pmax')
                self.rebuild_priorities()
            elif self.per is not None:
                print('FusedDQNLearner: the checkpoint holds no replay ring, so the priorities start again (every new transition at priority 1)')
                if self.prio is not None:
                    self.prio.zero_()
                    self.ssum.zero_()
                    self.pmax.fill_(1.0)

    def observe_step(self, replay, generator=None, updates=1):
        """One agent step of PFRL's DQN.observe(), in BatchedDQNLearner.observe_step's order: count it, copy the target network every
        ``target_update`` steps, then update once the ring holds a minibatch.  `generator` is ignored: the minibatches are drawn by
        the library's counter hash from (seed, Adam steps so far).  Returns .loss_out [S] after an update, else None."""
        self.t += 1
        if self.per is not None:
            self.attach(replay)
            self.fill_priorities((replay.head - 1) % replay.T)      # the slot just committed enters at the maximum priority
        if self.t % self.target_update == 0:
            self.sync_target()
        if len(replay) >= self.batch_size and updates >= 1:     # (no update asked for: nothing happens, as in BatchedDQNLearner's loop)
            return self.update(replay, updates)
        return None
