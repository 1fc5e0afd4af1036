"""MPLight's shared-DQN update on the device (include/resco_sim.h: rs_mplight_dqn_create / _sample / _grad / _step / _update;
resco_amd/csrc/resco_frap_train.h).

`FusedMPLightLearner(net)` does what `MPLightLearner` does per update -- MPLightReplay.sample, loss(), its backward through the ONE
shared FRAP network, torch.optim.Adam -- in HIP kernels, the replay ring read in place (the gradient is evaluated in double and rounded to fp32 once;
parameters, moments and the Adam step are fp32).  It owns five flat float32
device vectors in the packed layout of rs_mplight_create (parameters, target, gradients, Adam moments) and re-points every parameter
of `net` at its view of the parameter vector, in state_dict order: `net` stays the source of truth (state_dict(), load_state_dict()
and FusedMPLight.refresh_on_device() work unchanged), and the packed vector IS the parameters -- a policy bound to it once
(FusedMPLight.share_weights(learner.flat)) acts on the updated weights with no re-pack per step.  `.target` is a FRAP whose
parameters view the second vector (sync_target() is one device copy); `.grads`, `.m`, `.v` are name -> view dicts.  The library
owns only its workspace and the step counter (the handle's life cycle, .n_updates and .step() are learn_fused.FusedLearnerBase's).
The handle is created over the ring's signal count: at construction when `n_signals` is given, else at the first call that sees a
ring.  The minibatches come from the library's counter hash, not from a torch generator: the distribution is MPLightReplay.sample's,
the draws are not.  There is no CPU fallback.

`per=dict(alpha, beta0, beta_steps, eps)` turns prioritised experience replay on (rs_mplight_dqn_set_priorities;
resco_amd/csrc/resco_frap_per.h): the draw is by priority over the pooled rows (slot, environment, signal), the loss carries the
importance weights, and every update writes the rows' new priorities back.  The priorities (`.prio` [T, N, S], `.esum` [T, N], `.ssum`
[T], `.pmax` [1]) are torch tensors this object owns, sized from the replay ring at first use (`attach`).
"""
import ctypes as C

import torch

from ..sim import DQNConfig, MPLightPer, MPLightRing, load_library, torch_stream
from . import _state
from .idqn_learn import per_options, per_options_signature, target_options_signature
from .learn_fused import FusedLearnerBase
from .mplight import FRAP


def _views(flat, net):
    """name -> view of `flat` for every parameter of net, in state_dict order"""
    out, off = {}, 0
    for k, p in net.named_parameters():
        out[k] = flat[off:off + p.numel()].view(p.shape)
        off += p.numel()
    assert off == flat.numel(), (off, flat.numel())
    return out


class FusedMPLightLearner(FusedLearnerBase):
    NAME, PREFIX = 'FusedMPLightLearner', 'rs_mplight_dqn'
    STATE_FOLLOWS_REPLAY = True         # resco_amd/checkpoint.py: state_dict(replay=...) -- the priorities are saved with the ring only

    def __init__(self, net, gamma=0.99, lr=1e-3, target_update=500, batch_size=32, seed=0, n_signals=None, n_step=1, double_q=False, per=None):
        """n_step (1 .. 32): n-step returns, truncated at the newest slot of the ring and cut at an episode end; double_q: the
        bootstrap is the target network's value of the online network's best of ALL P outputs (rs_mplight_dqn_set_target has the
        definition).  per: None, or the options of prioritised replay, any of dict(alpha=0.6, beta0=0.4, beta_steps=0, eps=1e-6)
        (rs_mplight_dqn_set_priorities has the definition).  The defaults are PFRL's plain one-step DQN with uniform replay."""
        assert isinstance(net, FRAP)
        super().__init__(net)
        self._take_target_options(n_step, double_q)
        self.per = per_options(per, self.NAME)
        self.prio = self.esum = self.ssum = self.pmax = None
        self.gamma, self.lr, self.adam_eps = float(gamma), float(lr), 1e-8
        self.batch_size, self.target_update, self.seed = int(batch_size), int(target_update), int(seed) & 0xFFFFFFFF
        self.t = 0              # env-steps seen
        params = list(net.parameters())
        assert [k for k, _ in net.named_parameters()] == list(net.state_dict().keys()), 'the packed layout is the state_dict order'
        for p in params:
            if not (p.is_cuda and p.dtype == torch.float32):
                raise RuntimeError('FusedMPLightLearner needs contiguous float32 device parameters: the update is a HIP kernel (there is no CPU fallback)')
        self.device = params[0].device
        n = sum(p.numel() for p in params)
        self.flat, self.flat_target, self._g, self._m, self._v = (torch.zeros(n, dtype=torch.float32, device=self.device) for _ in range(5))
        with torch.no_grad():
            self.flat.copy_(torch.cat([p.detach().reshape(-1) for p in params]))
            for p, view in zip(params, _views(self.flat, net).values()):
                p.data = view                       # the parameter now IS its slice of the packed vector
            self.flat_target.copy_(self.flat)
        # the target: a FRAP of the same shape whose parameters view the second vector (no deepcopy of a net of views)
        with torch.random.fork_rng(devices=[]):     # (the constructor's initial draws are overwritten: they must not move the caller's generator)
            self.target = FRAP(net.oshape, net.phase_pairs, net.demand_shape).to(self.device)
        for p, view in zip(self.target.parameters(), _views(self.flat_target, self.target).values()):
            p.data = view
            p.requires_grad_(False)
        self.grads, self.m, self.v = _views(self._g, net), _views(self._m, net), _views(self._v, net)
        self.loss_out = torch.zeros((), dtype=torch.float32, device=self.device)
        self.n_signals = None
        if n_signals is not None:
            self._create(int(n_signals))

    def _create(self, n_signals):
        """The handle: rs_mplight_dqn_create(device, D, P, pairs, S, cfg, the five flat vectors, batch_size, &handle)."""
        self._lib = load_library()
        if not hasattr(self._lib, 'rs_mplight_dqn_create'):
            raise RuntimeError('the loaded library has no rs_mplight_dqn_create: rebuild it (there is no CPU fallback)')
        net = self.net
        pairs = (C.c_int32 * (2 * net.oshape))(*[m for p in net.phase_pairs for m in p])
        cfg = DQNConfig(self.lr, self.adam_eps, 0.9, 0.999, self.gamma)
        h = C.c_void_p()
        torch.cuda.synchronize(self.device)
        rc = self._lib.rs_mplight_dqn_create(self.device.index or 0, net.demand_shape, net.oshape, pairs, n_signals, C.byref(cfg), self.flat.data_ptr(),
                                             self.flat_target.data_ptr(), self._g.data_ptr(), self._m.data_ptr(), self._v.data_ptr(), self.batch_size,
                                             C.byref(h))
        if rc != 0:
            self._fail('rs_mplight_dqn_create', rc)
        self._h, self.n_signals = h, n_signals
        self._set_target_options()

    def _need_handle(self):
        if self._h is None:
            raise RuntimeError('FusedMPLightLearner has no handle yet: it is created over the first replay ring it sees (or pass n_signals)')

    def _ring(self, replay):
        """rs_mplight_ring over an MPLightReplay's own arrays (no copies) at its present position"""
        W = 1 + 12 * self.net.demand_shape
        for a in (replay.obs, replay.act, replay.rew, replay.done):
            if not a.is_cuda:
                raise RuntimeError('FusedMPLightLearner needs the replay ring on the device: the update is a HIP kernel (there is no CPU fallback)')
            assert a.is_contiguous()
        assert replay.obs.dtype == torch.float32 and tuple(replay.obs.shape) == (replay.T, replay.N, replay.S, W), 'obs must be f32 [T, N, S, 1 + 12 D]'
        assert replay.act.dtype == torch.int16 and replay.rew.dtype == torch.float32 and replay.done.dtype == torch.bool
        if self._h is None:
            self._create(replay.S)
        ring = MPLightRing(replay.obs.data_ptr(), replay.act.data_ptr(), replay.rew.data_ptr(), replay.done.data_ptr(), replay.T, replay.N, replay.S, W,
                           replay.head, replay.count)
        self._keep = (replay, ring)
        if self.per is not None:
            self.attach(replay)
        return ring

    # ---- prioritised replay
    def attach(self, replay):
        """The priorities of `replay`, at first use: every leaf at pmax = 1, the sums rebuilt; the handle borrows the four tensors.
        Every call that takes the replay comes through here; call it yourself before a checkpoint is loaded into a learner that
        has not seen its replay yet."""
        if self.per is None:
            return
        if self.prio is not None:
            if tuple(self.prio.shape) != (replay.T, replay.N, replay.S):
                raise ValueError('FusedMPLightLearner: the priorities were sized for a ring of %s, not %s' % (tuple(self.prio.shape), (replay.T, replay.N, replay.S)))
            return
        if self._h is None:
            self._create(replay.S)
        if not hasattr(self._lib, 'rs_mplight_dqn_set_priorities'):
            raise RuntimeError('the loaded library has no rs_mplight_dqn_set_priorities: rebuild it (there is no CPU fallback)')
        T, N, S = replay.T, replay.N, replay.S
        self.prio = torch.ones(T, N, S, dtype=torch.float32, device=self.device)
        self.esum = torch.zeros(T, N, dtype=torch.float32, device=self.device)
        self.ssum = torch.zeros(T, dtype=torch.float32, device=self.device)
        self.pmax = torch.ones(1, dtype=torch.float32, device=self.device)
        o = self.per
        per = MPLightPer(self.prio.data_ptr(), self.esum.data_ptr(), self.ssum.data_ptr(), self.pmax.data_ptr(), T, N, S, o['alpha'], o['beta0'], o['eps'],
                         o['beta_steps'])
        rc = self._lib.rs_mplight_dqn_set_priorities(self._h, C.byref(per))
        if rc != 0:
            self.prio = self.esum = self.ssum = self.pmax = None
            self._fail('rs_mplight_dqn_set_priorities', rc)
        self.per_rebuild()

    def _per_call(self, name, *args):
        rc = getattr(self._lib, name)(self._h, *args, torch_stream(self.device.index))
        if rc != 0:
            self._fail(name, rc)

    def per_rebuild(self):
        """esum <- the sums of prio, ssum <- the sums of esum (rs_mplight_dqn_per_rebuild)"""
        self._per_call('rs_mplight_dqn_per_rebuild')

    def per_fill(self, slot):
        """the transitions of `slot` enter at the maximum priority (rs_mplight_dqn_per_fill)"""
        self._per_call('rs_mplight_dqn_per_fill', int(slot))

    def per_commit(self, replay, idx):
        """the priorities of the rows idx of the last grad() <- their |delta| (rs_mplight_dqn_per_commit)"""
        idx32 = idx.to(torch.int32).contiguous()
        ring = self._ring(replay)
        self._keep += (idx32,)
        self._per_call('rs_mplight_dqn_per_commit', C.byref(ring), idx32.data_ptr(), idx32.shape[0])

    # ---- the pieces (what the tests compare one by one) and the update
    def sample(self, replay, batch_size=None, update_key=None):
        """The minibatch the next update would draw: int32 device tensor [B, 3] of (slot, environment, signal).
        update_key: the number of Adam steps taken so far unless given."""
        B = self.batch_size if batch_size is None else int(batch_size)
        ring = self._ring(replay)
        idx = torch.empty(max(B, 0), 3, dtype=torch.int32, device=self.device)
        key = self.n_updates if update_key is None else int(update_key)
        rc = self._lib.rs_mplight_dqn_sample(self._h, C.byref(ring), B, self.seed, key & 0xFFFFFFFF, idx.data_ptr(), torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_mplight_dqn_sample', rc)
        return idx

    def grad(self, replay, idx):
        """The gradient of the minibatch idx (integer device tensor [B, 3]: slot, environment, signal) into .grads and the mean Huber
        loss into .loss_out."""
        if not idx.is_cuda:
            raise RuntimeError('FusedMPLightLearner.grad needs a device index tensor (there is no CPU fallback)')
        assert idx.dim() == 2 and idx.shape[1] == 3
        idx32 = idx.to(torch.int32).contiguous()
        ring = self._ring(replay)
        self._keep += (idx32,)
        rc = self._lib.rs_mplight_dqn_grad(self._h, C.byref(ring), idx32.data_ptr(), idx32.shape[0], self.loss_out.data_ptr(), torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_mplight_dqn_grad', rc)
        return self.grads

    def update(self, replay, updates=1):
        """`updates` times [sample -> gradient -> Adam step (-> commit of the priorities)], enqueued by one call.  Returns .loss_out (the last update's)."""
        ring = self._ring(replay)
        rc = self._lib.rs_mplight_dqn_update(self._h, C.byref(ring), self.batch_size, self.seed, int(updates), self.loss_out.data_ptr(),
                                             torch_stream(self.device.index))
        if rc != 0:
            self._fail('rs_mplight_dqn_update', rc)
        return self.loss_out

    @torch.no_grad()
    def sync_target(self):
        """target <- parameters: one device-to-device copy into the vector the library reads"""
        self.flat_target.copy_(self.flat)

    # ---- checkpoints (resco_amd/checkpoint.py): the four flat vectors are loaded in place -- the library has borrowed them, the
    # parameters of net and target are views of them and a policy may share .flat --; the step count goes back through
    # rs_mplight_dqn_set_steps, so the handle has to exist (pass n_signals, or show the learner its ring first)
    _ATTACH_FIRST = ('FusedMPLightLearner: the priorities are sized from the replay ring at first use: call attach(replay) before '
                     'a checkpoint with the ring is written or loaded')

    def signature(self):
        fields = target_options_signature({'batch': self.batch_size, 'target_update': self.target_update, 'gamma': self.gamma}, self.n_step, self.double_q)
        return per_options_signature(fields, self.per)

    def state_dict(self, replay=True):
        """replay: the checkpoint holds the ring, and with it prio and pmax (the sums are rebuilt from them on load)"""
        sd = {'weights': {'flat': self.flat, 'flat_target': self.flat_target},
              'state': {'m': self._m, 'v': self._v, 't': int(self.t), 'steps': _state.fused_counter_state(self), 'seed': int(self.seed)}}
        if self.per is not None and replay:
            if self.prio is None:
                raise RuntimeError(self._ATTACH_FIRST)
            sd['state']['per'] = {'prio': self.prio, 'pmax': self.pmax}
        return sd

    def load_state_dict(self, sd, weights_only=False):
        _state.copy_into(self.flat, sd['weights']['flat'], 'FusedMPLightLearner.flat')
        _state.copy_into(self.flat_target, sd['weights']['flat_target'], 'FusedMPLightLearner.flat_target')
        if not weights_only:
            st = sd['state']
            _state.copy_into(self._m, st['m'], 'FusedMPLightLearner.m')
            _state.copy_into(self._v, st['v'], 'FusedMPLightLearner.v')
            _state.set_fused_counter(self, st['steps'], 'FusedMPLightLearner')
            self.t, self.seed = int(st['t']), int(st['seed']) & 0xFFFFFFFF
            if self.per is not None and 'per' in st:
                if self.prio is None:
                    raise RuntimeError(self._ATTACH_FIRST)
                _state.copy_into(self.prio, st['per']['prio'], 'FusedMPLightLearner.prio')
                _state.copy_into(self.pmax, st['per']['pmax'], 'FusedMPLightLearner.pmax')
                self.per_rebuild()
            elif self.per is not None:
                print('FusedMPLightLearner: the checkpoint holds no replay ring, so the priorities start again (every transition at priority 1)')
                if self.prio is not None:
                    self.prio.fill_(1.0)
                    self.pmax.fill_(1.0)
                    self.per_rebuild()

    def observe_step(self, replay, generator=None):
        """One env-step in MPLightLearner.observe_step's order: count it, copy the target every ``target_update`` env-steps, then one
        update once the ring holds a minibatch.  `generator` is ignored: the minibatches are drawn by the library's counter hash from
        (seed, Adam steps so far).  Returns .loss_out after an update, else None."""
        self.t += 1
        if self.per is not None:
            self.attach(replay)
            self.per_fill((replay.head - 1) % replay.T)     # the slot just committed enters at the maximum priority
        if self.t % self.target_update == 0:
            self.sync_target()
        if len(replay) >= self.batch_size:
            return self.update(replay)
        return None
