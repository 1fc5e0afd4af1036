"""What the fused learners share (idqn_learn_fused.FusedDQNLearner: rs_dqn_*, ippo_learn_fused.FusedPPOLearner: rs_ppo_*): the
library handle and its life cycle.  A handle is created over the network's own parameter storages and over gradients and Adam
moments that are torch tensors the learner owns (`.grads`, `.m`, `.v`: name -> tensor); the library owns only its workspace and the
step counter.  There is no CPU fallback.
"""
import ctypes as C

import torch

from ..sim import load_library, torch_stream


class FusedLearnerBase:
    NAME = None             # the learner's class name as its error texts give it
    PREFIX = None           # 'rs_dqn' / 'rs_ppo': the symbols are PREFIX_create, _step, _steps, _set_steps, _destroy
    TENSORS = None          # names of the parameters, in the order of the fields of
    TENSOR_SET = None       # the ctypes struct of one set of device pointers
    LOSS_SHAPE = ()         # .loss_out is float32 [S, *LOSS_SHAPE]
    SET_TARGET = None       # the DQN learners' setter of the target's options; None: PREFIX_set_target

    def __init__(self, net):
        self.net = net
        self._lib, self._h, self._keep = None, None, None
        self.grads = self.m = self.v = self.loss_out = None

    def _create(self, cfg, max_batch, more_nets=()):
        """The handle: PREFIX_create(device, S, lmax, lanes, actions, amax, cfg, the tensor sets of net, of `more_nets`, of .grads,
        .m and .v, max_batch, &handle)."""
        net = self.net
        for k in self.TENSORS:
            p = getattr(net, k)
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError('%s needs contiguous float32 device parameters: the update is a HIP kernel (there is no CPU fallback)' % self.NAME)
        self._lib = load_library()
        if not hasattr(self._lib, self.PREFIX + '_create'):
            raise RuntimeError('the loaded library has no %s_create: rebuild it (there is no CPU fallback)' % self.PREFIX)
        self.device = net.fc1_w.device
        S = len(net.lanes)
        zeros = lambda: {k: torch.zeros_like(getattr(net, k).detach()) for k in self.TENSORS}
        self.grads, self.m, self.v = zeros(), zeros(), zeros()
        self.loss_out = torch.zeros(S, *self.LOSS_SHAPE, dtype=torch.float32, device=self.device)
        sets = [self.TENSOR_SET(*[getattr(n, k).data_ptr() for k in self.TENSORS]) for n in (net,) + tuple(more_nets)]
        sets += [self.TENSOR_SET(*[d[k].data_ptr() for k in self.TENSORS]) for d in (self.grads, self.m, self.v)]
        lanes, acts = (C.c_int32 * S)(*net.lanes), (C.c_int32 * S)(*net.actions)
        h = C.c_void_p()
        torch.cuda.synchronize(self.device)
        rc = self._fn('create')(self.device.index or 0, S, net.lmax, lanes, acts, net.amax, C.byref(cfg), *[C.byref(t) for t in sets],
                                int(max_batch), C.byref(h))
        if rc != 0:
            self._fail(self.PREFIX + '_create', rc)
        self._h = h

    def _fn(self, name):
        return getattr(self._lib, '%s_%s' % (self.PREFIX, name))

    # ---- the target's options of the DQN learners (SET_TARGET: n-step returns, Double DQN)
    def _take_target_options(self, n_step, double_q):
        self.n_step, self.double_q = int(n_step), bool(double_q)
        if not 1 <= self.n_step <= 32:
            raise ValueError('%s: n_step must be in 1 .. 32, got %d' % (self.NAME, self.n_step))

    def _set_target_options(self):
        """on a fresh handle: nothing is called while the options are the defaults"""
        if (self.n_step, self.double_q) == (1, False):
            return
        name = self.SET_TARGET or self.PREFIX + '_set_target'
        if not hasattr(self._lib, name):
            raise RuntimeError('the loaded library has no %s: rebuild it (there is no CPU fallback)' % name)
        rc = getattr(self._lib, name)(self._h, self.n_step, int(self.double_q))
        if rc != 0:
            self._fail(name, rc)

    def _need_handle(self):
        """what a learner that creates its handle on first use overrides"""

    def close(self):
        if self._h is not None:
            self._fn('destroy')(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_updates(self):
        """Adam steps taken so far"""
        return 0 if self._h is None else int(self._fn('steps')(self._h))

    def _fail(self, name, rc):
        raise RuntimeError('%s failed (%d): %s' % (name, rc, (self._lib.rs_last_error(None) or b'').decode()))

    def step(self):
        """One Adam step on what .grads holds (.grads itself stays as it is)."""
        self._need_handle()
        rc = self._fn('step')(self._h, torch_stream(self.device.index))
        if rc != 0:
            self._fail(self.PREFIX + '_step', rc)
