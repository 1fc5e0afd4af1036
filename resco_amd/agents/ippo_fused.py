"""IPPO on the device: the actor-critic launch of the fused forward (rs_ippo_act), the trajectory segments the group path
records into (rs_group_rollout), and what the learner needs from them (include/resco_sim.h, resco_amd/csrc/resco_policy.h).

The reference's IPPO agent is one pfrl PPO per signal (resco_benchmark/agents/pfrl_ppo.py:38-75) driven by the loop of
main.py:104-108.  `FusedIPPO(net)` packs a `BatchedIPPO` like `FusedIDQN` packs the trunk and the policy head, plus the value
head Linear(64, 1) as column 8 of the fc3 tile: one launch gives, for every (environment, signal), the action drawn from
softmax(logits), ITS log-probability under the fp16 kernel that drew it, and the value -- what `make_dataset` otherwise computes
with a second, un-fused forward over the whole segment.  `DeviceRollout` owns the segments `SimGroup.rollout` fills without a
Python call per env-step; `BatchedPPOLearner.update_from_rollout` learns from them.
"""
import numpy as np
import torch

from ..sim import Rollout, torch_stream
from .idqn_fused import FusedIDQN, _b_fragments, _fragment_index, pack_idqn_weights, repack_index

VALUE_COL = 8               # POL_QMAX: the value head's column of the fc3 tile, its bias in b3[:, 8]


def pack_ippo_weights(net):
    """pack_idqn_weights(net) plus the value head: column 8 of the fc3 fragments and b3[:, 8].  Everything else is byte-identical."""
    w = pack_idqn_weights(net)
    S = len(net.lanes)
    f = lambda t: t.detach().float().cpu().numpy()
    full = np.zeros((S, 64, VALUE_COL + 1), np.float32)
    full[:, :, :net.amax] = f(net.fc3_w)
    full[:, :, VALUE_COL] = f(net.v_w)[:, :, 0]
    w['w3'] = np.ascontiguousarray(_b_fragments(full, 8, 1)[:, :, 0])
    w['b3'][:, VALUE_COL] = f(net.v_b)[:, 0]
    return w


def ippo_repack_index(lmax, amax):
    """repack_index with the value column: 'w3' indexes the per-signal [64, 9] matrix of `fc3_with_value` (flattened), -1 = padding."""
    idx = repack_index(lmax, amax)
    idx['w3'] = _fragment_index(64, VALUE_COL + 1, 8, 1, -1).reshape(-1)
    return idx


def fc3_with_value(net, out=None):
    """[S, 64, 9]: the policy head's columns 0 .. amax-1, zeros up to 7, the value head in column 8 -- what 'w3' is gathered from."""
    S = len(net.lanes)
    if out is None:
        out = torch.zeros(S, 64, VALUE_COL + 1, dtype=torch.float32, device=net.fc3_w.device)
    out[:, :, :net.amax] = net.fc3_w.detach()
    out[:, :, VALUE_COL] = net.v_w.detach()[:, :, 0]
    return out


class FusedIPPO(FusedIDQN):
    """The fused actor-critic of a BatchedIPPO.  refresh() / refresh_on_device() as FusedIDQN's, with the value column."""
    _pack = staticmethod(pack_ippo_weights)

    def __init__(self, net, device=0, seed=0):
        assert hasattr(net, 'v_w') and hasattr(net, 'v_b'), 'FusedIPPO packs a BatchedIPPO (policy and value head)'
        self._w3src = None
        super().__init__(net, device, seed)
        self._out = {}

    def _repack_index(self):
        return ippo_repack_index(self.lmax, self.net.amax)

    def _fc3_source(self):
        self._w3src = fc3_with_value(self.net, self._w3src)
        return self._w3src

    def _fill_b3(self, b3):
        b3[:, :self.net.amax] = self.net.fc3_b
        b3[:, VALUE_COL] = self.net.v_b[:, 0]

    def _buf(self, name, N, dtype, device):
        key = (name, N)
        if key not in self._out:
            self._out[key] = torch.empty(N, self.S, dtype=dtype, device=device)
        return self._out[key]

    def _check_obs(self, obs):
        assert obs.is_cuda and obs.dtype == torch.float16 and obs.is_contiguous()
        assert tuple(obs.shape[1:]) == (self.S, self.lmax, 5)
        return obs.shape[0]

    def _call(self, obs, N, env_base, step_key, dyn, actions, logp, value, logits, stream):
        st = torch_stream(self.device) if stream is None else stream
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = self._lib.rs_ippo_act(self._h, obs.data_ptr(), N, int(env_base), self.seed, int(step_key) & 0xFFFFFFFF, ptr(dyn),
                                   ptr(actions), ptr(logp), ptr(value), ptr(logits), st)
        if rc != 0:
            raise RuntimeError('rs_ippo_act failed (%d)' % rc)

    def act(self, obs, step_key=0, out=None, logp=None, value=None, want_logits=False, env_base=0, dyn=None, stream=None):
        """obs: fp16 CUDA tensor [N, S, lmax, 5].  Returns (actions int32 [N, S], logp float32 [N, S], value float32 [N, S]) and,
        with want_logits, the logits [N, S, 8] (-inf beyond a signal's actions).  out / logp / value: tensors to write into (e.g.
        the simulator's RS_BUF_ACTIONS, a slot of a segment); otherwise buffers reused between calls.  The draw is rs_idqn_act's
        mode 1, keyed by (seed; env_base + e, signal, step_key); dyn: optional CUDA tensor of two 32-bit words whose second is the
        step key (HIP-graph replay)."""
        N = self._check_obs(obs)
        dev = obs.device
        for t, dt in ((out, torch.int32), (logp, torch.float32), (value, torch.float32)):
            assert t is None or (t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == (N, self.S))
        actions = out if out is not None else self._buf('act', N, torch.int32, dev)
        logp = logp if logp is not None else self._buf('logp', N, torch.float32, dev)
        value = value if value is not None else self._buf('value', N, torch.float32, dev)
        logits = torch.empty(N, self.S, 8, dtype=torch.float32, device=dev) if want_logits else None
        self._call(obs, N, env_base, step_key, dyn, actions, logp, value, logits, stream)
        return (actions, logp, value, logits) if want_logits else (actions, logp, value)

    def value(self, obs, out=None, stream=None):
        """The value head alone, float32 [N, S]: the bootstrap value of the state after a segment (no draw, no log-probability)."""
        N = self._check_obs(obs)
        assert out is None or (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (N, self.S))
        value = out if out is not None else torch.empty(N, self.S, dtype=torch.float32, device=obs.device)
        self._call(obs, N, 0, 0, None, None, None, value, None, stream)
        return value


class DeviceRollout:
    """T slots of trajectory for every pipe of a group: per pipe obs f16 [T, n, S, lmax, 5] and act (int32), logp, value, rew
    (float32) [T, n, S], as torch tensors (`.pipes[i][name]`) that rs_group_rollout writes on the pipes' streams."""
    FIELDS = ('obs', 'act', 'logp', 'value', 'rew')

    def __init__(self, T, sims):
        self.T, self.sims = int(T), list(sims)
        self.pipes = []
        for s in self.sims:
            lmax = s.device_pointer('drq_norm_f16')[1][2]
            dev = 'cuda:%d' % s.device
            z = lambda dt: torch.zeros(self.T, s.n_envs, s.S, dtype=dt, device=dev)
            self.pipes.append(dict(obs=torch.zeros(self.T, s.n_envs, s.S, lmax, 5, dtype=torch.float16, device=dev), act=z(torch.int32),
                                   logp=z(torch.float32), value=z(torch.float32), rew=z(torch.float32)))
        self._segs = (Rollout * len(self.sims))(*[Rollout(*[p[k].data_ptr() for k in self.FIELDS], self.T) for p in self.pipes])

    def segments(self, sims):
        """the rs_rollout array for rs_group_rollout over exactly these pipes"""
        assert [id(s) for s in sims] == [id(s) for s in self.sims], 'the rollout was allocated for other pipes'
        return self._segs

    # ---- checkpoints (resco_amd/checkpoint.py): a segment spans episodes, so its filled slots are training state; in place
    def signature(self):
        return {'T': self.T, 'n_envs': [int(s.n_envs) for s in self.sims]}

    def state_dict(self):
        return {'state': {'pipes': [{k: p[k] for k in self.FIELDS} for p in self.pipes]}}

    def load_state_dict(self, sd, weights_only=False):
        from . import _state
        if weights_only:
            return
        if len(sd['state']['pipes']) != len(self.pipes):
            raise ValueError('DeviceRollout: the checkpoint holds %d pipes, the rollout %d' % (len(sd['state']['pipes']), len(self.pipes)))
        for i, (p, src) in enumerate(zip(self.pipes, sd['state']['pipes'])):
            _state.copy_dict_into(p, src, 'DeviceRollout.pipes[%d]' % i)

    def cat(self, name):
        """[T, N, ...] over all pipes in order (the single pipe's own tensor, a copy otherwise)"""
        return self.pipes[0][name] if len(self.pipes) == 1 else torch.cat([p[name] for p in self.pipes], dim=1)
