"""The training loops in the library: the DQN loop of IDQN and MPLight (include/resco_sim.h: rs_group_train;
resco_amd/csrc/resco_group_train.h) and the PPO loop of IPPO (rs_group_ppo_train; resco_amd/csrc/resco_ppo_loop.h).

`DeviceTrainer(envs, learner, policy, replay)` joins what the loops of tools/idqn_train.py and tools/mplight_train.py --device-update
join in Python -- policy.act, replay.stage, env.step, replay.commit, ret += rew, learner.observe_step, policy.refresh_on_device --
and `run(n_steps)` enqueues that many iterations with ONE call through the ABI.  It owns nothing new: the environments (one
VecMultiSignal, or a list of them that split one batch over pipes with contiguous env_base values), the fused learner
(FusedDQNLearner / FusedMPLightLearner), the fused policy (FusedIDQN / FusedMPLight) and the replay ring (DeviceReplay /
MPLightReplay over ALL environments) stay the caller's and are advanced here exactly as the Python loop advances them, so the two
can be mixed step by step and give the same bits.  The reset between episodes stays with the caller.  There is no CPU fallback.

`DevicePPOTrainer(env, learner, policy, rollout)` does the same for the loop of tools/ippo_train.py --device-update: grp.rollout,
policy.value, learner.update_from_rollout with the learner's device_perm shuffles, policy.refresh_on_device.  One environment (one
handle), a FusedPPOLearner, a FusedIPPO and a DeviceRollout over that handle; the trainer owns the update's buffers (done bytes,
bootstrap value, advantages, returns, shuffles).

`DeviceA2CTrainer(env, learner, policy, full=False)` does the same for the loop of tools/fma2c_train.py --device-update
(rs_group_fma2c_train; resco_amd/csrc/resco_fma2c_loop.h): policy.act into the learner's slot, env.step, the rewards (by the reward
kernel of rs_fma2c_record, not the dense product), ret += rew and FusedA2CLearner.observe.  One environment, a FusedA2CLearner and a
FusedFMA2C; the trainer owns the uploaded reward table, the bootstrap value and the return accumulator.
"""
import torch

from ..sim import DQNRing, Fma2cRewardTable, MPLightRing, SimGroup
from .fma2c import FusedFMA2C
from .fma2c_learn_fused import FusedA2CLearner
from .idqn_learn import linear_epsilon
from .idqn_learn_fused import FusedDQNLearner
from .ippo_fused import FusedIPPO
from .ippo_learn_fused import FusedPPOLearner
from .mplight_learn_fused import FusedMPLightLearner


class DeviceTrainer:
    def __init__(self, envs, learner, policy, replay, eps_start=1.0, eps_end=0.0, decay_steps=0, updates_per_step=1):
        self.envs = list(envs.envs) if hasattr(envs, 'envs') else (list(envs) if isinstance(envs, (list, tuple)) else [envs])
        self.learner, self.policy, self.replay = learner, policy, replay
        self.eps_start, self.eps_end, self.decay_steps = float(eps_start), float(eps_end), int(decay_steps)
        if isinstance(learner, FusedDQNLearner):
            self.agent, self.updates_per_step = 'idqn', int(updates_per_step)
            learner.attach(replay)              # (prioritised replay: the learner's handle carries the priorities, sized from this ring)
            if not hasattr(policy, '_dev'):
                policy.refresh_on_device()      # the library re-packs into the policy's own device buffers: they have to exist
        elif isinstance(learner, FusedMPLightLearner):
            if int(updates_per_step) != 1:
                raise ValueError('MPLight runs one update per env-step (FusedMPLightLearner.observe_step)')
            self.agent, self.updates_per_step = 'mplight', 1
            learner._ring(replay)               # (creates the handle over the ring's signal count if it has none yet; prioritised
                                                #  replay: attaches the priorities, sized from this ring)
        else:
            raise TypeError('DeviceTrainer needs a FusedDQNLearner or a FusedMPLightLearner: the loop runs in the library (there is no CPU fallback)')
        if sum(e.n_envs for e in self.envs) != replay.N:
            raise ValueError('the environments (%d) are not the replay ring\'s (%d)' % (sum(e.n_envs for e in self.envs), replay.N))
        self.group = SimGroup([e.sim for e in self.envs])

    def signature(self):
        """what of the trajectory this object decides (resco_amd/checkpoint.py); it holds no counters of its own, so no state"""
        return {'eps_start': self.eps_start, 'eps_end': self.eps_end, 'decay_steps': self.decay_steps, 'updates_per_step': self.updates_per_step}

    def epsilon(self, t):
        """the exploration rate of agent step t, as the loop evaluates it"""
        return linear_epsilon(t, self.eps_start, self.eps_end, self.decay_steps)

    def run(self, n_steps, ret=None):
        """n_steps env-steps of training, enqueued by one call; asynchronous.  ret: None or a float32 device tensor [N, S] that
        accumulates the rewards (ret += rew per step).  Advances replay.head / replay.count, learner.t and the environments' step
        counters and returns done (the episode's horizon is reached)."""
        n, env0 = int(n_steps), self.envs[0]
        if n < 1:
            raise ValueError('need n_steps >= 1')
        if any(e.steps != env0.steps or e.horizon_steps != env0.horizon_steps for e in self.envs):
            raise RuntimeError('the pipes are not at the same step of the episode')
        if env0.steps + n > env0.horizon_steps:
            raise ValueError('%d steps from step %d would cross the horizon (%d): the reset between episodes is the caller\'s' %
                             (n, env0.steps, env0.horizon_steps))
        if torch.cuda.current_stream().cuda_stream != 0:
            raise RuntimeError('DeviceTrainer needs PyTorch\'s default stream current: only that one is ordered with the pipes\' streams')
        learner, replay = self.learner, self.replay
        ring = learner._ring(replay)
        assert isinstance(ring, DQNRing if self.agent == 'idqn' else MPLightRing)
        if ret is not None:
            assert ret.is_cuda and ret.dtype == torch.float32 and ret.is_contiguous() and tuple(ret.shape) == (replay.N, replay.S)
        done_step = n - 1 if env0.steps + n == env0.horizon_steps else -1
        self.group.train(n, self.agent, self.policy.handle, learner._h, ring, learner.t, done_step=done_step, batch=learner.batch_size,
                         updates_per_step=self.updates_per_step, target_update=learner.target_update, eps_start=self.eps_start,
                         eps_end=self.eps_end, decay_steps=self.decay_steps, policy_seed=self.policy.seed, learner_seed=learner.seed,
                         ret=ret.data_ptr() if ret is not None else None, loss_out=learner.loss_out.data_ptr())
        replay.head = (replay.head + n) % replay.T
        replay.count = min(replay.count + n, replay.T)
        if hasattr(replay, '_pos'):             # DeviceReplay mirrors its position on the device for the graph-captured PyTorch learner
            replay._pos[0] = replay.head
            replay._pos[1] = replay.count
        learner.t += n
        return [e.advance(n) for e in self.envs][0]


class DevicePPOTrainer:
    def __init__(self, env, learner, policy, rollout):
        if not isinstance(learner, FusedPPOLearner) or not isinstance(policy, FusedIPPO):
            raise TypeError('DevicePPOTrainer needs a FusedPPOLearner and a FusedIPPO: the loop runs in the library (there is no CPU fallback)')
        if len(rollout.sims) != 1 or rollout.sims[0] is not env.sim:
            raise ValueError('the rollout must be this one environment\'s: a segment has no row stride, pipes cannot share one dataset')
        self.env, self.learner, self.policy, self.rollout = env, learner, policy, rollout
        learner._need_handle()
        if not hasattr(policy, '_dev'):
            policy.refresh_on_device()          # the library re-packs into the policy's own device buffers: they have to exist
        self.group = SimGroup([env.sim])
        T, N, S, dev = rollout.T, env.sim.n_envs, env.sim.S, learner.device
        f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.done = torch.zeros(T, dtype=torch.uint8, device=dev)
        self.last_value, self.adv, self.ret, self._scratch = f(N, S), f(T, N, S), f(T, N, S), f(N, S)
        self.perm = torch.zeros(learner.epochs, T * N, dtype=torch.int32, device=dev)
        self.slot, self.t, self.updates = 0, 0, 0       # filled slots of the segment, env-steps and updates so far

    # ---- checkpoints (resco_amd/checkpoint.py): a segment spans episodes, so where it stands is training state
    def state_dict(self):
        return {'state': {'done': self.done, 'slot': int(self.slot), 't': int(self.t), 'updates': int(self.updates)}}

    def load_state_dict(self, sd, weights_only=False):
        from . import _state
        if not weights_only:
            st = sd['state']
            if not 0 <= int(st['slot']) < self.rollout.T:
                raise ValueError('DevicePPOTrainer: slot %d lies outside a segment of %d' % (int(st['slot']), self.rollout.T))
            _state.copy_into(self.done, st['done'], 'DevicePPOTrainer.done')
            self.slot, self.t, self.updates = int(st['slot']), int(st['t']), int(st['updates'])

    def run(self, n_steps):
        """n_steps env-steps of training, enqueued by one call; asynchronous.  Advances the slot, the step and the update counter and
        the environment's step counter and returns done (the episode's horizon is reached)."""
        n, env = int(n_steps), self.env
        if n < 1:
            raise ValueError('need n_steps >= 1')
        if env.steps + n > env.horizon_steps:
            raise ValueError('%d steps from step %d would cross the horizon (%d): the reset between episodes is the caller\'s' %
                             (n, env.steps, env.horizon_steps))
        if torch.cuda.current_stream().cuda_stream != 0:
            raise RuntimeError('DevicePPOTrainer needs PyTorch\'s default stream current: the loop is launched on the legacy stream')
        L, T = self.learner, self.rollout.T
        done_step = n - 1 if env.steps + n == env.horizon_steps else -1
        ptr = lambda t: t.data_ptr()
        self.group.ppo_train(n, self.policy.handle, L._h, self.rollout.segments([env.sim])[0], ptr(self.done), ptr(self.last_value), ptr(self.adv),
                             ptr(self.ret), ptr(self._scratch), ptr(self.perm), self.t, self.updates, self.slot, done_step=done_step,
                             epochs=L.epochs, minibatch=L.minibatch, gamma=L.gamma, lambd=L.lambd, policy_seed=self.policy.seed,
                             learner_seed=L.seed, loss_out=ptr(L.loss_out))
        self.updates += (self.slot + n) // T
        self.slot = (self.slot + n) % T
        self.t += n
        return env.advance(n)


class DeviceA2CTrainer:
    def __init__(self, env, learner, policy, full=False):
        if not isinstance(learner, FusedA2CLearner) or not isinstance(policy, FusedFMA2C):
            raise TypeError('DeviceA2CTrainer needs a FusedA2CLearner and a FusedFMA2C: the loop runs in the library (there is no CPU fallback)')
        if learner.policy is not policy:
            raise ValueError('the learner was created for another policy')
        if learner.N != env.sim.n_envs or policy.max_envs != env.sim.n_envs:
            raise ValueError('learner (%d) and policy (%d) must be built for the environment\'s %d environments' % (learner.N, policy.max_envs, env.sim.n_envs))
        self.env, self.learner, self.policy, self.full = env, learner, policy, bool(full)
        self.group = SimGroup([env.sim])
        L = policy.L
        self.table = Fma2cRewardTable(env.scenario, L.cfg, full, env.sim.device)
        dev = 'cuda:%d' % env.sim.device
        self.R_boot = torch.zeros(env.sim.n_envs, L.K, dtype=torch.float32, device=dev)
        self.ret = torch.zeros(env.sim.n_envs, L.K, dtype=torch.float32, device=dev)    # the episode's return: zero it at a reset
        self.t = 0                              # env-steps so far: the key of the next act

    # ---- checkpoints (resco_amd/checkpoint.py): the key of the next act
    def state_dict(self):
        return {'state': {'t': int(self.t)}}

    def load_state_dict(self, sd, weights_only=False):
        if not weights_only:
            self.t = int(sd['state']['t'])

    def run(self, n_steps):
        """n_steps env-steps of training, enqueued by one call; asynchronous.  Advances the step counter, the environment's step
        counter and the learner's host counters (n, steps_done, updates, dones, last_loss) as FusedA2CLearner.observe would have, so
        calls and Python observe steps can alternate, and returns done (the episode's horizon is reached)."""
        n, env, L = int(n_steps), self.env, self.learner
        if n < 1:
            raise ValueError('need n_steps >= 1')
        if env.steps + n > env.horizon_steps:
            raise ValueError('%d steps from step %d would cross the horizon (%d): the reset between episodes is the caller\'s' %
                             (n, env.steps, env.horizon_steps))
        if torch.cuda.current_stream().cuda_stream != 0:
            raise ValueError('DeviceA2CTrainer needs PyTorch\'s default stream current: the loop is launched on the legacy stream')
        done_step = n - 1 if env.steps + n == env.horizon_steps else -1
        ptr = lambda t: t.data_ptr()
        self.group.fma2c_train(n, self.policy.handle, L.handle, self.table, ptr(L.rows), ptr(L.acts), ptr(L.rews), ptr(L.vals), ptr(L.dones_dev),
                               ptr(self.R_boot), L.T, self.t, L.n, done_step=done_step, policy_seed=self.policy.seed, ret=ptr(self.ret),
                               loss_out=ptr(L._loss))
        updated = False
        for k in range(n):                      # FusedA2CLearner.observe's bookkeeping, step by step
            done = k == done_step
            L.dones.append(done)
            L.n += 1
            L.steps_done += 1
            if L.steps_done % L.T == 0 or done:
                L.dones, L.n = [L.dones[-1]], 0
                L.updates += 1
                updated = True
            if done:
                L.steps_done = 0
        if updated:
            L.last_loss = L._loss.clone()
        self.t += n
        return env.advance(n)
