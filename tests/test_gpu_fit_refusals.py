"""GPU: "does this policy fit this handle?" and "may this handle take part in a loop?" at the entry points and agent kinds whose
refusals no other file asks for: rs_group_step with an IDQN or MPLight policy of the wrong kind or scenario and with MPLight's buffer
switched off (each demand shape names its own), rs_group_ppo_train with a policy of another scenario, the observation switched off,
rs_timing on and a handle on a plain stream, rs_group_rollout with another agent kind.  cologne1 x 16; the policies "built for
another scenario" are ingolstadt21's.  Every case has ONE fault, answers RS_EINVAL, names the entry point and the reason (and the
buffer, where there is one) and launches nothing: RS_BUF_ACTIONS and the environments' clocks stay as they were."""
import ctypes as C

import numpy as np
import pytest
import torch

from resco_amd.agents.idqn_fused import FusedIDQN
from resco_amd.agents.idqn_rollout import BatchedIDQN
from resco_amd.agents.ippo import BatchedIPPO
from resco_amd.agents.ippo_fused import DeviceRollout, FusedIPPO
from resco_amd.agents.ippo_learn_fused import FusedPPOLearner
from resco_amd.agents.mplight import FusedMPLight, frap_from_scenario
from resco_amd.agents.train_fused import DevicePPOTrainer
from resco_amd.multi_signal import VecMultiSignal, load_scenario, map_configs
from resco_amd.sim import AGENT, SimGroup

pytestmark = pytest.mark.gpu

RS_EINVAL = -1
N, T = 16, 6


def scenario(map_name):
    return load_scenario(map_name, None, map_configs.get(map_name, {}).get('lights', ()), 3)


def idqn_policy(sc, seed):
    net = BatchedIDQN.from_scenario(sc, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=seed)
    return FusedIDQN(net, seed=seed)


def ippo_policy(sc, seed):
    net = BatchedIPPO.from_scenario(sc, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=seed)
    pol = FusedIPPO(net, seed=seed)
    pol.refresh_on_device()             # off its create-time copy: what rs_group_ppo_train asks of a policy that fits
    return net, pol


def test_single_fault_refusals(monkeypatch):
    env = VecMultiSignal('cologne1', N, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
    sim, sc, other_sc = env.sim, env.scenario, scenario('ingolstadt21')
    lib = sim._lib
    monkeypatch.setenv('RESCO_PLAIN_STREAMS', '1')
    plain = VecMultiSignal('cologne1', N, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0, scenario=sc)
    monkeypatch.delenv('RESCO_PLAIN_STREAMS')
    idqn, idqn_other = idqn_policy(sc, 1), idqn_policy(other_sc, 2)
    mplight = {D: FusedMPLight(frap_from_scenario(sc, D).cuda().init_like_reference(3), sc, seed=3) for D in (1, 4)}
    net, ippo = ippo_policy(sc, 4)
    _, ippo_other = ippo_policy(other_sc, 5)
    learner = FusedPPOLearner(net, epochs=2, minibatch=40, seed=11)
    rec = DeviceRollout(T, [sim])
    trainer = DevicePPOTrainer(env, learner, ippo, rec)
    grp, plain_grp = SimGroup([sim]), SimGroup([plain.sim])

    def ppo_train(group=grp, policy=ippo.handle):
        ptr = lambda t: t.data_ptr()
        group.ppo_train(3, policy=policy, learner=learner._h, seg=rec.segments([sim])[0], done=ptr(trainer.done), last_value=ptr(trainer.last_value),
                        adv=ptr(trainer.adv), ret=ptr(trainer.ret), gae_scratch=ptr(trainer._scratch), perm=ptr(trainer.perm), t0=0, update0=0, slot0=0,
                        done_step=-1, epochs=learner.epochs, minibatch=learner.minibatch, gamma=learner.gamma, lambd=learner.lambd,
                        policy_seed=ippo.seed, learner_seed=learner.seed, loss_out=ptr(learner.loss_out))

    def rollout_as(kind):
        """rs_group_rollout with agent->kind = kind (SimGroup.rollout always says RS_AGENT_IPPO); as the wrapper, the failure raises"""
        a = grp._agent
        a.kind, a.step_key, a.policy, a.mode, a.epsilon, a.epsilon_step, a.seed = AGENT[kind], 0, ippo.handle, 0, 0.0, 0.0, 0
        rc = lib.rs_group_rollout(grp._hs, 1, C.byref(a), rec.segments([sim]), 0, 1)
        if rc != 0:
            raise RuntimeError('rs_group_rollout failed (%d): %s' % (rc, (lib.rs_last_error(sim._h) or b'').decode()))

    all_on = lambda s: s.set_outputs(None)
    # (entry point, the call, what is done to the handle before / after it, the reason as the message gives it)
    cases = [
        ('rs_group_step', lambda: grp.step('idqn', policy=idqn_other.handle), None, None, 'policy built for this scenario (n_signals, lmax)'),
        ('rs_group_step', lambda: grp.step('idqn', policy=mplight[1].handle), None, None, 'policy built for this scenario (n_signals, lmax)'),
        ('rs_group_step', lambda: grp.step('mplight', policy=idqn.handle), None, None, 'rs_mplight_create policy built for this scenario (n_signals)'),
        ('rs_group_step', lambda: grp.step('mplight', policy=mplight[1].handle), lambda s: s.set_outputs(('mplight_full', 'drq_norm_f16')), all_on,
         'reads RS_BUF_MPLIGHT, which rs_set_outputs has switched off'),
        ('rs_group_step', lambda: grp.step('mplight', policy=mplight[4].handle), lambda s: s.set_outputs(('mplight', 'drq_norm_f16')), all_on,
         'reads RS_BUF_MPLIGHT_FULL, which rs_set_outputs has switched off'),
        ('rs_group_ppo_train', lambda: ppo_train(policy=ippo_other.handle), None, None, 'rs_idqn_create policy built for this scenario (n_signals, lmax)'),
        ('rs_group_ppo_train', ppo_train, lambda s: s.set_outputs(('mplight', 'mplight_full')), all_on,
         'reads RS_BUF_DRQ_NORM_F16, which rs_set_outputs has switched off'),
        ('rs_group_ppo_train', ppo_train, lambda s: s.timing(True), lambda s: s.timing(False), 'rs_timing is enabled on this handle'),
        ('rs_group_ppo_train', lambda: ppo_train(group=plain_grp), None, None, "this handle's stream is a non-blocking stream"),
        ('rs_group_rollout', lambda: rollout_as('idqn'), None, None, 'the agent must be RS_AGENT_IPPO'),
        ('rs_group_rollout', lambda: rollout_as('mplight'), None, None, 'the agent must be RS_AGENT_IPPO'),
    ]

    def state():
        torch.cuda.synchronize()
        return [np.concatenate([s.read(b) for s in (sim, plain.sim)]) for b in ('actions', 'env')]

    for s in (sim, plain.sim):
        all_on(s)
        s.reset()
    grp.step('random', step_key=0, n_steps=3)           # actions and clocks that a launch would change
    plain_grp.step('random', step_key=0, n_steps=3)
    before = state()
    assert before[0].max() > 0 and (before[1][:, 0] > 0).all()
    for entry, call, arm, disarm, reason in cases:
        if arm:
            arm(sim)
        with pytest.raises(RuntimeError) as e:
            call()
        if disarm:
            disarm(sim)
        msg = str(e.value)
        assert msg.startswith('%s failed (%d): ' % (entry, RS_EINVAL)), (entry, msg)
        assert entry + ': ' in msg and reason in msg, (entry, reason, msg)
        for a, b in zip(before, state()):
            np.testing.assert_array_equal(a, b, err_msg='%s: %s' % (entry, reason))
    # the same calls go through once nothing is wrong with them: the refusals above are the faults', not the cases'
    grp.step('idqn', policy=idqn.handle)
    grp.step('mplight', policy=mplight[4].handle)
    rollout_as('ippo')
    ppo_train()
    torch.cuda.synchronize()
    assert (sim.read('env')[:, 0] > before[1][:N, 0]).all()
    for o in (idqn, idqn_other, mplight[1], mplight[4], ippo, ippo_other, learner, plain, env):
        o.close()
