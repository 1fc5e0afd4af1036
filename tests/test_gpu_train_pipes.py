"""GPU: what tools/train_pipes_ab.py compares is like with like: its training on K pipes (one rs_group_step call per env-step, ring
and learner on the concatenation) is the training of tools/idqn_train.py / tools/mplight_train.py --device-update bit for bit.  The
environments are keyed by their global index, the policy kernels draw by it, the fused learners draw from a counter hash: every
figure of an episode's row must be EQUAL, no tolerance.  One short episode each (the horizon is cut)."""
import numpy as np
import pytest
import torch

from resco_amd.multi_signal import VecMultiSignal
from tools.train_pipes_ab import PipedEnvs, train_one_handle, train_piped

pytestmark = pytest.mark.gpu

KEYS = ('episode', 'epsilon', 'mean_return', 'avg_delay_s', 'arrived_per_env', 'updates')


@pytest.fixture
def short_episode(monkeypatch):
    init = VecMultiSignal.__init__

    def short(self, *a, **kw):
        init(self, *a, **kw)
        self.horizon_steps = 20

    monkeypatch.setattr(VecMultiSignal, '__init__', short)


def figures(rows):
    return [{k: r[k] for k in KEYS} for r in rows]


def test_piped_random_episode_equals_the_single_handle(short_episode):
    """the concatenated buffers of 6 + 5 + 5 environments are the single batch's"""
    one = VecMultiSignal('cologne1', 16, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
    pe = PipedEnvs('cologne1', 16, 3, states=('drq_norm_f16',), rewards=('wait_norm',), seed=0)
    assert [e.n_envs for e in pe.envs] == [6, 5, 5] and [e.sim.env_base for e in pe.envs] == [0, 6, 11]
    one.sim.set_seed(77)
    pe.set_seed(77)
    one.reset()
    pe.reset()
    for k in range(20):
        one.act_random(k)
        one.step(None)
        pe.step('random', step_key=k)
    torch.cuda.synchronize()
    for name in ('drq_norm_f16', 'wait_norm', 'actions'):
        assert torch.equal(pe.cat(name), one.tensor(name)), name
    assert pe.delay() == (float(one.sim.trip_delay().mean()), float(one.sim.stats()['arrived'].mean()))
    assert all(e.steps == 20 for e in pe.envs)
    with torch.cuda.stream(torch.cuda.Stream()), pytest.raises(RuntimeError, match='default stream'):
        pe.step('random', step_key=20)          # a side stream is not ordered with the pipes: refused
    pe.close()
    one.close()


@pytest.mark.parametrize('agent,map_name,n,pipes,full', [('idqn', 'cologne1', 16, 2, False), ('idqn', 'cologne1', 16, 3, False),
                                                         ('mplight', 'cologne1', 16, 2, False), ('mplight', 'cologne1', 16, 2, True),
                                                         ('mplight', 'ingolstadt21', 8, 2, False)])
def test_training_on_pipes_equals_one_handle(short_episode, agent, map_name, n, pipes, full):
    want = train_one_handle(agent, map_name, n, 2, batch=32, full=full)
    got = train_piped(agent, map_name, n, 2, batch=32, pipes=pipes, full=full)
    assert figures(got) == figures(want) and want[-1]['updates'] > 0 and np.isfinite(want[-1]['mean_return'])
