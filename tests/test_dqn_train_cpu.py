"""CPU: the scalar pieces of the fused DQN update (resco_amd/csrc/resco_dqn_train.h) through a host build of the same header
(tests/dqn_train_host) -- the per-row loss gradient against torch in float64 with torch's own float32 distance from it as the
yardstick, the minibatch draw against the oracle's counter hash -- the float64 reference itself (tests/dqn_train_ref.py), the C ABI
of the update (header, ABI_SYMBOLS, exports, struct mirrors); no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from dqn_train_ref import (ACTIONS, NAMES, RING_STATES, build_dqn_train_host, case, check_sample, lanes_of, predict_sample, torch_grads)
from resco_amd import sim as rsim

DQN_CALLS = ['rs_dqn_create', 'rs_dqn_destroy', 'rs_dqn_grad', 'rs_dqn_sample', 'rs_dqn_step', 'rs_dqn_steps', 'rs_dqn_update']


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return build_dqn_train_host(tmp_path_factory.mktemp('dqn_train_host'))


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _row_torch(q, act, tgt, A, dtype):
    """autograd of mean_i smooth_l1(q[i][act[i]], tgt[i]) with q as the leaf -> (dq [n, A], terms [n]) as float64 numpy"""
    lg = torch.from_numpy(q[:, :A]).to(dtype).requires_grad_()
    y = lg.gather(-1, torch.from_numpy(act).long().unsqueeze(-1)).squeeze(-1)
    per = torch.nn.functional.smooth_l1_loss(y, torch.from_numpy(tgt).to(dtype), reduction='none')
    per.mean().backward()
    return lg.grad.double().numpy(), per.detach().double().numpy()


@pytest.mark.parametrize('A', range(1, 9))
def test_row_loss_gradient(host, A):
    """96 rows: both Huber branches and both signs, four rows with |delta| exactly 1 (either branch gives the same gradient), two with an
    action outside 0 .. A - 1 (clamped as the kernel clamps it)"""
    n = 96
    rng = np.random.default_rng(20 + A)
    q = np.zeros((n, 8), np.float32)
    q[:, :A] = rng.standard_normal((n, A)).astype(np.float32)
    act = rng.integers(0, A, n).astype(np.int32)
    y = q[np.arange(n), act]
    tgt = (y + 1.5 * rng.standard_normal(n)).astype(np.float32)
    y[:4] = np.float32([0.5, -0.25, 2.0, -3.0])                 # y -+ 1 is exact in float32
    q[np.arange(4), act[:4]] = y[:4]
    tgt[:4] = y[:4] + np.float32([1.0, -1.0, 1.0, -1.0])
    delta = y.astype(np.float64) - tgt
    assert (np.abs(delta[:4]) == 1.0).all() and (np.abs(delta) > 1).sum() > 10 and (np.abs(delta) < 1).sum() > 10
    assert (delta > 1).any() and (delta < -1).any()
    clamped = act.copy()
    act_in = act.copy()
    act_in[4], act_in[5] = -3, A + 2
    clamped[4], clamped[5] = 0, A - 1
    dq, tm = np.full((n, 8), np.nan, np.float32), np.empty(n, np.float32)
    ptr = lambda a: a.ctypes.data
    assert host.dqn_train_rows(ptr(q), A, n, ptr(act_in), ptr(tgt), float(n), ptr(dq), ptr(tm)) == 0
    assert np.isnan(dq[:, A:]).all(), 'columns beyond the signal\'s actions must not be written'
    truth, ref = _row_torch(q, clamped, tgt, A, torch.float64), _row_torch(q, clamped, tgt, A, torch.float32)
    for name, got, t64, t32 in zip(('dq', 'terms'), (dq[:, :A], tm), truth, ref):
        err, e_ref = np.abs(got.astype(np.float64) - t64), np.abs(t32 - t64).max()
        print('A %d %-5s |host - truth| %.3e  e_ref %.3e  (max |truth| %.3e)' % (A, name, err.max(), e_ref, np.abs(t64).max()))
        assert (err <= 4 * e_ref + 2 * _ulp(t64)).all(), name
    assert (np.count_nonzero(dq[:, :A], axis=1) <= 1).all()
    assert (np.abs(dq[:4, :A]).max(1) == np.float32(1.0) / np.float32(n)).all()


@pytest.mark.parametrize('T,N,head,count', RING_STATES)
def test_sampling_against_the_counter_hash(host, T, N, head, count):
    """dqn_sample_index of the header through the host build.  The hash it calls there is tests/dqn_train_host's RESTATEMENT of d_hash
    (resco_step.h's own is device code): this test holds the index arithmetic and that copy against the oracle's hash; the device
    function itself is held against the same prediction by tests/test_gpu_dqn_train.py::test_sample_on_the_device."""
    B, S, seed = 33, 3, 0x5EED
    draws = []
    for u in (0, 1, 77):
        idx = np.full((B, S, 2), -1, np.int32)
        assert host.dqn_train_sample(seed, u, S, T, N, head, count, B, idx.ctypes.data) == 0
        assert np.array_equal(idx, predict_sample(seed, u, S, T, N, head, count, B))
        check_sample(idx, T, N, head, count)
        draws.append(idx)
    if T * N > 2:
        assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[1], draws[2])
        assert len(np.unique(draws[0][..., 0])) == count - 1, 'every slot with a successor is drawn by 99 draws'
    assert host.dqn_train_sample(seed, 0, S, T, N, head, 1, B, draws[0].ctypes.data) == -1


def test_reference_case_and_yardstick():
    """the float64 reference on a ring of a few slots by a few environments: three signals (2, mid, lmax) lanes x (1, 3, 8) actions,
    both Huber branches well populated (asserted on the float64 values), masked gradients exactly zero, float32 close to it"""
    lmax, T, N, B = 9, 4, 6, 40
    c = case(lmax, T, N, seed=3, done_slots=(1,))
    assert tuple(c['net'].lanes) == lanes_of(lmax) == (2, 5, 9) and tuple(c['net'].actions) == ACTIONS
    rng = np.random.default_rng(0)
    idx = np.stack([rng.integers(0, T, (B, 3)), rng.integers(0, N, (B, 3))], -1)
    g64, l64, d64 = torch_grads(c, idx, torch.float64)
    g32, l32, _ = torch_grads(c, idx, torch.float32)
    frac = (np.abs(d64) > 1).mean()
    assert 0.2 <= frac <= 0.8, frac
    for k in NAMES:
        e_ref = np.abs(g32[k] - g64[k]).max()
        assert 0 < e_ref < 1e-4 * np.abs(g64[k]).max(), (k, e_ref)
    assert (g64['fc1_w'][0, :, :].reshape(64, 8, 4, 64)[:, 1:] == 0).all() and np.abs(g64['fc1_w'][0]).max() > 0
    assert (g64['fc3_w'][0, :, 1:] == 0).all() and (g64['fc3_b'][1, 3:] == 0).all()
    assert np.abs(l32 - l64).max() < 1e-5 and (l64 > 0).all()
    # a NaN successor behind an episode end never reaches the reference
    c['obs'][2] = np.nan
    only_done = idx.copy()
    only_done[..., 0] = 1
    assert all(np.isfinite(v).all() for v in torch_grads(c, only_done, torch.float64)[0].values())


def _header():
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        return f.read()


def test_abi_declares_and_exports_the_update():
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = set(re.findall(r'\b(rs_[a-z_]+)\s*\(', text))
    from resco_amd.build import build_library
    build_library()
    L = rsim.load_library()
    for name in DQN_CALLS:
        assert name in declared and name in rsim.ABI_SYMBOLS and hasattr(L, name), name


def _fields(text, name):
    body = text[text.index('typedef struct %s {' % name) + len('typedef struct %s {' % name):text.index('} %s;' % name)]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = re.sub(r'^(const\s+)?(float|double|void|int16_t|int32_t|uint8_t)\s*', '', decl.strip())
        names += [n.strip().lstrip('*') for n in decl.split(',') if n.strip()]
    return names


def test_struct_mirrors_list_the_headers_fields():
    text = _header()
    assert [f[0] for f in rsim.DQNTensors._fields_] == _fields(text, 'rs_dqn_tensors') == list(NAMES)
    assert C.sizeof(rsim.DQNTensors) == 8 * 8
    assert [f[0] for f in rsim.DQNConfig._fields_] == _fields(text, 'rs_dqn_config') == ['lr', 'adam_eps', 'beta1', 'beta2', 'gamma']
    assert C.sizeof(rsim.DQNConfig) == 8 * 5
    assert [f[0] for f in rsim.DQNRing._fields_] == _fields(text, 'rs_dqn_ring') == ['obs', 'act', 'rew', 'done', 'capacity', 'n_envs', 'head', 'count']
    assert C.sizeof(rsim.DQNRing) == 4 * 8 + 4 * 4


def test_learner_refuses_a_cpu_net():
    from resco_amd.agents.idqn_learn_fused import FusedDQNLearner
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        FusedDQNLearner(case(3, 2, 2, seed=0)['net'])
