"""CPU: the scalar pieces of the fused PPO update (resco_amd/csrc/resco_ppo_train.h) through a host build of the same header
(tests/ppo_train_host) against torch in float64, with torch's own float32 distance from it as the yardstick (tests/ppo_train_ref.py);
the C ABI of the update (header, ABI_SYMBOLS, exports, struct mirrors); no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from idqn_kernel_ref import make_net
from ppo_train_ref import HYPER, NAMES, build_ppo_train_host, state_arrays, torch_step
from resco_amd import sim as rsim
from resco_amd.agents.ippo import BatchedIPPO

PPO_CALLS = ['rs_ppo_create', 'rs_ppo_destroy', 'rs_ppo_fit', 'rs_ppo_grad', 'rs_ppo_step', 'rs_ppo_steps']


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return build_ppo_train_host(tmp_path_factory.mktemp('ppo_train_host'))


def _row_case(A, n, seed):
    """n samples of a signal with A actions, none within 1e-4 of a clip boundary; about a fifth clipped, both signs of adv"""
    rng = np.random.default_rng(seed)
    logits = np.zeros((n, 8), np.float32)
    logits[:, :A] = rng.standard_normal((n, A)).astype(np.float32)
    act = rng.integers(0, A, n).astype(np.int32)
    lg = torch.from_numpy(logits[:, :A]).double()
    lp = torch.log_softmax(lg, -1).gather(-1, torch.from_numpy(act).long().unsqueeze(-1)).squeeze(-1).numpy()
    noise = rng.standard_normal(n)
    for _ in range(100):
        logp = (lp + 0.08 * noise).astype(np.float32)
        ratio = np.exp(lp - logp.astype(np.float64))
        near = (np.abs(ratio - 0.9) < 1e-4) | (np.abs(ratio - 1.1) < 1e-4)
        if not near.any():
            break
        noise[near] = rng.standard_normal(int(near.sum()))
    assert not near.any()
    adv = rng.standard_normal(n).astype(np.float32)
    value = rng.standard_normal(n).astype(np.float32)
    ret = (value + rng.standard_normal(n)).astype(np.float32)
    clipped = (ratio < 0.9) | (ratio > 1.1)
    return dict(logits=logits, act=act, logp=logp, adv=adv, value=value, ret=ret, clipped=clipped)


def _row_torch(c, A, dtype):
    """autograd of sum_i inv_b (per-row loss) with logits and value as leaves -> dlogits [n, A], dvalue [n], terms [n, 3] (float64 numpy)"""
    n = len(c['act'])
    lg = torch.from_numpy(c['logits'][:, :A]).to(dtype).requires_grad_()
    v = torch.from_numpy(c['value']).to(dtype).requires_grad_()
    t = lambda k: torch.from_numpy(c[k]).to(dtype)
    lp_all = torch.log_softmax(lg, -1)
    lp = lp_all.gather(-1, torch.from_numpy(c['act']).long().unsqueeze(-1)).squeeze(-1)
    ratio = torch.exp(lp - t('logp'))
    e = HYPER['clip_eps']
    pg = -torch.minimum(ratio * t('adv'), torch.clamp(ratio, 1.0 - e, 1.0 + e) * t('adv'))
    vf = (v - t('ret')) ** 2
    ent = -(torch.exp(lp_all) * lp_all).sum(-1)
    (pg + HYPER['value_coef'] * vf - HYPER['entropy_coef'] * ent).mean().backward()
    f = lambda x: x.detach().double().numpy()
    return f(lg.grad), f(v.grad), np.stack([f(pg), f(vf), f(ent)], 1)


@pytest.mark.parametrize('A', range(1, 9))
def test_row_loss_gradient(host, A):
    n = 96
    c = _row_case(A, n, seed=10 + A)
    assert c['clipped'].any() and (~c['clipped']).any() and (c['adv'] > 0).any() and (c['adv'] < 0).any()
    dl, dv, tm = np.full((n, 8), np.nan, np.float32), np.empty(n, np.float32), np.empty((n, 3), np.float32)
    ptr = lambda a: a.ctypes.data
    rc = host.ppo_train_rows(ptr(c['logits']), A, n, ptr(c['value']), ptr(c['act']), ptr(c['logp']), ptr(c['adv']), ptr(c['ret']), 1.0 / n,
                             HYPER['clip_eps'], HYPER['entropy_coef'], HYPER['value_coef'], ptr(dl), ptr(dv), ptr(tm))
    assert rc == 0
    assert np.isnan(dl[:, A:]).all(), 'columns beyond the signal\'s actions must not be written'
    truth, ref = _row_torch(c, A, torch.float64), _row_torch(c, A, torch.float32)
    for name, got, t64, t32 in zip(('dlogits', 'dvalue', 'terms'), (dl[:, :A], dv, tm), truth, ref):
        err, e_ref = np.abs(got.astype(np.float64) - t64).max(), np.abs(t32 - t64).max()
        print('A %d %-7s |host - truth| %.3e  e_ref %.3e  (max |truth| %.3e)' % (A, name, err, e_ref, np.abs(t64).max()))
        assert err <= 4 * e_ref, name
    if A == 1:
        assert (dl[:, 0] == 0.0).all()


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize('gscale', [1.0, 100.0])
def test_adam_elements_and_clip_scale(host, gscale):
    """three consecutive steps (bias correction at t = 1, 2, 3), gradients as they are (the clip does not bind) and x 100 (it binds)"""
    net, _ = make_net(3, seed=2, cls=BatchedIPPO)
    S = len(net.lanes)
    rng = np.random.default_rng(5)
    masks = dict(fc1_w=net.fc1_mask.numpy(), fc3_w=net.action_mask.unsqueeze(1).numpy(), fc3_b=net.action_mask.numpy())
    st64 = st32 = None
    p = {k: getattr(net, k).detach().numpy().copy() for k in NAMES}
    m = {k: np.zeros_like(p[k]) for k in NAMES}
    v = {k: np.zeros_like(p[k]) for k in NAMES}
    for t in (1, 2, 3):
        g = {k: (gscale * 1e-3 * rng.standard_normal(p[k].shape) * masks.get(k, 1.0)).astype(np.float32) for k in NAMES}
        st64, st32 = torch_step(net, g, st64, torch.float64), torch_step(net, g, st32, torch.float32)
        assert ((st64['scale'] < 1.0) == (gscale > 1.0)).all()
        # the clip scale (an fp32 pair) from the squared norm
        sq = sum((g[k].astype(np.float64).reshape(S, -1) ** 2).sum(1) for k in NAMES)
        scale = np.zeros((S, 2), np.float32)
        for s in range(S):
            host.ppo_train_clip(float(sq[s]), HYPER['max_grad_norm'], scale[s].ctypes.data)
        e_ref = np.abs(st32['scale'] - st64['scale']).max()
        err = np.abs(scale.astype(np.float64).sum(1) - st64['scale']).max()
        print('t %d scale: |host - truth| %.3e e_ref %.3e' % (t, err, e_ref))
        assert err <= 4 * e_ref + _ulp(st64['scale']).max()
        for k in NAMES:
            for s in range(S):
                a = [x[k].reshape(S, -1)[s] for x in (p, m, v, g)]
                assert all(x.flags.c_contiguous for x in a)
                host.ppo_train_adam(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, scale[s].ctypes.data, a[0].size,
                                    HYPER['lr'], HYPER['adam_eps'], 0.9, 0.999, t)
        for name, mine, t64, t32, ulps in zip('pmv', (p, m, v), state_arrays(st64), state_arrays(st32), (1.0, 0.0, 0.0)):
            for k in NAMES:
                err, e_ref = np.abs(mine[k].astype(np.float64) - t64[k]), np.abs(t32[k] - t64[k]).max()
                excess = (err - (4 * e_ref + ulps * _ulp(t64[k]))).max()
                assert excess <= 0.0, (t, name, k, err.max(), e_ref)
    assert np.abs(p['fc2_w'] - net.fc2_w.detach().numpy()).max() > 1e-4


def _header():
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        return f.read()


def test_abi_declares_and_exports_the_update():
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = set(re.findall(r'\b(rs_[a-z_]+)\s*\(', text))
    from resco_amd.build import build_library
    build_library()
    L = rsim.load_library()
    for name in PPO_CALLS:
        assert name in declared and name in rsim.ABI_SYMBOLS and hasattr(L, name), name


def _fields(text, name):
    body = text[text.index('typedef struct %s {' % name) + len('typedef struct %s {' % name):text.index('} %s;' % name)]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = re.sub(r'^(float|double)\s*', '', decl.strip())
        names += [n.strip().lstrip('*') for n in decl.split(',') if n.strip()]
    return names


def test_struct_mirrors_list_the_headers_fields():
    text = _header()
    assert [f[0] for f in rsim.PPOTensors._fields_] == _fields(text, 'rs_ppo_tensors') == list(NAMES)
    assert C.sizeof(rsim.PPOTensors) == 8 * 10
    assert [f[0] for f in rsim.PPOConfig._fields_] == _fields(text, 'rs_ppo_config')
    assert C.sizeof(rsim.PPOConfig) == 8 * 8 and 'double lr' in text


def test_update_refuses_cpu_tensors():
    from resco_amd.agents.ippo_learn_fused import FusedPPOLearner
    net, _ = make_net(3, seed=0, cls=BatchedIPPO)
    learner = FusedPPOLearner(net)
    T, N, S = 4, 6, len(net.lanes)

    class CpuRollout:
        def cat(self, name):
            if name == 'obs':
                return torch.zeros(T, N, S, net.lmax, 5, dtype=torch.float16)
            return torch.zeros(T, N, S, dtype=torch.int32 if name == 'act' else torch.float32)

    with pytest.raises(RuntimeError, match='no CPU fallback'):
        learner.update_from_rollout(CpuRollout(), torch.zeros(N, S), torch.zeros(T, dtype=torch.bool))
    ds = dict(obs=torch.zeros(8, S, net.lmax, 5, dtype=torch.float16), act=torch.zeros(8, S, dtype=torch.long), logp=torch.zeros(8, S),
              adv=torch.zeros(8, S), ret=torch.zeros(8, S))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        learner.grad(ds, torch.arange(8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        learner.step()
    assert learner.n_updates == 0
