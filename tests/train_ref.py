"""Tests-only: what the references of the two fused updates share (tests/dqn_train_ref.py, tests/ppo_train_ref.py; the networks are
one trunk, resco_amd/agents/trunk.py) and what their GPU tests share (tests/test_gpu_dqn_train.py, tests/test_gpu_ppo_train.py).

The yardstick of both: truth = torch in float64, e_ref = torch in float32 against it, a candidate gets 4 e_ref per tensor, for a
different fixed summation order and nothing else.  Cases are kept TAU away from every ReLU's zero, so that float32 and float64 take
the same branches.  Everything asserted on the way to a case is asserted on the references alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 2e-5                  # distance kept from a ReLU's zero


def param_names(net):
    return tuple(k for k, _ in net.named_parameters())


def net_as(net, dtype):
    """a network of net's class and signals with net's parameters in `dtype` (CPU)"""
    m = type(net)(net.lanes, net.actions, dtype=dtype)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(getattr(net, k).detach().cpu().to(dtype))
    return m


# ---- the trunk with every pre-activation, and the cases that stay away from its kinks
def trunk_forward(net, obs):
    """BatchedTrunk.features restated with every pre-activation returned: conv [n, S, 64, H, 4], z1, z2 [n, S, 64], and the
    features [S, n, 64] the heads read -- in the dtype of net's parameters"""
    n, S = obs.shape[0], obs.shape[1]
    H = net.lmax - 1
    c = torch.nn.functional.conv2d(obs.to(net.conv_w.dtype), net.conv_w, net.conv_b, groups=S)
    y = torch.relu(c).reshape(n, S, -1).transpose(0, 1)
    z1 = torch.baddbmm(net.fc1_b.unsqueeze(1), y, net.fc1_w)
    z2 = torch.baddbmm(net.fc2_b.unsqueeze(1), torch.relu(z1), net.fc2_w)
    return c.reshape(n, S, 64, H, 4), z1.transpose(0, 1), z2.transpose(0, 1), torch.relu(z2)


def fc3_head(net, a2):
    """fc3 on the features: [n, S, amax], -inf beyond a signal's actions"""
    return torch.baddbmm(net.fc3_b.unsqueeze(1), a2, net.fc3_w).transpose(0, 1).masked_fill(~net.action_mask, float('-inf'))


def _real_conv(net):
    """bool [S, 1, H, 1]: conv rows a signal really has (h < L_s - 1)"""
    H = net.lmax - 1
    return (torch.arange(H)[None, :] < (torch.tensor(net.lanes)[:, None] - 1)).reshape(len(net.lanes), 1, H, 1)


def near_relu_kinks(net, c, z1, z2):
    """bool tensor [n, S]: a real unit's pre-activation within TAU of zero"""
    return ((c.abs() < TAU) & _real_conv(net)).flatten(2).any(-1) | (z1.abs() < TAU).any(-1) | (z2.abs() < TAU).any(-1)


def relu_masks(net, c, z1, z2):
    """which real units are on: numpy bool (conv, fc1, fc2)"""
    return ((c > 0) & _real_conv(net)).numpy(), (z1 > 0).numpy(), (z2 > 0).numpy()


def redraw_near_kinks(obs, lanes, rng, near):
    """observations whose forward comes near a ReLU's zero (near(obs) -> numpy bool [n, S]) are drawn again, in place"""
    for _ in range(100):
        hit = near(obs)
        if not hit.any():
            break
        for r, s in zip(*np.nonzero(hit)):
            obs[r, s, :lanes[s]] = rng.random((lanes[s], 5)).astype(np.float16)


# ---- Adam from given gradients
def grads_as(grads, names, dtype):
    return {k: torch.as_tensor(np.asarray(grads[k])).to(dtype).clone() for k in names}


def adam_step(params, g, state, dtype, **adam):
    """torch.optim.Adam(**adam).step from GIVEN gradients g (name -> tensor in dtype).  params: the network (read when state is None);
    state: what the previous call returned, or None.  -> state: dict(net, opt)"""
    if state is None:
        net = net_as(params, dtype)
        state = dict(net=net, opt=torch.optim.Adam(net.parameters(), **adam))
    for k, p in state['net'].named_parameters():
        p.grad = g[k].reshape(p.shape)
    state['opt'].step()
    return state


def state_arrays(state):
    """(params, m, v): dicts name -> float64 numpy of an adam_step state"""
    net, opt = state['net'], state['opt']
    f = lambda t: t.detach().double().numpy()
    names = param_names(net)
    return ({k: f(getattr(net, k)) for k in names}, {k: f(opt.state[getattr(net, k)]['exp_avg']) for k in names},
            {k: f(opt.state[getattr(net, k)]['exp_avg_sq']) for k in names})


def build_host(name, out_dir, signatures):
    """tests/<name>_host/<name>_host.cpp: the scalar functions of a header of resco_amd/csrc, compiled for the host without
    contraction.  signatures: function -> argtypes, or (argtypes, restype)"""
    out = os.path.join(str(out_dir), name + '_host.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math', '-shared',
                           '-I' + os.path.join(ROOT, 'resco_amd', 'csrc'), os.path.join(ROOT, 'tests', name + '_host', name + '_host.cpp'),
                           '-o', out])
    L = C.CDLL(out)
    for fn, sig in signatures.items():
        if isinstance(sig, tuple):
            getattr(L, fn).argtypes, getattr(L, fn).restype = sig
        else:
            getattr(L, fn).argtypes = sig
    return L


# ---- the GPU tests' side
def _np(d):
    """name -> numpy copy of a dict of device tensors or of a network's parameters, after the device has finished"""
    torch.cuda.synchronize()
    items = d.items() if isinstance(d, dict) else d.named_parameters()
    return {k: v.detach().cpu().numpy().copy() for k, v in items}


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _device_net(net):
    m = type(net)(net.lanes, net.actions)
    m.load_state_dict(net.state_dict())
    return m.cuda()


def check_4_e_ref(name, got, t64, t32, worst):
    """prints |got - truth| next to e_ref = |float32 - truth|; more than 4 e_ref is added to `worst`"""
    err, e_ref = np.abs(got.astype(np.float64) - t64).max(), np.abs(t32 - t64).max()
    print('  %-12s max |truth| %.3e  |dev - truth| %.3e  e_ref %.3e  ratio %.2f' % (name, np.abs(t64).max(), err, e_ref, err / max(e_ref, 1e-300)))
    if err > 4 * e_ref:
        worst.append((name, err, e_ref))


def compare_gradients(names, got, g64, g32):
    """every tensor finite and within 4 e_ref of the truth -> the list of those that are not, for the caller to extend and assert"""
    worst = []
    for k in names:
        assert np.isfinite(got[k]).all(), k
        check_4_e_ref(k, got[k], g64[k], g32[k], worst)
    return worst


def assert_adam_state(t, names, mine, st64, st32):
    """mine = (parameters, m, v) of the device after step t against adam_step states in float64 and float32: 4 e_ref per tensor,
    plus one float32 ulp on the parameters"""
    for name, got, t64, t32, ulps in zip(('param', 'm', 'v'), mine, state_arrays(st64), state_arrays(st32), (1.0, 0.0, 0.0)):
        for k in names:
            err, e_ref = np.abs(got[k].astype(np.float64) - t64[k]), np.abs(t32[k] - t64[k]).max()
            excess = (err - (4 * e_ref + ulps * _ulp(t64[k]))).max()
            if excess > 0:
                print('t %d %s %s: |dev - truth| %.3e e_ref %.3e' % (t, name, k, err.max(), e_ref))
            assert excess <= 0.0, (t, name, k, err.max(), e_ref)
