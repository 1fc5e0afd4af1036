"""Tests-only helpers of the fused PPO update (resco_amd/csrc/resco_ppo_train.h): kink-free cases, the truth its results are measured
against -- the loss of BatchedPPOLearner.loss, clip_grad_per_signal and torch.optim.Adam of resco_amd/agents/ippo.py, evaluated by
torch in float64 -- the same in float32, whose distance from the truth is the yardstick e_ref (a candidate gets 4 e_ref per tensor,
for a different fixed summation order and nothing else), and the host build of the header's scalar functions (tests/ppo_train_host).
Everything asserted in here is asserted on the references alone.  What it shares with the DQN update's reference
(tests/dqn_train_ref.py) -- the trunk, the kink-free redraw, Adam from given gradients, the host build -- is tests/train_ref.py."""
import ctypes as C

import numpy as np
import torch

from idqn_kernel_ref import make_net, random_obs
from resco_amd.agents.ippo import BatchedIPPO
from train_ref import adam_step, build_host, fc3_head, grads_as, near_relu_kinks, net_as, redraw_near_kinks, relu_masks, state_arrays, trunk_forward  # noqa: F401

RATIO_GAP = 1e-4                            # distance kept from ratio = 1 -+ clip_eps (from a ReLU's zero: train_ref.TAU)
HYPER = dict(lr=2.5e-4, adam_eps=1e-5, clip_eps=0.1, entropy_coef=0.001, value_coef=1.0, max_grad_norm=0.5)
NAMES = ('conv_w', 'conv_b', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'fc3_w', 'fc3_b', 'v_w', 'v_b')


def forward_all(net, obs):
    """BatchedIPPO.forward restated with every pre-activation returned: conv [B, S, 64, H, 4], z1, z2 [B, S, 64], logits [B, S, amax]
    (-inf beyond a signal's actions), value [B, S] -- in the dtype of net's parameters"""
    c, z1, z2, a2 = trunk_forward(net, obs)
    return c, z1, z2, fc3_head(net, a2), torch.baddbmm(net.v_b.unsqueeze(1), a2, net.v_w).squeeze(-1).transpose(0, 1)


def _near_kinks(net64, obs, act, logp_old):
    """(bool [n, S]: a real unit's pre-activation within TAU of zero, bool [n, S]: ratio within RATIO_GAP of 1 -+ clip_eps, lp64, v64)"""
    with torch.no_grad():
        c, z1, z2, logits, v = forward_all(net64, torch.from_numpy(obs))
        near = near_relu_kinks(net64, c, z1, z2)
        lp = torch.log_softmax(logits, -1).gather(-1, torch.from_numpy(act).long().unsqueeze(-1)).squeeze(-1)
        if logp_old is None:
            return near, None, lp, v
        ratio = torch.exp(lp - torch.from_numpy(logp_old).double())
        e = HYPER['clip_eps']
        return near, ((ratio - (1 - e)).abs() < RATIO_GAP) | ((ratio - (1 + e)).abs() < RATIO_GAP), lp, v


def relu_masks_and_clipped(net, case):
    with torch.no_grad():
        c, z1, z2, logits, _ = forward_all(net, torch.from_numpy(case['obs']))
        lp = torch.log_softmax(logits, -1).gather(-1, torch.from_numpy(case['act']).long().unsqueeze(-1)).squeeze(-1)
        ratio = torch.exp(lp - torch.from_numpy(case['logp']).to(lp.dtype))
        e = HYPER['clip_eps']
        return relu_masks(net, c, z1, z2) + (((ratio < 1 - e) | (ratio > 1 + e)).numpy(),)


def case(lmax, n, seed):
    """A kink-free dataset of n rows for make_net(lmax): dict(net, obs f16 [n, S, lmax, 5], act int32, logp, adv, ret float32 [n, S])"""
    net, _ = make_net(lmax, seed=seed, cls=BatchedIPPO)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        net.fc3_w.mul_(30.0)
        net.fc3_b.add_(0.2 * torch.randn(net.fc3_b.shape, generator=g) * net.action_mask)
        net.v_b.add_(torch.randn(net.v_b.shape, generator=g))
    rng = np.random.default_rng(seed)
    S = len(net.lanes)
    obs = random_obs(net.lanes, lmax, n, rng)
    act = np.stack([rng.integers(0, a, n) for a in net.actions], 1).astype(np.int32)
    net64 = net_as(net, torch.float64)
    redraw_near_kinks(obs, net.lanes, rng, lambda o: _near_kinks(net64, o, act, None)[0].numpy())      # 1. - 2.
    noise = rng.standard_normal((n, S))
    for _ in range(100):                                # 3. the logp_old noise of samples whose ratio comes near a clip boundary likewise
        _, _, lp, v = _near_kinks(net64, obs, act, None)
        logp = (lp.numpy() + 0.08 * noise).astype(np.float32)
        near_r = _near_kinks(net64, obs, act, logp)[1].numpy()
        if not near_r.any():
            break
        noise[near_r] = rng.standard_normal(int(near_r.sum()))
    adv = rng.standard_normal((n, S)).astype(np.float32)
    ret = (v.numpy() + rng.standard_normal((n, S))).astype(np.float32)
    out = dict(net=net, obs=obs, act=act, logp=logp, adv=adv, ret=ret)
    near, near_r, _, _ = _near_kinks(net64, obs, act, logp)
    assert not near.any() and not near_r.any(), 'the case generator left a kink'
    m64, m32 = relu_masks_and_clipped(net64, out), relu_masks_and_clipped(net_as(net, torch.float32), out)
    for a, b in zip(m64, m32):
        assert np.array_equal(a, b), 'float32 and float64 disagree on a ReLU mask or on the clipped set'
    out['clipped_fraction'] = float(m64[3].mean())
    return out


def torch_grads(case, idx, dtype):
    """BatchedPPOLearner.loss (ippo.py) restated without its .float() casts, on rows idx, in dtype, and its backward.
    -> (dict name -> float64 numpy gradient, with the masks of BatchedIPPO's hooks; float64 numpy [S, 3]: policy, value, entropy term)"""
    net = net_as(case['net'], dtype)
    idx = torch.as_tensor(np.asarray(idx)).long()
    t = lambda k: torch.from_numpy(case[k])[idx]
    logits, v = net(t('obs'))
    lp_all = torch.log_softmax(logits, -1)
    lp = lp_all.gather(-1, t('act').long().unsqueeze(-1)).squeeze(-1)
    ratio = torch.exp(lp - t('logp').to(dtype))
    a = t('adv').to(dtype)
    e = HYPER['clip_eps']
    pg = -torch.minimum(ratio * a, torch.clamp(ratio, 1.0 - e, 1.0 + e) * a).mean(0)
    vf = ((v - t('ret').to(dtype)) ** 2).mean(0)
    ent = -(torch.exp(lp_all) * lp_all.masked_fill(~net.action_mask, 0.0)).sum(-1).mean(0)
    (pg + HYPER['value_coef'] * vf - HYPER['entropy_coef'] * ent).sum().backward()
    grads = {k: getattr(net, k).grad.detach().double().numpy() for k in NAMES}
    return grads, torch.stack([pg, vf, ent], 1).detach().double().numpy()


def torch_step(params, grads, state, dtype):
    """clip_grad_per_signal (restated without its .float() casts) + torch.optim.Adam.step from GIVEN gradients in dtype.
    params: a BatchedIPPO (read when state is None); grads: dict name -> array; state: what the previous call returned, or None.
    -> state: dict(net, opt, scale [S] of this step); the parameters are state['net']'s, the moments state['opt'].state[p]"""
    S = len(params.lanes)
    g = grads_as(grads, NAMES, dtype)
    sq = torch.zeros(S, dtype=dtype)
    for k in NAMES:
        sq += (g[k].reshape(S, -1) ** 2).sum(1)
    scale = torch.clamp(HYPER['max_grad_norm'] / (sq.sqrt() + 1e-6), max=1.0)
    g = {k: g[k].reshape(S, -1) * scale.unsqueeze(1) for k in NAMES}
    state = adam_step(params, g, state, dtype, lr=HYPER['lr'], eps=HYPER['adam_eps'])
    state['scale'] = scale.double().numpy()
    return state


def build_ppo_train_host(out_dir):
    vp, i32, f32, f64 = C.c_void_p, C.c_int32, C.c_float, C.c_double
    return build_host('ppo_train', out_dir, dict(ppo_train_rows=[vp, i32, i32, vp, vp, vp, vp, vp, f32, f32, f32, f32, vp, vp, vp],
                                                 ppo_train_clip=([f64, f64, vp], None),
                                                 ppo_train_adam=[vp, vp, vp, vp, vp, i32, f64, f64, f64, f64, i32]))
