"""Tests-only helpers of the fused DQN update (resco_amd/csrc/resco_dqn_train.h): kink-free replay rings, the truth its results are
measured against -- BatchedDQNLearner.loss of resco_amd/agents/idqn_learn.py and torch.optim.Adam, evaluated by torch in float64 --
the same in float32, whose distance from the truth is the yardstick e_ref (a candidate gets 4 e_ref per tensor, for a different
fixed summation order and nothing else), the Python twin of the minibatch draw, and the host build of the header's scalar functions
(tests/dqn_train_host).  Everything asserted in here is asserted on the references alone.  What it shares with the PPO update's
reference (tests/ppo_train_ref.py) -- the trunk, the kink-free redraw, Adam from given gradients, the host build -- is tests/train_ref.py.

The net is small and stacked as idqn_kernel_ref.make_net stacks its own (BatchedIDQN.init_like_reference), but of three signals that
pair the extremes: lane counts (2, mid, lmax) with action counts (1, 3, 8)."""
import ctypes as C

import numpy as np
import torch

from idqn_kernel_ref import random_obs
from oracle_batch import murmur_hash
from resco_amd.agents.idqn_rollout import BatchedIDQN
from resco_amd.agents.trunk import fc1_row_mask
from train_ref import adam_step, build_host, fc3_head, grads_as, near_relu_kinks, net_as, redraw_near_kinks, relu_masks, state_arrays, trunk_forward

NAMES = ('conv_w', 'conv_b', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'fc3_w', 'fc3_b')
GAMMA, LR = 0.99, 1e-3
ACTIONS = (1, 3, 8)


def lanes_of(lmax):
    return (2, (2 + lmax) // 2, lmax)


def make_net(lmax, seed):
    net = BatchedIDQN(lanes_of(lmax), ACTIONS)
    net.init_like_reference(seed=seed)
    return net


def forward_all(net, obs):
    """BatchedIDQN.forward restated with every pre-activation returned: conv [n, S, 64, H, 4], z1, z2 [n, S, 64], q [n, S, amax]"""
    c, z1, z2, a2 = trunk_forward(net, obs)
    return c, z1, z2, fc3_head(net, a2)


def _relu_masks(net, obs):
    with torch.no_grad():
        return relu_masks(net, *forward_all(net, torch.from_numpy(obs))[:3])


def _near_kinks(nets64, obs):
    """bool [n, S]: a real unit's pre-activation of one of the nets within TAU of zero"""
    near = np.zeros(obs.shape[:2], bool)
    with torch.no_grad():
        for net in nets64:
            near |= near_relu_kinks(net, *forward_all(net, torch.from_numpy(obs))[:3]).numpy()
    return near


def case(lmax, T, N, seed, done_slots=()):
    """A kink-free ring of T slots x N environments for make_net(lmax): dict(net, target, obs f16 [T, N, S, lmax, 5], act int16, rew
    float32 [T, N, S], done bool [T]).  The rewards put the temporal-difference error of a row at 1.5 x a standard normal draw, so
    that about half of the rows fall on either branch of the Huber loss."""
    net, target = make_net(lmax, seed), make_net(lmax, seed + 1000)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in (net, target):
            m.fc3_w.mul_(10.0)
            m.fc3_b.add_(0.2 * torch.randn(m.fc3_b.shape, generator=g) * m.action_mask)
    rng = np.random.default_rng(seed)
    S = 3
    obs = random_obs(net.lanes, lmax, T * N, rng)
    nets64 = [net_as(net, torch.float64), net_as(target, torch.float64)]
    redraw_near_kinks(obs, net.lanes, rng, lambda o: _near_kinks(nets64, o))
    assert not _near_kinks(nets64, obs).any(), 'the case generator left a kink'
    for m64 in nets64:
        m32 = net_as(m64, torch.float32)
        for a, b in zip(_relu_masks(m64, obs), _relu_masks(m32, obs)):
            assert np.array_equal(a, b), 'float32 and float64 disagree on a ReLU mask'
    act = np.stack([rng.integers(0, a, T * N) for a in net.actions], 1).astype(np.int16).reshape(T, N, S)
    done = np.zeros(T, bool)
    done[list(done_slots)] = True
    obs = obs.reshape(T, N, S, lmax, 5)
    with torch.no_grad():
        q = forward_all(nets64[0], torch.from_numpy(obs.reshape(T * N, S, lmax, 5)))[3].reshape(T, N, S, -1)
        y = q.gather(-1, torch.from_numpy(act).long().unsqueeze(-1)).squeeze(-1)
        nxt = forward_all(nets64[1], torch.from_numpy(obs.reshape(T * N, S, lmax, 5)))[3].reshape(T, N, S, -1).max(-1).values
        boot = GAMMA * torch.roll(nxt, -1, 0) * torch.from_numpy(~done).double().reshape(T, 1, 1)
    rew = (y - boot).numpy() + 1.5 * rng.standard_normal((T, N, S))
    return dict(net=net, target=target, obs=obs, act=act, rew=rew.astype(np.float32), done=done)


def _batch(case, idx, dtype):
    """(o, a, r, o2, d) of DeviceReplay.sample's shapes for idx [B, S, 2]; the successor of a row whose slot ended an episode is
    all zeros (whatever the ring holds there: the bootstrap is cut, so it must never matter)"""
    idx = np.asarray(idx)
    T = case['obs'].shape[0]
    t, e, s = idx[..., 0], idx[..., 1], np.arange(idx.shape[1])[None, :]
    d = case['done'][t]
    o2 = case['obs'][(t + 1) % T, e, s].copy()
    o2[d] = 0
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    return (f(case['obs'][t, e, s]), f(case['act'][t, e, s]).long(), f(case['rew'][t, e, s]).to(dtype), f(o2), f(d).to(dtype))


def _loss(net, target, batch):
    """BatchedDQNLearner.loss restated without its .float() casts -> (per-signal mean Huber loss [S], delta [B, S])"""
    o, a, r, o2, d = batch
    y = net(o).gather(-1, a.unsqueeze(-1)).squeeze(-1)
    with torch.no_grad():
        tgt = r + GAMMA * (1.0 - d) * target(o2).max(dim=-1).values
    return torch.nn.functional.smooth_l1_loss(y, tgt, reduction='none').mean(0), (y - tgt).detach()


def torch_grads(case, idx, dtype, target=None):
    """The loss on rows idx [B, S, 2] in dtype and its backward.  -> (dict name -> float64 numpy gradient, with the fc1 mask of
    BatchedDQNLearner's hook; float64 numpy [S] loss; float64 numpy [B, S] delta = Q[a] - target value)"""
    net, tgt = net_as(case['net'], dtype), net_as(case['target'] if target is None else target, dtype)
    per, delta = _loss(net, tgt, _batch(case, idx, dtype))
    per.sum().backward()
    grads = {k: getattr(net, k).grad.detach().double() for k in NAMES}
    grads['fc1_w'] = grads['fc1_w'] * fc1_row_mask(net.lanes, net.lmax, torch.float64)
    return {k: v.numpy() for k, v in grads.items()}, per.detach().double().numpy(), delta.double().numpy()


def torch_step(params, grads, state, dtype):
    """torch.optim.Adam(lr=1e-3).step from GIVEN gradients in dtype.  params: a BatchedIDQN (read when state is None); grads: dict name
    -> array; state: what the previous call returned, or None.  -> state: dict(net, opt)"""
    return adam_step(params, grads_as(grads, NAMES, dtype), state, dtype, lr=LR)


def torch_update(case, idx, dtype):
    """one whole update (loss, backward, Adam) in dtype -> dict name -> float64 numpy parameters"""
    grads, _, _ = torch_grads(case, idx, dtype)
    return state_arrays(torch_step(case['net'], grads, None, dtype))[0]


def predict_sample(seed, u, S, T, N, head, count, B):
    """the minibatch rs_dqn_sample draws for update u: int32 [B, S, 2] of (slot, environment), from the oracle's counter hash"""
    idx = np.zeros((B, S, 2), np.int32)
    for i in range(B):
        for s in range(S):
            k = murmur_hash(seed, u, s, i, 0) % (count - 1)
            idx[i, s] = ((head - count + k) % T, murmur_hash(seed, u, s, i, 1) % N)
    return idx


RING_STATES = [(2, 1, 0, 2), (5, 7, 3, 3), (5, 7, 1, 5)]      # (T, N, head, count): the smallest ring; not yet full; full and wrapped


def check_sample(idx, T, N, head, count):
    """what every minibatch must satisfy, whoever drew it"""
    t, e = idx[..., 0], idx[..., 1]
    assert ((t >= 0) & (t < T) & (e >= 0) & (e < N)).all()
    assert (t != (head - 1) % T).all(), 'the newest slot has no successor yet'
    if count < T:
        assert (t < count).all(), 'an unwritten slot was drawn'


def build_dqn_train_host(out_dir):
    vp, i32, u32, f32 = C.c_void_p, C.c_int32, C.c_uint32, C.c_float
    return build_host('dqn_train', out_dir, dict(dqn_train_rows=[vp, i32, i32, vp, vp, f32, vp, vp],
                                                 dqn_train_sample=[u32, u32, i32, i32, i32, i32, i32, i32, vp]))
