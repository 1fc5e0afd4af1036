"""CPU: the rounding-faithful reference of the fused IDQN forward (tests/idqn_kernel_ref.py) reads pack_idqn_weights' fragments with
the kernel's index arithmetic and computes the reference architecture (pfrl_dqn.py:30-39) for every head size HP = 1..8, every lane
count 2..17 and every action count 1..8; the device re-pack of FusedIDQN.refresh_on_device yields pack_idqn_weights' fragments."""
import numpy as np
import pytest
import torch

from idqn_kernel_ref import QMAX, first_max, idqn_kernel_ref, make_net, random_obs, select_actions
from resco_amd.agents.idqn_fused import pack_idqn_weights, repack_index
from resco_amd.agents.idqn_rollout import BatchedIDQN
from resco_amd.sim import _murmur

LMAX = (2, 3, 9, 16, 17)


def fp16_weights(net, mods):
    """round what the kernel reads as fp16 (conv weight + bias, fc weights) to fp16 values in the modules, keep the fc biases fp32"""
    with torch.no_grad():
        for m in mods:
            for p in (m[0].weight, m[0].bias, m[3].weight, m[5].weight, m[7].weight):
                p.copy_(p.half().float())
    net.load_reference_modules(mods)
    return pack_idqn_weights(net)


@pytest.mark.parametrize('lmax', LMAX)
def test_unrounded_reference_equals_the_per_signal_modules(lmax):
    net, mods = make_net(lmax, seed=lmax)
    with torch.no_grad():                                   # Q of O(1), not the fresh 1e-2 head
        for m in mods:
            m[7].weight.mul_(30.0)
    pk = fp16_weights(net, mods)
    n = 7
    obs = random_obs(net.lanes, lmax, n, np.random.default_rng(lmax))
    q, bound = idqn_kernel_ref(pk, net.lanes, obs, n, rounding=False)
    assert q.shape == (n, len(net.lanes), QMAX)
    for s, (L, A) in enumerate(zip(net.lanes, net.actions)):
        ref = mods[s].double()(torch.from_numpy(obs[:, s, :L].astype(np.float64)).unsqueeze(1)).detach().numpy()
        scale = np.abs(ref).max()
        assert scale > 0.05
        np.testing.assert_allclose(q[:, s, :A], ref, rtol=1e-9, atol=1e-9 * scale)
        assert np.isneginf(q[:, s, A:]).all() and not bound[:, s, A:].any()
        assert (bound[:, s, :A] > 0).all() and (bound[:, s, :A] < 1e-2 * scale).all()      # fp32 accumulation only


@pytest.mark.parametrize('lmax', LMAX)
def test_rounded_reference_stays_near_the_fp32_forward(lmax):
    """the fp16 emulation is a small perturbation of the fp32 network (and its bound is a small fraction of |Q|)"""
    net, _ = make_net(lmax, seed=lmax + 1)
    with torch.no_grad():
        net.fc3_w.mul_(30.0)
    pk = pack_idqn_weights(net)
    n = 40
    obs = random_obs(net.lanes, lmax, n, np.random.default_rng(lmax + 1))
    q, bound = idqn_kernel_ref(pk, net.lanes, obs, n)
    ref = net(torch.from_numpy(obs.astype(np.float32))).detach().numpy()
    ok = np.isfinite(ref)
    assert np.array_equal(ok, np.isfinite(q))
    assert np.abs(q[ok] - ref[ok]).max() < 3e-2
    scale = np.abs(ref[ok]).max()
    assert 0.3 < scale < 10.0
    assert bound[ok].max() < 1e-2 * scale and np.median(bound[ok]) < 1e-2 * np.median(np.abs(q[ok]))
    # hp_sig beyond the signal's own k-steps (rs_idqn_set_lanes with lmax everywhere): the extra fc1 rows are zero
    q_all, _ = idqn_kernel_ref(pk, [lmax] * len(net.lanes), obs, n)
    np.testing.assert_allclose(q_all, q, rtol=0, atol=1e-12)


@pytest.mark.parametrize('lmax', range(2, 18))
@pytest.mark.parametrize('amax', range(1, 9))
def test_device_repack_index_reproduces_pack_idqn_weights(lmax, amax):
    """refresh_on_device's gather (index_select + mask + casting copy over repack_index) == pack_idqn_weights, fragment for fragment"""
    S = 2
    net = BatchedIDQN([lmax, max(2, lmax - 3)], [amax, max(1, amax - 2)])
    g = torch.Generator().manual_seed(lmax * 10 + amax)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    pk = pack_idqn_weights(net)
    for k, w in repack_index(lmax, amax).items():
        idx = torch.as_tensor(np.maximum(w, 0))
        mask = torch.as_tensor((w >= 0).astype(np.float32))
        src = {'w1': net.fc1_w, 'w2': net.fc2_w, 'w3': net.fc3_w}[k]
        got = torch.empty(S, len(w), dtype=torch.float16)
        got.copy_(torch.index_select(src.detach().reshape(S, -1).float(), 1, idx).mul_(mask))
        got = got.numpy()
        want = pk[k].reshape(S, -1)
        assert got.shape == want.shape
        pad = w < 0
        assert (want[:, pad] == 0).all() and (got[:, pad] == 0).all()          # (+0 or -0: a masked product of a negative weight)
        assert np.array_equal(got[:, ~pad].view(np.uint16), want[:, ~pad].view(np.uint16))


def test_selection_restates_the_epilogue():
    """first maximum with strict >, padded columns never win; the epsilon draw and the categorical draw by the hash words 0/1 and 2"""
    q = np.full((4, 2, QMAX), -np.inf)
    q[0, 0, :3] = [0.5, 0.5, 0.1]               # tie: the lower index
    q[1, 0, :3] = [-2.0, -1.0, -1.0]
    q[2, 0, :3] = [-3.0, -1.0, -0.5]
    q[3, 0, :3] = [1.0, 2.0, 2.0]
    q[:, 1, :1] = -4.0                          # one action
    q[:, 1, 1:] = 0.0                           # padded columns above every valid Q must not be chosen
    na = [3, 1]
    assert first_max(q, na).tolist() == [[0, 0], [1, 0], [2, 0], [1, 0]]
    a, margin = select_actions(q, na, mode=0, eps=0.0)
    assert a.tolist() == [[0, 0], [1, 0], [2, 0], [1, 0]] and np.isinf(margin).all()
    key = 7 ^ 0x1D0A17
    a, _ = select_actions(q, na, mode=0, eps=1.0, seed=7, env_base=100, step_key=9)
    assert a[:, 1].tolist() == [0] * 4
    assert a[:, 0].tolist() == [_murmur(key, (100 + m, 0, 9, 1)) % 3 for m in range(4)]
    a, margin = select_actions(q, na, mode=1, seed=7, env_base=100, step_key=9)
    assert a[:, 1].tolist() == [0] * 4 and np.isinf(margin[:, 1]).all()
    for m in range(4):
        e = np.exp(q[m, 0, :3] - q[m, 0, :3].max())
        t = (_murmur(key, (100 + m, 0, 9, 2)) >> 8) / 2.0 ** 24 * e.sum()
        assert a[m, 0] == int(np.searchsorted(np.cumsum(e), t, side='right'))
