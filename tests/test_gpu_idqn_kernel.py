"""GPU: rs_idqn_forward_kernel (resco_amd/csrc/resco_policy.h) against the rounding-faithful reference of tests/idqn_kernel_ref.py,
element-wise within the reference's error bound, for every head size HP = 1..8 (odd and even lane counts), every action count 1..8,
batch sizes around the 64-environment workgroup; the epilogue (greedy first maximum, epsilon-greedy and categorical draws) row for
row; no writes past n_envs; padded lanes; device re-pack; the ABI's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from idqn_kernel_ref import QMAX, first_max, idqn_kernel_ref, make_net, random_obs, select_actions
from resco_amd.agents.idqn_fused import FusedIDQN, pack_idqn_weights
from resco_amd.sim import torch_stream

pytestmark = pytest.mark.gpu

ACT_SENTINEL, Q_SENTINEL, PAD_ROWS = -777, 1234.5, 3
# (lmax, n_envs): the networks of make_net cover lane counts 2..lmax, the batches one partial / full / one-over workgroup
CASES = [(2, 64), (3, 65), (9, 1), (9, 130), (16, 63), (17, 1000)]


def _net(lmax, seed, cls=None, fc3_scale=30.0):
    net, _ = make_net(lmax, seed=seed, cls=cls)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                       # Q of O(1) (the fresh head gives ~1e-2) and not all alike
        net.fc3_w.mul_(fc3_scale)
        net.fc3_b.add_(0.2 * torch.randn(net.fc3_b.shape, generator=g) * net.action_mask)
    return net.cuda()


def _act(fused, obs, n, mode=0, eps=0.0, step_key=0, env_base=0):
    """rs_idqn_act into buffers with PAD_ROWS sentinel rows after n_envs; asserts they stay untouched.  -> numpy actions, Q"""
    S = fused.S
    acts = torch.full((n + PAD_ROWS, S), ACT_SENTINEL, dtype=torch.int32, device='cuda')
    q = torch.full((n + PAD_ROWS, S, QMAX), Q_SENTINEL, dtype=torch.float32, device='cuda')
    rc = fused._lib.rs_idqn_act(fused._h, obs.data_ptr(), n, env_base, mode, float(eps), fused.seed, step_key & 0xFFFFFFFF, None,
                                acts.data_ptr(), q.data_ptr(), torch_stream(fused.device))
    assert rc == 0
    torch.cuda.synchronize()
    a, qn = acts.cpu().numpy(), q.cpu().numpy()
    assert (a[n:] == ACT_SENTINEL).all() and (qn[n:] == Q_SENTINEL).all()
    return a[:n], qn[:n]


def _check_q(q, n_actions, ref, bound, what):
    """q_out within the bound of the reference, exactly -inf beyond each signal's actions; prints the largest error / bound"""
    valid = np.arange(QMAX)[None, None, :] < np.asarray(n_actions)[None, :, None]
    valid = np.broadcast_to(valid, q.shape)
    assert np.isneginf(q[~valid]).all()
    assert np.isfinite(q[valid]).all()
    ratio = np.abs(q[valid].astype(np.float64) - ref[valid]) / bound[valid]
    print('%s: max |q - ref| / bound = %.3f (median bound / |Q| %.1e)' % (what, ratio.max(), np.median(bound[valid] / np.abs(ref[valid]))))
    assert ratio.max() <= 1.0, ratio.max()


def _set_lanes(fused, lanes):
    arr = np.asarray(lanes, np.int32)
    return fused._lib.rs_idqn_set_lanes(fused._h, arr.ctypes.data)


@pytest.mark.parametrize('lmax,n', CASES)
def test_kernel_against_rounding_faithful_reference(lmax, n):
    net = _net(lmax, seed=lmax * 7 + n)
    S, na = len(net.lanes), net.actions
    rng = np.random.default_rng(lmax + n)
    obs = random_obs(net.lanes, lmax, n, rng)
    obs_t = torch.from_numpy(obs).cuda()
    fused = FusedIDQN(net, seed=1234 + n)
    pk = pack_idqn_weights(net)
    ref, bound = idqn_kernel_ref(pk, net.lanes, obs, n)

    # Q within the bound; greedy = the first maximum of the kernel's own Q, and the reference's choice where that is clear
    acts, q = _act(fused, obs_t, n)
    _check_q(q, na, ref, bound, 'lmax %d n %d' % (lmax, n))
    assert np.array_equal(acts, first_max(q, na))
    top2 = -np.sort(-ref, axis=-1)[..., :2]
    clear = (np.asarray(na)[None, :] == 1) | (top2[..., 0] - top2[..., 1] > 2 * bound.max(-1))
    assert clear.mean() > 0.7
    assert np.array_equal(acts[clear], first_max(ref, na)[clear])

    # epsilon-greedy with a non-zero env_base and step key: every row is the formula (the kernel's own greedy where u >= eps)
    acts_e, q_e = _act(fused, obs_t, n, eps=0.37, step_key=0x9E3779B9, env_base=1000)
    assert np.array_equal(q_e, q)
    want, _ = select_actions(q, na, mode=0, eps=0.37, seed=fused.seed, env_base=1000, step_key=0x9E3779B9)
    assert np.array_equal(acts_e, want)
    if n >= 64:
        assert 0.1 < (acts_e != acts).mean() < 0.37

    # finite garbage in the observation rows past each signal's lanes: the same Q, bit for bit
    garbage = obs.copy()
    for s, L in enumerate(net.lanes):
        garbage[:, s, L:] = rng.uniform(-4.0, 4.0, (n, lmax - L, 5)).astype(np.float16)
    _, q_g = _act(fused, torch.from_numpy(garbage).cuda(), n)
    assert np.array_equal(q_g.view(np.uint32), q.view(np.uint32))

    # every k-step run (rs_idqn_set_lanes with lmax everywhere): within the bound of the reference that runs them all too
    assert _set_lanes(fused, [lmax] * S) == 0
    _, q_all = _act(fused, obs_t, n)
    ref_all, bound_all = idqn_kernel_ref(pk, [lmax] * S, obs, n)
    _check_q(q_all, na, ref_all, bound_all, 'lmax %d n %d, all k-steps' % (lmax, n))
    assert _set_lanes(fused, net.lanes) == 0

    # weights changed as a learner changes them, re-packed on the device and on the host: the same Q, that of the new weights
    g = torch.Generator(device='cuda').manual_seed(n)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g, device='cuda') * (p != 0))
    fused.refresh_on_device()
    _, q_dev = _act(fused, obs_t, n)
    fused.refresh()
    _, q_host = _act(fused, obs_t, n)
    assert np.array_equal(q_dev.view(np.uint32), q_host.view(np.uint32)) and not np.array_equal(q_dev, q)
    if n <= 130:
        ref2, bound2 = idqn_kernel_ref(pack_idqn_weights(net), net.lanes, obs, n)
        _check_q(q_dev, na, ref2, bound2, 'lmax %d n %d, re-packed' % (lmax, n))
    fused.close()


def test_greedy_ties_and_all_negative_q():
    """Duplicated fc3 columns (weights and bias) give exact ties in q_out: the lowest tied index is chosen (strict >).  With every
    valid Q below zero, the padded columns (Q = 0 inside the kernel) must not win: the argmax runs over the signal's actions only."""
    lmax, n = 16, 130
    net = _net(lmax, seed=5)
    na = net.actions
    with torch.no_grad():
        for s, A in enumerate(na):
            if A >= 2:                          # column A - 1 := column 0; column 2 := column 1
                net.fc3_w[s, :, A - 1] = net.fc3_w[s, :, 0]
                net.fc3_b[s, A - 1] = net.fc3_b[s, 0]
            if A >= 4:
                net.fc3_w[s, :, 2] = net.fc3_w[s, :, 1]
                net.fc3_b[s, 2] = net.fc3_b[s, 1]
    obs = random_obs(net.lanes, lmax, n, np.random.default_rng(3))
    obs_t = torch.from_numpy(obs).cuda()
    fused = FusedIDQN(net, seed=3)
    acts, q = _act(fused, obs_t, n)
    assert np.array_equal(acts, first_max(q, na))
    mx = np.where(np.arange(QMAX) < np.asarray(na)[:, None], q, -np.inf).max(-1)
    n_top = ((q == mx[..., None]) & (np.arange(QMAX) < np.asarray(na)[:, None])).sum(-1)
    tied = n_top > 1
    assert tied.sum() > n // 2                  # many rows hold an exact tie at the top
    assert (acts[tied] == np.argmax(q[tied] == mx[tied][:, None], axis=-1)).all()

    with torch.no_grad():
        net.fc3_b.sub_(10.0 * net.action_mask)
    fused.refresh()
    acts, q = _act(fused, obs_t, n)
    valid = np.arange(QMAX)[None, None, :] < np.asarray(na)[None, :, None]
    assert (np.broadcast_to(q < -1.0, q.shape) | ~valid).all()
    assert (acts < np.asarray(na)[None, :]).all() and (acts >= 0).all()
    assert np.array_equal(acts, first_max(q, na))
    ref, bound = idqn_kernel_ref(pack_idqn_weights(net), net.lanes, obs, n)
    _check_q(q, na, ref, bound, 'negative Q')
    fused.close()


@pytest.mark.parametrize('lmax,n', [(9, 1000), (17, 257)])
def test_sampling_mode_is_the_categorical_draw(lmax, n):
    """mode 1 (the IPPO head on the same trunk): every row is the draw u z against the cumulative exp(q - max) of the kernel's own
    q_out, u from hash word 2; rows whose u z lies within 1e-4 z of a cumulative boundary (the host's exp is not __expf) are skipped"""
    from resco_amd.agents.ippo import BatchedIPPO
    net = _net(lmax, seed=lmax, cls=BatchedIPPO, fc3_scale=40.0)
    na = net.actions
    obs = random_obs(net.lanes, lmax, n, np.random.default_rng(lmax))
    fused = FusedIDQN(net, seed=21)
    acts, q = _act(fused, torch.from_numpy(obs).cuda(), n, mode=1, step_key=5, env_base=77)
    ref, bound = idqn_kernel_ref(pack_idqn_weights(net), net.lanes, obs, n)
    _check_q(q, na, ref, bound, 'IPPO trunk lmax %d' % lmax)
    want, margin = select_actions(q, na, mode=1, seed=21, env_base=77, step_key=5)
    checked = margin > 1e-4
    assert checked.mean() >= 0.99
    assert np.array_equal(acts[checked], want[checked])
    greedy = first_max(q, na)
    assert 0.05 < (acts != greedy)[np.asarray(na)[None, :].repeat(n, 0) > 1].mean() < 0.95     # the policy is neither greedy nor uniform
    fused.close()


def test_refusals():
    """rs_idqn_create: lmax outside 2..17, action counts outside 1..8; rs_idqn_set_lanes: lane counts outside 2..lmax (the handle keeps
    working as before); FusedIDQN: non-zero fc1 rows on a padded lane"""
    from resco_amd.agents.idqn_rollout import BatchedIDQN
    lmax, n = 9, 64
    net = _net(lmax, seed=1)
    fused = FusedIDQN(net, seed=1)
    L = fused._lib
    pk = pack_idqn_weights(net)
    S = len(net.lanes)

    def create(lm, n_actions):
        h = C.c_void_p()
        arrays = dict(pk, n_actions=np.asarray(n_actions, np.int32))
        rc = L.rs_idqn_create(0, S, lm, *[arrays[k].ctypes.data for k in
                                          ('n_actions', 'conv_w', 'conv_b', 'w1', 'b1', 'w2', 'b2', 'w3', 'b3')], C.byref(h))
        if rc == 0:
            L.rs_idqn_destroy(h)
        return rc, h.value

    assert create(lmax, net.actions)[0] == 0
    for lm in (1, 18):
        rc, h = create(lm, net.actions)
        assert rc != 0 and h is None
    for bad in (0, 9):
        acts = list(net.actions)
        acts[S // 2] = bad
        rc, h = create(lmax, acts)
        assert rc != 0 and h is None

    obs_t = torch.from_numpy(random_obs(net.lanes, lmax, n, np.random.default_rng(0))).cuda()
    _, q0 = _act(fused, obs_t, n)
    for bad in (1, lmax + 1):
        lanes = list(net.lanes)
        lanes[1] = bad
        assert _set_lanes(fused, lanes) != 0
    _, q1 = _act(fused, obs_t, n)
    assert np.array_equal(q0.view(np.uint32), q1.view(np.uint32))
    fused.close()

    bad_net = BatchedIDQN([3, 6], [2, 4], device='cuda')
    bad_net.init_like_reference(seed=0)
    with torch.no_grad():
        bad_net.fc1_w[0].view(64, 5, 4, 64)[7, 2, 1, 3] = 0.25        # signal 0 observes 3 lanes: conv row h = 2 is padding
    with pytest.raises(ValueError, match='padded lanes'):
        FusedIDQN(bad_net)
