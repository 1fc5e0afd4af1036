"""The fused FRAP kernel (rs_mplight_act, resco_amd/csrc/resco_frap.h) at every lane-group width against the float64 reference
(tests/frap_ref.py) on synthetic phase-pair sets, no simulator: P = 2, 3, 4 run frap_body<4>, P = 5, 8 frap_body<8>, P = 9, 13, 16
frap_body<16>.  Q under 4 e_ref + 2 ulp32(|Q64|) per class of rows (e_ref from the fp32 PyTorch FRAP on the CPU, never from the kernel),
the greedy margin rule, exact ties, the 0 < epsilon < 1 draws predicted from the counter hash, refresh_on_device at the 8-lane width.
Every launch goes through the C ABI into buffers with sentinel rows behind n_envs, which must stay untouched."""
import copy
import functools

import numpy as np
import pytest
import torch

import frap_ref as fr
from resco_amd.agents.mplight import FusedMPLight
from resco_amd.sim import torch_stream

pytestmark = pytest.mark.gpu
PAIR_COUNTS = [2, 3, 4, 5, 8, 9, 13, 16]
PAD_ROWS = 3
ACT_SENTINEL, F_SENTINEL = -77, -12345.5
N_SIGNALS = 5


def _lanes(P):
    return 4 if P <= 4 else (8 if P <= 8 else 16)


@functools.lru_cache(maxsize=None)
def _case(P, D, n, repeated=False):
    """one synthetic set, network (x 3) and the four classes of n rows each with their float64 truth and fp32 yardstick, computed once"""
    rng = np.random.default_rng(7000 + 100 * P + 10 * D + n + 50 * repeated)
    S = N_SIGNALS if P != 4 else 4
    pairs, valid, order, sc = fr.synthetic_signal_set(P, S, rng, repeated_movement=repeated)
    net = fr.make_net(pairs, D, 3.0, seed=P + D)
    cls = fr.obs_classes(P, D, n, S, rng)
    q64 = {k: fr.frap_ref(net.state_dict(), pairs, D, v).reshape(n, S, P) for k, v in cls.items()}
    q32 = {k: fr.fp32_frap(net, v) for k, v in cls.items()}
    return dict(P=P, D=D, S=S, n=n, pairs=pairs, valid=valid, order=order, sc=sc, net=net, cls=cls, q64=q64, q32=q32)


def _act(pol, obs, eps=0.0, seed=0, step_key=0, env_base=0, dyn=None, want_q=True, want_pair=True):
    """rs_mplight_act through the C ABI on obs [n, S, W] (numpy) into buffers with PAD_ROWS sentinel rows behind n_envs -> numpy
    actions [n, S], pair [n, S] or None, q [n, S, 16] or None.  A buffer that is not asked for is passed as NULL."""
    n, S = obs.shape[:2]
    dev = torch.as_tensor(obs).cuda().contiguous()
    acts = torch.full((n + PAD_ROWS, S), ACT_SENTINEL, dtype=torch.int32, device='cuda')
    pair = torch.full((n + PAD_ROWS, S), ACT_SENTINEL, dtype=torch.int32, device='cuda')
    q = torch.full((n + PAD_ROWS, S, 16), F_SENTINEL, dtype=torch.float32, device='cuda')
    rc = pol._lib.rs_mplight_act(pol._h, dev.data_ptr(), n, int(env_base), float(eps), int(seed) & 0xFFFFFFFF, int(step_key) & 0xFFFFFFFF,
                                 dyn.data_ptr() if dyn is not None else None, acts.data_ptr(), pair.data_ptr() if want_pair else None,
                                 q.data_ptr() if want_q else None, torch_stream(pol.device))
    assert rc == 0
    torch.cuda.synchronize()
    a, p, qq = acts.cpu().numpy(), pair.cpu().numpy(), q.cpu().numpy()
    assert (a[n:] == ACT_SENTINEL).all() and (p[n:] == ACT_SENTINEL).all() and (qq[n:] == F_SENTINEL).all()
    if not want_pair:
        assert (p == ACT_SENTINEL).all()
    if not want_q:
        assert (qq == F_SENTINEL).all()
    assert (a[:n] != ACT_SENTINEL).all()
    return a[:n], (p[:n] if want_pair else None), (qq[:n] if want_q else None)


def _check_q(c):
    P, n, S = c['P'], c['n'], c['S']
    pol = FusedMPLight(c['net'], c['sc'])
    obs = np.concatenate([c['cls'][k] for k in fr.CLASSES])                 # one launch of 4 n rows, judged per class
    act, pair, q = _act(pol, obs)
    pol.close()
    assert np.all(np.isneginf(q[..., P:])) and np.all(np.isfinite(q[..., :P]))
    np.testing.assert_array_equal(act, c['valid'][np.arange(S)[None, :], pair])
    worst = 0.0
    for k, name in enumerate(fr.CLASSES):
        qd = q[k * n:(k + 1) * n, :, :P].astype(np.float64)
        tol, e_ref = fr.q_tolerance(c['q64'][name], c['q32'][name])
        err = np.abs(qd - c['q64'][name])
        ratio = (err / tol).max()
        worst = max(worst, ratio)
        print('G %2d P %2d D %d n %3d %-5s  |dev - truth| %.3e = %.2f e_ref, %.2f of the tolerance  (max |Q| %.3e)' %
              (_lanes(P), P, c['D'], n, name, err.max(), err.max() / max(e_ref, 1e-300), ratio, np.abs(c['q64'][name]).max()))
        assert np.all(err <= tol), (name, err.max(), e_ref, ratio)
    print('G %2d P %2d D %d n %3d worst %.2f of the tolerance' % (_lanes(P), P, c['D'], n, worst))


@pytest.mark.parametrize('n', [1, 131])
@pytest.mark.parametrize('D', [1, 4])
@pytest.mark.parametrize('P', PAIR_COUNTS)
def test_q_against_float64(P, D, n):
    _check_q(_case(P, D, n))


@pytest.mark.parametrize('D', [1, 4])
def test_q_with_a_pair_that_repeats_a_movement(D):
    """[m, m] against a pair that shares nothing: three distinct movements, so the reference's relation bit is 1 (frap_comp)"""
    c = _case(5, D, 131, True)
    assert len(set(c['pairs'][0].tolist() + c['pairs'][1].tolist())) == 3
    _check_q(c)


@pytest.mark.parametrize('n', [1, 131])
@pytest.mark.parametrize('D', [1, 4])
@pytest.mark.parametrize('P', PAIR_COUNTS)
def test_greedy_pair_and_action(P, D, n):
    """The margin rule on the `small` class (wide and sat rows saturate into exact symmetries, zero rows are all alike: those get the
    Q bound only).  At most 10 % of the rows may lie below the margin: a condition on the fixture (float64 truth and e_ref, both from
    the CPU), not on the kernel; with n = 1 there are S rows, so there it means none."""
    c = _case(P, D, n)
    S = c['S']
    pol = FusedMPLight(c['net'], c['sc'])
    obs = c['cls']['small']
    act, pair, _ = _act(pol, obs)
    act2, pair2, _ = _act(pol, obs, want_q=False)                           # pruned: only the valid pairs' Q
    act3, _, _ = _act(pol, obs, want_q=False, want_pair=False)              # nothing but actions
    pol.close()
    _, e_ref = fr.q_tolerance(c['q64']['small'], c['q32']['small'])
    share = fr.greedy_check(pair, c['q64']['small'], c['order'], e_ref)
    print('G %2d P %2d D %d n %3d small  rows below the 8 e_ref margin: %.1f %%' % (_lanes(P), P, D, n, 100 * share))
    assert share <= 0.10
    np.testing.assert_array_equal(act, c['valid'][np.arange(S)[None, :], pair])
    assert act2.tobytes() == act.tobytes() and pair2.tobytes() == pair.tobytes() and act3.tobytes() == act.tobytes()


@pytest.mark.parametrize('P', [4, 8, 13])
def test_exact_ties_take_the_first_pair_in_dict_order(P):
    """before_merge.weight = 0, bias = 0.5: every y_ij is 0.5 and every Q is (P - 1) / 2 exactly, in any summation order"""
    c = _case(P, 1, 131)
    net = copy.deepcopy(c['net'])
    with torch.no_grad():
        net.before_merge.weight.zero_()
        net.before_merge.bias.fill_(0.5)
    order, S = c['order'], c['S']
    first = order[:, 0]
    counts = (order >= 0).sum(1)
    skewed = [s for s in range(S) if counts[s] > 1]
    assert skewed and all(first[s] != order[s][order[s] >= 0].min() for s in skewed)   # lowest pair index != first in dict order
    pol = FusedMPLight(net, c['sc'])
    obs = np.concatenate([c['cls'][k] for k in fr.CLASSES])
    act, pair, q = _act(pol, obs)
    act2, pair2, _ = _act(pol, obs, want_q=False)
    pol.close()
    assert np.all(q[..., :P] == np.float32((P - 1) / 2.0))
    np.testing.assert_array_equal(pair, np.broadcast_to(first[None, :], pair.shape))
    np.testing.assert_array_equal(pair2, pair)
    assert not act.any() and not act2.any()                                 # the first pair in dict order is local action 0


def test_one_valid_pair_per_signal():
    P, S, n = 8, 4, 131
    rng = np.random.default_rng(81)
    pairs, valid, order, sc = fr.synthetic_signal_set(P, S, rng, counts=[1] * S)
    net = fr.make_net(pairs, 1, 3.0, seed=8)
    obs = fr.obs_classes(P, 1, n, S, rng)['small']
    pol = FusedMPLight(net, sc)
    E = fr.EPS_CASE
    for eps in (0.0, E['eps']):
        for want_q in (True, False):
            act, pair, _ = _act(pol, obs, eps=eps, seed=E['seed'], step_key=E['step_key'], env_base=E['env_base'], want_q=want_q)
            np.testing.assert_array_equal(pair, np.broadcast_to(order[None, :, 0], pair.shape))
            assert not act.any()
    pol.close()


@pytest.mark.parametrize('P', [4, 8, 13])
def test_epsilon_between_zero_and_one_follows_the_counter_hash(P):
    c = _case(P, 1, 131)
    E, order, S, n = fr.EPS_CASE, c['order'], c['S'], c['n']
    pol = FusedMPLight(c['net'], c['sc'], seed=E['seed'])
    obs = c['cls']['small']
    kw = dict(seed=E['seed'], step_key=E['step_key'], env_base=E['env_base'])
    _, greedy, q0 = _act(pol, obs, **kw)
    want, mask = fr.select_pairs(None, order, eps=E['eps'], greedy=greedy, **kw)
    assert 0.20 <= mask.mean() <= 0.55                                      # a sanity bound on the fixture, from the hash alone
    print('P %2d: %.1f %% of %d rows explore' % (P, 100 * mask.mean(), n * S))
    dyn = torch.tensor(np.array([np.float32(E['eps']).view(np.int32), np.int64(E['step_key']).astype(np.int32)], np.int32), device='cuda')
    runs = [_act(pol, obs, eps=E['eps'], **kw),
            _act(pol, obs, eps=E['eps'], want_q=False, **kw),
            _act(pol, obs, eps=0.0, seed=E['seed'], step_key=1, env_base=E['env_base'], dyn=dyn),
            _act(pol, obs, eps=0.0, seed=E['seed'], step_key=1, env_base=E['env_base'], dyn=dyn, want_q=False)]
    pol.close()
    for act, pair, q in runs:
        # explorers hold the k-th valid pair of the word-1 hash, the rest the greedy pair of the epsilon = 0 launch
        np.testing.assert_array_equal(pair, want)
        np.testing.assert_array_equal(act, c['valid'][np.arange(S)[None, :], pair])
        if q is not None:
            assert q.tobytes() == q0.tobytes()                              # the Q-values do not depend on who explores
    moved = want != greedy
    assert moved.any() and not (moved & ~mask).any()


def test_refresh_on_device_equals_refresh_at_eight_lanes():
    c = _case(8, 1, 131)
    net = copy.deepcopy(c['net']).cuda()
    pol = FusedMPLight(net, c['sc'])
    obs = c['cls']['wide']
    _, _, q_before = _act(pol, obs)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in net.parameters():                                          # perturb every parameter
            p.add_((0.05 * torch.randn(p.shape, generator=gen)).cuda())
    pol.refresh_on_device()
    _, _, qa = _act(pol, obs)
    pol.refresh()
    _, _, qb = _act(pol, obs)
    pol.close()
    assert qa.tobytes() == qb.tobytes()
    assert not np.array_equal(qa[..., :8], q_before[..., :8])
