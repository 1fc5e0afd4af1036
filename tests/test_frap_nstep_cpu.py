"""CPU: the target's options of the MPLight learners (n-step returns, Double DQN) before they meet a GPU -- the float64 reference and its
conditions (tests/frap_nstep_ref.py), the option phases of resco_amd/csrc/resco_frap_train.h run over whole minibatches on the host
(tests/frap_nstep_host) against it, the PyTorch learner MPLightLearner(n_step, double_q) and MPLightReplay.sample(n_step=..), the tie
rule of a*, the checkpoint signatures, and the C ABI of the four new functions."""
import re
import os

import numpy as np
import pytest
import torch

import frap_nstep_ref as fn
import frap_train_ref as ft
from conftest import ROOT
from resco_amd import sim as rsim
from resco_amd.agents.idqn_learn import nstep_walk
from resco_amd.agents.mplight import MPLightLearner, MPLightReplay

CALLS = ['rs_mplight_dqn_set_target', 'rs_mplight_dqn_get_target', 'rs_mplight_maps_set_target', 'rs_mplight_maps_get_target']
IDS = ['P%d-D%d-T%d-B%d-n%d-dq%d' % (s[0], s[1], s[2], s[5], s[8], s[9]) for s in fn.SHAPES]


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return fn.build_frap_nstep_host(tmp_path_factory.mktemp('frap_nstep_host'))


def _case(shape, **kw):
    P, D, T, N, S, B, head, count, n_step, dq, done_slots = shape
    return fn.ring_case(P, D, T, N, S, head, count, n_step, dq, done_slots, **kw)


def _cpu_ring(c, arrays=None):
    """an MPLightReplay on the CPU over the case's ring at its position"""
    T, N, S, W = c['obs'].shape
    obs, act, rew = (c['obs'], c['act'], c['rew']) if arrays is None else arrays
    rp = MPLightReplay(T, N, S, W, device='cpu')
    rp.obs.copy_(torch.from_numpy(obs))
    rp.act.copy_(torch.from_numpy(act))
    rp.rew.copy_(torch.from_numpy(rew))
    rp.done.copy_(torch.from_numpy(c['done']))
    rp.head, rp.count = c['head'], c['count']
    return rp


def test_the_scalar_walk_is_the_headers(host):
    """fn.walk against dqn_nstep_walk through the host build, on every slot a draw can name of every shape's ring"""
    for shape in fn.SHAPES:
        c = _case(shape)
        T, N, S = c['obs'].shape[:3]
        slots = fn.valid_slots(T, c['head'], c['count'])
        idx = np.array([(t, 0, 0) for t in slots], np.int32)
        m = fn.host_grads(host, c, idx)[2]
        assert m.tolist() == [fn.walk(c['done'], T, c['head'], t, c['n_step'])[0] for t in slots]


@pytest.mark.parametrize('shape', fn.SHAPES, ids=IDS)
def test_yardstick_is_satisfiable_by_float32(shape):
    """every member of the float32 family is within 4 e_ref of the truth on every tensor and the loss; the conditions of the module
    docstring of frap_nstep_ref hold (reference asserts 2 - 4, ring_case 1)"""
    idx, g64, e_ref, l64, e_loss, family, d64, info = fn.reference(*shape)
    n_step = shape[8]
    assert fn.covers(info, n_step) and 0.25 <= (np.abs(d64) > 1).mean() <= 0.75
    for label, g, l in family:
        for k in g64:
            assert np.abs(g[k] - g64[k]).max() <= 4 * e_ref[k], (label, k)
            assert (g[k][g64[k] == 0] == 0).all(), (label, k)
        assert abs(l - l64) <= 4 * e_loss, label
    assert all(e_ref[k] >= ft.ulp32(np.abs(g64[k]).max()) for k in g64)


@pytest.mark.parametrize('shape', fn.SHAPES, ids=IDS)
def test_host_minibatch_gradient(host, shape):
    """the option phases accumulated over a whole minibatch on the host against the float64 truth, on a ring whose forbidden places
    hold NaN; the walk lengths and a* are the reference's"""
    c = _case(shape)
    idx, g64, e_ref, l64, e_loss, _, _, info = fn.reference(*shape)
    got, loss, m, astar = fn.host_grads(host, c, idx, fn.sentinel_arrays(c))
    print(shape)
    worst = fn.compare(ft.names_of(c['net']), got, loss, g64, e_ref, l64, e_loss, who='host')
    assert not worst, worst
    assert np.array_equal(m, info['m'])
    if c['double_q']:
        assert np.array_equal(astar[~info['cut']], info['a_online'][~info['cut']]) and (astar[info['cut']] == 0).all()


def test_host_ring_semantics(host):
    """rows of slots 3, 4, 5 are cut after 3, 2, 1 rewards, rows of slots 0 and 1 are truncated at the newest slot; slots 6 and 7,
    behind the cut, hold NaN everywhere, as do reward and action of the newest slot"""
    c = _case(fn.SEMANTICS)
    idx, g64, e_ref, l64, e_loss, _, _, info = fn.reference(*fn.SEMANTICS, slots=fn.SEMANTICS_SLOTS)
    assert info['read'] == {3, 4, 5, 0, 1} and set(info['u_m'][~info['cut']].tolist()) == {2}
    by_slot = {t: (set(info['m'][idx[:, 0] == t].tolist()), set(info['cut'][idx[:, 0] == t].tolist())) for t in fn.SEMANTICS_SLOTS}
    assert by_slot == {3: ({3}, {True}), 4: ({2}, {True}), 5: ({1}, {True}), 0: ({2}, {False}), 1: ({1}, {False})}
    arrays = fn.sentinel_arrays(c, unreadable=(6, 7))
    assert np.isnan(arrays[0][[6, 7]]).all() and np.isnan(arrays[2][2]).all() and not np.isnan(arrays[0][2]).any()
    got, loss, _, _ = fn.host_grads(host, c, idx, arrays)
    worst = fn.compare(ft.names_of(c['net']), got, loss, g64, e_ref, l64, e_loss, who='host')
    assert not worst, worst


def test_host_tie_takes_the_lowest_index(host):
    """before_merge.weight of the online network is zero: all online Q are equal, a* must be 0 and the bootstrap Q_target[0]"""
    c = _case(fn.SEMANTICS, tie=True)
    idx, g64, e_ref, l64, e_loss, _, _, info = fn.reference(*fn.SEMANTICS, tie=True)
    assert (info['a_online'] == 0).all() and (info['a_target'][~info['cut']] != 0).any()
    got, loss, _, astar = fn.host_grads(host, c, idx, fn.sentinel_arrays(c))
    assert (astar == 0).all()
    worst = fn.compare(ft.names_of(c['net']), got, loss, g64, e_ref, l64, e_loss, who='host')
    assert not worst, worst


def _learner_grads(c, idx, rp):
    """MPLightLearner(n_step, double_q).loss on the rows idx of the ring rp (the walk: idqn_learn.nstep_walk, as MPLightReplay.sample
    takes it) and its backward -> (dict name -> float64 gradient, loss)"""
    net = type(c['net'])(c['net'].oshape, c['net'].phase_pairs, c['net'].demand_shape)
    net.load_state_dict(c['net'].state_dict())
    learner = MPLightLearner(net, gamma=fn.GAMMA, batch_size=len(idx), n_step=c['n_step'], double_q=c['double_q'])
    learner.target.load_state_dict(c['target'].state_dict())
    t, e, s = (torch.from_numpy(idx[:, k].astype(np.int64)) for k in range(3))
    o, g = rp.obs[t, e, s], rp.act[t, e, s].long().clamp(0, c['P'] - 1)
    if c['n_step'] == 1:
        batch = (o, g, rp.rew[t, e, s], rp.obs[(t + 1) % rp.T, e, s], rp.done[t].float())
    else:
        R, u_m, cut, disc = nstep_walk(rp, t, e, rp.head, c['n_step'], fn.GAMMA, s)
        batch = (o, g, R, rp.obs[u_m, e, s], cut.float(), disc)
    batch = tuple(torch.nan_to_num(x) if x.dtype.is_floating_point and x.dim() == 2 else x for x in batch[:4]) + batch[4:]
    loss = learner.loss(*batch)
    loss.backward()
    return {k: p.grad.detach().double().numpy() for k, p in net.named_parameters()}, float(loss.detach())


@pytest.mark.parametrize('shape', fn.SHAPES, ids=IDS)
def test_pytorch_learner(shape):
    """MPLightLearner(n_step, double_q) within the bound of the device, on the ring with its sentinels (the successor of a cut row
    holds NaN there; the learner multiplies its bootstrap by zero, so those observations alone are zeroed for it)"""
    c = _case(shape)
    idx, g64, e_ref, l64, e_loss, _, _, _ = fn.reference(*shape)
    got, loss = _learner_grads(c, idx, _cpu_ring(c, fn.sentinel_arrays(c)))
    worst = fn.compare(ft.names_of(c['net']), got, loss, g64, e_ref, l64, e_loss, who='torch')
    assert not worst, worst


@pytest.mark.parametrize('shape', [fn.SHAPES[0], fn.SHAPES[2], fn.SHAPES[4]], ids=[IDS[0], IDS[2], IDS[4]])
def test_replay_sample_gives_the_references_rows(shape):
    """MPLightReplay.sample(n_step, gamma): the draws of sample() without the option, and per row the reference's float32 return,
    discount, cut flag and bootstrap observation"""
    c = _case(shape)
    rp = _cpu_ring(c)
    B = 64
    gen = lambda: torch.Generator().manual_seed(5)
    o1, g1, r1, o21, d1 = rp.sample(B, gen())
    o, g, R, o2, cut, disc = rp.sample(B, gen(), c['n_step'], fn.GAMMA)
    assert torch.equal(o, o1) and torch.equal(g, g1)
    G = gen()
    k = torch.randint(0, rp.count - 1, (B,), generator=G)
    t = (rp.head - rp.count + k) % rp.T
    e, s = torch.randint(0, rp.N, (B,), generator=G), torch.randint(0, rp.S, (B,), generator=G)
    idx = torch.stack((t, e, s), -1).numpy().astype(np.int32)
    assert torch.equal(o, rp.obs[t, e, s])
    want = fn.rows(c, idx, np.float32)
    assert R.numpy().tobytes() == want['R'].tobytes() and disc.numpy().tobytes() == want['g'].tobytes()
    assert np.array_equal(cut.numpy() != 0, want['cut'])
    assert torch.equal(o2, rp.obs[torch.from_numpy(want['u_m']), e, s])
    with pytest.raises(AssertionError):
        rp.sample(B, gen(), 3)              # n-step rows need gamma


def test_two_map_reference_meets_the_conditions(host):
    """the two maps of the device's grouped test: either reference exists (its conditions hold), the combination weights by the group
    sizes, and the host build is inside the bound on each map"""
    idx, counts, g64, e_ref, l64, e_loss = fn.two_map_reference()
    assert counts == [5, 7] and idx.shape == (12, 4) and idx[:, 0].tolist() == [0] * 5 + [1] * 7
    for m, shape in enumerate(fn.TWO_MAPS):
        c = _case(shape)
        rows, g, e, l, el = fn.reference(*shape)[:5]
        assert np.array_equal(rows, idx[idx[:, 0] == m][:, 1:])
        got, loss, _, _ = fn.host_grads(host, c, rows, fn.sentinel_arrays(c))
        assert not fn.compare(ft.names_of(c['net']), got, loss, g, e, l, el, who='host')
    assert all(e_ref[k] >= ft.ulp32(np.abs(g64[k]).max()) for k in g64) and e_loss > 0


def test_signatures_enter_a_checkpoint_only_when_not_default():
    c = _case(fn.SHAPES[0])
    plain = {'batch': 32, 'target_update': 500, 'gamma': 0.99}
    assert MPLightLearner(c['net']).signature() == plain
    assert MPLightLearner(c['net'], n_step=3, double_q=True).signature() == dict(plain, n_step=3, double_q=True)
    assert MPLightLearner(c['net'], n_step=2).signature() == dict(plain, n_step=2)
    with pytest.raises(ValueError, match='n_step'):
        MPLightLearner(c['net'], n_step=33)
    from resco_amd.agents.mplight_learn_fused import FusedMPLightLearner
    from resco_amd.agents.mplight_multi import MultiMapMPLightLearner
    for cls, args in ((FusedMPLightLearner, (c['net'],)), (MultiMapMPLightLearner, ([c['net']], [2]))):
        with pytest.raises(ValueError, match='n_step'):
            cls(*args, n_step=0)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            cls(*args, n_step=3, double_q=True)


def test_tools_take_the_flags():
    from tools import mplight_multimap_train, mplight_train
    for tool in (mplight_train, mplight_multimap_train):
        assert tool.target_flags(['--n-step', '3', 'cologne1', '--double-q', '8']) == (dict(n_step=3, double_q=True), ['cologne1', '8'])
        for bad in (['--n-step', '0'], ['--n-step', '33'], ['--n-step']):
            with pytest.raises(SystemExit):
                tool.target_flags(bad)
        assert {'n_step', 'double_q'} <= set(tool.main.__code__.co_varnames[:tool.main.__code__.co_argcount])


def test_abi_declares_and_exports_the_functions():
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    declared = set(re.findall(r'\b(rs_[a-z_]+)\s*\(', text))
    from resco_amd.build import build_library
    build_library()
    L = rsim.load_library()
    for name in CALLS:
        assert name in declared and name in rsim.ABI_SYMBOLS and hasattr(L, name), name
