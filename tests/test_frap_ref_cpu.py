"""The float64 FRAP reference (tests/frap_ref.py) and its yardstick, without a GPU: frap_ref against the reference's own Q-values
(tests/golden/mplight_frap.npz), then the host build of the kernel's per-lane arithmetic (tests/frap_host) against frap_ref on
synthetic phase-pair sets of every lane-group width, all four observation classes, under |Q_host - Q64| <= 4 e_ref + 2 ulp32(|Q64|)
(e_ref = max |fp32 PyTorch FRAP - Q64| over the class), the greedy margin rule, and the epsilon-greedy draws restated in Python."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import frap_ref as fr
from conftest import GOLDEN, ROOT, load_scenario
from resco_amd.agents.mplight import mplight_tables, pack_mplight_weights

MAPS = ['cologne1', 'cologne3', 'cologne8', 'ingolstadt1', 'ingolstadt7', 'ingolstadt21']
PAIR_COUNTS = [2, 3, 4, 5, 8, 9, 13, 16]
N_ROWS, N_SIGNALS = 131, 5


@pytest.fixture(scope='module')
def fx():
    return dict(np.load(os.path.join(GOLDEN, 'mplight_frap.npz')))


@pytest.mark.parametrize('D', [1, 4])
@pytest.mark.parametrize('name', MAPS)
def test_frap_ref_reproduces_the_reference_s_q_values(fx, name, D):
    """the new truth is the reference's network, not a restatement of ours"""
    tag = '%s_d%d' % (name, D)
    sd = {k[len(tag) + 4:]: v for k, v in fx.items() if k.startswith(tag + '_sd_')}
    obs, qref = fx[tag + '_obs'], fx[tag + '_q']
    q = fr.frap_ref(sd, load_scenario(name).phase_pairs, D, obs).reshape(qref.shape)
    np.testing.assert_allclose(q, qref, rtol=1e-5, atol=1e-6)


def test_sigmoid_is_stable_and_the_fixtures_are_what_they_claim():
    with np.errstate(over='raise', invalid='raise', divide='raise'):    # exp(-5000) underflows to 0, which is the answer
        s = fr._sigmoid(np.array([-5000.0, -1000.0, 0.0, 1000.0, 5000.0]))
    np.testing.assert_array_equal(s, [0.0, 0.0, 0.5, 1.0, 1.0])
    for P in PAIR_COUNTS:
        rng = np.random.default_rng(P)
        pairs, valid, order, sc = fr.synthetic_signal_set(P, N_SIGNALS, rng)
        assert len({frozenset(p) for p in pairs.tolist()}) == P and all(a != b for a, b in pairs.tolist())
        pairs2, valid2, order2 = mplight_tables(sc)                 # the stand-in is accepted unchanged and gives the same tables
        np.testing.assert_array_equal(pairs2, pairs)
        np.testing.assert_array_equal(valid2, valid)
        np.testing.assert_array_equal(order2, order)
        counts = (order >= 0).sum(1)
        assert {1, 2, P} <= set(counts.tolist()) and (P < 4 or any(2 < c < P for c in counts))
        skewed = 0
        for s in range(N_SIGNALS):
            lst = order[s][order[s] >= 0]
            np.testing.assert_array_equal(valid[s, lst], np.arange(len(lst)))
            if len(lst) > 1:
                assert lst[0] != lst.min()
                skewed += 1
        assert skewed >= 1
        for D in (1, 4):
            cls = fr.obs_classes(P, D, N_ROWS, N_SIGNALS, rng)
            for name, rows in cls.items():
                assert rows.shape == (N_ROWS, N_SIGNALS, 1 + 12 * D) and rows.dtype == (np.int32 if D == 1 else np.float32)
                assert set(np.unique(rows[..., 0]).astype(int).tolist()) == set(range(-2, P + 3)), name
            assert not cls['zero'][..., 1:].any() and np.all(np.abs(cls['sat'][..., 1:]) == 1000)
    pairs, _, _, _ = fr.synthetic_signal_set(5, 4, np.random.default_rng(1), repeated_movement=True)
    assert pairs[0, 0] == pairs[0, 1] and not set(pairs[0].tolist()) & set(pairs[1].tolist())


# ---- the kernel's own arithmetic, compiled for the host (as tests/test_mplight_cpu.py builds it)
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('frap_ref') / 'frap_host.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math', '-w', '-shared',
                           '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'resco_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'frap_host', 'frap_host.cpp'), '-o', out])
    L = C.CDLL(out)
    vp, i32 = C.c_void_p, C.c_int32
    L.frap_rows.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, i32, i32, C.c_float, C.c_uint32, C.c_uint32, i32, vp, vp, vp]
    return L


def _host_rows(L, net, tables, obs, eps=0.0, seed=0, step_key=0, env_base=0):
    pairs, valid, order = tables
    w = np.ascontiguousarray(pack_mplight_weights(net).numpy())
    o = np.ascontiguousarray(obs, np.float32)
    N, S = o.shape[:2]
    act = np.zeros((N, S), np.int32)
    pi = np.zeros((N, S), np.int32)
    q = np.zeros((N, S, 16), np.float32)
    L.frap_rows(w.ctypes.data, net.demand_shape, net.oshape, pairs.ctypes.data, S, valid.ctypes.data, order.ctypes.data, o.ctypes.data, N,
                env_base, eps, seed, step_key, 1, act.ctypes.data, pi.ctypes.data, q.ctypes.data)
    return act, pi, q


@functools.lru_cache(maxsize=None)
def _case(P, D, scale, repeated=False):
    rng = np.random.default_rng(1000 * P + 10 * D + int(scale) + 500 * repeated)
    pairs, valid, order, sc = fr.synthetic_signal_set(P, N_SIGNALS, rng, repeated_movement=repeated)
    net = fr.make_net(pairs, D, scale, seed=P + D)
    cls = fr.obs_classes(P, D, N_ROWS, N_SIGNALS, rng)
    q64 = {k: fr.frap_ref(net.state_dict(), pairs, D, v).reshape(N_ROWS, N_SIGNALS, P) for k, v in cls.items()}
    q32 = {k: fr.fp32_frap(net, v) for k, v in cls.items()}
    return net, (pairs, valid, order), cls, q64, q32


def _check_host(host, P, D, scale, repeated=False):
    net, tables, cls, q64, q32 = _case(P, D, scale, repeated)
    valid, order = tables[1], tables[2]
    for name in fr.CLASSES:
        act, pair, q = _host_rows(host, net, tables, cls[name])
        assert np.all(np.isneginf(q[..., P:])) and np.all(np.isfinite(q[..., :P]))
        tol, e_ref = fr.q_tolerance(q64[name], q32[name])
        err = np.abs(q[..., :P].astype(np.float64) - q64[name])
        print('P %2d D %d x%d %-5s  |host - truth| %.3e = %.2f e_ref, %.2f of the tolerance  (max |Q| %.3e)' %
              (P, D, scale, name, err.max(), err.max() / max(e_ref, 1e-300), (err / tol).max(), np.abs(q64[name]).max()))
        assert np.all(err <= tol), (name, err.max(), e_ref)
        np.testing.assert_array_equal(act, valid[np.arange(N_SIGNALS)[None, :], pair])
        if name == 'small':
            # wide and sat rows saturate into exact symmetries and zero rows are all alike: those three get the Q bound only
            share = fr.greedy_check(pair, q64[name], order, e_ref)
            print('P %2d D %d x%d small  rows below the 8 e_ref margin: %.1f %%' % (P, D, scale, 100 * share))
            assert share <= 0.10


@pytest.mark.parametrize('scale', [1, 3])
@pytest.mark.parametrize('D', [1, 4])
@pytest.mark.parametrize('P', PAIR_COUNTS)
def test_host_build_against_float64_on_synthetic_sets(host, P, D, scale):
    _check_host(host, P, D, scale)


@pytest.mark.parametrize('D', [1, 4])
def test_host_build_with_a_pair_that_repeats_a_movement(host, D):
    """[m, m] against a pair that shares nothing: three distinct movements, the reference's relation bit is 1"""
    _, (pairs, _, _), _, _, _ = _case(5, D, 3, True)
    assert len(set(pairs[0].tolist() + pairs[1].tolist())) == 3
    _check_host(host, 5, D, 3, repeated=True)


def test_the_epsilon_fixture_explores_a_fair_share_and_the_host_build_follows_the_restated_draws(host):
    E = fr.EPS_CASE
    net, tables, cls, _, _ = _case(8, 1, 3)
    order = tables[2]
    obs = cls['small']
    _, greedy, q = _host_rows(host, net, tables, obs)
    _, pair, _ = _host_rows(host, net, tables, obs, eps=E['eps'], seed=E['seed'], step_key=E['step_key'], env_base=E['env_base'])
    want, mask = fr.select_pairs(q, order, eps=E['eps'], seed=E['seed'], env_base=E['env_base'], step_key=E['step_key'])
    assert 0.20 <= mask.mean() <= 0.55
    np.testing.assert_array_equal(pair, want)                           # greedy rows from the host's own q: bit-exact epilogue
    np.testing.assert_array_equal(pair[~mask], greedy[~mask])
    for s in range(N_SIGNALS):                                          # explorers hold valid pairs, and more than one of them
        lst = order[s][order[s] >= 0]
        assert np.all(np.isin(pair[mask[:, s], s], lst))
        assert len(lst) == 1 or len(set(pair[mask[:, s], s].tolist())) > 1
    assert not fr.select_pairs(q, order, eps=0.0, seed=E['seed'])[1].any()
    assert fr.select_pairs(q, order, eps=1.0, seed=E['seed'])[1].all()
