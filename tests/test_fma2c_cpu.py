"""CPU: FMA2C's layout, PyTorch nets, the host build of the fused kernel's per-row pieces (tests/fma2c_host) and the A2C learner
against the float64 restatement of the reference (tests/fma2c_ref.py).  Yardstick: truth = float64; e_ref = max |plain float32
per-agent evaluation - truth| over a tensor class; a candidate gets 4 e_ref + 2 ulp32(|truth|) per element."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import fma2c_ref as R
from conftest import ROOT
from fma2c_check import A_MAX, Case, compare, reference

UNIFORM_SEED = 20240611         # the uniforms of every draw in this module: np.random.default_rng(UNIFORM_SEED)

_cases = {}


def case(map_name, full=False):
    key = (map_name, full)
    if key not in _cases:
        _cases[key] = Case(map_name, full)
    else:       # FMA2CLayout and the reference read the ACTIVE mdp config: re-activate this map's
        from resco_amd.config.mdp_config import activate
        activate('FMA2CFull' if full else 'FMA2C', map_name)
    return _cases[key]


def _all_maps():
    from resco_amd.config.mdp_config import _ALL
    return [(m, False) for m in _ALL['FMA2C']] + [(m, True) for m in _ALL['FMA2CFull']]


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize('map_name,full', _all_maps())
def test_layout_matches_reference_sizes(map_name, full):
    c = case(map_name, full)
    L = c.layout
    assert L.agents == c.names
    for k, name in enumerate(c.names):
        a = c.table[name]
        assert L.sizes(k) == (a['n_a'], a['n_s'], a['n_w'], a['n_f']), name
        assert [L.agents[j] for j in L.fp_src[k]] == a['fp_src'], name
        assert [L.agents[j] for j in L.mgr_src[k]] == a['mgr_src'], name


def test_layout_known_maps():
    L = case('cologne1').layout
    assert L.K == 2 and L.n_f == [0, 0]
    L = case('ingolstadt21').layout
    assert L.K == 26 and L.M == 5 and all(L.n_f[k] == 8 for k in range(L.M))


@pytest.mark.parametrize('map_name,full', [('cologne3', False), ('ingolstadt21', False), ('ingolstadt7', True)])
def test_assembled_rows(map_name, full):
    """rows = [manager actions] ++ states row ++ fingerprints in the reference's order, on lane aggregates on both sides of every
    clip.  Bound: a row element is at most four float32 roundings (sum, one or two divisions... , scale) away from float64: 3 ulp32."""
    c = case(map_name, full)
    L, rng = c.layout, np.random.default_rng(UNIFORM_SEED)
    N = 4
    agg = c.lane_agg(rng, 1, N)[0]
    F = L.features(torch.as_tensor(agg)).numpy()
    nb = L.n_blocks
    hi = np.array([c.mdp['clip_wave']] * (nb - 1) + [c.mdp['clip_wait']]).repeat(L.O)
    assert ((F == 0) | (F < hi)).any() and (F == hi).any(), 'the synthetic input must lie on both sides of the clips'
    macts = rng.integers(0, 4, (N, L.M))
    fp = rng.uniform(0, 1, (N, L.K, A_MAX)).astype(np.float32)
    for k in range(L.K):
        fp[:, k, L.n_a[k]:] = 0
    rows = L.assemble(L.obs_rows(torch.as_tensor(agg)), torch.as_tensor(macts), torch.as_tensor(fp)).numpy()
    for n in range(N):
        obs = R.states_rows(c.mdp, full, agg[n], c.s_idx, c.s_scale)
        for k, name in enumerate(c.names):
            a = c.table[name]
            want = R.assemble(c.table, name, obs[name], {m: macts[n, c.names.index(m)] for m in a['mgr_src']},
                              {s: fp[n, c.names.index(s), :c.table[s]['n_a']] for s in a['fp_src']})
            assert len(want) == L.width[k]
            assert (np.abs(rows[n, k, :len(want)] - want) <= 3 * R.ulp32(want)).all(), (name, n)
            assert (rows[n, k, len(want):] == 0).all()


# ------------------------------------------------------------------------------------------------ net
def _torch_steps(c, agg, u):
    L, net = c.layout, c.net
    T, N = agg.shape[:2]
    state, fp, steps = torch.zeros(N, L.K, 4, 64), torch.zeros(N, L.K, A_MAX), []
    with torch.no_grad():
        for t in range(T):
            out = net.act(L.obs_rows(torch.as_tensor(agg[t])), state, fp, torch.as_tensor(u[t], dtype=torch.float32))
            state, fp = out['state'], out['fingerprints']
            steps.append({k: out[k].numpy() for k in ('pi', 'value', 'state', 'rows', 'actions')})
    return steps


@pytest.mark.parametrize('map_name', ['cologne1', 'cologne3', 'ingolstadt21'])
def test_batched_net_against_float64(map_name):
    """BatchedFMA2C over T = 5 chained steps at N = 3: pi (= the fingerprints), value, (c, h), rows"""
    c = case(map_name)
    rng = np.random.default_rng(UNIFORM_SEED)
    agg = c.lane_agg(rng, 5, 3)
    u = rng.uniform(0, 1, (5, 3, c.layout.K)).astype(np.float32).astype(np.float64)
    truth, e_ref = reference(c, agg, u)
    compare(c, truth, e_ref, u, _torch_steps(c, agg, u), label='torch ' + map_name)


def test_padded_parameters_have_zero_gradient():
    from resco_amd.agents.fma2c import A2CLearner
    c = case('cologne3')
    L, net = c.layout, c.net
    rng = np.random.default_rng(UNIFORM_SEED)
    T, N = 3, 2
    steps = _torch_steps(c, c.lane_agg(rng, T, N), rng.uniform(0, 1, (T, N, L.K)))
    lr = A2CLearner(net, N, batch_size=T)
    rows = torch.as_tensor(np.stack([s['rows'] for s in steps]), dtype=torch.float32)
    acts = torch.as_tensor(np.stack([s['actions'] for s in steps]))
    loss = lr.loss(rows, acts, torch.zeros(T, dtype=torch.bool), torch.randn(T, N, L.K), torch.randn(T, N, L.K), torch.zeros(N, L.K, 4, 64))
    grads = dict(zip([n for n, _ in net.named_parameters()], torch.autograd.grad(loss.sum(), list(net.parameters()))))
    for k in range(L.K):
        n_a, n_s, n_w, n_f = L.sizes(k)
        assert (grads['fcw_w'][k, :, n_s:] == 0).all() and (grads['fcf_w'][k, :, n_f:] == 0).all() and (grads['fct_w'][k, :, n_w:] == 0).all()
        assert (grads['head_w'][k, 0, :, n_a:] == 0).all() and (grads['head_b'][k, 0, n_a:] == 0).all()
        assert (grads['head_w'][k, 1, :, 1:] == 0).all() and (grads['head_b'][k, 1, 1:] == 0).all()
        if n_w == 0:
            assert (grads['fct_w'][k] == 0).all() and (grads['fct_b'][k] == 0).all() and (grads['wx'][k, :, 192:] == 0).all()
        assert grads['fcw_w'][k, :, :n_s].abs().max() > 0 and grads['fcf_b'][k].abs().max() > 0        # n_f = 0 still trains the fcf bias


# ------------------------------------------------------------------------------------------------ host build of the kernel's pieces
@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('fma2c_host') / 'fma2c_host.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math', '-w', '-shared',
                           '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'resco_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'fma2c_host', 'fma2c_host.cpp'), '-o', out])
    return C.CDLL(out)


def _host_steps(lib, c, agg, u, N_max=None, env_base=0):
    from resco_amd.sim import Fma2cDesc
    L = c.layout
    T, N = agg.shape[:2]
    E = N_max or N
    keep = L.desc_arrays()
    d = Fma2cDesc(L.K, L.M, L.S, L.O, 1 if L.full else 0, float(c.mdp['norm_wave']), float(c.mdp['clip_wave']), float(c.mdp['norm_wait']),
                  float(c.mdp['clip_wait']), *[keep[n].ctypes.data for n in Fma2cDesc.ARRAYS])
    w = np.ascontiguousarray(c.net.packed().numpy(), np.float32)
    state, fp = np.zeros((E, L.K, 4, 64), np.float32), np.zeros((2, E, L.K, A_MAX), np.float32)
    macts, parity = np.zeros((E, L.M), np.int32), np.zeros((E, L.K), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    steps = []
    for t in range(T):
        acts, pi, val = np.zeros((N, L.S), np.int32), np.zeros((N, L.K, A_MAX), np.float32), np.zeros((N, L.K), np.float32)
        rows = np.zeros((N, L.K, L.W), np.float32)
        a_t, u_t = np.ascontiguousarray(agg[t], np.float32), np.ascontiguousarray(u[t], np.float32)
        W = lib.fma2c_host_act(C.byref(d), p(w), E, p(state), p(fp), p(macts), p(parity), p(a_t), N, env_base, 0, t, p(u_t), 0,
                               p(acts), p(pi), p(val), p(rows))
        assert W == L.W
        steps.append(dict(pi=pi.copy(), value=val.copy(), state=state[env_base:env_base + N].copy(), rows=rows.copy(),
                          actions=np.concatenate([macts[env_base:env_base + N], acts], axis=1)))
    return steps


@pytest.mark.parametrize('map_name,full', [('cologne1', False), ('cologne3', False), ('ingolstadt21', False), ('ingolstadt7', True)])
def test_host_build_of_kernel_pieces(host_lib, map_name, full):
    """the kernel's own arithmetic (gather, fc and LSTM rows in the MFMA's summation order, softmax, draw) on the CPU: same inputs,
    same bound, and the action rule with its 1 % cap"""
    c = case(map_name, full)
    rng = np.random.default_rng(UNIFORM_SEED)
    agg = c.lane_agg(rng, 5, 3)
    u = rng.uniform(0, 1, (5, 3, c.layout.K)).astype(np.float32).astype(np.float64)
    truth, e_ref = reference(c, agg, u)
    compare(c, truth, e_ref, u, _host_steps(host_lib, c, agg, u), label='host ' + map_name)


# ------------------------------------------------------------------------------------------------ learner
def test_returns_and_advantages_with_dones():
    """a done in the middle of a segment and one at its end, against the restated OnPolicyBuffer; rewards r / 2000 clipped to +-2"""
    from resco_amd.agents.fma2c import A2CLearner
    c = case('cologne1')
    K, N, T = c.layout.K, 2, 6
    rng = np.random.default_rng(UNIFORM_SEED)
    lr = A2CLearner(c.net, N, batch_size=T)
    rew, val = rng.uniform(-9000, 3000, (T, N, K)), rng.normal(0, 1, (T, N, K))
    dones = [False, False, True, False, False, True]
    for t in range(T):
        lr.add(torch.zeros(N, K, c.layout.W), torch.zeros(N, K, dtype=torch.long), torch.as_tensor(rew[t], dtype=torch.float32),
               torch.as_tensor(val[t], dtype=torch.float32), dones[t])
    Rs, Advs = lr.returns(torch.zeros(N, K))
    r32, v32 = rew.astype(np.float32).astype(np.float64), val.astype(np.float32).astype(np.float64)
    want_R, want_A = R.buffer_returns(list(R.clip_reward(r32)), list(v32), [False] + dones, np.zeros((N, K)), 0.96)
    assert np.abs(R.clip_reward(r32)).max() == 2.0
    # T chained multiply-adds in float32 against float64: T ulp32 of the largest magnitude
    assert np.abs(Rs.numpy() - np.stack(want_R)).max() <= T * R.ulp32(np.abs(np.stack(want_R)).max())
    assert np.abs(Advs.numpy() - np.stack(want_A)).max() <= (T + 1) * R.ulp32(np.abs(np.stack(want_A)).max())
    # no bootstrap across the done in the middle: R_2 is r_2 alone
    assert np.allclose(Rs[2].numpy(), R.clip_reward(r32)[2], rtol=0, atol=1e-7)


def _segment(c, T, N, seed):
    rng = np.random.default_rng(seed)
    L = c.layout
    steps = _torch_steps(c, c.lane_agg(rng, T, N), rng.uniform(0, 1, (T, N, L.K)))
    rows = np.stack([s['rows'] for s in steps]).astype(np.float32)
    acts = np.stack([s['actions'] for s in steps])
    Rs = rng.normal(0, 1, (T, N, L.K)).astype(np.float32)
    Advs = rng.normal(0, 1, (T, N, L.K)).astype(np.float32)
    state0 = rng.normal(0, 0.3, (N, L.K, 4, 64)).astype(np.float32)
    return rows, acts, Rs, Advs, state0


def _ref_grads(c, rows, acts, dones, Rs, Advs, state0, dt):
    params = c.ref_params()
    out = {}
    for k, name in enumerate(c.names):
        a = c.table[name]
        w = a['n_s'] + a['n_w'] + a['n_f']
        out[name] = R.agent_loss_grads(params[name], a, rows[:, :, k, :w].astype(np.float64), acts[:, :, k], dones, Rs[:, :, k].astype(np.float64),
                                       Advs[:, :, k].astype(np.float64), state0[:, k].astype(np.float64), dt)
    return out


_PAD = dict(fcw_w=lambda a: (slice(0, a['n_s']),), fcf_w=lambda a: (slice(0, a['n_f']),), fct_w=lambda a: (slice(0, a['n_w']),),
            wx=lambda a: (slice(0, 224 if a['n_w'] else 192),))


def test_loss_and_gradients_of_one_update():
    """T = 6, N = 3, cologne3, a pre-step done inside the segment: per-agent loss and every gradient within 4 e_ref (+ 2 ulp32) of float64"""
    from resco_amd.agents.fma2c import A2CLearner
    c = case('cologne3')
    T, N = 6, 3
    rows, acts, Rs, Advs, state0 = _segment(c, T, N, UNIFORM_SEED)
    dones = np.array([False, False, False, True, False, False])
    truth, plain = _ref_grads(c, rows, acts, dones, Rs, Advs, state0, np.float64), _ref_grads(c, rows, acts, dones, Rs, Advs, state0, np.float32)
    lr = A2CLearner(c.net, N, batch_size=T)
    loss = lr.loss(torch.as_tensor(rows), torch.as_tensor(acts), torch.as_tensor(dones), torch.as_tensor(Rs), torch.as_tensor(Advs), torch.as_tensor(state0))
    grads = dict(zip([n for n, _ in c.net.named_parameters()], torch.autograd.grad(loss.sum(), list(c.net.parameters()))))
    e_loss = max(abs(float(plain[n][0]) - float(truth[n][0])) for n in c.names)
    e_grad = max(float(np.abs(np.asarray(plain[n][1][net][t], np.float64) - truth[n][1][net][t]).max()) for n in c.names for net in ('pi', 'v') for t in truth[n][1][net] if truth[n][1][net][t].size)
    print('e_ref loss %.3e grad %.3e' % (e_loss, e_grad))
    for k, name in enumerate(c.names):
        a = c.table[name]
        assert abs(float(loss[k]) - float(truth[name][0])) <= R.bound(e_loss, truth[name][0]), name
        for ni, net in enumerate(('pi', 'v')):
            for t, want in truth[name][1][net].items():
                got = grads[t][k, ni].numpy().astype(np.float64)
                if t in _PAD:
                    got = got[_PAD[t](a)]
                elif t in ('head_w', 'head_b'):
                    got = got[..., :want.shape[-1]]
                err = np.abs(got - want)
                assert (err <= R.bound(e_grad, want)).all(), (name, net, t, float(err.max()), e_grad)


def test_clipped_norm_scale_per_agent():
    """one agent pushed above max_grad_norm = 40 by scaled advantages: its gradients are scaled by 40 / norm, the others' by 1"""
    from resco_amd.agents.fma2c import A2CLearner
    c = case('cologne3')
    T, N = 6, 3
    rows, acts, Rs, Advs, state0 = _segment(c, T, N, UNIFORM_SEED + 1)
    Advs[:, :, 3] *= 4000.0
    dones = np.zeros(T, bool)
    truth = _ref_grads(c, rows, acts, dones, Rs, Advs, state0, np.float64)
    lr = A2CLearner(c.net, N, batch_size=T)
    loss = lr.loss(torch.as_tensor(rows), torch.as_tensor(acts), torch.as_tensor(dones), torch.as_tensor(Rs), torch.as_tensor(Advs), torch.as_tensor(state0))
    scales, norms = lr.clip_scales(torch.autograd.grad(loss.sum(), list(c.net.parameters())))
    want = [R.global_norm_scale(truth[n][1]) for n in c.names]
    assert want[3][1] > 40.0 and all(w[1] < 40.0 for i, w in enumerate(want) if i != 3)
    for k in range(c.layout.K):
        assert abs(float(scales[k]) - want[k][0]) <= 1e-5 * want[k][0], (k, float(scales[k]), want[k])     # a norm over ~1e5 float32 gradients
    assert all(float(scales[k]) == 1.0 for k in range(c.layout.K) if k != 3)


def test_rmsprop_known_answer():
    """TF1 RMSProp on a three-element parameter, by hand: ms starts at ONE and eps sits under the root.
    g = (1, -2, 0): ms = 0.99 + 0.01 g^2 = (1.0, 1.03, 0.99); w' = w - 2.5e-4 g / sqrt(ms + 1e-5)"""
    from resco_amd.agents.fma2c import A2CLearner

    class One(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor([[0.5, -0.25, 1.0]], dtype=torch.float64))
            self.fcw_w, self.layout = self.w, type('L', (), dict(K=1, W=1))
    net = One()
    lr = A2CLearner(net, 1, batch_size=1)
    assert float(lr.ms[0].min()) == 1.0 and float(lr.ms[0].max()) == 1.0
    lr.rmsprop_step([torch.tensor([[1.0, -2.0, 0.0]], dtype=torch.float64)])
    want = [0.5 - 2.5e-4 * 1.0 / (1.0 + 1e-5) ** 0.5, -0.25 + 2.5e-4 * 2.0 / (1.03 + 1e-5) ** 0.5, 1.0]
    assert np.allclose(net.w.detach().numpy()[0], want, rtol=0, atol=1e-15)
    assert np.allclose(lr.ms[0].numpy()[0], [1.0, 1.03, 0.99], rtol=0, atol=1e-15)
    # eps OUTSIDE the root (torch.optim.RMSprop) or ms starting at zero would give other numbers
    assert abs(want[0] - (0.5 - 2.5e-4 / (1.0 + 1e-5))) > 1e-10 and abs(want[0] - (0.5 - 2.5e-4 / (0.01 ** 0.5))) > 1e-4
    w2, ms2 = R.tf_rmsprop(np.array([0.5, -0.25, 1.0]), np.array([1.0, -2.0, 0.0]), np.ones(3))
    assert np.allclose(w2, want, rtol=0, atol=1e-15)


def test_states_bw_follows_the_acting_state():
    """two consecutive updates: each re-runs its segment from the acting state at the segment's start; after a done that start is zero"""
    from resco_amd.agents.fma2c import A2CLearner
    c = case('cologne1')
    L, N, T = c.layout, 2, 3
    net = Case('cologne1', seed=5).net
    rng = np.random.default_rng(UNIFORM_SEED)
    lr = A2CLearner(net, N, batch_size=T)
    seen = []
    orig = lr.loss
    lr.loss = lambda rows, acts, dones, Rs, Advs, state0: (seen.append((state0.clone(), dones.clone())), orig(rows, acts, dones, Rs, Advs, state0))[1]
    state, fp = torch.zeros(N, L.K, 4, 64), torch.zeros(N, L.K, A_MAX)
    starts = [state.clone()]
    for t in range(2 * T):
        with torch.no_grad():
            out = net.act(L.obs_rows(torch.as_tensor(c.lane_agg(rng, 1, N)[0])), state, fp, torch.rand(N, L.K))
        state, fp = out['state'], out['fingerprints']
        done = t == 2 * T - 1
        res = lr.observe(out['rows'], out['actions'], torch.randn(N, L.K) * 1000, out['value'], done, state, lambda: torch.zeros(N, L.K))
        assert (res is not None) == (t % T == T - 1)
        if res is not None:
            starts.append(state.clone())
    assert len(seen) == 2
    assert torch.equal(seen[0][0], starts[0]) and torch.equal(seen[1][0], starts[1]) and starts[1].abs().max() > 0
    assert not seen[0][1].any() and not seen[1][1].any()
    assert float(lr.states_bw.abs().max()) == 0.0 and lr.dones == [True] and lr.steps_done == 0     # after the done: model.reset()


def test_agent_config_registers_fma2c():
    from resco_amd import rewards, states
    from resco_amd.agents.fma2c import FMA2C
    from resco_amd.config.agent_config import agent_configs
    for key, st, rw, dist in (('FMA2C', states.fma2c, rewards.fma2c, 200), ('FMA2CFULL', states.fma2c_full, rewards.fma2c_full, 200),
                              ('FMA2CVAL', states.fma2c, rewards.fma2c, 50)):
        cfg = agent_configs[key]
        assert cfg['agent'] is FMA2C and cfg['state'] is st and cfg['reward'] is rw and cfg['max_distance'] == dist
        assert (cfg['management_acts'], cfg['batch_size'], cfg['gamma'], cfg['lr_init'], cfg['rmsp_alpha'], cfg['rmsp_epsilon']) == (4, 120, 0.96, 2.5e-4, 0.99, 1e-5)
        assert (cfg['max_grad_norm'], cfg['value_coef'], cfg['entropy_coef_init'], cfg['reward_norm'], cfg['reward_clip']) == (40, 0.5, 0.001, 2000.0, 2.0)


def test_dict_agent_acts_and_learns():
    """the reference's interface for one environment: act on a states.fma2c dict, observe, an update at done moves the weights"""
    from resco_amd.agents.fma2c import FMA2C
    from resco_amd.config.agent_config import agent_configs
    c = case('cologne1')
    cfg = dict(agent_configs['FMA2C'], steps=10)
    agent = FMA2C(cfg, None, 'cologne1', 0, scenario=c.sc, seed=1)
    rng = np.random.default_rng(UNIFORM_SEED)
    before = agent.net.packed().clone()
    for t in range(4):
        obs = R.states_rows(c.mdp, False, c.lane_agg(rng, 1, 1)[0, 0], c.s_idx, c.s_scale)
        acts = agent.act(obs)
        assert set(acts) == set(c.names) and all(0 <= acts[n] < c.table[n]['n_a'] for n in c.names)
        agent.observe(obs, {n: -500.0 * (t + 1) for n in c.names}, t == 3, {'eps': 1})
    assert agent.learner.updates == 1 and not torch.equal(before, agent.net.packed())
    assert float(agent.state.abs().max()) == 0.0 and float(agent.fp.abs().max()) > 0     # the state is reset at done, the fingerprints are kept


def test_abi_lists_the_fma2c_entry_points():
    """include/resco_sim.h declares exactly the rs_fma2c_* functions resco_amd/sim.py binds, and the library exports them"""
    import re
    from resco_amd import sim as rsim
    from resco_amd.build import build_library
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(rs_fma2c_[a-z_]+)\s*\(', text))) == sorted(rsim.FMA2C_SYMBOLS)
    build_library()
    L = rsim.load_library()
    for s in rsim.FMA2C_SYMBOLS:
        assert hasattr(L, s), s
    body = text[text.index('typedef struct rs_fma2c_desc {') + len('typedef struct rs_fma2c_desc {'):text.index('} rs_fma2c_desc;')]
    names = []
    for decl in body.split(';'):
        decl = re.sub(r'^(const\s+)?(int32_t|float)\s*', '', decl.strip())
        names += [n.strip().lstrip('*') for n in decl.split(',') if n.strip()]
    assert [f[0] for f in rsim.Fma2cDesc._fields_] == names
