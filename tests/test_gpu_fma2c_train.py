"""GPU: the fused A2C update of FMA2C (rs_fma2c_learn_*; resco_amd/csrc/resco_fma2c_train.h, resco_amd/agents/fma2c_learn_fused.py)
against the float64 restatement of the reference (tests/fma2c_ref.py): gradients and losses of one update, determinism and
grouping, the clip, TF1's RMSProp, two consecutive updates beside the PyTorch learner, the policy reading the learner's vector, the
refusals and a training smoke run.  Yardstick: truth = float64; e_ref = max |plain float32 evaluation - truth| per tensor class; a
candidate gets 4 e_ref + 2 ulp32(|truth|) per element.  Returns and advantages are read back from the learner and are the
reference's inputs, as the actions are, so no row is ever left out."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import fma2c_ref as R
from fma2c_check import A_MAX, Case

pytestmark = pytest.mark.gpu

SEED = 20240918
SLOT = 904                  # resco_fma2c_train.h: FT_SLOT, the floats of a workspace slot
_cases = {}


def case(map_name):
    from resco_amd.config.mdp_config import activate
    if map_name not in _cases:
        _cases[map_name] = Case(map_name)
        _cases[map_name].net.cuda()
    activate('FMA2C', map_name)
    return _cases[map_name]


def make(c, N, T, net=None, seed=11, **kw):
    from resco_amd.agents.fma2c import FusedFMA2C
    from resco_amd.agents.fma2c_learn_fused import FusedA2CLearner
    net = net if net is not None else c.net
    pol = FusedFMA2C(net, N, seed=seed)
    return pol, FusedA2CLearner(net, pol, N, batch_size=T, **kw)


def segment(c, T, N, seed, values_scale=None):
    """the _segment recipe of tests/test_fma2c_cpu.py (rows and actions of T chained acts of the PyTorch net on synthetic lane
    aggregates, a non-zero start state), with raw rewards on both sides of the clip, acting values and a bootstrap value in place of
    ready-made returns: the kernel forms those.  T >= 3: a pre-step done inside the segment."""
    rng = np.random.default_rng(seed)
    L, net = c.layout, c.net
    agg, u = c.lane_agg(rng, T, N), rng.uniform(0, 1, (T, N, L.K))
    state, fp, rows, acts = torch.zeros(N, L.K, 4, 64, device='cuda'), torch.zeros(N, L.K, A_MAX, device='cuda'), [], []
    with torch.no_grad():
        for t in range(T):
            out = net.act(L.obs_rows(torch.as_tensor(agg[t]).cuda()), state, fp, torch.as_tensor(u[t], dtype=torch.float32).cuda())
            state, fp = out['state'], out['fingerprints']
            rows.append(out['rows']); acts.append(out['actions'])
    seg = dict(rows=torch.stack(rows).float().contiguous(), acts=torch.stack(acts).int().contiguous(),
               rewards=torch.as_tensor(rng.uniform(-9000, 3000, (T, N, L.K)), dtype=torch.float32).cuda(),
               values=torch.as_tensor(rng.normal(0, 1, (T, N, L.K)), dtype=torch.float32).cuda(),
               boot=torch.as_tensor(rng.normal(0, 1, (N, L.K)), dtype=torch.float32).cuda(),
               state0=torch.as_tensor(rng.normal(0, 0.3, (N, L.K, 4, 64)), dtype=torch.float32).cuda(),
               dones=np.zeros(T + 1, np.int32))
    if values_scale is not None:
        seg['values'] = seg['values'] * torch.as_tensor(values_scale, dtype=torch.float32).cuda()
    if T >= 3:
        seg['dones'][T // 2] = 1
    return seg


def load(lr, seg):
    T = seg['rows'].shape[0]
    lr.rows[:T], lr.acts[:T], lr.rews[:T], lr.vals[:T] = seg['rows'], seg['acts'], seg['rewards'], seg['values']
    lr.dones_dev[:T + 1] = torch.as_tensor(seg['dones']).cuda()
    lr.dones, lr.n = [bool(d) for d in seg['dones'][:T + 1]], T
    lr.buffer('states_bw').copy_(seg['state0'])


def named(lr, flat):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in lr.unpack(flat).items()}


def ref_grads(c, seg, Rs, Advs, dt, net=None):
    """fma2c_ref.agent_loss_grads per agent on the padding-stripped rows (tests/test_fma2c_cpu.py: _ref_grads)"""
    params = c.ref_params(net)
    rows, acts, state0 = seg['rows'].cpu().numpy(), seg['acts'].cpu().numpy().astype(np.int64), seg['state0'].cpu().numpy()
    T, out = rows.shape[0], {}
    for k, name in enumerate(c.names):
        a = c.table[name]
        w = a['n_s'] + a['n_w'] + a['n_f']
        out[name] = R.agent_loss_grads(params[name], a, rows[:, :, k, :w].astype(np.float64), acts[:, :, k], seg['dones'][:T].astype(bool),
                                       Rs[:, :, k].astype(np.float64), Advs[:, :, k].astype(np.float64), state0[:, k].astype(np.float64), dt)
    return out


def reference(c, seg, Rs, Advs, net=None):
    """truth, and e_ref per tensor class (the eleven tensors over all agents and both nets, and the loss)"""
    truth, plain = ref_grads(c, seg, Rs, Advs, np.float64, net), ref_grads(c, seg, Rs, Advs, np.float32, net)
    e_ref = {'loss': max(abs(float(plain[n][0]) - float(truth[n][0])) for n in c.names)}
    for n in c.names:
        for net_ in ('pi', 'v'):
            for t, want in truth[n][1][net_].items():
                if want.size:
                    e_ref[t] = max(e_ref.get(t, 0.0), float(np.abs(np.asarray(plain[n][1][net_][t], np.float64) - want).max()))
    return truth, e_ref


_PAD = dict(fcw_w=lambda a: (slice(0, a['n_s']),), fcf_w=lambda a: (slice(0, a['n_f']),), fct_w=lambda a: (slice(0, a['n_w']),),
            wx=lambda a: (slice(0, 224 if a['n_w'] else 192),))


def strip(c, k, ni, t, got, want):
    """the live part of agent k's tensor t of net ni as the reference shapes it, and a mask of its padding"""
    a = c.table[c.names[k]]
    live = np.zeros(got.shape, bool)
    if t in _PAD:
        live[_PAD[t](a)] = True
    elif t in ('head_w', 'head_b'):
        live[..., :(a['n_a'] if ni == 0 else 1)] = True
    elif t == 'fct_b':
        live[...] = a['n_w'] > 0
    else:
        live[...] = True
    return got[live].reshape(want.shape) if want is not None and want.size else None, ~live


def check_grads(c, truth, e_ref, loss, grads, label):
    worst = {}
    for k, name in enumerate(c.names):
        err = abs(float(loss[k]) - float(truth[name][0]))
        worst['loss'] = max(worst.get('loss', 0.0), err / e_ref['loss'] if e_ref['loss'] else 0.0)
        assert err <= R.bound(e_ref['loss'], truth[name][0]), (label, name, 'loss', err, e_ref['loss'])
        for ni, net_ in enumerate(('pi', 'v')):
            for t in grads:
                want = truth[name][1][net_].get(t)
                got, pad = strip(c, k, ni, t, grads[t][k, ni], want)
                assert (grads[t][k, ni][pad] == 0).all(), (label, name, net_, t, 'a padded gradient element is not exactly zero')
                if got is None:
                    continue
                err = np.abs(got - want)
                worst[t] = max(worst.get(t, 0.0), float(err.max()) / e_ref[t] if e_ref[t] else 0.0)
                assert (err <= R.bound(e_ref[t], want)).all(), (label, name, net_, t, float(err.max()), e_ref[t])
    print('%s  error / e_ref per class: %s' % (label, '  '.join('%s %.2f' % (t, worst[t]) for t in worst)))


# ------------------------------------------------------------------------------------------------ gradients against float64
@pytest.mark.parametrize('map_name,T,N', [(m, t, n) for m in ('cologne1', 'cologne3') for t, n in ((1, 1), (3, 3), (6, 33))] + [('ingolstadt21', 2, 3)])
def test_gradients_of_one_update(map_name, T, N):
    """one rs_fma2c_learn_grad from a non-zero states_bw: returns and advantages within the chained-operation bound of
    R.buffer_returns, the per-agent loss and every gradient tensor within 4 e_ref + 2 ulp32 of float64, every padded element zero"""
    c = case(map_name)
    seg = segment(c, T, N, SEED + T + N)
    pol, lr = make(c, N, T)
    load(lr, seg)
    loss = lr.grad(seg['boot']).cpu().numpy()
    torch.cuda.synchronize()
    Rs, Advs = lr.buffer('returns')[:T].cpu().numpy(), lr.buffer('advantages')[:T].cpu().numpy()
    r64 = R.clip_reward(seg['rewards'].cpu().numpy().astype(np.float64))
    want_R, want_A = R.buffer_returns(list(r64), list(seg['values'].cpu().numpy().astype(np.float64)), list(seg['dones'].astype(np.float64)),
                                      seg['boot'].cpu().numpy().astype(np.float64), 0.96)
    # T chained multiply-adds and the reward's division in float32 against float64 (tests/test_fma2c_cpu.py)
    assert np.abs(Rs - np.stack(want_R)).max() <= (T + 1) * R.ulp32(np.abs(np.stack(want_R)).max())
    assert np.abs(Advs - np.stack(want_A)).max() <= (T + 2) * R.ulp32(np.abs(np.stack(want_A)).max())
    truth, e_ref = reference(c, seg, Rs, Advs)
    check_grads(c, truth, e_ref, loss, named(lr, lr.buffer('grads')), '%s T=%d N=%d' % (map_name, T, N))
    np.testing.assert_array_equal(lr.buffer('states_bw').cpu().numpy(), seg['state0'].cpu().numpy())      # grad leaves the start state alone
    lr.close(); pol.close()


# ------------------------------------------------------------------------------------------------ determinism and grouping
def test_two_runs_and_any_grouping_give_the_same_bits():
    c = case('cologne3')
    T, N = 3, 33
    seg = segment(c, T, N, SEED)
    pol, lr = make(c, N, T)
    load(lr, seg)
    l1, g1 = lr.grad(seg['boot']).cpu().numpy().copy(), lr.buffer('grads').cpu().numpy().copy()
    lr.buffer('grads').fill_(7.0)
    l2, g2 = lr.grad(seg['boot']).cpu().numpy().copy(), lr.buffer('grads').cpu().numpy().copy()
    np.testing.assert_array_equal(g1, g2); np.testing.assert_array_equal(l1, l2)
    assert np.abs(g1).max() > 0
    pol2, one = make(c, N, T, workspace_bytes=2 * T * N * SLOT * 4)         # exactly one agent's need: K groups of one
    load(one, seg)
    l3, g3 = one.grad(seg['boot']).cpu().numpy().copy(), one.buffer('grads').cpu().numpy().copy()
    np.testing.assert_array_equal(g1, g3); np.testing.assert_array_equal(l1, l3)
    for x in (lr, one, pol, pol2):
        x.close()


# ------------------------------------------------------------------------------------------------ clip
def test_clip_scale_per_agent():
    """agent 3's advantages about 4000 times the others' (its acting values are): its norm exceeds 40 and its gradients are scaled by
    40 / norm, the others' by exactly 1"""
    c = case('cologne3')
    T, N, K = 6, 3, c.layout.K
    scale = np.ones(K); scale[3] = 4000.0
    seg = segment(c, T, N, SEED + 1, values_scale=scale)
    seg['dones'][:] = 0
    seg['rewards'] *= 0.1                   # returns of order one, as the advantages of the other agents
    pol, lr = make(c, N, T)
    load(lr, seg)
    lr.grad(seg['boot'])
    grads = named(lr, lr.buffer('grads'))
    Rs, Advs = lr.buffer('returns')[:T].cpu().numpy(), lr.buffer('advantages')[:T].cpu().numpy()
    assert np.abs(Advs[:, :, 3]).mean() > 1000 * np.abs(Advs[:, :, 0]).mean()
    w0 = lr.buffer('weights').clone()
    lr.step()
    torch.cuda.synchronize()
    truth = ref_grads(c, seg, Rs, Advs, np.float64)
    want = [R.global_norm_scale(truth[n][1]) for n in c.names]
    norms, scales = lr.buffer('norms').cpu().numpy(), lr.buffer('scales').cpu().numpy()
    assert want[3][1] > 40.0 and norms[3] > 40.0 and all(w[1] < 40.0 for i, w in enumerate(want) if i != 3)
    assert abs(float(scales[3]) - want[3][0]) <= 1e-5 * want[3][0], (float(scales[3]), want[3])
    assert all(float(scales[k]) == 1.0 for k in range(K) if k != 3)
    assert all(abs(float(norms[k]) - want[k][1]) <= 1e-5 * want[k][1] for k in range(K))
    # the scale reached the weights: agent 3's head bias moved by lr g scale / sqrt(ms + eps), ms = 0.99 + 0.01 (g scale)^2
    g = grads['head_b'][3, 1, 0] * float(scales[3])
    was = named(lr, w0)['head_b'][3, 1, 0]
    moved = was - named(lr, lr.buffer('weights'))['head_b'][3, 1, 0]
    assert abs(moved - 2.5e-4 * g / np.sqrt(0.99 + 0.01 * g * g + 1e-5)) <= 1e-6 * abs(moved) + 4 * R.ulp32(was)
    lr.close(); pol.close()


# ------------------------------------------------------------------------------------------------ RMSProp
def test_rmsprop_known_answer():
    """a known gradient (1, -2, 0 and a random tensor, its norm below the clip) through rs_fma2c_learn_step, twice: ms and w against
    R.tf_rmsprop in float64.  Bounds from the roundings of the step, not measured: 2 ulp32 for ms, 2 ulp32(|w'|) + 4 ulp32(|w' - w|) for w."""
    c = case('cologne1')
    pol, lr = make(c, 2, 1)
    ms, w, g = lr.buffer('ms'), lr.buffer('weights'), lr.buffer('grads')
    assert float(ms.min()) == 1.0 and float(ms.max()) == 1.0
    np.testing.assert_array_equal(w.cpu().numpy(), c.net.packed().cpu().numpy())
    gen = torch.Generator(device='cuda').manual_seed(SEED)
    g.copy_(0.01 * torch.randn(g.shape, generator=gen, device='cuda'))
    g[:3] = torch.tensor([1.0, -2.0, 0.0], device='cuda')
    w64, ms64, g64 = w.cpu().numpy().astype(np.float64), np.ones(g.numel()), g.cpu().numpy().astype(np.float64)
    for step in range(2):
        lr.step()
        torch.cuda.synchronize()
        assert (lr.buffer('scales').cpu().numpy() == 1.0).all() and float(lr.buffer('norms').max()) < 40.0
        want_w, want_ms = R.tf_rmsprop(w64, g64, ms64)
        got_w, got_ms = w.cpu().numpy().astype(np.float64), ms.cpu().numpy().astype(np.float64)
        assert (np.abs(got_ms - want_ms) <= 2 * R.ulp32(want_ms)).all(), step
        assert (np.abs(got_w - want_w) <= 2 * R.ulp32(want_w) + 4 * R.ulp32(want_w - w64)).all(), step
        w64, ms64 = got_w, got_ms                      # the second step continues from the first ms
    assert np.allclose(ms64[:3], [1.0, 0.99 * 1.03 + 0.04, 0.99 * 0.99], rtol=1e-6, atol=0)
    lr.close(); pol.close()


# ------------------------------------------------------------------------------------------------ beside the PyTorch learner
def test_two_consecutive_updates_follow_the_pytorch_learner():
    """cologne1, N = 3, T = 3, six acts of rs_fma2c_act: FusedA2CLearner.observe beside A2CLearner.observe on the same recorded
    inputs.  Both update at the same steps; the second fused update starts from the acting state at the first; after the done
    states_bw is zero and dones == [True].  After the first update the weights agree within lr (4 e_ref + 2 ulp32(|g|)) / sqrt(alpha)
    + 2 ulp32(|w|): ms >= alpha after one step from one, so a gradient error e moves a weight by at most lr e / sqrt(alpha)."""
    from resco_amd.agents.fma2c import A2CLearner, PARAMS
    c = case('cologne1')
    L, N, T = c.layout, 3, 3
    rng = np.random.default_rng(SEED + 2)
    net_f, net_t = copy.deepcopy(c.net), copy.deepcopy(c.net)
    pol, fused = make(c, N, T, net=net_f)
    ref = A2CLearner(net_t, N, batch_size=T)
    agg = torch.as_tensor(c.lane_agg(rng, 2 * T + 1, N)).cuda()
    state, macts = pol.buffer('state'), pol.buffer('mgr_actions')
    seen = []
    for t in range(2 * T):
        out = pol.act(agg[t].contiguous(), step_key=t, want=('value', 'rows'), out=fused.slot())
        assert out['rows'].data_ptr() == fused.rows[fused.n].data_ptr()        # the rows landed in the segment slot, no copy
        acts = torch.cat([macts, out['actions']], dim=1).long()
        rew = torch.as_tensor(rng.normal(0, 1000, (N, L.K)), dtype=torch.float32).cuda()
        done = t == 2 * T - 1
        boot = pol.value(agg[t + 1].contiguous()) if not done else None
        rows_c, val_c, state_c = out['rows'].clone(), out['value'].clone(), state.clone()
        if t % T == T - 1:
            seen.append((state_c, fused.states_bw.clone()))
        a = fused.observe(out['rows'], acts, rew, out['value'], done, state, lambda: boot)
        b = ref.observe(rows_c, acts, rew, val_c, done, state_c, lambda: boot)
        assert (a is not None) == (b is not None) == (t % T == T - 1)
        if t == T - 1:
            torch.cuda.synchronize()
            seg = dict(rows=fused.rows.clone(), acts=fused.acts.clone(), dones=np.zeros(T + 1, np.int32), state0=torch.zeros(N, L.K, 4, 64))
            Rs, Advs = fused.buffer('returns').cpu().numpy(), fused.buffer('advantages').cpu().numpy()
            truth, e_ref = reference(c, seg, Rs, Advs, net=c.net)
            for k, name in enumerate(c.names):
                assert abs(float(a[k]) - float(b[k])) <= 2 * R.bound(e_ref['loss'], truth[name][0]), name
            got, want = fused.unpack(fused.buffer('weights')), dict(net_t.named_parameters())
            for name in PARAMS:
                gw, ww = got[name].cpu().numpy().astype(np.float64), want[name].detach().cpu().numpy().astype(np.float64)
                if not gw.size:
                    continue
                g64 = np.zeros(gw.shape)                        # the truth's gradient in the padded layout
                for k, nm in enumerate(c.names):
                    for ni, net_ in enumerate(('pi', 'v')):
                        wt = truth[nm][1][net_].get(name)
                        if wt is not None and wt.size:
                            g64[k, ni][~strip(c, k, ni, name, gw[k, ni], None)[1]] = wt.ravel()
                lim = 2.5e-4 * (4 * e_ref[name] + 2 * R.ulp32(g64)) / np.sqrt(0.99) + 2 * R.ulp32(ww)
                assert (np.abs(gw - ww) <= lim).all(), (name, float(np.abs(gw - ww).max()), float(lim.min()))
                assert np.abs(ww - getattr(c.net, name).detach().cpu().numpy()).max() > 0, name        # and they did move
    torch.cuda.synchronize()
    assert fused.updates == ref.updates == 2
    # the first update ran from zeros, the second from the acting state at the first update
    assert float(seen[0][1].abs().max()) == 0.0
    assert torch.equal(seen[1][1], seen[0][0]) and float(seen[0][0].abs().max()) > 0
    assert float(fused.states_bw.abs().max()) == 0.0 and fused.dones == [True] and fused.steps_done == 0 and fused.n == 0
    assert int(fused.dones_dev[0]) == 1
    fused.close(); pol.close()


# ------------------------------------------------------------------------------------------------ the policy reads the learner's vector
def test_policy_acts_with_the_updated_vector():
    from resco_amd.agents.fma2c import FusedFMA2C
    c = case('cologne3')
    L, N, T = c.layout, 5, 3
    net = copy.deepcopy(c.net)
    seg = segment(c, T, N, SEED + 3)
    pol, lr = make(c, N, T, net=net)
    agg = torch.as_tensor(c.lane_agg(np.random.default_rng(SEED + 4), 3, N)).cuda()
    pol.act(agg[0].contiguous(), step_key=0)                        # state, fingerprints and parity in use
    load(lr, seg)
    before = lr.buffer('weights').clone()
    lr.update(seg['boot'], pol.buffer('state'))
    torch.cuda.synchronize()
    assert not torch.equal(before, lr.buffer('weights'))
    lr.pull()
    assert torch.equal(net.packed(), lr.buffer('weights'))
    fresh = FusedFMA2C(net, N, seed=11)
    for b in ('state', 'fingerprints', 'mgr_actions', 'parity'):
        fresh.buffer(b).copy_(pol.buffer(b))
    for key in (1, 2):
        a, b = pol.act(agg[key].contiguous(), step_key=key), fresh.act(agg[key].contiguous(), step_key=key)
        torch.cuda.synchronize()
        for k in ('actions', 'pi', 'value', 'rows'):
            np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=k)
        np.testing.assert_array_equal(pol.buffer('state').cpu().numpy(), fresh.buffer('state').cpu().numpy())
        if key == 1:
            lr.close()                                              # the policy goes on with the last weights, in its own vector
    pol.close(); fresh.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from resco_amd.agents.mplight import FusedMPLight, frap_from_scenario
    from resco_amd.sim import Fma2cLearnConfig
    c = case('cologne3')
    L, N, T = c.layout, 4, 3
    seg = segment(c, T, N, SEED + 5)
    pol, lr = make(c, N, T)
    load(lr, seg)
    lib = pol._lib
    err = lambda: (lib.rs_last_error(None) or b'').decode()
    grads = lr.buffer('grads')
    grads.fill_(-7.0)
    w0, s0 = lr.buffer('weights').clone(), lr.buffer('states_bw').clone()
    ptr = [lr.rows.data_ptr(), lr.acts.data_ptr(), lr.rews.data_ptr(), lr.vals.data_ptr(), lr.dones_dev.data_ptr(), seg['boot'].data_ptr()]
    st = pol.buffer('state')

    def untouched():
        torch.cuda.synchronize()
        assert int((grads != -7.0).sum()) == 0 and torch.equal(w0, lr.buffer('weights')) and torch.equal(s0, lr.buffer('states_bw'))

    # NULL handles and pointers
    assert lib.rs_fma2c_learn_grad(None, *ptr, T, None, 1) == -1 and 'NULL' in err()
    assert lib.rs_fma2c_learn_update(None, *ptr, T, None, st.data_ptr(), 1) == -1 and 'NULL' in err()
    for i in range(6):
        bad = list(ptr); bad[i] = None
        assert lib.rs_fma2c_learn_grad(lr.handle, *bad, T, None, 1) == -1 and 'NULL' in err()
        assert lib.rs_fma2c_learn_update(lr.handle, *bad, T, None, st.data_ptr(), 1) == -1 and 'NULL' in err()
    assert lib.rs_fma2c_learn_update(lr.handle, *ptr, T, None, None, 1) == -1 and 'NULL' in err()
    assert lib.rs_fma2c_learn_step(None, 1) == -1 and 'NULL' in err()
    assert lib.rs_fma2c_learn_reset(None, 1) == -1 and 'NULL' in err()
    assert lib.rs_fma2c_learn_buffer(None, 0, C.byref(C.c_void_p())) == -1 and 'NULL' in err()
    assert lib.rs_fma2c_learn_buffer(lr.handle, 0, None) == -1 and 'NULL' in err()
    assert lib.rs_fma2c_learn_buffer(lr.handle, 8, C.byref(C.c_void_p())) == -1 and 'which' in err()
    untouched()
    # T outside 1 .. t_max
    for bad_T in (0, -1, T + 1):
        assert lib.rs_fma2c_learn_grad(lr.handle, *ptr, bad_T, None, 1) == -1 and '1 <= T <= t_max' in err()
        assert lib.rs_fma2c_learn_update(lr.handle, *ptr, bad_T, None, st.data_ptr(), 1) == -1 and '1 <= T <= t_max' in err()
    untouched()
    # create: NULLs, a policy of another kind, another n_envs, a cap below one agent's need
    cfg = Fma2cLearnConfig(0.96, 2.5e-4, 0.99, 1e-5, 40.0, 0.5, 0.001, 2000.0, 2.0, 0)

    def create(p, cf, n, t):
        h = C.c_void_p()
        rc = lib.rs_fma2c_learn_create(p, C.byref(cf) if cf is not None else None, n, t, C.byref(h))
        assert h.value is None
        return rc
    mnet = frap_from_scenario(c.sc, 1).cuda()
    mnet.init_like_reference(0)
    mpl = FusedMPLight(mnet, c.sc)
    assert create(None, cfg, N, T) == -1 and 'NULL' in err()
    assert create(pol.handle, None, N, T) == -1 and 'NULL' in err()
    assert lib.rs_fma2c_learn_create(pol.handle, C.byref(cfg), N, T, None) == -1 and 'NULL' in err()
    assert create(mpl.handle, cfg, N, T) == -1 and 'not an rs_fma2c_create policy' in err()
    assert create(pol.handle, cfg, N - 1, T) == -1 and "must equal the policy's max_envs" in err()
    assert create(pol.handle, cfg, N + 1, T) == -1 and "must equal the policy's max_envs" in err()
    assert create(pol.handle, cfg, N, 0) == -1 and 't_max >= 1' in err()
    small = Fma2cLearnConfig(0.96, 2.5e-4, 0.99, 1e-5, 40.0, 0.5, 0.001, 2000.0, 2.0, 2 * T * N * SLOT * 4 - 1)
    assert create(pol.handle, small, N, T) == -1 and "below one agent's need" in err()
    untouched()
    # the refused creates left the policy pointed at the learner: a grad still works and writes the buffer
    lr.grad(seg['boot'])
    torch.cuda.synchronize()
    assert int((grads == -7.0).sum()) == 0
    for x in (lr, pol, mpl):
        x.close()


# ------------------------------------------------------------------------------------------------ training smoke
def test_training_smoke_with_device_update():
    """tools/fma2c_train.py --device-update --steps-per-episode 7 cologne1 32 2: two updates (one per episode end), finite losses, every
    agent's weights moved, the padding still zero.  No claim about learning."""
    from resco_amd.agents.fma2c import BatchedFMA2C, PARAMS
    from resco_amd.agents.fma2c_learn_fused import FusedA2CLearner
    from tools.fma2c_train import main
    c0 = Case('cologne1', seed=0)
    start = BatchedFMA2C(c0.layout).init_like_reference(0)
    keep = {}
    rows, final = main('cologne1', 32, 2, seed=0, steps_per_episode=7, quiet=True, keep=keep, device_update=True)
    net, lr, L = keep['net'], keep['learner'], keep['layout']
    assert isinstance(lr, FusedA2CLearner) and lr.updates == 2 and len(rows) == 2
    assert all(r['loss'] is not None and np.isfinite(r['loss']) for r in rows) and bool(torch.isfinite(lr.last_loss).all())
    assert torch.equal(net.packed(), lr.buffer('weights'))          # main() pulled the learner's weights into the net
    for name in PARAMS:
        now, was = getattr(net, name).detach().cpu().numpy(), getattr(start, name).detach().numpy()
        for k in range(L.K):
            for ni in range(2):
                _, pad = strip(c0, k, ni, name, now[k, ni], None)
                assert (now[k, ni][pad] == 0).all(), (name, k, ni)
        # (fcf_b of an agent without fingerprints starts at relu(0): no gradient until it is positive; a manager has no fct block)
        if name in ('fcw_w', 'wx', 'wh', 'lb', 'head_w', 'head_b', 'fcw_b'):
            assert all((now[k] != was[k]).any() for k in range(L.K)), name
    keep['policy'].close()
    keep['env'].close()
