"""CPU: the per-element pieces of the fused A2C update of FMA2C (resco_amd/csrc/resco_fma2c_train.h), built for the host
(tests/fma2c_train_host), against the float64 restatement of the reference (tests/fma2c_ref.py), and the rs_fma2c_learn_* header.
Yardstick: truth = float64; e_ref = max |plain float32 evaluation - truth| over a tensor class; a candidate gets 4 e_ref + 2 ulp32(|truth|)
per element."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fma2c_ref as R
from conftest import ROOT

SEED = 20240917
F = C.c_float


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('fma2c_train_host') / 'fma2c_train_host.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math', '-w', '-shared',
                           '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'resco_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'fma2c_train_host', 'fma2c_train_host.cpp'), '-o', out])
    lib = C.CDLL(out)
    lib.ft_host_returns.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, F, C.c_int, F, F, F, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ft_host_row_loss_grad.argtypes = [C.c_void_p, C.c_int, C.c_int, F, F, F, F, F, F, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ft_host_gate_fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ft_host_gate_bwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, F, C.c_int, C.c_void_p, C.c_void_p]
    lib.ft_host_rmsprop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, F, C.c_int, C.c_double, C.c_double, C.c_double]
    lib.ft_host_splits.argtypes = [C.c_longlong, C.POINTER(C.c_int)]
    return lib


def p(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------ the row's loss gradient
def _row_ref(logits, acts, adv, ret, v, NT, dt, v_coef=0.5, beta=0.001):
    """fma2c_ref.agent_loss_grads:159-169 for rows of logits [n, n_a] and values [n]: douts of both nets and the three un-scaled terms"""
    logits, adv, ret, v, NT = np.asarray(logits, dt), np.asarray(adv, dt), np.asarray(ret, dt), np.asarray(v, dt), dt(NT)
    pi = R.softmax(logits)
    lp = np.log(np.clip(pi, 1e-10, 1.0))
    ent = -(pi * lp).sum(axis=1)
    onehot = np.eye(logits.shape[1], dtype=dt)[acts]
    dl = -(adv[:, None] / NT) * (onehot - pi) + dt(beta) / NT * pi * (lp + ent[:, None])
    dv = dt(v_coef) * (v - ret) / NT
    return dl, dv, np.stack([-(lp * onehot).sum(axis=1) * adv, (ret - v) ** 2, ent], axis=1)


def test_row_restatement_is_agent_loss_grads():
    """the restated lines above against agent_loss_grads itself at T = N = 1, where head_b's gradient IS the row's dout"""
    rng = np.random.default_rng(SEED)
    a = dict(n_a=4, n_s=5, n_w=3, n_f=4)
    mk = lambda n_out: dict(fcw_w=rng.normal(0, .3, (5, 128)), fcw_b=rng.normal(0, .1, 128), fcf_w=rng.normal(0, .3, (4, 64)), fcf_b=rng.normal(0, .1, 64),
                            fct_w=rng.normal(0, .3, (3, 32)), fct_b=rng.normal(0, .1, 32), wx=rng.normal(0, .1, (224, 256)), wh=rng.normal(0, .1, (64, 256)),
                            lb=rng.normal(0, .1, 256), head_w=rng.normal(0, .3, (64, n_out)), head_b=rng.normal(0, .1, n_out))
    params = {'pi': mk(4), 'v': mk(1)}
    x, st = rng.uniform(0, 2, (1, 1, 12)), rng.normal(0, .3, (1, 4, 64))
    loss, g = R.agent_loss_grads(params, a, x, np.array([[2]]), np.array([False]), np.array([[0.7]]), np.array([[-1.3]]), st)
    lg = R.net_forward(params['pi'], a, x[0], st[:, 0], st[:, 1], 0.0, np.float64)[0]
    v = R.net_forward(params['v'], a, x[0], st[:, 2], st[:, 3], 0.0, np.float64)[0][:, 0]
    dl, dv, terms = _row_ref(lg, np.array([2]), [-1.3], [0.7], v, 1, np.float64)
    assert np.abs(dl[0] - g['pi']['head_b']).max() < 1e-14 and abs(dv[0] - g['v']['head_b'][0]) < 1e-14
    assert abs(loss - (terms[0, 0] + 0.25 * terms[0, 1] - 0.001 * terms[0, 2])) < 1e-13


@pytest.mark.parametrize('n_a', [2, 4, 8])
def test_row_loss_gradient(host_lib, n_a):
    """ft_pi_row_grad / ft_v_row_grad on 96 rows, advantages of both signs, 1 / (T N) with T N = 198"""
    rng = np.random.default_rng(SEED + n_a)
    n, NT = 96, 198
    logits = rng.normal(0, 1.5, (n, n_a)).astype(np.float32)
    acts = rng.integers(0, n_a, n)
    adv, ret, v = [rng.normal(0, 1, n).astype(np.float32) for _ in range(3)]
    assert (adv > 0).any() and (adv < 0).any()
    truth = _row_ref(logits.astype(np.float64), acts, adv.astype(np.float64), ret.astype(np.float64), v.astype(np.float64), NT, np.float64)
    plain = _row_ref(logits, acts, adv, ret, v, NT, np.float32)
    e_ref = [float(np.abs(np.asarray(q, np.float64) - t).max()) for q, t in zip(plain, truth)]
    dl, dv, terms = np.zeros((n, 8), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    for r in range(n):
        host_lib.ft_host_row_loss_grad(p(logits[r]), n_a, int(acts[r]), adv[r], v[r], ret[r], np.float32(1.0) / np.float32(NT), 0.5, 0.001,
                                       p(dl[r]), p(dv[r:r + 1]), p(terms[r]))
    assert (dl[:, n_a:] == 0).all()
    for name, got, want, e in (('dlogits', dl[:, :n_a], truth[0], e_ref[0]), ('dv', dv, truth[1], e_ref[1]), ('terms', terms, truth[2], e_ref[2])):
        err = np.abs(got.astype(np.float64) - want)
        print('n_a %d %-7s max err %.3e  e_ref %.3e  ratio %.2f' % (n_a, name, err.max(), e, err.max() / e))
        assert (err <= R.bound(e, want)).all(), name


def test_clamped_probability_passes_no_gradient(host_lib):
    """pi[act] < 1e-10: log(clamp(pi)) is a constant there, so autograd gives the policy term no gradient; the entropy term's stays"""
    import torch
    logits = np.array([30.0, 0.0, -2.0, 1.0], np.float32)
    lt = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    pi = torch.softmax(lt, 0)
    lp = torch.log(torch.clamp(pi, 1e-10, 1.0))
    (-(lp[2] * 1.7) - 0.001 * -(pi * lp).sum()).backward()
    dl, dv, terms = np.zeros(8, np.float32), np.zeros(1, np.float32), np.zeros(3, np.float32)
    host_lib.ft_host_row_loss_grad(p(logits), 4, 2, 1.7, 0.0, 0.0, 1.0, 0.5, 0.001, p(dl), p(dv), p(terms))
    want = lt.grad.numpy()
    assert float(pi[2]) < 1e-10
    assert np.abs(dl[:4] - want).max() <= 1e-6 * np.abs(want).max() + 1e-12       # float32 softmax of float32 logits against float64
    assert abs(want).max() < 1e-3                                                    # no -adv (onehot - pi) term: that would be ~1.7


# ------------------------------------------------------------------------------------------------ returns
def test_returns_piece(host_lib):
    """a done in the middle and one at the end, rewards on both sides of the clip, against R.buffer_returns / R.clip_reward"""
    rng = np.random.default_rng(SEED)
    T, cols, gamma = 6, 8, 0.96
    rew, val = rng.uniform(-9000, 3000, (T, cols)).astype(np.float32), rng.normal(0, 1, (T, cols)).astype(np.float32)
    dones = np.array([0, 0, 0, 1, 0, 0, 1], np.int32)          # pre-step done of step 0, then the post-step done of every step
    boot = rng.normal(0, 1, cols).astype(np.float32)
    want_r = R.clip_reward(rew.astype(np.float64))
    assert np.abs(want_r).max() == 2.0 and (np.abs(want_r) < 2.0).any()
    want_R, want_A = R.buffer_returns(list(want_r), list(val.astype(np.float64)), list(dones.astype(np.float64)), boot.astype(np.float64), gamma)
    want_R, want_A = np.stack(want_R), np.stack(want_A)
    got_r, got_R, got_A = np.zeros((T, cols), np.float32), np.zeros((T, cols), np.float32), np.zeros((T, cols), np.float32)
    for c in range(cols):
        cr, cR, cA = np.zeros(T, np.float32), np.zeros(T, np.float32), np.zeros(T, np.float32)
        host_lib.ft_host_returns(p(np.ascontiguousarray(rew[:, c])), p(np.ascontiguousarray(val[:, c])), p(dones), boot[c], T, gamma, 2000.0, 2.0, p(cr), p(cR), p(cA))
        got_r[:, c], got_R[:, c], got_A[:, c] = cr, cR, cA
    assert (np.abs(got_r - want_r) <= R.ulp32(want_r)).all()                     # one division
    # T chained multiply-adds in float32 against float64: T ulp32 of the largest magnitude (tests/test_fma2c_cpu.py)
    assert np.abs(got_R - want_R).max() <= T * R.ulp32(np.abs(want_R).max())
    assert np.abs(got_A - want_A).max() <= (T + 1) * R.ulp32(np.abs(want_A).max())
    np.testing.assert_array_equal(got_R[2], got_r[2])                              # no bootstrap across the done after step 2
    np.testing.assert_array_equal(got_R[5], got_r[5])                              # ... nor across the one at the end
    # no clip and no norm when the configuration says 0
    cr, cR, cA = np.zeros(T, np.float32), np.zeros(T, np.float32), np.zeros(T, np.float32)
    host_lib.ft_host_returns(p(np.ascontiguousarray(rew[:, 0])), p(np.ascontiguousarray(val[:, 0])), p(dones), 0.0, T, gamma, 0.0, 0.0, p(cr), p(cR), p(cA))
    np.testing.assert_array_equal(cr, rew[:, 0])


# ------------------------------------------------------------------------------------------------ one LSTM backward step
def _gate_bwd_ref(dh, dc_next, g, c_in, keep, dt):
    """fma2c_ref.agent_loss_grads:176-182 from the activated gates (tc = tanh(f c_in + i u), as net_forward forms it)"""
    dh, dc_next, c_in = np.asarray(dh, dt), np.asarray(dc_next, dt), np.asarray(c_in, dt)
    i, f, o, u = [np.asarray(x, dt) for x in g]
    tc = np.tanh(f * c_in + i * u)
    do = dh * tc
    dc = dc_next + dh * o * (1 - tc ** 2)
    df, di, du = dc * c_in, dc * u, dc * i
    dz = np.stack([di * i * (1 - i), df * f * (1 - f), do * o * (1 - o), du * (1 - u ** 2)])
    return dz, dc * f * dt(keep)


@pytest.mark.parametrize('keep', [0.0, 1.0])
def test_gate_backward_step(host_lib, keep):
    rng = np.random.default_rng(SEED + int(keep))
    n = 512
    z = rng.normal(0, 1.5, (4, n)).astype(np.float32)
    c_in = (rng.normal(0, 0.5, n) * keep).astype(np.float32)
    g, c, h = np.zeros((4, n), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    host_lib.ft_host_gate_fwd(p(z), p(c_in), n, p(g), p(c), p(h))
    # the forward is fm_lstm_gate's: expf within 1 ulp32, the sum and the quotient half an ulp each, tanhf within 2: below 4 ulp32
    z64 = z.astype(np.float64)
    want_g = np.stack([R.sigmoid(z64[0]), R.sigmoid(z64[1]), R.sigmoid(z64[2]), np.tanh(z64[3])])
    assert (np.abs(g - want_g) <= 4 * R.ulp32(want_g)).all()
    dh, dc_next = rng.normal(0, 1e-2, n).astype(np.float32), rng.normal(0, 1e-2, n).astype(np.float32)
    truth = _gate_bwd_ref(dh.astype(np.float64), dc_next.astype(np.float64), g.astype(np.float64), c_in.astype(np.float64), keep, np.float64)
    plain = _gate_bwd_ref(dh, dc_next, g, c_in, keep, np.float32)
    dz, dcp = np.zeros((4, n), np.float32), np.zeros(n, np.float32)
    host_lib.ft_host_gate_bwd(p(dh), p(dc_next), p(g), p(c_in), keep, n, p(dz), p(dcp))
    for name, got, want, pl in (('dz', dz, truth[0], plain[0]), ('dc_prev', dcp, truth[1], plain[1])):
        e = float(np.abs(pl.astype(np.float64) - want).max())
        err = np.abs(got.astype(np.float64) - want)
        print('keep %.0f %-7s max err %.3e  e_ref %.3e' % (keep, name, err.max(), e))
        assert (err <= R.bound(e, want)).all(), name
    if keep == 0.0:
        assert (dcp == 0).all() and (dz[1] == 0).all()          # nothing flows into the state before a done; f's gradient is dc c_in = 0


# ------------------------------------------------------------------------------------------------ RMSProp element
def test_rmsprop_element(host_lib):
    """TF1's RMSProp formed in double and rounded once: 2 ulp32(|w'|) + 4 ulp32(|w' - w|) for w, 2 ulp32 for ms (the GPU test's bound)"""
    rng = np.random.default_rng(SEED)
    g = np.concatenate([[1.0, -2.0, 0.0], rng.normal(0, 1, 509)]).astype(np.float32)
    w, ms = rng.normal(0, 0.5, 512).astype(np.float32), np.ones(512, np.float32)
    for _ in range(2):
        w0 = w.copy()
        want_w, want_ms = R.tf_rmsprop(w.astype(np.float64), g.astype(np.float64), ms.astype(np.float64))
        host_lib.ft_host_rmsprop(p(w), p(ms), p(g), 1.0, 512, 2.5e-4, 0.99, 1e-5)
        assert (np.abs(ms - want_ms) <= 2 * R.ulp32(want_ms)).all()
        assert (np.abs(w - want_w) <= 2 * R.ulp32(want_w) + 4 * R.ulp32(want_w - w0)).all()
    assert np.allclose(ms[:3], [0.99 * 1.0 + 0.01, 0.99 * 1.03 + 0.04, 0.99 * 0.99], rtol=1e-6)      # the second step continued from the first ms


def test_row_partition_is_fixed_and_covers(host_lib):
    """the splits of the T N rows of a weight gradient depend on T N alone, are even-sized and cover every row once"""
    for rows in (1, 2, 9, 198, 127, 128, 129, 2049, 30720, 122880):
        per = C.c_int()
        P = host_lib.ft_host_splits(rows, C.byref(per))
        assert 1 <= P <= 16 and per.value % 2 == 0 and (P - 1) * per.value < rows <= P * per.value, (rows, P, per.value)


# ------------------------------------------------------------------------------------------------ header
def test_abi_lists_the_learner_entry_points():
    """include/resco_sim.h declares exactly the rs_fma2c_learn_* functions resco_amd/sim.py binds, the library exports them, and the
    config struct's fields are the ctypes mirror's"""
    from resco_amd import sim as rsim
    from resco_amd.build import build_library
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    names = sorted(set(re.findall(r'\b(rs_fma2c_learn_[a-z_]+)\s*\(', text)))
    assert names == sorted(s for s in rsim.FMA2C_SYMBOLS if s.startswith('rs_fma2c_learn_')) and len(names) == 7
    build_library()
    L = rsim.load_library()
    for s in names:
        assert hasattr(L, s), s
    body = text[text.index('typedef struct rs_fma2c_learn_config {') + len('typedef struct rs_fma2c_learn_config {'):text.index('} rs_fma2c_learn_config;')]
    fields = []
    for decl in body.split(';'):
        m = re.match(r'^(double|int64_t)\s+(.*)$', decl.strip(), flags=re.S)
        if m:
            fields += [(n.strip(), C.c_double if m.group(1) == 'double' else C.c_int64) for n in m.group(2).split(',')]
    assert fields == list(rsim.Fma2cLearnConfig._fields_)
    assert [n for n, _ in fields] == ['gamma', 'lr', 'alpha', 'eps', 'max_grad_norm', 'value_coef', 'entropy_coef', 'reward_norm', 'reward_clip', 'workspace_bytes']
