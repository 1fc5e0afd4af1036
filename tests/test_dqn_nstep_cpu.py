"""CPU: the target's options of the IDQN learners (n-step returns, Double DQN) without a GPU -- the walk of the fused update's header
through a host build (tests/dqn_nstep_host) against the Python twin, exhaustively on small rings; BatchedDQNLearner.loss on
DeviceReplay.sample's n-step rows against the float64 reference (tests/dqn_nstep_ref.py); sampling at the defaults unchanged; the
learners' signature rule and the checkpoint loader's refusal; the C ABI's two new calls."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from dqn_nstep_ref import GAMMA, NAMES, ring_case, rows, valid_slots, walk
from resco_amd import checkpoint
from resco_amd import sim as rsim
from resco_amd.agents.idqn_learn import BatchedDQNLearner, DeviceReplay, _sample_from_device_position, nstep_walk
from resco_amd.agents.idqn_rollout import BatchedIDQN
from train_ref import _ulp, build_host, net_as

RING = dict(lmax=9, T=8, N=9, head=3, count=8, done_slots=(5,))


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    vp, i32 = C.c_void_p, C.c_int32
    return build_host('dqn_nstep', tmp_path_factory.mktemp('dqn_nstep_host'), dict(dqn_nstep_walk_host=[vp, i32, i32, i32, i32, vp]))


def test_walk_of_the_header_against_the_twin(host):
    """every ring of T <= 6 slots: every head, every count >= 2, every subset of done, every slot the draw can name, n_step <= 5.
    The twin itself is held to the definition: rewards only of written slots before the newest, the bootstrap row written."""
    out = np.zeros(2, np.int32)
    n_walks = 0
    for T in range(2, 7):
        for head, count in itertools.product(range(T), range(2, T + 1)):
            ok = valid_slots(T, head, count)
            written, newest = set(ok) | {(head - 1) % T}, (head - 1) % T
            for bits in range(1 << T):
                done = np.array([(bits >> i) & 1 for i in range(T)], np.uint8)
                for t, n in itertools.product(ok, range(1, 6)):
                    m, cut = walk(done, T, head, t, n)
                    assert host.dqn_nstep_walk_host(done.ctypes.data, T, head, t, n, out.ctypes.data) == 0
                    assert (int(out[0]), bool(out[1])) == (m, cut), (T, head, count, bits, t, n)
                    taken = [(t + j) % T for j in range(m)]
                    assert 1 <= m <= n and set(taken) <= set(ok) and newest not in taken
                    assert not done[taken[:-1]].any() and cut == bool(done[taken[-1]])
                    assert cut or (t + m) % T in written
                    assert cut or m == n or (t + m) % T == newest, 'a walk stops early only at a cut or at the newest slot'
                    n_walks += 1
    assert n_walks > 30000
    assert host.dqn_nstep_walk_host(None, 3, 0, 0, 1, out.ctypes.data) == -1


def _cpu_ring(c, head, count):
    T, N, S, lmax = c['obs'].shape[:4]
    rp = DeviceReplay(T, N, S, lmax, device='cpu')
    rp.obs.copy_(torch.from_numpy(c['obs']))
    rp.act.copy_(torch.from_numpy(c['act']))
    rp.rew.copy_(torch.from_numpy(c['rew']))
    rp.done.copy_(torch.from_numpy(c['done']))
    rp.head, rp.count = head, count
    rp._pos[0], rp._pos[1] = head, count
    return rp


def _drawn(rp, B, seed):
    """the rows DeviceReplay.sample draws from a generator seeded with `seed`"""
    gen = torch.Generator().manual_seed(seed)
    k = torch.randint(0, rp.count - 1, (B, rp.S), generator=gen)
    t = (rp.head - rp.count + k) % rp.T
    return t, torch.randint(0, rp.N, (B, rp.S), generator=gen)


def test_the_ring_of_the_loss_test_holds_every_kind_of_row():
    c = ring_case(RING['lmax'], RING['T'], RING['N'], RING['done_slots'])
    T, head = RING['T'], RING['head']
    kinds = {t: walk(c['done'], T, head, t, 3) for t in valid_slots(T, head, RING['count'])}
    assert kinds == {3: (3, True), 4: (2, True), 5: (1, True), 6: (3, False), 7: (3, False), 0: (2, False), 1: (1, False)}


@pytest.mark.parametrize('n_step,double_q', [(3, True), (3, False), (1, True), (5, True)])
def test_torch_learner_against_the_float64_reference(n_step, double_q):
    """BatchedDQNLearner(n_step, double_q).loss on DeviceReplay.sample(..., n_step) rows: the sampled tensors are the walk's (bit for
    bit: the same float32 operations in the same order), loss and gradients are within 4 e_ref of the float64 truth (the loss gets
    4 float32 ulp besides: e_ref of ONE number can be zero by chance)"""
    B, seed = 96, 11
    c = ring_case(RING['lmax'], RING['T'], RING['N'], RING['done_slots'])
    rp = _cpu_ring(c, RING['head'], RING['count'])
    t, e = _drawn(rp, B, seed)
    idx = torch.stack([t, e], -1).numpy()
    assert set(idx[..., 0].ravel()) == set(valid_slots(RING['T'], RING['head'], RING['count'])), 'every kind of row is drawn'
    batch = rp.sample(B, torch.Generator().manual_seed(seed), n_step, GAMMA)
    w = rows(c, idx, RING['head'], n_step, np.float32)
    sig = np.arange(3)[None, :]
    assert np.array_equal(batch[0].numpy(), c['obs'][idx[..., 0], idx[..., 1], sig]) and np.array_equal(batch[1].numpy(), c['act'][idx[..., 0], idx[..., 1], sig])
    assert batch[2].numpy().tobytes() == w['R'].tobytes() and np.array_equal(batch[4].numpy() != 0, w['cut'])
    assert np.array_equal(batch[3].numpy(), c['obs'][w['u_m'], idx[..., 1], sig])
    if n_step > 1:
        assert len(batch) == 6 and batch[5].numpy().tobytes() == w['g'].tobytes()
    else:
        assert len(batch) == 5
    # the walk with the ring's position on the "device" (what the graph-captured update reads) is the same walk
    R, u_m, cut, g = nstep_walk(rp, t, e, rp._pos[0], n_step, GAMMA)
    assert R.numpy().tobytes() == w['R'].tobytes() and np.array_equal(u_m.numpy(), w['u_m']) and np.array_equal(cut.numpy(), w['cut'])

    import dqn_nstep_ref
    g64, l64, _, _ = dqn_nstep_ref.torch_grads(c, idx, torch.float64, RING['head'], n_step, double_q)
    g32, l32, _, _ = dqn_nstep_ref.torch_grads(c, idx, torch.float32, RING['head'], n_step, double_q)
    net = net_as(c['net'], torch.float32)
    learner = BatchedDQNLearner(net, gamma=GAMMA, batch_size=B, n_step=n_step, double_q=double_q)
    learner.target.load_state_dict(c['target'].state_dict())
    loss = learner.loss(*batch)
    loss.backward()
    err, e_ref = abs(float(loss.detach()) - l64.sum()), abs(l32.sum() - l64.sum())
    print('n %d dq %d loss |torch - truth| %.3e e_ref %.3e' % (n_step, double_q, err, e_ref))
    assert err <= 4 * e_ref + 4 * _ulp(np.float64(l64.sum()))
    for k in NAMES:
        err, e_ref = np.abs(getattr(net, k).grad.double().numpy() - g64[k]).max(), np.abs(g32[k] - g64[k]).max()
        print('  %-7s |torch - truth| %.3e  e_ref %.3e' % (k, err, e_ref))
        assert err <= 4 * e_ref, k


def test_default_sampling_is_unchanged():
    """sample(n_step=1) and the device-position twin return the five tensors of the one-step transition, from the same draws"""
    c = ring_case(RING['lmax'], RING['T'], RING['N'], RING['done_slots'])
    rp = _cpu_ring(c, RING['head'], RING['count'])
    B = 40
    t, e = _drawn(rp, B, 5)
    sig = rp._sig
    today = (rp.obs[t, e, sig], rp.act[t, e, sig].long(), rp.rew[t, e, sig], rp.obs[(t + 1) % rp.T, e, sig], rp.done[t].to(torch.float32))
    for got in (rp.sample(B, torch.Generator().manual_seed(5)), rp.sample(B, torch.Generator().manual_seed(5), n_step=1, gamma=GAMMA)):
        assert len(got) == 5
        for a, b in zip(got, today):
            assert a.dtype == b.dtype and torch.equal(a, b)
    torch.manual_seed(3)
    one = _sample_from_device_position(rp, B)
    torch.manual_seed(3)
    again = _sample_from_device_position(rp, B, 1, GAMMA)
    assert len(one) == len(again) == 5 and all(torch.equal(a, b) for a, b in zip(one, again))
    with pytest.raises(AssertionError, match='gamma'):
        rp.sample(B, n_step=3)


def _objects(n_step=1, double_q=False):
    net = BatchedIDQN((5, 3), (4, 2))
    net.init_like_reference(1)
    return dict(net=net, learner=BatchedDQNLearner(net, target_update=2, batch_size=4, n_step=n_step, double_q=double_q))


def test_signature_and_checkpoint_refusal(tmp_path):
    plain = {'batch': 4, 'target_update': 2, 'gamma': 0.99}
    assert _objects()['learner'].signature() == plain, 'the option keys are absent at the defaults'
    assert _objects(3, False)['learner'].signature() == dict(plain, n_step=3)
    assert _objects(1, True)['learner'].signature() == dict(plain, double_q=True)
    assert _objects(3, True)['learner'].signature() == dict(plain, n_step=3, double_q=True)
    import inspect
    from resco_amd.agents.idqn_learn_fused import FusedDQNLearner
    assert 'target_options_signature' in inspect.getsource(FusedDQNLearner.signature), 'one rule for both learners'
    path = str(tmp_path / 'a.pt')
    checkpoint.save(path, agent='IDQN', map_name='synthetic', objects=_objects(3, True), progress={})
    checkpoint.load(path, agent='IDQN', map_name='synthetic', objects=_objects(3, True))
    with pytest.raises(ValueError, match=r'learner\.n_step'):
        checkpoint.load(path, agent='IDQN', map_name='synthetic', objects=_objects())
    with pytest.raises(ValueError, match=r'mismatch in learner\.n_step\b'):
        checkpoint.load(path, agent='IDQN', map_name='synthetic', objects=_objects(1, True))
    checkpoint.save(path, agent='IDQN', map_name='synthetic', objects=_objects(), progress={})      # a file without the keys: a default learner
    checkpoint.load(path, agent='IDQN', map_name='synthetic', objects=_objects())
    with pytest.raises(ValueError, match=r'mismatch in learner\.double_q\b'):
        checkpoint.load(path, agent='IDQN', map_name='synthetic', objects=_objects(1, True))
    for bad in (0, 33):
        with pytest.raises(ValueError, match='n_step'):
            _objects(bad)


def test_abi_declares_and_exports_the_options():
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert re.search(r'int rs_dqn_set_target\(rs_dqn_handle p, int32_t n_step, int32_t double_q\);', text)
    assert re.search(r'int rs_dqn_get_target\(rs_dqn_handle p, int32_t \*n_step, int32_t \*double_q\);', text)
    from resco_amd.build import build_library
    build_library()
    L = rsim.load_library()
    for name in ('rs_dqn_set_target', 'rs_dqn_get_target'):
        assert name in rsim.ABI_SYMBOLS and hasattr(L, name), name
    # a NULL handle is refused with a text before anything touches a device
    assert L.rs_dqn_set_target(None, 1, 0) == -1 and b'rs_dqn_set_target' in L.rs_last_error(None)
    n, dq = C.c_int32(7), C.c_int32(7)
    assert L.rs_dqn_get_target(None, C.byref(n), C.byref(dq)) == -1 and (n.value, dq.value) == (7, 7)


def test_training_tool_flags():
    from tools import idqn_train
    assert idqn_train.target_flags(['--device-loop', 'cologne1', '--n-step', '3', '256', '--double-q']) == (dict(n_step=3, double_q=True), ['--device-loop', 'cologne1', '256'])
    assert idqn_train.target_flags(['cologne1']) == ({}, ['cologne1'])
    for bad in (['--n-step'], ['--n-step', '0'], ['--n-step', '33']):
        with pytest.raises(SystemExit):
            idqn_train.target_flags(bad)
