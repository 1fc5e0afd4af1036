"""GPU: the DQN update on the device (rs_dqn_sample / rs_dqn_grad / rs_dqn_step / rs_dqn_update, resco_amd/csrc/resco_dqn_train.h;
FusedDQNLearner).  The chain: a minibatch gradient against float64 autograd of BatchedDQNLearner.loss; the ring's semantics (wrap,
episode ends, the signal's own actions in the target's max); the draw against the counter hash; Adam against torch from equal
gradients; rs_dqn_update against the loop of the three, bit for bit; then the learner's bookkeeping and the training tool end to end.
Yardstick (tests/dqn_train_ref.py): truth = torch in float64, e_ref = torch in float32 against it, the device gets 4 e_ref per tensor.

Every ring is a DeviceReplay with three sentinel environments past the case's N; they and every slot a test declares unreadable hold
NaN observations, action -777 and NaN rewards: one of them read, and a gradient is NaN."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dqn_train_ref import NAMES, RING_STATES, _batch, case, check_sample, predict_sample, torch_grads, torch_step, torch_update
from resco_amd.agents.idqn_learn import BatchedDQNLearner, DeviceReplay
from resco_amd.agents.idqn_learn_fused import FusedDQNLearner
from resco_amd.sim import DQNConfig, DQNRing, DQNTensors, load_library, torch_stream
from train_ref import _device_net, _np, assert_adam_state, check_4_e_ref, compare_gradients

pytestmark = pytest.mark.gpu

RS_EINVAL = -1
PAD_ENVS = 3
SEED = 0x5EED


@functools.lru_cache(maxsize=None)
def _case(lmax, T, N):
    return case(lmax, T, N, seed=lmax, done_slots=(1,))


def _draw_idx(T, N, B, slots=None):
    rng = np.random.default_rng(B)
    t = rng.integers(0, T, (B, 3)) if slots is None else rng.choice(np.asarray(slots), (B, 3))
    return np.stack([t, rng.integers(0, N, (B, 3))], -1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _reference(lmax, T, N, B, slots=None):
    """(idx, truth gradients, float32 gradients, truth loss, float32 loss): computed once, shared, never changed"""
    c = _case(lmax, T, N)
    idx = _draw_idx(T, N, B, slots)
    g64, l64, d64 = torch_grads(c, idx, torch.float64)
    g32, l32, _ = torch_grads(c, idx, torch.float32)
    frac = (np.abs(d64) > 1).mean()
    assert 0.2 <= frac <= 0.8, 'both branches of the Huber loss must be well populated: %.2f' % frac
    return idx, g64, g32, l64, l32


def _learner(c, B, **kw):
    """a FusedDQNLearner on a device copy of the case's network, its target network the case's"""
    net = _device_net(c['net'])
    learner = FusedDQNLearner(net, batch_size=B, seed=SEED, **kw)
    with torch.no_grad():
        for k in NAMES:
            getattr(learner.target, k).copy_(getattr(c['target'], k))
    return net, learner


def _sentinel_ring(T, N, S, lmax):
    """an empty DeviceReplay whose every slot holds what must not be read: NaN observations, action -777, NaN rewards"""
    rp = DeviceReplay(T, N, S, lmax, device='cuda')
    rp.obs.fill_(float('nan'))
    rp.act.fill_(-777)
    rp.rew.fill_(float('nan'))
    return rp


def _device_ring(c, unreadable=(), head=0, count=None, pad=PAD_ENVS):
    """the case's ring on the device with `pad` sentinel environments; `unreadable`: slots that hold sentinels in every environment"""
    T, N, S, lmax = c['obs'].shape[:4]
    rp = _sentinel_ring(T, N + pad, S, lmax)
    keep = [t for t in range(T) if t not in unreadable]
    rp.obs[keep, :N] = torch.from_numpy(c['obs'][keep]).cuda()
    rp.act[keep, :N] = torch.from_numpy(c['act'][keep]).cuda()
    rp.rew[keep, :N] = torch.from_numpy(c['rew'][keep]).cuda()
    rp.done.copy_(torch.from_numpy(c['done']))
    rp.head, rp.count = head, T if count is None else count
    return rp


def _compare(got, loss, g64, g32, l64, l32):
    worst = compare_gradients(NAMES, got, g64, g32)
    check_4_e_ref('loss', loss, l64, l32, worst)
    assert not worst, worst


@pytest.mark.parametrize('lmax,T,N,B', [(2, 3, 5, 33), (9, 6, 9, 96), (17, 4, 11, 70), (5, 8, 40, 530)])
def test_minibatch_gradient(lmax, T, N, B):
    """B below and across a 64-row tile, the narrowest and the widest signal; B = 530 = 9 tiles in 2 chunks of the fc1 backward
    (PPT_CH = 512 rows), the second of one tile with 18 real rows"""
    c = _case(lmax, T, N)
    idx, g64, g32, l64, l32 = _reference(lmax, T, N, B)
    net, learner = _learner(c, B)
    rp = _device_ring(c)
    idx_t = torch.from_numpy(idx).cuda()
    got = _np(learner.grad(rp, idx_t))
    loss = learner.loss_out.cpu().numpy().copy()
    print('lmax %d ring %d x %d, B %d' % (lmax, T, N, B))
    _compare(got, loss, g64, g32, l64, l32)
    # padded fc1 rows and fc3 columns: exactly zero
    H = lmax - 1
    for s, l in enumerate(net.lanes):
        assert (got['fc1_w'][s].reshape(64, H, 4, 64)[:, l - 1:] == 0).all()
    amask = net.action_mask.cpu().numpy()
    assert (got['fc3_b'][~amask] == 0).all() and (got['fc3_w'][np.broadcast_to(~amask[:, None, :], got['fc3_w'].shape)] == 0).all()
    assert all(np.abs(got[k]).max() > 0 for k in NAMES)
    # the same bits again
    again = _np(learner.grad(rp, idx_t))
    for k in NAMES:
        assert got[k].tobytes() == again[k].tobytes(), k
    assert loss.tobytes() == learner.loss_out.cpu().numpy().tobytes()
    learner.close()


def test_ring_semantics():
    """Rows of the last slot (their successor is slot 0), rows of slot 1, which ended an episode -- slot 2 behind it is unreadable in
    every environment, so a bootstrap that is multiplied by zero instead of cut gives NaN -- and a signal with one action that trains"""
    lmax, T, N, B = 9, 6, 9, 96
    c = _case(lmax, T, N)
    assert c['done'][1] and not c['done'][T - 1]
    idx, g64, g32, l64, l32 = _reference(lmax, T, N, B, slots=(0, 1, 3, T - 1))
    assert (idx[..., 0] == T - 1).sum() > 10 and (idx[..., 0] == 1).sum() > 10
    net, learner = _learner(c, B)
    got = _np(learner.grad(_device_ring(c, unreadable=(2,)), torch.from_numpy(idx).cuda()))
    _compare(got, learner.loss_out.cpu().numpy(), g64, g32, l64, l32)
    assert net.actions[0] == 1 and all(np.abs(got[k][0]).max() > 0 for k in NAMES if k not in ('conv_w', 'conv_b'))
    assert np.abs(got['conv_w'][:64]).max() > 0
    learner.close()


def test_target_max_takes_the_signals_own_actions():
    lmax, T, N, B = 9, 6, 9, 96
    c = _case(lmax, T, N)
    idx = torch.from_numpy(_reference(lmax, T, N, B)[0]).cuda()
    rp = _device_ring(c)
    net, learner = _learner(c, B)
    clean = _np(learner.grad(rp, idx))
    loss = learner.loss_out.cpu().numpy().copy()
    with torch.no_grad():
        learner.target.fc3_w.masked_fill_(~learner.target.action_mask.unsqueeze(1), 1e30)
        learner.target.fc3_b.masked_fill_(~learner.target.action_mask, 1e30)
    assert (learner.target.fc3_w == 1e30).any()
    dirty = _np(learner.grad(rp, idx))
    for k in NAMES:
        assert clean[k].tobytes() == dirty[k].tobytes(), k
    assert loss.tobytes() == learner.loss_out.cpu().numpy().tobytes()
    learner.close()


@pytest.mark.parametrize('T,N,head,count', RING_STATES)
def test_sample_on_the_device(T, N, head, count):
    c = _case(2, 3, 5)
    net, learner = _learner(c, 33)
    rp = _sentinel_ring(T, N, 3, 2)               # (the draw reads nothing of it)
    rp.head, rp.count = head, count
    draws = []
    for u in (0, 1, 77):
        idx = learner.sample(rp, update_key=u).cpu().numpy()
        assert idx.shape == (33, 3, 2) and np.array_equal(idx, predict_sample(SEED, u, 3, T, N, head, count, 33))
        check_sample(idx, T, N, head, count)
        draws.append(idx)
    if T * N > 2:
        assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[1], draws[2])
    assert np.array_equal(learner.sample(rp).cpu().numpy(), draws[0]), 'the default key is the number of Adam steps so far'
    learner.close()


def test_adam_step():
    """Equal gradients into both sides, three steps against torch.optim.Adam(lr=1e-3); the yardstick of the PPO update's Adam test"""
    c = _case(9, 6, 9)
    g32 = _reference(9, 6, 9, 96)[2]
    g = {k: g32[k].astype(np.float32) for k in NAMES}
    net, learner = _learner(c, 96)
    for k in NAMES:
        learner.grads[k].copy_(torch.from_numpy(g[k]))
    st64 = st32 = None
    for t in (1, 2, 3):
        st64, st32 = torch_step(c['net'], g, st64, torch.float64), torch_step(c['net'], g, st32, torch.float32)
        learner.step()
        assert learner.n_updates == t
        mine = (_np(net), _np(learner.m), _np(learner.v))
        assert_adam_state(t, NAMES, mine, st64, st32)
    for k in NAMES:                                         # the gradients stay as they were loaded
        assert np.array_equal(learner.grads[k].cpu().numpy(), g[k])
    assert np.abs(_np(net)['fc2_w'] - c['net'].fc2_w.detach().numpy()).max() > 1e-4
    learner.close()


def test_update_is_the_loop_of_single_calls():
    """rs_dqn_update(n_updates = 3) against sample (keyed by the steps so far), grad, step, three times, from the same state"""
    c = _case(9, 6, 9)
    rp = _device_ring(c, head=4, pad=0)         # (the draws cover every environment of the ring: none is a sentinel)

    def run(fused):
        net, learner = _learner(c, 40)
        if fused:
            learner.update(rp, updates=3)
        else:
            for _ in range(3):
                learner.grad(rp, learner.sample(rp))
                learner.step()
        assert learner.n_updates == 3
        out = (_np(net), _np(learner.m), _np(learner.v), learner.loss_out.cpu().numpy().copy())
        learner.close()
        return out

    one, loop, again = run(True), run(False), run(True)
    for other in (loop, again):
        for a, b in zip(one[:3], other[:3]):
            for k in NAMES:
                assert a[k].tobytes() == b[k].tobytes(), k
        assert one[3].tobytes() == other[3].tobytes()
    assert all(np.isfinite(one[0][k]).all() for k in NAMES) and np.isfinite(one[3]).all()
    assert np.abs(one[0]['fc2_w'] - c['net'].fc2_w.detach().numpy()).max() > 1e-4


def test_learner_counts_and_syncs_as_the_torch_learner():
    """12 agent steps with target_update = 5 on a ring of 8 slots x 4 environments fed by hand, a BatchedDQNLearner counting next to it.
    PFRL's order: the target is copied BEFORE the step's update, so after steps 5 and 10 it holds, bit for bit, the parameters those
    steps began with; at step 11 it still does and differs from the parameters."""
    c = _case(9, 6, 9)
    net, learner = _learner(c, 6, target_update=5)
    twin = BatchedDQNLearner(_device_net(c['net']), target_update=5, batch_size=6)
    gen = torch.Generator(device='cuda').manual_seed(0)
    S, lmax = 3, 9
    rp = _sentinel_ring(8, 4, S, lmax)           # unwritten slots are unreadable; every environment is drawn from, so none is a sentinel
    f = lambda k, i: torch.from_numpy(c[k][i % 6, :4]).cuda()
    synced = None
    for step in range(1, 13):
        rp.push(f('obs', step), f('act', step), f('rew', step), step == 7)
        before = _np(net)
        out = learner.observe_step(rp, generator=gen)
        twin.observe_step(rp, gen)
        assert (out is None) == (len(rp) < 6)
        assert (learner.t, learner.n_updates) == (twin.t, twin.n_updates) == (step, max(0, step - 2))
        if step in (5, 10):
            synced = before
        if synced is not None:
            target = _np(learner.target)
            assert all(target[k].tobytes() == synced[k].tobytes() for k in NAMES), step
        if step == 11:
            now = _np(net)
            assert any(target[k].tobytes() != now[k].tobytes() for k in NAMES)
    assert all(np.isfinite(v).all() for v in _np(net).values())
    assert learner.observe_step(rp, updates=0) is None and (learner.t, learner.n_updates) == (13, 10)      # no update asked for: none made
    learner.close()


def test_one_update_against_the_torch_learner():
    """From the same state and the same explicit minibatch: one fused update and one BatchedDQNLearner.update agree within 4 x the
    distance of the float32 torch update from the float64 one"""
    lmax, T, N, B = 9, 6, 9, 96
    c = _case(lmax, T, N)
    idx = _reference(lmax, T, N, B)[0]
    p64 = torch_update(c, idx, torch.float64)
    net, learner = _learner(c, B)
    learner.grad(_device_ring(c), torch.from_numpy(idx).cuda())
    learner.step()
    fused = _np(net)
    twin = BatchedDQNLearner(_device_net(c['net']), batch_size=B)
    twin.target.load_state_dict(c['target'].state_dict())
    twin.update(tuple(x.cuda() for x in _batch(c, idx, torch.float32)))
    p32 = _np(twin.q)
    for k in NAMES:
        yard, err = np.abs(p32[k] - p64[k]).max(), np.abs(fused[k].astype(np.float64) - p32[k]).max()
        print('  %-7s |fused - torch32| %.3e  |torch32 - torch64| %.3e' % (k, err, yard))
        assert err <= 4 * yard, k
        assert np.abs(fused[k] - c['net'].state_dict()[k].numpy()).max() > 1e-4, k
    learner.close()


def test_refusals():
    """every RS_EINVAL of the header, with a message, and nothing launched"""
    c = _case(2, 3, 5)
    net, learner = _learner(c, 33)
    rp = _device_ring(c)
    L, h, st = load_library(), learner._h, torch_stream(0)
    idx = torch.from_numpy(_draw_idx(3, 5, 33)).cuda()
    p0 = _np(net)

    def ring(**kw):
        r = DQNRing(rp.obs.data_ptr(), rp.act.data_ptr(), rp.rew.data_ptr(), rp.done.data_ptr(), rp.T, rp.N, 0, rp.T)
        for k, v in kw.items():
            setattr(r, k, v)
        return C.byref(r)

    def refused(r, batch=33, word=b''):
        for rc in (L.rs_dqn_sample(h, r, batch, SEED, 0, idx.data_ptr(), st), L.rs_dqn_grad(h, r, idx.data_ptr(), batch, None, st),
                   L.rs_dqn_update(h, r, batch, SEED, 1, None, st)):
            assert rc == RS_EINVAL and word in L.rs_last_error(None)

    refused(ring(), 0, b'max_batch')
    refused(ring(), 34, b'max_batch')
    refused(ring(count=1), word=b'count >= 2')
    refused(ring(count=0))
    refused(ring(capacity=1, count=1), word=b'capacity >= 2')
    refused(ring(n_envs=0))
    refused(ring(head=-1), word=b'outside the ring')
    refused(ring(head=3), word=b'outside the ring')
    refused(ring(count=4), word=b'outside the ring')
    refused(ring(obs=None), word=b'NULL')
    refused(None, word=b'NULL')
    assert L.rs_dqn_sample(None, ring(), 33, SEED, 0, idx.data_ptr(), st) == RS_EINVAL
    assert L.rs_dqn_sample(h, ring(), 33, SEED, 0, None, st) == RS_EINVAL
    assert L.rs_dqn_grad(h, ring(), None, 33, None, st) == RS_EINVAL
    assert L.rs_dqn_update(h, ring(), 33, SEED, 0, None, st) == RS_EINVAL
    assert L.rs_dqn_step(None, st) == RS_EINVAL and L.rs_dqn_steps(None) == -1
    host = np.zeros((33, 3, 2), np.int32)               # memory the runtime does not know as the handle's device's: index arrays, a ring array
    assert L.rs_dqn_sample(h, ring(), 33, SEED, 0, host.ctypes.data, st) == RS_EINVAL and b'not device memory' in L.rs_last_error(None)
    assert L.rs_dqn_grad(h, ring(), host.ctypes.data, 33, None, st) == RS_EINVAL and b'not device memory' in L.rs_last_error(None)
    host_rew = np.zeros((rp.T, rp.N, 3), np.float32)
    refused(ring(rew=host_rew.ctypes.data), word=b'not device memory')
    if torch.cuda.device_count() > 1:       # the handle lives on device 0, this ring on device 1
        other = DeviceReplay(rp.T, rp.N, 3, 2, device='cuda:1')
        r = DQNRing(other.obs.data_ptr(), other.act.data_ptr(), other.rew.data_ptr(), other.done.data_ptr(), rp.T, rp.N, 0, rp.T)
        refused(C.byref(r), word=b'not device memory')

    # rs_dqn_create
    sets = [DQNTensors(*[getattr(n, k).data_ptr() for k in NAMES]) for n in (net, learner.target)]
    sets += [DQNTensors(*[d[k].data_ptr() for k in NAMES]) for d in (learner.grads, learner.m, learner.v)]
    cfg = DQNConfig(1e-3, 1e-8, 0.9, 0.999, 0.99)

    def create(device=0, lmax=2, lanes=(2, 2, 2), actions=(1, 3, 8), amax=8, max_batch=33, drop=None):
        out = C.c_void_p()
        refs = [C.byref(t) if i != drop else None for i, t in enumerate(sets)]
        rc = L.rs_dqn_create(device, 3, lmax, (C.c_int32 * 3)(*lanes), (C.c_int32 * 3)(*actions), amax, C.byref(cfg), *refs, max_batch, C.byref(out))
        if rc == 0:
            L.rs_dqn_destroy(out)
        else:
            assert out.value is None
        return rc

    assert create() == 0
    for bad in (dict(lmax=1), dict(lmax=18), dict(amax=0, actions=(0, 0, 0)), dict(amax=9), dict(lanes=(1, 2, 2)), dict(lanes=(2, 3, 2)),
                dict(actions=(0, 3, 8)), dict(actions=(1, 3, 8), amax=7), dict(max_batch=0), dict(drop=1), dict(device=-1),
                dict(device=torch.cuda.device_count())):
        assert create(**bad) == RS_EINVAL, bad
        assert L.rs_last_error(None).startswith(b'rs_dqn_create')
    with pytest.raises(RuntimeError, match=r'rs_dqn_grad failed \(-1\).*max_batch'):
        learner.grad(rp, torch.from_numpy(_draw_idx(3, 5, 40)).cuda())
    p1 = _np(net)
    assert all(p0[k].tobytes() == p1[k].tobytes() for k in NAMES) and learner.n_updates == 0
    learner.close()


def test_training_tool_with_the_fused_learner(monkeypatch):
    from tools import idqn_train
    made = []

    class Recorded(FusedDQNLearner):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(idqn_train, 'FusedDQNLearner', Recorded)
    monkeypatch.setattr(BatchedDQNLearner, 'capture_update', lambda *a, **kw: pytest.fail('the device update captures no graph'))
    rows, final = idqn_train.main('cologne1', 16, 1, 32, device_update=True, evaluate=False, quiet=True)
    assert len(made) == 1 and made[0]._h is None, 'the tool closes its learner'
    params = _np(made[0].net)
    assert all(np.isfinite(params[k]).all() for k in NAMES) and np.isfinite(rows[-1]['mean_return'])
    monkeypatch.undo()
    torch_rows, _ = idqn_train.main('cologne1', 16, 1, 32, use_graph=False, evaluate=False, quiet=True)
    assert rows[-1]['updates'] == torch_rows[-1]['updates'] > 0
