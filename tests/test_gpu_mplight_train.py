"""GPU: MPLight's shared-DQN update on the device (rs_mplight_dqn_sample / _grad / _step / _update, resco_amd/csrc/resco_frap_train.h;
FusedMPLightLearner).  The chain: a minibatch gradient against float64 autograd of MPLightLearner.loss; the ring's semantics (wrap,
episode ends, clamped actions); the target's max over all P outputs; the draw against the counter hash; Adam against torch from equal
gradients; rs_mplight_dqn_update against the loop of the three, bit for bit; one update against MPLightLearner.update; the views
(state_dict, load_state_dict, the policy bound by share_weights, the target's bookkeeping); the refusals; the training tool end to end.
Yardstick (tests/frap_train_ref.py): truth = torch in float64, e_ref = the largest distance of a family of float32 evaluations from it,
floored at one ulp32 of the tensor's largest element; the device gets 4 e_ref per tensor.

Every ring is an MPLightReplay with three sentinel environments past the case's N and one sentinel signal past its S; they and every
slot a test declares unreadable hold NaN observations, action -777 and NaN rewards: one of them read, and a gradient is NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import frap_train_ref as ft
from dqn_train_ref import RING_STATES
from resco_amd.agents.mplight import FRAP, FusedMPLight, MPLightLearner, MPLightReplay, pack_mplight_weights
from resco_amd.agents.mplight_learn_fused import FusedMPLightLearner
from resco_amd.sim import DQNConfig, MPLightRing, load_library, torch_stream
from train_ref import _np, assert_adam_state

pytestmark = pytest.mark.gpu

RS_EINVAL = -1
PAD_ENVS, PAD_SIGNALS = 3, 1
SEED = 0x5EED
MID = (5, 4, 5, 6, 3)       # (P, D, T, N, S) of the case most tests share


def _device_net(net):
    m = FRAP(net.oshape, net.phase_pairs, net.demand_shape)
    m.load_state_dict(net.state_dict())
    return m.cuda()


def _learner(c, B, n_signals=None, **kw):
    """a FusedMPLightLearner on a device copy of the case's network, its target the case's"""
    net = _device_net(c['net'])
    learner = FusedMPLightLearner(net, batch_size=B, seed=SEED, n_signals=n_signals, **kw)
    learner.target.load_state_dict(c['target'].state_dict())
    return net, learner


def _sentinel_ring(T, N, S, W):
    """an empty MPLightReplay whose every slot holds what must not be read: NaN observations, action -777, NaN rewards"""
    rp = MPLightReplay(T, N, S, W, device='cuda')
    rp.obs.fill_(float('nan'))
    rp.act.fill_(-777)
    rp.rew.fill_(float('nan'))
    return rp


def _device_ring(c, unreadable=(), head=0, count=None, pad=(PAD_ENVS, PAD_SIGNALS), act=None):
    """the case's ring on the device with sentinel environments and a sentinel signal; `unreadable`: slots that hold sentinels everywhere"""
    T, N, S, W = c['obs'].shape
    rp = _sentinel_ring(T, N + pad[0], S + pad[1], W)
    keep = [t for t in range(T) if t not in unreadable]
    rp.obs[keep, :N, :S] = torch.from_numpy(c['obs'][keep]).cuda()
    rp.act[keep, :N, :S] = torch.from_numpy((c['act'] if act is None else act)[keep]).cuda()
    rp.rew[keep, :N, :S] = torch.from_numpy(c['rew'][keep]).cuda()
    rp.done.copy_(torch.from_numpy(c['done']))
    rp.head, rp.count = head, T if count is None else count
    return rp


def _grads_np(learner):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in learner.grads.items()}


def _loss_np(learner):
    return learner.loss_out.detach().cpu().numpy().copy()


@pytest.mark.parametrize('P,D,T,N,S,B', ft.GPU_CASES)
def test_minibatch_gradient(P, D, T, N, S, B):
    """P: both ends and the three lane-group widths of the forward (4, 8, 16 lanes).  B, with tiles of ft.TILE_ROWS = 4 rows: 1; 3, below
    one tile; 5, across a tile boundary; 11 = two whole tiles and a ragged third of 3 rows; 70 and 45: 18 and 12 tiles' partials, the last
    of 2 rows and of 1.  The Huber branches are asserted on the truth where the batch has rows enough for a share to mean something."""
    c = ft.case(P, D, T, N, S)
    idx, g64, e_ref, l64, e_loss, _, d64 = ft.reference(P, D, T, N, S, B)
    if B >= 10:
        assert 0.2 <= ft.huber_fraction(d64) <= 0.8, 'both branches of the Huber loss must be well populated'
    net, learner = _learner(c, B)
    rp = _device_ring(c)
    idx_t = torch.from_numpy(idx).cuda()
    learner.grad(rp, idx_t)
    got, loss = _grads_np(learner), _loss_np(learner)
    print('P %d D %d ring %d x %d x %d, B %d' % (P, D, T, N, S, B))
    worst = ft.compare(ft.names_of(net), got, loss, g64, e_ref, l64, e_loss)
    assert not worst, worst
    learner.grad(rp, idx_t)                                 # the same bits again
    again = _grads_np(learner)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    assert loss.tobytes() == _loss_np(learner).tobytes()
    learner.close()


def test_every_tensor_has_gradient_in_some_case():
    """(on the truth alone) each of the 14 tensors has a non-zero truth gradient in at least one case of test_minibatch_gradient"""
    alive = set()
    for case in ft.GPU_CASES:
        g64 = ft.reference(*case)[1]
        alive |= {k for k, v in g64.items() if np.abs(v).max() > 0}
    assert alive == set(ft.names_of(ft.case(*MID)['net']))


def test_ring_semantics():
    """Rows of the last slot (their successor is slot 0), rows of slot 1, which ended an episode -- slot 2 behind it is unreadable in
    every environment, so a bootstrap that is multiplied by zero instead of cut gives NaN -- and actions outside 0 .. P - 1, clamped"""
    P, D, T, N, S = MID
    B = 40
    c = ft.case(P, D, T, N, S)
    assert c['done'][1] and not c['done'][T - 1]
    idx, g64, e_ref, l64, e_loss, _, _ = ft.reference(P, D, T, N, S, B, slots=(0, 1, 3, T - 1))
    assert (idx[:, 0] == T - 1).sum() > 3 and (idx[:, 0] == 1).sum() > 3
    act = c['act'].copy()
    a = act[idx[:, 0], idx[:, 1], idx[:, 2]]
    hi, lo = idx[a == P - 1], idx[a == 0]
    assert len(hi) and len(lo)
    act[tuple(hi[0])], act[tuple(lo[0])] = P + 3, -2
    net, learner = _learner(c, B)
    learner.grad(_device_ring(c, unreadable=(2,), act=act), torch.from_numpy(idx).cuda())
    worst = ft.compare(ft.names_of(net), _grads_np(learner), _loss_np(learner), g64, e_ref, l64, e_loss)
    assert not worst, worst
    learner.close()


def test_target_max_runs_over_all_pairs():
    """The learner takes no valid table at all.  Against the truth whose max is over all P the device is inside the bound; the truth of
    a learner that restricted the max to each signal's valid pairs is a different one, by far more than the bound"""
    P, D, T, N, S = 13, 1, 8, 11, 4
    B = 70
    c = ft.case(P, D, T, N, S)
    idx, g64, e_ref, l64, e_loss, _, d64 = ft.reference(P, D, T, N, S, B)
    m64, ml64, md64 = ft.torch_grads(c, idx, torch.float64, masked=True)
    assert (np.abs(md64 - d64) > 1e-3).mean() > 0.2, 'the valid lists would pick another maximum on a good share of the rows'
    assert abs(ml64 - l64) > 100 * e_loss and np.abs(m64['hidden_layer.weight'] - g64['hidden_layer.weight']).max() > 100 * e_ref['hidden_layer.weight']
    net, learner = _learner(c, B)
    learner.grad(_device_ring(c), torch.from_numpy(idx).cuda())
    worst = ft.compare(ft.names_of(net), _grads_np(learner), _loss_np(learner), g64, e_ref, l64, e_loss)
    assert not worst, worst
    learner.close()


@pytest.mark.parametrize('T,N,head,count', RING_STATES)
def test_sample_on_the_device(T, N, head, count):
    c = ft.case(2, 1, 3, 4, 2)
    S = 3
    net, learner = _learner(c, 33)
    rp = _sentinel_ring(T, N, S, 13)              # (the draw reads nothing of it)
    rp.head, rp.count = head, count
    draws = []
    for u in (0, 1, 77):
        idx = learner.sample(rp, update_key=u).cpu().numpy()
        assert idx.shape == (33, 3) and np.array_equal(idx, ft.predict_sample(SEED, u, T, N, S, head, count, 33))
        ft.check_sample(idx, T, N, S, head, count)
        draws.append(idx)
    assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[1], draws[2])
    assert np.array_equal(learner.sample(rp).cpu().numpy(), draws[0]), 'the default key is the number of Adam steps so far'
    learner.close()


def test_adam_step():
    """Equal gradients into both sides, three steps against torch.optim.Adam(lr=1e-3) in float64 and float32"""
    P, D, T, N, S = MID
    c = ft.case(P, D, T, N, S)
    family = ft.reference(P, D, T, N, S, 40)[5]
    g = {k: v.astype(np.float32) for k, v in family[0][1].items()}
    net, learner = _learner(c, 40, n_signals=S)
    names = ft.names_of(net)
    for k in names:
        learner.grads[k].copy_(torch.from_numpy(g[k]))
    st64 = st32 = None
    anames = [ft.adam_name(k) for k in names]
    rename = lambda d: {ft.adam_name(k): v for k, v in d.items()}
    for t in (1, 2, 3):
        st64, st32 = ft.adam_step(c['net'], g, st64, torch.float64), ft.adam_step(c['net'], g, st32, torch.float32)
        learner.step()
        assert learner.n_updates == t
        mine = (rename(_np(net)), rename(_np(learner.m)), rename(_np(learner.v)))
        assert_adam_state(t, anames, mine, st64, st32)
    for k in names:                                         # the gradients stay as they were loaded
        assert np.array_equal(learner.grads[k].cpu().numpy(), g[k])
    assert np.abs(_np(net)['hidden_layer.weight'] - c['net'].state_dict()['hidden_layer.weight'].numpy()).max() > 1e-4
    learner.close()


def test_update_is_the_loop_of_single_calls():
    """rs_mplight_dqn_update(n_updates = 3) against sample (keyed by the steps so far), grad, step, three times, from the same state"""
    c = ft.case(*MID)
    rp = _device_ring(c, head=3, pad=(0, 0))        # (the draws cover every environment and signal of the ring: none is a sentinel)

    def run(fused):
        net, learner = _learner(c, 21)
        if fused:
            learner.update(rp, updates=3)
        else:
            for _ in range(3):
                learner.grad(rp, learner.sample(rp))
                learner.step()
        assert learner.n_updates == 3
        torch.cuda.synchronize()
        out = (learner.flat.cpu().numpy().copy(), learner._m.cpu().numpy().copy(), learner._v.cpu().numpy().copy(), _loss_np(learner))
        learner.close()
        return out

    one, loop, again = run(True), run(False), run(True)
    for other in (loop, again):
        for a, b in zip(one, other):
            assert a.tobytes() == b.tobytes()
    assert all(np.isfinite(a).all() for a in one)
    assert np.abs(one[0] - pack_mplight_weights(c['net']).numpy()).max() > 1e-4


def test_one_update_against_the_torch_learner():
    """From the same state and the same explicit minibatch: one fused update and one MPLightLearner.update agree within 4 x the
    distance of the float32 torch update from the float64 one, per tensor; every tensor moved"""
    P, D, T, N, S = MID
    B = 40
    c = ft.case(P, D, T, N, S)
    idx, g64 = ft.reference(P, D, T, N, S, B)[:2]
    p64 = {k: v.detach().double().numpy() for k, v in ft.adam_step(c['net'], g64, None, torch.float64)['net'].named_parameters()}
    net, learner = _learner(c, B)
    learner.grad(_device_ring(c), torch.from_numpy(idx).cuda())
    learner.step()
    fused = _np(net)
    twin = MPLightLearner(_device_net(c['net']), batch_size=B)
    twin.target.load_state_dict(c['target'].state_dict())
    twin.update(tuple(x.cuda() for x in ft.batch_of(c, idx, torch.float32)))
    p32 = _np(twin.q)
    for k in ft.names_of(net):
        yard = np.abs(p32[k] - p64[ft.adam_name(k)]).max()
        err = np.abs(fused[k].astype(np.float64) - p32[k]).max()
        print('  %-28s |fused - torch32| %.3e  |torch32 - torch64| %.3e' % (k, err, yard))
        assert err <= 4 * yard, k
        assert np.abs(fused[k] - c['net'].state_dict()[k].numpy()).max() > 1e-4, k
    learner.close()


def test_views_policy_and_target_bookkeeping():
    """After an update net.state_dict() is the flat vector; load_state_dict writes through to it; a policy bound by share_weights gives
    the bytes of a policy freshly created from the updated weights; then 12 env-steps with target_update = 5, an MPLightLearner
    counting next to it: the target is copied BEFORE the step's update."""
    P, D, T, N, S = MID
    c = ft.case(P, D, T, N, S)
    net, learner = _learner(c, 21, target_update=5)
    rp = _device_ring(c, head=3, pad=(0, 0))
    policy = FusedMPLight(net, c['sc'], seed=3)
    policy.share_weights(learner.flat)
    obs = torch.from_numpy(c['obs'][0]).cuda().contiguous()
    q_before = policy.act(obs, want_q=True)[1].cpu().numpy()
    learner.update(rp, updates=2)
    torch.cuda.synchronize()
    flat = learner.flat.cpu().numpy()
    assert np.array_equal(pack_mplight_weights(net).cpu().numpy(), flat) and not np.array_equal(flat, pack_mplight_weights(c['net']).numpy())
    q_shared = policy.act(obs, want_q=True)[1].cpu().numpy()
    fresh = FusedMPLight(net, c['sc'], seed=3)
    q_fresh = fresh.act(obs, want_q=True)[1].cpu().numpy()
    assert q_shared.tobytes() == q_fresh.tobytes() and not np.array_equal(q_shared, q_before)
    fresh.close()
    sd = {k: v + 0.25 for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    torch.cuda.synchronize()
    assert np.array_equal(learner.flat.cpu().numpy(), flat + np.float32(0.25))
    policy.refresh_on_device()                              # still works: packs the views into the shared vector itself
    assert policy._wdev is learner.flat
    policy.close()
    learner.close()

    net, learner = _learner(c, 6, target_update=5)
    twin = MPLightLearner(_device_net(c['net']), target_update=5, batch_size=6)
    W = c['obs'].shape[-1]
    rp = _sentinel_ring(8, 2, 1, W)              # unwritten slots are unreadable; every environment and signal is drawn from
    f = lambda k, i: torch.from_numpy(np.ascontiguousarray(c[k][i % T, :2, :1])).cuda()
    gen = torch.Generator(device='cuda').manual_seed(0)
    synced = None
    for step in range(1, 13):
        rp.push(f('obs', step), f('act', step), f('rew', step), step == 7)
        torch.cuda.synchronize()
        before = learner.flat.cpu().numpy().copy()
        out = learner.observe_step(rp, generator=gen)
        twin.observe_step(rp, gen)
        assert (out is None) == (len(rp) < 6)
        assert (learner.t, learner.n_updates) == (twin.t, twin.n_updates) == (step, max(0, step - 3))
        if step in (5, 10):
            synced = before
        torch.cuda.synchronize()
        if synced is not None:
            assert learner.flat_target.cpu().numpy().tobytes() == synced.tobytes(), step
            assert pack_mplight_weights(learner.target).cpu().numpy().tobytes() == synced.tobytes()
        if step == 11:
            assert learner.flat_target.cpu().numpy().tobytes() != learner.flat.cpu().numpy().tobytes()
    assert np.isfinite(learner.flat.cpu().numpy()).all()
    learner.close()


def test_refusals():
    """every RS_EINVAL of the header, with its word in the message; parameters and step count unchanged"""
    c = ft.case(2, 1, 3, 4, 2)
    T, N, S, W = c['obs'].shape
    net, learner = _learner(c, 33)
    rp = _device_ring(c, pad=(0, 0))
    idx = torch.from_numpy(ft.draw_idx(c, 33)).cuda()
    learner.sample(rp)                           # (creates the handle over the ring's S)
    torch.cuda.synchronize()
    L, h, st = load_library(), learner._h, torch_stream(0)
    p0 = learner.flat.cpu().numpy().copy()

    def ring(**kw):
        r = MPLightRing(rp.obs.data_ptr(), rp.act.data_ptr(), rp.rew.data_ptr(), rp.done.data_ptr(), T, N, S, W, 0, T)
        for k, v in kw.items():
            setattr(r, k, v)
        return C.byref(r)

    def refused(r, batch=33, word=b''):
        for rc in (L.rs_mplight_dqn_sample(h, r, batch, SEED, 0, idx.data_ptr(), st), L.rs_mplight_dqn_grad(h, r, idx.data_ptr(), batch, None, st),
                   L.rs_mplight_dqn_update(h, r, batch, SEED, 1, None, st)):
            assert rc == RS_EINVAL and word in L.rs_last_error(None), (rc, L.rs_last_error(None))

    refused(ring(), 0, b'max_batch')
    refused(ring(), 34, b'max_batch')
    refused(ring(count=1), word=b'count >= 2')
    refused(ring(count=0), word=b'count >= 2')
    refused(ring(capacity=1, count=1), word=b'capacity >= 2')
    refused(ring(n_envs=0), word=b'n_envs >= 1')
    refused(ring(n_signals=S + 1), word=b'n_signals')
    refused(ring(width=W + 1), word=b'width')
    refused(ring(width=49), word=b'width')
    refused(ring(head=-1), word=b'outside the ring')
    refused(ring(head=T), word=b'outside the ring')
    refused(ring(count=T + 1), word=b'outside the ring')
    refused(ring(obs=None), word=b'NULL')
    refused(ring(done=None), word=b'NULL')
    refused(None, word=b'NULL')
    assert L.rs_mplight_dqn_sample(None, ring(), 33, SEED, 0, idx.data_ptr(), st) == RS_EINVAL and b'NULL handle' in L.rs_last_error(None)
    assert L.rs_mplight_dqn_sample(h, ring(), 33, SEED, 0, None, st) == RS_EINVAL and b'NULL' in L.rs_last_error(None)
    assert L.rs_mplight_dqn_grad(h, ring(), None, 33, None, st) == RS_EINVAL and b'NULL' in L.rs_last_error(None)
    assert L.rs_mplight_dqn_update(h, ring(), 33, SEED, 0, None, st) == RS_EINVAL and b'n_updates' in L.rs_last_error(None)
    assert L.rs_mplight_dqn_step(None, st) == RS_EINVAL and L.rs_mplight_dqn_steps(None) == -1
    host = np.zeros((33, 3), np.int32)           # memory the runtime does not know as the handle's device's: index arrays, a ring array
    assert L.rs_mplight_dqn_sample(h, ring(), 33, SEED, 0, host.ctypes.data, st) == RS_EINVAL and b'not device memory' in L.rs_last_error(None)
    assert L.rs_mplight_dqn_grad(h, ring(), host.ctypes.data, 33, None, st) == RS_EINVAL and b'not device memory' in L.rs_last_error(None)
    host_rew = np.zeros((T, N, S), np.float32)
    refused(ring(rew=host_rew.ctypes.data), word=b'not device memory')

    # rs_mplight_dqn_create
    cfg = DQNConfig(1e-3, 1e-8, 0.9, 0.999, 0.99)
    vecs = [learner.flat, learner.flat_target, learner._g, learner._m, learner._v]

    def create(device=0, D=1, P=2, pairs=(0, 1, 2, 3), S=2, max_batch=33, drop=None, cfg_ref=C.byref(cfg)):
        out = C.c_void_p()
        ptrs = [v.data_ptr() if i != drop else None for i, v in enumerate(vecs)]
        rc = L.rs_mplight_dqn_create(device, D, P, (C.c_int32 * len(pairs))(*pairs) if pairs is not None else None, S, cfg_ref, *ptrs, max_batch, C.byref(out))
        if rc == 0:
            L.rs_mplight_dqn_destroy(out)
        else:
            assert out.value is None
        return rc

    assert create() == 0
    for bad in (dict(D=2), dict(D=0), dict(P=1), dict(P=17, pairs=tuple(range(12)) * 3), dict(pairs=(0, 1, 2, 12)), dict(pairs=(0, -1, 2, 3)),
                dict(pairs=None), dict(S=0), dict(max_batch=0), dict(drop=1), dict(drop=4), dict(cfg_ref=None), dict(device=-1),
                dict(device=torch.cuda.device_count())):
        assert create(**bad) == RS_EINVAL, bad
        assert L.rs_last_error(None).startswith(b'rs_mplight_dqn_create'), bad
    with pytest.raises(RuntimeError, match=r'rs_mplight_dqn_grad failed \(-1\).*max_batch'):
        learner.grad(rp, torch.from_numpy(ft.draw_idx(c, 40)).cuda())
    torch.cuda.synchronize()
    assert p0.tobytes() == learner.flat.cpu().numpy().tobytes() and learner.n_updates == 0
    learner.close()


def test_training_tool_with_the_fused_learner(monkeypatch):
    from tools import mplight_train
    made = []

    class Recorded(FusedMPLightLearner):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(mplight_train, 'FusedMPLightLearner', Recorded)
    rows, final = mplight_train.main('cologne1', 16, 1, 32, quiet=True, device_update=True)
    assert len(made) == 1 and made[0]._h is None, 'the tool closes its learner'
    torch.cuda.synchronize()
    assert np.isfinite(made[0].flat.cpu().numpy()).all() and np.isfinite(rows[-1]['mean_return'])
    assert np.array_equal(pack_mplight_weights(made[0].net).cpu().numpy(), made[0].flat.cpu().numpy())
    monkeypatch.undo()
    torch_rows, _ = mplight_train.main('cologne1', 16, 1, 32, quiet=True)
    assert rows[-1]['updates'] == torch_rows[-1]['updates'] > 0
