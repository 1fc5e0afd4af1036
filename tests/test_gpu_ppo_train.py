"""GPU: the PPO update on the device (rs_ppo_grad / rs_ppo_step / rs_ppo_fit, resco_amd/csrc/resco_ppo_train.h; FusedPPOLearner).
The chain: a minibatch gradient against float64 autograd of BatchedPPOLearner.loss; clip + Adam against torch from equal gradients;
rs_ppo_fit against the loop of the two, bit for bit; then a recorded segment and the training tool end to end.  Yardstick
(tests/ppo_train_ref.py): truth = torch in float64, e_ref = torch in float32 against it, the device gets 4 e_ref per tensor."""
import copy
import functools
import json

import numpy as np
import pytest
import torch

from conftest import load_scenario
from ppo_train_ref import NAMES, case, torch_grads, torch_step
from resco_amd.agents.ippo import BatchedIPPO
from resco_amd.agents.ippo_fused import DeviceRollout, FusedIPPO
from resco_amd.agents.ippo_learn_fused import FusedPPOLearner
from resco_amd.sim import BatchedSim, SimGroup, load_library, torch_stream
from train_ref import _device_net, _np, assert_adam_state, check_4_e_ref, compare_gradients

pytestmark = pytest.mark.gpu

RS_EINVAL = -1
PAD_ROWS = 3


@functools.lru_cache(maxsize=None)
def _case(lmax, n):
    return case(lmax, n, seed=lmax)


@functools.lru_cache(maxsize=None)
def _reference(lmax, n, B):
    """(idx, truth gradients, float32 gradients, truth loss terms, float32 loss terms): computed once, shared, never changed"""
    c = _case(lmax, n)
    idx = np.random.default_rng(B).permutation(n)[:B]
    g64, l64 = torch_grads(c, idx, torch.float64)
    g32, l32 = torch_grads(c, idx, torch.float32)
    return idx, g64, g32, l64, l32


def _device_dataset(c, pad=PAD_ROWS):
    """the case's rows followed by `pad` sentinel rows (NaN, action -777) that no kernel may read"""
    S, lmax = c['obs'].shape[1], c['obs'].shape[2]
    f = lambda k: torch.cat([torch.from_numpy(c[k]), torch.full((pad, S), float('nan'))]).cuda()
    return dict(obs=torch.cat([torch.from_numpy(c['obs']), torch.full((pad, S, lmax, 5), float('nan'), dtype=torch.float16)]).cuda(),
                act=torch.cat([torch.from_numpy(c['act']), torch.full((pad, S), -777, dtype=torch.int32)]).cuda(),
                logp=f('logp'), adv=f('adv'), ret=f('ret'))


@pytest.mark.parametrize('lmax,n,B', [(2, 40, 33), (9, 130, 96), (17, 100, 70), (5, 1100, 1050)])
def test_minibatch_gradient(lmax, n, B):
    """B below and across a 64-row tile, every lane count 2 .. 17; B = 1050 = 17 tiles in 3 chunks of the fc1 backward (PPT_CH = 512
    rows), the last of 64 rows with 38 real ones: the chunk offsets and the chunk sums of the reduction, which every real minibatch
    (1920, 7680 rows) goes through"""
    c = _case(lmax, n)
    idx, g64, g32, l64, l32 = _reference(lmax, n, B)
    net = _device_net(c['net'])
    learner = FusedPPOLearner(net, minibatch=B)
    ds = _device_dataset(c)
    idx_t = torch.from_numpy(idx).cuda()
    got = _np(learner.grad(ds, idx_t))
    loss = learner.loss_out.cpu().numpy().copy()
    print('lmax %d n %d B %d: %.0f %% of the samples clipped' % (lmax, n, B, 100 * c['clipped_fraction']))
    worst = compare_gradients(NAMES, got, g64, g32)
    for q, name in enumerate(('policy', 'value', 'entropy')):
        check_4_e_ref('loss ' + name, loss[:, q], l64[:, q], l32[:, q], worst)
    assert not worst, worst
    # padded fc1 rows and fc3 columns: exactly zero
    pad1 = c['net'].fc1_mask.numpy() == 0
    assert (got['fc1_w'][np.broadcast_to(pad1, got['fc1_w'].shape)] == 0).all()
    amask = c['net'].action_mask.numpy()
    assert (got['fc3_b'][~amask] == 0).all() and (got['fc3_w'][np.broadcast_to(~amask[:, None, :], got['fc3_w'].shape)] == 0).all()
    assert all(np.abs(got[k]).max() > 0 for k in NAMES)
    # the same bits again
    again = _np(learner.grad(ds, idx_t))
    for k in NAMES:
        assert got[k].tobytes() == again[k].tobytes(), k
    assert loss.tobytes() == learner.loss_out.cpu().numpy().tobytes()
    learner.close()


@pytest.mark.parametrize('gscale', [1.0, 100.0, 0.01])
def test_clip_and_adam_step(gscale):
    """Equal gradients into both sides, three steps: as they are, x 100 (the clip binds on every signal) and x 0.01 (it binds on
    none: on this case the per-signal norms are 0.7 .. 2.5, so that the gradients as they are already bind on every signal)."""
    c = _case(9, 130)
    _, _, g32, _, _ = _reference(9, 130, 96)
    g = {k: (gscale * g32[k]).astype(np.float32) for k in NAMES}
    net = _device_net(c['net'])
    learner = FusedPPOLearner(net, minibatch=96)
    for k in NAMES:
        learner.grads[k].copy_(torch.from_numpy(g[k]))
    st64 = st32 = None
    for t in (1, 2, 3):
        st64, st32 = torch_step(c['net'], g, st64, torch.float64), torch_step(c['net'], g, st32, torch.float32)
        assert ((st64['scale'] < 1.0) == (gscale >= 1.0)).all(), st64['scale']
        learner.step()
        assert learner.n_updates == t
        mine = (_np({k: getattr(net, k) for k in NAMES}), _np(learner.m), _np(learner.v))
        assert_adam_state(t, NAMES, mine, st64, st32)
    for k in NAMES:                                         # the gradients stay as they were loaded
        assert np.array_equal(learner.grads[k].cpu().numpy(), g[k])
    learner.close()


@pytest.mark.parametrize('lmax,n,mb,epochs,steps', [(9, 130, 64, 2, 6), (5, 1100, 600, 1, 2)])
def test_fit_is_the_loop_of_single_calls(lmax, n, mb, epochs, steps):
    """130 rows in minibatches of 64, 64 and 2, two epochs; 1100 rows in minibatches of 600 and 500 (two chunks of the fc1 backward each)"""
    c = _case(lmax, n)
    ds = _device_dataset(c, pad=0)
    perm = torch.stack([torch.randperm(n, generator=torch.Generator().manual_seed(e)) for e in range(epochs)]).cuda()

    def run(fit):
        net = _device_net(c['net'])
        learner = FusedPPOLearner(net, minibatch=mb, epochs=epochs)
        if fit:
            learner.fit(ds, perm)
        else:
            for e in range(epochs):
                for i in range(0, n, mb):
                    learner.grad(ds, perm[e, i:i + mb])
                    learner.step()
        out = (_np({k: getattr(net, k) for k in NAMES}), _np(learner.m), _np(learner.v), learner.loss_out.cpu().numpy().copy())
        assert learner.n_updates == steps
        return net, learner, out

    net, learner, fit1 = run(True)
    _, l2, loop = run(False)
    _, l3, fit2 = run(True)                                  # again from the restored state: a fresh copy of the same parameters
    for other in (loop, fit2):
        for a, b in zip(fit1[:3], other[:3]):
            for k in NAMES:
                assert a[k].tobytes() == b[k].tobytes(), k
        assert fit1[3].tobytes() == other[3].tobytes()
    assert all(np.isfinite(fit1[0][k]).all() for k in NAMES)
    assert np.abs(fit1[0]['fc2_w'] - c['net'].fc2_w.detach().numpy()).max() > 1e-4
    # the net stays the source of truth: the device re-pack of the updated parameters gives the bits of the host pack
    fused = FusedIPPO(net, seed=1)
    obs = ds['obs'][:100].contiguous()
    fused.refresh_on_device()
    dev = [t.cpu().numpy().copy() for t in fused.act(obs, step_key=5, want_logits=True)]
    fused.refresh()
    host = [t.cpu().numpy().copy() for t in fused.act(obs, step_key=5, want_logits=True)]
    for d, h in zip(dev, host):
        assert d.tobytes() == h.tobytes()
    fused.close()
    for l in (learner, l2, l3):
        l.close()


def test_update_from_recorded_segment():
    """cologne8, 64 environments, T = 8 through rs_group_rollout; then the refusals"""
    sc = load_scenario('cologne8')
    n, T = 64, 8
    sim = BatchedSim(sc, n, seed=4)
    grp = SimGroup([sim])
    grp.step('random', step_key=0, n_steps=20)
    net = BatchedIPPO.from_scenario(sc, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=5)
    with torch.no_grad():
        net.fc3_w.mul_(30.0)
        net.v_b.add_(0.5)
    pol = FusedIPPO(net, seed=9)
    rec = DeviceRollout(T, [sim])
    grp.rollout(rec, pol.handle, t0=0, n_steps=T, step_key=0, seed=9)
    grp.sync()
    last_value = pol.value(sim.tensor('drq_norm_f16'))
    done = torch.zeros(T, dtype=torch.bool, device='cuda')
    done[T // 2] = True
    p0 = _np({k: getattr(net, k) for k in NAMES})

    # one epoch of one minibatch: the update's gradient is grad() of the same rows
    nets = [copy.deepcopy(net) for _ in range(2)]
    one = FusedPPOLearner(nets[0], minibatch=T * n, epochs=1)
    one.update_from_rollout(rec, last_value, done, generator=torch.Generator(device='cuda').manual_seed(0))
    ref = FusedPPOLearner(nets[1], minibatch=T * n, epochs=1)
    idx = torch.randperm(T * n, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0))
    ref.grad(ref._dataset_from_rollout(rec, last_value, done), idx)
    ga, gb = _np(one.grads), _np(ref.grads)
    for k in NAMES:
        assert ga[k].tobytes() == gb[k].tobytes() and np.abs(ga[k]).max() > 0, k
    assert one.n_updates == 1 and ref.n_updates == 0

    # the whole update with the default settings: 4 epochs x 2 minibatches of 256
    learner = FusedPPOLearner(net)
    loss = learner.update_from_rollout(rec, last_value, done, generator=torch.Generator(device='cuda').manual_seed(0))
    assert learner.n_updates == 8 and torch.isfinite(loss).item()
    p1 = _np({k: getattr(net, k) for k in NAMES})
    assert all(np.isfinite(p1[k]).all() for k in NAMES)
    moved = max(np.abs(p1[k] - p0[k]).max() for k in NAMES)
    print('parameters moved by up to %.3e in 8 Adam steps' % moved)
    assert moved > 1e-4
    assert all(np.isfinite(x[k]).all() for x in (_np(learner.m), _np(learner.v)) for k in NAMES)

    # ---- refusals: RS_EINVAL with a message, nothing launched
    L = load_library()
    ds, _ = learner._device_dataset(learner._dataset_from_rollout(rec, last_value, done))
    idx32 = idx.to(torch.int32)
    args = [ds[k].data_ptr() for k in ('obs', 'act', 'logp', 'adv', 'ret')]
    st = torch_stream(0)
    assert L.rs_ppo_grad(learner._h, *args, idx32.data_ptr(), 257, None, st) == RS_EINVAL
    assert b'max_minibatch' in L.rs_last_error(None)
    assert L.rs_ppo_grad(learner._h, *args, idx32.data_ptr(), 0, None, st) == RS_EINVAL
    assert L.rs_ppo_grad(learner._h, *args, None, 16, None, st) == RS_EINVAL
    assert b'NULL' in L.rs_last_error(None)
    assert L.rs_ppo_grad(learner._h, None, *args[1:], idx32.data_ptr(), 16, None, st) == RS_EINVAL
    assert L.rs_ppo_grad(None, *args, idx32.data_ptr(), 16, None, st) == RS_EINVAL
    assert L.rs_ppo_fit(learner._h, *args, T * n, idx32.data_ptr(), 1, 257, None, st) == RS_EINVAL
    assert L.rs_ppo_fit(learner._h, *args, T * n, None, 1, 256, None, st) == RS_EINVAL
    assert L.rs_ppo_step(None, st) == RS_EINVAL
    torch.cuda.synchronize()
    p2 = _np({k: getattr(net, k) for k in NAMES})
    assert all(p1[k].tobytes() == p2[k].tobytes() for k in NAMES) and learner.n_updates == 8
    with pytest.raises(RuntimeError, match=r'rs_ppo_grad failed \(-1\).*max_minibatch'):
        learner.grad(ds, idx[:300])
    for l in (one, ref, learner):
        l.close()
    pol.close()
    sim.close()


def test_training_tool_with_the_fused_learner(capsys):
    from tools import ippo_train
    ippo_train.main_device_rollout('cologne1', 64, 1, 30, 4, device_update=True)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')]
    out = json.loads(lines[-1])
    assert len(lines) == 1 and np.isfinite(out['avg_delay_s']) and out['adam_steps'] > 0
