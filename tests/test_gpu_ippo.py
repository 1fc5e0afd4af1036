"""GPU: IPPO on the device.  The actor-critic launch of the fused forward (rs_ippo_act) against the rounding-faithful reference of
tests/idqn_kernel_ref.py and against rs_idqn_act mode 1; the value-only call; the rollout recorder of the group path
(rs_group_rollout) against a Python loop of single calls and against one handle with the whole batch; the fused GAE (rs_ppo_gae)
against the host build of the same header; BatchedPPOLearner.update_from_rollout against update()."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_scenario
from idqn_kernel_ref import QMAX, idqn_kernel_ref, make_net, random_obs
from ppo_ref import build_ppo_host, gae_case, gae_errors, host_gae, torch_gae
from resco_amd.agents.idqn_fused import _b_fragments, pack_idqn_weights
from resco_amd.agents.ippo import BatchedIPPO, BatchedPPOLearner
from resco_amd.agents.ippo_fused import DeviceRollout, FusedIPPO
from resco_amd.sim import BatchedSim, SimGroup, load_library, torch_stream

pytestmark = pytest.mark.gpu

RS_EINVAL = -1
ACT_SENTINEL, F_SENTINEL, PAD_ROWS = -777, 1234.5, 3


def _net(lmax, seed, fc3_scale=30.0):
    """make_net's BatchedIPPO with logits of O(1) (the fresh policy head gives ~1e-2) and a value bias that is not zero"""
    net, _ = make_net(lmax, seed=seed, cls=BatchedIPPO)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        net.fc3_w.mul_(fc3_scale)
        net.fc3_b.add_(0.2 * torch.randn(net.fc3_b.shape, generator=g) * net.action_mask)
        net.v_b.add_(torch.randn(net.v_b.shape, generator=g))
    return net.cuda()


def _ippo_act(fused, obs, n, step_key=0, env_base=0, value_only=False):
    """rs_ippo_act into buffers with PAD_ROWS sentinel rows after n_envs, which must stay untouched -> numpy act, logp, value, logits"""
    S = fused.S
    acts = torch.full((n + PAD_ROWS, S), ACT_SENTINEL, dtype=torch.int32, device='cuda')
    logp = torch.full((n + PAD_ROWS, S), F_SENTINEL, dtype=torch.float32, device='cuda')
    value = torch.full((n + PAD_ROWS, S), F_SENTINEL, dtype=torch.float32, device='cuda')
    logits = torch.full((n + PAD_ROWS, S, QMAX), F_SENTINEL, dtype=torch.float32, device='cuda')
    rc = fused._lib.rs_ippo_act(fused._h, obs.data_ptr(), n, env_base, fused.seed, step_key & 0xFFFFFFFF, None,
                                None if value_only else acts.data_ptr(), None if value_only else logp.data_ptr(), value.data_ptr(),
                                None if value_only else logits.data_ptr(), torch_stream(fused.device))
    assert rc == 0
    torch.cuda.synchronize()
    a, lp, v, lg = acts.cpu().numpy(), logp.cpu().numpy(), value.cpu().numpy(), logits.cpu().numpy()
    assert (a[n:] == ACT_SENTINEL).all() and (lp[n:] == F_SENTINEL).all() and (v[n:] == F_SENTINEL).all() and (lg[n:] == F_SENTINEL).all()
    if value_only:
        assert (a == ACT_SENTINEL).all() and (lp == F_SENTINEL).all() and (lg == F_SENTINEL).all()
    return a[:n], lp[:n], v[:n], lg[:n]


def _value_as_action_pack(net):
    """the pack of an IDQN whose ONE action per signal is the value head: what idqn_kernel_ref computes for its column 0 is what the
    kernel computes for column 8 (a column's dot product does not depend on the column of the tile it occupies)"""
    pk = dict(pack_idqn_weights(net))
    S = len(net.lanes)
    pk['w3'] = np.ascontiguousarray(_b_fragments(net.v_w.detach().float().cpu().numpy(), 8, 1)[:, :, 0])
    pk['b3'] = np.zeros((S, 32), np.float32)
    pk['b3'][:, 0] = net.v_b.detach().float().cpu().numpy()[:, 0]
    pk['n_actions'] = np.ones(S, np.int32)
    return pk


@pytest.mark.parametrize('lmax', [2, 9, 17])
@pytest.mark.parametrize('n', [1, 100])
def test_actor_critic_kernel(lmax, n):
    net = _net(lmax, seed=lmax * 11 + n)
    na = np.asarray(net.actions)
    obs = random_obs(net.lanes, lmax, n, np.random.default_rng(lmax + n))
    obs_t = torch.from_numpy(obs).cuda()
    fused = FusedIPPO(net, seed=4321 + n)
    key, base = 0x9E3779B9, 1000
    acts, logp, value, logits = _ippo_act(fused, obs_t, n, step_key=key, env_base=base)

    # logits: within the bound of the rounding-faithful reference, -inf beyond a signal's actions
    ref, bound = idqn_kernel_ref(pack_idqn_weights(net), net.lanes, obs, n)
    valid = np.broadcast_to(np.arange(QMAX)[None, None, :] < na[None, :, None], logits.shape)
    assert np.isneginf(logits[~valid]).all() and np.isfinite(logits[valid]).all()
    ratio = np.abs(logits[valid].astype(np.float64) - ref[valid]) / bound[valid]
    print('lmax %d n %d: logits max |x - ref| / bound = %.3f' % (lmax, n, ratio.max()))
    assert ratio.max() <= 1.0

    # value: within the bound of the same reference run on the value head as the single action of every signal
    vref, vbound = idqn_kernel_ref(_value_as_action_pack(net), net.lanes, obs, n)
    vratio = np.abs(value.astype(np.float64) - vref[:, :, 0]) / vbound[:, :, 0]
    print('lmax %d n %d: value max |v - ref| / bound = %.3f (median |v| %.2f)' % (lmax, n, vratio.max(), np.median(np.abs(vref[:, :, 0]))))
    assert np.isfinite(value).all() and vratio.max() <= 1.0

    # actions: bit-identical to rs_idqn_act mode 1 on the same policy, observations, seed, key and env_base
    a1 = torch.full((n, fused.S), ACT_SENTINEL, dtype=torch.int32, device='cuda')
    rc = fused._lib.rs_idqn_act(fused._h, obs_t.data_ptr(), n, base, 1, 0.0, fused.seed, key, None, a1.data_ptr(), None, torch_stream(0))
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(acts, a1.cpu().numpy())
    assert (acts >= 0).all() and (acts < na[None, :]).all()

    # log-probability of the drawn action: log_softmax (float64) of the device's own logits over the signal's actions
    lg64 = np.where(valid, logits.astype(np.float64), -np.inf)
    mx = lg64.max(-1, keepdims=True)
    lsm = lg64 - mx - np.log(np.exp(lg64 - mx).sum(-1, keepdims=True))
    want = np.take_along_axis(lsm, acts[..., None].astype(np.int64), -1)[..., 0]
    err = np.abs(logp.astype(np.float64) - want).max()
    print('lmax %d n %d: max |logp - log_softmax64(logits)[a]| = %.2e' % (lmax, n, err))
    assert err <= 1e-4
    assert (logp[:, na == 1] == 0.0).all()

    # the device re-pack carries the value column too: the same bits as the host pack of the changed weights
    g = torch.Generator(device='cuda').manual_seed(n)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g, device='cuda') * (p != 0))
    fused.refresh_on_device()
    dev = _ippo_act(fused, obs_t, n, step_key=key, env_base=base)
    fused.refresh()
    host = _ippo_act(fused, obs_t, n, step_key=key, env_base=base)
    for d, h in zip(dev, host):
        assert d.tobytes() == h.tobytes()
    assert not np.array_equal(dev[2], value)
    fused.close()


@pytest.mark.parametrize('lmax,n', [(9, 100), (17, 65)])
def test_value_only_call(lmax, n):
    """actions = logp = NULL: the same value bits as the full call, nothing else written; one of the two alone is refused"""
    net = _net(lmax, seed=lmax)
    obs_t = torch.from_numpy(random_obs(net.lanes, lmax, n, np.random.default_rng(7))).cuda()
    fused = FusedIPPO(net, seed=5)
    _, _, value, _ = _ippo_act(fused, obs_t, n, step_key=3)
    _, _, v_only, _ = _ippo_act(fused, obs_t, n, step_key=3, value_only=True)
    assert value.tobytes() == v_only.tobytes()
    assert fused.value(obs_t).cpu().numpy().tobytes() == value.tobytes()
    buf = torch.zeros(n, fused.S, dtype=torch.float32, device='cuda')
    L = fused._lib
    assert L.rs_ippo_act(fused._h, obs_t.data_ptr(), n, 0, 0, 0, None, buf.data_ptr(), None, buf.data_ptr(), None, torch_stream(0)) == RS_EINVAL
    assert L.rs_ippo_act(fused._h, obs_t.data_ptr(), n, 0, 0, 0, None, None, buf.data_ptr(), buf.data_ptr(), None, torch_stream(0)) == RS_EINVAL
    fused.close()


def _cologne8_policy(sc, seed=5):
    net = BatchedIPPO.from_scenario(sc, dtype=torch.float32, device='cuda')
    net.init_like_reference(seed=seed)
    with torch.no_grad():                       # a policy that is not uniform and a value that is not ~0
        net.fc3_w.mul_(30.0)
        net.v_b.add_(0.5)
    return net


def test_rollout_recorder():
    """cologne8, 2 pipes x 64 environments, 12 steps in calls of 5 + 7 through rs_group_rollout: every recorded tensor and the
    simulator state equal (i) a Python loop of FusedIPPO.act, copies and rs_step per pipe, (ii) ONE handle with the 128 environments
    through the same call.  Then the refusals."""
    sc = load_scenario('cologne8')
    n, T = 128, 12
    mk = lambda cnt, base: BatchedSim(sc, cnt, seed=4, env_base=base)
    net = _cologne8_policy(sc)
    pol = FusedIPPO(net, seed=9)
    pipes, solo, whole = [mk(n // 2, 0), mk(n // 2, n // 2)], [mk(n // 2, 0), mk(n // 2, n // 2)], [mk(n, 0)]
    groups = [SimGroup(pipes), SimGroup(solo), SimGroup(whole)]
    for g in groups:                            # traffic on the network before the policy takes over
        g.step('random', step_key=0, n_steps=20)
        g.sync()
    key0 = 77
    # (i) the Python loop, everything on torch's stream
    st = torch_stream(0)
    loop = DeviceRollout(T, solo)
    for k in range(T):
        for s_, seg in zip(solo, loop.pipes):
            obs = s_.tensor('drq_norm_f16')
            seg['obs'][k].copy_(obs)
            pol.act(obs, step_key=key0 + k, out=s_.tensor('actions'), logp=seg['logp'][k], value=seg['value'][k], env_base=s_.env_base)
            seg['act'][k].copy_(s_.tensor('actions'))
            s_.step(None, stream=st)
            seg['rew'][k].copy_(s_.tensor('wait_norm'))
    torch.cuda.synchronize()
    # the group path: 5 + 7 steps
    rec, rec_whole = DeviceRollout(T, pipes), DeviceRollout(T, whole)
    for g, r in ((groups[0], rec), (groups[2], rec_whole)):
        g.rollout(r, pol.handle, t0=0, n_steps=5, step_key=key0, seed=9)
        g.rollout(r, pol.handle, t0=5, n_steps=7, step_key=key0 + 5, seed=9)
        g.sync()
    for name in DeviceRollout.FIELDS:
        got = rec.cat(name).cpu().numpy()
        assert got.tobytes() == loop.cat(name).cpu().numpy().tobytes(), name
        assert got.tobytes() == rec_whole.cat(name).cpu().numpy().tobytes(), name
    assert rec.cat('obs').float().abs().sum() > 0 and (rec.cat('rew') != 0).any() and (rec.cat('logp') < 0).any()
    acts = rec.cat('act').cpu().numpy()
    assert len(np.unique(acts)) > 1 and (acts >= 0).all() and (acts < np.asarray(net.actions)[None, None, :]).all()
    for name in ('stats', 'veh_pos', 'veh_lane', 'phase', 'actions', 'drq_norm_f16', 'wait_norm'):
        a = np.concatenate([p.read(name) for p in pipes])
        np.testing.assert_array_equal(a, np.concatenate([p.read(name) for p in solo]), err_msg=name)
        np.testing.assert_array_equal(a, whole[0].read(name), err_msg=name)
    # the last recorded action is what RS_BUF_ACTIONS holds
    np.testing.assert_array_equal(acts[-1], np.concatenate([p.read('actions') for p in pipes]))

    # ---- refusals: RS_EINVAL with a message, nothing launched
    before = np.concatenate([p.read('stats') for p in pipes])
    grp = groups[0]
    with pytest.raises(RuntimeError, match=r'rs_group_rollout failed \(-1\).*exceeds the segment'):
        grp.rollout(rec, pol.handle, t0=6, n_steps=7, step_key=0, seed=9)
    pipes[1].set_outputs(['drq_norm'])
    with pytest.raises(RuntimeError, match=r'rs_group_rollout failed \(-1\).*RS_BUF_DRQ_NORM_F16'):
        grp.rollout(rec, pol.handle, t0=0, n_steps=1, step_key=0, seed=9)
    pipes[1].set_outputs(None)
    other = FusedIPPO(_net(17, seed=1), seed=9)          # a policy of another scenario (16 signals, lmax 17)
    with pytest.raises(RuntimeError, match=r'rs_group_rollout failed \(-1\).*built for this scenario'):
        grp.rollout(rec, other.handle, t0=0, n_steps=1, step_key=0, seed=9)
    with pytest.raises(RuntimeError, match=r'rs_group_step failed'):
        grp.step('ippo', policy=pol.handle)         # rs_group_step records nothing: the kind belongs to rs_group_rollout
    grp.sync()
    np.testing.assert_array_equal(before, np.concatenate([p.read('stats') for p in pipes]))
    other.close()

    # an MPLight handle is no actor-critic
    from resco_amd.agents.mplight import FusedMPLight, frap_from_scenario
    mp = FusedMPLight(frap_from_scenario(sc, 1).cuda(), sc, seed=1)
    obs = pipes[0].tensor('drq_norm_f16')
    v = torch.zeros(n // 2, pol.S, device='cuda')
    assert pol._lib.rs_ippo_act(mp.handle, obs.data_ptr(), n // 2, 0, 0, 0, None, None, None, v.data_ptr(), None, torch_stream(0)) == RS_EINVAL
    with pytest.raises(RuntimeError, match=r'rs_group_rollout failed \(-1\)'):
        grp.rollout(rec, mp.handle, t0=0, n_steps=1)
    pol.close()
    for s_ in pipes + solo + whole:
        s_.close()


def _device_gae(rew, val, last, done, gamma=0.99, lambd=0.95):
    T, N, S = rew.shape
    r, v, l = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rew, val, last))
    d8 = torch.from_numpy(done.astype(np.uint8)).cuda()
    adv, ret = torch.full_like(r, float('nan')), torch.full_like(r, float('nan'))
    scratch = torch.empty(N, S, dtype=torch.float32, device='cuda')
    rc = load_library().rs_ppo_gae(r.data_ptr(), v.data_ptr(), l.data_ptr(), d8.data_ptr(), T, N, S, gamma, lambd, adv.data_ptr(),
                                   ret.data_ptr(), scratch.data_ptr(), torch_stream(0))
    assert rc == 0
    torch.cuda.synchronize()
    return adv.cpu().numpy(), ret.cpu().numpy()


@pytest.mark.parametrize('T,N,S', [(32, 48, 5), (30, 1000, 21), (7, 300, 1)])
def test_gae_on_the_device(T, N, S, tmp_path):
    """rs_ppo_gae: the bits of the host build of the same header (both compiled with -ffp-contract=off), hence within 4 e_ref of
    gae() + standardisation in float64; the same bits again in a second run"""
    rew, val, last, done = gae_case(T, N, S, seed=T + N)
    adv, ret = _device_gae(rew, val, last, done)
    ea, er, ref_a, ref_r = gae_errors(adv, ret, rew, val, last, done)
    print('T %d N %d S %d  adv: |dev - truth| %.3e, e_ref %.3e;  ret: |dev - truth| %.3e, e_ref %.3e' % (T, N, S, ea, ref_a, er, ref_r))
    assert ea <= 4 * ref_a and er <= 4 * ref_r
    h_adv, h_ret = host_gae(build_ppo_host(tmp_path), rew, val, last, done)
    print('  max |dev - host| adv %.3e ret %.3e' % (np.abs(adv - h_adv).max(), np.abs(ret - h_ret).max()))
    assert adv.tobytes() == h_adv.tobytes() and ret.tobytes() == h_ret.tobytes()
    adv2, ret2 = _device_gae(rew, val, last, done)
    assert adv.tobytes() == adv2.tobytes() and ret.tobytes() == ret2.tobytes()
    assert load_library().rs_ppo_gae(None, None, None, None, T, N, S, 0.99, 0.95, None, None, None, None) == RS_EINVAL


def test_update_from_rollout_matches_update():
    """A recorded segment whose logp / value are overwritten with the fp32 network's own: update_from_rollout (no second forward,
    rs_ppo_gae) gives the parameters update() gives on the same data and generator -- up to the largest difference between the
    two sets of advantages plus one fp32 ulp of the parameter (the Adam step)."""
    sc = load_scenario('cologne8')
    n, T = 64, 8
    sim = BatchedSim(sc, n, seed=4)
    grp = SimGroup([sim])
    grp.step('random', step_key=0, n_steps=20)
    net = _cologne8_policy(sc)
    pol = FusedIPPO(net, seed=9)
    rec = DeviceRollout(T, [sim])
    grp.rollout(rec, pol.handle, t0=0, n_steps=T, step_key=0, seed=9)
    grp.sync()
    seg = rec.pipes[0]
    last_obs = sim.tensor('drq_norm_f16').clone()
    done = torch.zeros(T, dtype=torch.bool, device='cuda')
    done[T // 2] = True
    with torch.no_grad():
        # (one forward over the segment and the state after it, as make_dataset does it: the same GEMM shapes, the same bits)
        lg, v = net(torch.cat([seg['obs'].reshape(T * n, *seg['obs'].shape[2:]), last_obs], 0))
        lp = torch.log_softmax(lg[:T * n].float(), -1).gather(-1, seg['act'].reshape(T * n, -1, 1).long()).squeeze(-1)
        kernel_gap = (lp.reshape(T, n, -1) - seg['logp']).abs().max().item()
        seg['logp'].copy_(lp.reshape(T, n, -1))
        seg['value'].copy_(v[:T * n].float().reshape(T, n, -1))
        last_value = v[T * n:].float().contiguous()
    print('max |logp_fp32net - logp_kernel| on this rollout: %.3e' % kernel_gap)

    nets = [copy.deepcopy(net) for _ in range(2)]
    learners = [BatchedPPOLearner(m, minibatch=256) for m in nets]
    gens = [torch.Generator(device='cuda').manual_seed(0) for _ in range(2)]
    ds_a = learners[0].make_dataset(seg['obs'], seg['act'], seg['rew'], done, last_obs)
    ds_b = learners[1].dataset_from_rollout(rec, last_value, done)
    adv_gap = (ds_a['adv'] - ds_b['adv']).abs().max().item()
    assert torch.equal(ds_a['act'], ds_b['act']) and torch.equal(ds_a['obs'], ds_b['obs'])
    learners[0].update(seg['obs'], seg['act'], seg['rew'], done, last_obs, generator=gens[0])
    learners[1].update_from_rollout(rec, last_value, done, generator=gens[1])
    assert learners[0].n_updates == learners[1].n_updates == 4 * 2
    worst, moved = 0.0, 0.0
    for (name, a), b, p0 in zip(nets[0].named_parameters(), nets[1].parameters(), net.parameters()):
        ulp = torch.from_numpy(np.spacing(np.abs(a.detach().cpu().numpy()).astype(np.float32))).cuda()
        excess = ((a - b).abs() - (adv_gap + ulp)).max().item()
        worst = max(worst, (a - b).abs().max().item())
        moved = max(moved, (a - p0).abs().max().item())
        assert excess <= 0.0, (name, excess, adv_gap)
    print('max |adv_torch - adv_kernel| %.3e; max parameter difference after one update %.3e (parameters moved by up to %.3e)'
          % (adv_gap, worst, moved))
    assert moved > 1e-4
    pol.close()
    sim.close()
