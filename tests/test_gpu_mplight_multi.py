"""GPU: MPLight's shared FRAP trained on several maps at once (rs_mplight_multi_*, resco_amd/csrc/resco_frap_multi.h;
MultiMapMPLightLearner; tools/mplight_multimap_train.py).  The chain: a grouped minibatch gradient against the yardstick of
tests/frap_multi_ref.py; one map against rs_mplight_dqn_grad bit for bit; the draw against its rule; rs_mplight_multi_update against
the loop of sample, grad and step; the Adam step against the single-map learner's; two policies on different phase pairs reading the
one vector; the refusals; the tool end to end with zero-shot evaluation, bit-exact resume and a single-map checkpoint.

Rings are the sentinel rings of tests/test_gpu_mplight_train.py: environments and a signal past the case's hold NaN observations,
action -777 and NaN rewards -- one of them read, and a gradient is NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import frap_multi_ref as fm
import frap_ref as fr
import frap_train_ref as ft
import test_gpu_mplight_train as tm
from resco_amd.agents.mplight import FusedMPLight, pack_mplight_weights
from resco_amd.agents.mplight_multi import MultiMapMPLightLearner
from resco_amd.sim import DQNConfig, MPLightMap, MPLightRing, load_library, torch_stream

pytestmark = pytest.mark.gpu

RS_EINVAL = -1
SEED = tm.SEED


def _learner(cases, B, pad_signals=tm.PAD_SIGNALS, **kw):
    """a MultiMapMPLightLearner on device copies of the cases' (one shared) network, its target the cases'"""
    _, target = fm.shared_weights(cases)
    nets = [tm._device_net(c['net']) for c in cases]
    learner = MultiMapMPLightLearner(nets, [c['obs'].shape[2] + pad_signals for c in cases], batch_size=B, seed=SEED, **kw)
    learner.target.load_state_dict(target.state_dict())
    return nets, learner


def _state_np(learner):
    torch.cuda.synchronize()
    return tuple(x.detach().cpu().numpy().copy() for x in (learner.flat, learner._m, learner._v, learner._g, learner.loss_out))


@pytest.mark.parametrize('D,maps,counts', fm.CASES)
def test_grouped_minibatch_gradient(D, maps, counts):
    """counts over tiles of 4 rows: (5, 3, 4) a map across a tile boundary, a ragged single tile, one whole tile; (4, 4, 4); (0, 7, 0)
    the first and the last map empty; D = 4 with P = 13"""
    cases = fm.map_cases(D, maps)
    idx, g64, e_ref, l64, e_loss = fm.reference(D, maps, counts)
    nets, learner = _learner(cases, sum(counts))
    rings = [tm._device_ring(c) for c in cases]
    idx_t = torch.from_numpy(idx).cuda()
    learner.grad(rings, idx_t, counts)
    got, loss = tm._grads_np(learner), tm._loss_np(learner)
    print('D %d maps %s counts %s' % (D, maps, counts))
    worst = ft.compare(ft.names_of(nets[0]), got, loss, g64, e_ref, l64, e_loss)
    assert not worst, worst
    wrong = idx.copy()
    wrong[:, 0] = (wrong[:, 0] + 1) % len(maps)             # a tag that disagrees with its group is ignored; and the same bits again
    learner.grad(rings, torch.from_numpy(wrong).cuda(), counts)
    again = tm._grads_np(learner)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    assert loss.tobytes() == tm._loss_np(learner).tobytes()
    learner.close()


@pytest.mark.parametrize('B', [3, 11])
def test_one_map_is_rs_mplight_dqn_grad(B):
    """n_maps = 1 on the same rows: gradients and loss bit for bit (the reuse of the row arithmetic and the summation order)"""
    c = ft.case(*tm.MID)
    idx = ft.draw_idx(c, B)
    ring = tm._device_ring(c)
    _, single = tm._learner(c, B)
    single.grad(ring, torch.from_numpy(idx).cuda())
    _, multi = _learner([c], B)
    multi.grad([ring], torch.from_numpy(np.concatenate((np.zeros((B, 1), np.int32), idx), -1)).cuda(), [B])
    torch.cuda.synchronize()
    assert single._g.cpu().numpy().tobytes() == multi._g.cpu().numpy().tobytes()
    assert tm._loss_np(single).tobytes() == tm._loss_np(multi).tobytes() and np.isfinite(tm._loss_np(multi)).all()
    single.close()
    multi.close()


@pytest.mark.parametrize('rings', fm.RING_SETS)
def test_sample_on_the_device(rings):
    """idx_out and counts_out against the restatement of the rule at B = 33 and 300 (two chunks of the sampler, the second ragged);
    grouped, stable, check_sample per map; a ring with count < 2 never drawn; the default key is the number of Adam steps"""
    c = ft.case(2, 1, 3, 4, 2)
    nets = [tm._device_net(c['net']) for _ in rings]
    learner = MultiMapMPLightLearner(nets, [r[2] for r in rings], batch_size=300, seed=SEED)
    rps = []
    for T, N, S, head, count in rings:
        rp = tm._sentinel_ring(T, N, S, 13)         # (the draw reads nothing of it)
        rp.head, rp.count = head, count
        rps.append(rp)
    draws = []
    for B in (33, 300):
        for u in (0, 1, 77):
            idx, counts = learner.sample(rps, batch_size=B, update_key=u)
            idx = idx.cpu().numpy()
            want, want_counts = fm.predict_sample(SEED, u, rings, B)
            assert idx.shape == (B, 4) and counts == want_counts and np.array_equal(idx, want)
            fm.check_grouped(idx, counts, rings)
            assert counts == [int((idx[:, 0] == m).sum()) for m in range(len(rings))]
            draws.append(idx)
    assert [c > 0 for c in counts] == [r[4] >= 2 for r in rings]
    assert not np.array_equal(draws[0], draws[1])
    assert np.array_equal(learner.sample(rps, batch_size=33)[0].cpu().numpy(), draws[0])
    learner.close()


def _written_rings(cases):
    return [tm._device_ring(c, head=h, pad=(0, 0)) for c, h in zip(cases, (3, 1, 2))]


def test_update_is_the_loop_of_single_calls():
    """rs_mplight_multi_update(n_updates = 3) against sample (keyed by the steps so far), grad, step, three times; and again"""
    cases = fm.map_cases(1, fm.MAPS_D1)
    rings = _written_rings(cases)

    def run(fused):
        nets, learner = _learner(cases, 21, pad_signals=0)
        if fused:
            learner.update(rings, updates=3)
        else:
            for _ in range(3):
                idx, counts = learner.sample(rings)
                learner.grad(rings, idx, counts)
                learner.step()
        assert learner.n_updates == 3
        out = _state_np(learner)
        learner.close()
        return out

    one, loop, again = run(True), run(False), run(True)
    for other in (loop, again):
        for a, b in zip(one, other):
            assert a.tobytes() == b.tobytes()
    assert all(np.isfinite(a).all() for a in one)
    assert np.abs(one[0] - pack_mplight_weights(cases[0]['net']).numpy()).max() > 1e-4


def test_adam_step_is_the_single_map_step():
    """the same gradient vector into a multi-map and a single-map learner: two Adam steps, parameters and moments bit for bit"""
    cases = fm.map_cases(1, fm.MAPS_D1)
    idx = fm.reference(1, fm.MAPS_D1, (5, 3, 4))[0]
    nets, multi = _learner(cases, 12)
    multi.grad([tm._device_ring(c) for c in cases], torch.from_numpy(idx).cuda(), (5, 3, 4))
    _, single = tm._learner(cases[0], 12, n_signals=1)
    single._g.copy_(multi._g)
    for t in (1, 2):
        multi.step()
        single.step()
        assert multi.n_updates == single.n_updates == t
        torch.cuda.synchronize()
        for a, b in ((multi.flat, single.flat), (multi._m, single._m), (multi._v, single._v), (multi._g, single._g)):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert np.abs(multi.flat.cpu().numpy() - pack_mplight_weights(cases[0]['net']).numpy()).max() > 1e-4
    multi.close()
    single.close()


def test_policies_on_different_pairs_share_the_vector():
    """Two FusedMPLight policies on different phase pairs (P = 4 and 9) bound to learner.flat: after an update both return the Q of
    the UPDATED weights (against float64 at test_gpu_mplight.py's tolerance, e_ref from the fp32 torch FRAP); every per-map
    FRAP.state_dict() is then the same tensors; sync_target copies them"""
    maps = (fm.MAPS_D1[0], fm.MAPS_D1[2])
    cases = fm.map_cases(1, maps)
    nets, learner = _learner(cases, 16, pad_signals=0)
    rings = [tm._device_ring(c, head=h, pad=(0, 0)) for c, h in zip(cases, (3, 2))]
    policies = [FusedMPLight(n, c['sc'], seed=3 + m) for m, (n, c) in enumerate(zip(nets, cases))]
    for p in policies:
        p.share_weights(learner.flat)
    rows = [np.ascontiguousarray(c['obs'][0]) for c in cases]
    obs = [torch.from_numpy(r.astype(np.int32)).cuda().contiguous() for r in rows]      # (demand_shape 1: the kernel reads int32 rows)
    before = [p.act(o, want_q=True)[1].cpu().numpy() for p, o in zip(policies, obs)]
    learner.update(rings, updates=2)
    torch.cuda.synchronize()
    flat = learner.flat.cpu().numpy()
    assert not np.array_equal(flat, pack_mplight_weights(cases[0]['net']).numpy())
    for m, (p, o, c, n) in enumerate(zip(policies, obs, cases, nets)):
        P = c['P']
        q = p.act(o, want_q=True)[1].cpu().numpy()
        assert np.array_equal(pack_mplight_weights(n).cpu().numpy(), flat)
        q64 = fr.frap_ref(n.state_dict(), c['pairs'], 1, rows[m]).reshape(q.shape[0], q.shape[1], P)
        tol, e_ref = fr.q_tolerance(q64, fr.fp32_frap(n, rows[m]).reshape(q64.shape))
        err = np.abs(q[..., :P].astype(np.float64) - q64)
        print('map %d P %d: |dev - truth| %.3e = %.2f e_ref' % (m, P, err.max(), err.max() / max(e_ref, 1e-300)))
        assert np.all(np.isfinite(q[..., :P])) and np.all(err <= tol) and not np.array_equal(q, before[m])
    sd0 = nets[0].state_dict()
    for n in nets[1:]:
        assert all(sd0[k].cpu().numpy().tobytes() == v.cpu().numpy().tobytes() for k, v in n.state_dict().items())
    assert learner.flat_target.cpu().numpy().tobytes() != flat.tobytes()
    learner.sync_target()
    torch.cuda.synchronize()
    assert learner.flat_target.cpu().numpy().tobytes() == flat.tobytes()
    for p in policies:
        p.close()
    learner.close()


def test_refusals():
    """every RS_EINVAL of the header, with its word in the message; nothing launched: parameters and step count unchanged"""
    cases = fm.map_cases(1, fm.MAPS_D1)
    B = 12
    nets, learner = _learner(cases, B, pad_signals=0)
    rps = _written_rings(cases)
    idx = torch.from_numpy(fm.reference(1, fm.MAPS_D1, (5, 3, 4))[0]).cuda()
    torch.cuda.synchronize()
    L, h, st = load_library(), learner._h, torch_stream(0)
    p0 = learner.flat.cpu().numpy().copy()
    n = len(cases)

    def rings(which=1, **kw):
        arr = (MPLightRing * n)()
        for k, rp in enumerate(rps):
            arr[k] = MPLightRing(rp.obs.data_ptr(), rp.act.data_ptr(), rp.rew.data_ptr(), rp.done.data_ptr(), rp.T, rp.N, rp.S, 13, rp.head, rp.count)
        for k, v in kw.items():
            setattr(arr[which], k, v)
        return arr

    counts = (C.c_int32 * n)(5, 3, 4)
    out_counts = (C.c_int32 * n)()

    def refused(r, batch=B, word=b'', cnt=counts):
        for rc in (L.rs_mplight_multi_sample(h, r, batch, SEED, 0, idx.data_ptr(), out_counts, st),
                   L.rs_mplight_multi_grad(h, r, idx.data_ptr(), cnt, batch, None, st), L.rs_mplight_multi_update(h, r, batch, SEED, 1, None, st)):
            assert rc == RS_EINVAL and word in L.rs_last_error(None), (rc, L.rs_last_error(None))

    assert L.rs_mplight_multi_grad(h, rings(), idx.data_ptr(), counts, B, None, st) == 0        # (the arguments the refusals vary are good)
    refused(rings(), 0, b'max_batch')
    refused(rings(), B + 1, b'max_batch')
    refused(rings(capacity=1, count=1, head=0), word=b'capacity >= 2')
    refused(rings(n_envs=0), word=b'n_envs >= 1')
    refused(rings(n_signals=rps[1].S + 1), word=b'n_signals')
    refused(rings(which=2, n_signals=rps[1].S), word=b'map 2')
    refused(rings(width=49), word=b'width')
    refused(rings(head=-1), word=b'outside the ring')
    refused(rings(head=rps[1].T), word=b'outside the ring')
    refused(rings(count=rps[1].T + 1), word=b'outside the ring')
    refused(rings(count=-1), word=b'outside the ring')
    refused(rings(obs=None), word=b'NULL')
    refused(rings(which=0, done=None), word=b'NULL')
    refused(None, word=b'NULL')
    refused(rings(capacity=3, count=3, head=0, n_envs=2 ** 30), word=b'2^31')
    host_rew = np.zeros((rps[1].T, rps[1].N, rps[1].S), np.float32)
    refused(rings(rew=host_rew.ctypes.data), word=b'not device memory')
    empty = rings()
    for k in range(n):
        empty[k].count, empty[k].head = 1, 1
    refused(empty, word=b'total == 0')
    one_drawable = rings(which=0, count=1, head=1)              # (count < 2 alone is no refusal: that ring is never drawn)
    assert L.rs_mplight_multi_sample(h, one_drawable, B, SEED, 0, idx.data_ptr(), out_counts, st) == 0 and out_counts[0] == 0
    for bad, word in (((5, 3, 5), b'sum'), ((6, 3, 4), b'sum'), ((13, -1, 0), b'negative'), ((5, 3, 3), b'sum')):
        assert L.rs_mplight_multi_grad(h, rings(), idx.data_ptr(), (C.c_int32 * n)(*bad), B, None, st) == RS_EINVAL and word in L.rs_last_error(None), bad
    assert L.rs_mplight_multi_grad(h, rings(), idx.data_ptr(), None, B, None, st) == RS_EINVAL and b'NULL' in L.rs_last_error(None)
    assert L.rs_mplight_multi_sample(h, rings(), B, SEED, 0, idx.data_ptr(), None, st) == RS_EINVAL and b'NULL' in L.rs_last_error(None)
    assert L.rs_mplight_multi_sample(None, rings(), B, SEED, 0, idx.data_ptr(), out_counts, st) == RS_EINVAL and b'NULL handle' in L.rs_last_error(None)
    assert L.rs_mplight_multi_sample(h, rings(), B, SEED, 0, None, out_counts, st) == RS_EINVAL and b'NULL' in L.rs_last_error(None)
    assert L.rs_mplight_multi_grad(h, rings(), None, counts, B, None, st) == RS_EINVAL and b'NULL' in L.rs_last_error(None)
    assert L.rs_mplight_multi_update(h, rings(), B, SEED, 0, None, st) == RS_EINVAL and b'n_updates' in L.rs_last_error(None)
    assert L.rs_mplight_multi_step(None, st) == RS_EINVAL and L.rs_mplight_multi_sync_target(None, st) == RS_EINVAL and L.rs_mplight_multi_steps(None) == -1
    assert L.rs_mplight_multi_set_steps(h, -1) == RS_EINVAL
    host = np.zeros((B, 4), np.int32)
    assert L.rs_mplight_multi_sample(h, rings(), B, SEED, 0, host.ctypes.data, out_counts, st) == RS_EINVAL and b'not device memory' in L.rs_last_error(None)
    assert L.rs_mplight_multi_grad(h, rings(), host.ctypes.data, counts, B, None, st) == RS_EINVAL and b'not device memory' in L.rs_last_error(None)

    # rs_mplight_multi_create
    cfg = DQNConfig(1e-3, 1e-8, 0.9, 0.999, 0.99)
    vecs = [learner.flat, learner.flat_target, learner._g, learner._m, learner._v]
    good = (0, 1, 2, 3)

    def create(device=0, D=1, n_maps=2, P=2, pairs=good, S=2, max_batch=B, drop=None, cfg_ref=C.byref(cfg), no_maps=False):
        out = C.c_void_p()
        k_maps = max(n_maps, 1)                             # the LAST map carries what the call varies; the others are good
        tabs = [(C.c_int32 * 4)(*good) for _ in range(k_maps - 1)] + [(C.c_int32 * len(pairs))(*pairs) if pairs is not None else None]
        maps = (MPLightMap * k_maps)()
        for k, tab in enumerate(tabs):
            maps[k].n_pairs, maps[k].pairs, maps[k].n_signals = (P if k == k_maps - 1 else 2), (C.addressof(tab) if tab is not None else None), S
        ptrs = [v.data_ptr() if i != drop else None for i, v in enumerate(vecs)]
        rc = L.rs_mplight_multi_create(device, D, n_maps, None if no_maps else maps, cfg_ref, *ptrs, max_batch, C.byref(out))
        if rc == 0:
            L.rs_mplight_multi_destroy(out)
        else:
            assert out.value is None
        return rc

    assert create() == 0 and create(n_maps=1) == 0 and create(n_maps=8) == 0
    for bad in (dict(n_maps=0), dict(n_maps=9), dict(D=2), dict(P=1), dict(P=17, pairs=tuple(range(12)) * 3), dict(pairs=(0, 1, 2, 12)),
                dict(pairs=(0, -1, 2, 3)), dict(pairs=None), dict(S=0), dict(max_batch=0), dict(drop=1), dict(drop=4), dict(cfg_ref=None),
                dict(no_maps=True), dict(device=-1), dict(device=torch.cuda.device_count())):
        assert create(**bad) == RS_EINVAL, bad
        assert L.rs_last_error(None).startswith(b'rs_mplight_multi_create'), bad
    with pytest.raises(RuntimeError, match=r'rs_mplight_multi_grad failed \(-1\).*sum'):
        learner.grad(rps, idx, (5, 3, 3))
    torch.cuda.synchronize()
    assert p0.tobytes() == learner.flat.cpu().numpy().tobytes() and learner.n_updates == 0
    learner.close()


# ---- the tool end to end: cologne1 (P = 4) + ingolstadt1 (P = 3) at 3 and 2 environments, 2 episodes, batch 8
TOOL = dict(maps=('cologne1', 'ingolstadt1'), n_envs=(3, 2), episodes=2, batch=8, replay_steps=64, quiet=True)


def _tool_run(**kw):
    from tools import mplight_multimap_train as tool
    made = {}
    rows, final = tool.main(**dict(TOOL, made=made, **kw))
    torch.cuda.synchronize()
    assert made['learner']._h is None, 'the tool closes its learner'
    return rows, final, made['learner'].flat.cpu().numpy().copy()


@pytest.fixture(scope='module')
def whole_run(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('multimap') / 'whole.pt')
    return _tool_run(eval_on=('cologne3',), save=path, save_replay=True) + (path,)


def test_tool_trains_and_evaluates_zero_shot(whole_run):
    rows, final, flat, _ = whole_run
    assert len(rows) == 2 and rows[-1]['updates'] > 0 and np.isfinite(flat).all()
    assert all(np.isfinite(r['avg_delay_s'][m]) for r in rows for m in TOOL['maps'])
    zs = final['zero_shot']['cologne3']
    assert np.isfinite(zs['greedy_avg_delay_s']) and np.isfinite(zs['random_avg_delay_s'])
    from tools import mplight_multimap_train as tool
    with pytest.raises(ValueError, match='environment counts'):
        tool.main(maps=('cologne1', 'ingolstadt1'), n_envs=(3, 2, 1), quiet=True)


def test_tool_resumes_to_the_same_weights(whole_run, tmp_path):
    """save, leave after 1 of 2 episodes, load with the replay ring: the final weights are the uninterrupted run's bit for bit"""
    rows, _, flat, _ = whole_run
    path = str(tmp_path / 'half.pt')
    first, final, _ = _tool_run(save=path, save_replay=True, stop_after=1)
    assert final is None and len(first) == 1
    resumed, final, flat2 = _tool_run(load=path)
    assert len(resumed) == 2 and final is not None
    assert flat2.tobytes() == flat.tobytes()
    assert [r['avg_delay_s'] for r in resumed] == [r['avg_delay_s'] for r in rows]


def test_tool_evaluates_a_single_map_checkpoint_on_another_map(whole_run, tmp_path):
    """a checkpoint of tools/mplight_train.py --device-update on cologne1 (P = 4) evaluates on ingolstadt1 (P = 3); so does the
    multi-map checkpoint"""
    from tools import mplight_train
    path = str(tmp_path / 'single.pt')
    mplight_train.main('cologne1', 3, 1, 8, 64, quiet=True, device_update=True, save=path)
    ck = torch.load(path, weights_only=True, map_location='cpu')
    want = torch.cat([v.reshape(-1) for v in ck['objects']['net']['weights'].values()]).numpy()
    for src, flat_want in ((path, want), (whole_run[3], whole_run[2])):
        rows, final, flat = _tool_run(maps=('ingolstadt1',), n_envs=(2,), episodes=1, load=src, eval_only=True)
        assert flat.tobytes() == flat_want.tobytes()
        assert np.isfinite(final['greedy_avg_delay_s']['ingolstadt1']) and np.isfinite(final['random_avg_delay_s']['ingolstadt1'])
