"""GPU: per-environment demand (rs_set_demand): environment e of a handle with demand variants equals, bit for bit, the CPU oracle run
on the scenario that holds e's trips -- through the literal kernel of a shipped map and through the generic kernels, at the default
workgroup shape and at an explicit one of another register budget; the trip log, rs_group_step, the training loop in one library
call, the snapshot rule and the way back to the scenario's own trips."""
import dataclasses

import numpy as np
import pytest

from conftest import load_scenario, preroll_actions
from test_gpu_parity import assert_env_equal

pytestmark = pytest.mark.gpu

SEED, N, K, BASE = 11, 5, 3, 1          # as tests/test_demand_cpu.py: environment 0 reads variant 1, and 5 is no multiple of 3
KW = dict(seed=SEED, sigma=-1.0, speed_dev=1)
STATE = ['env', 'tls', 'stats', 'dep_next', 'veh_lane', 'veh_trip', 'veh_pos', 'veh_speed', 'veh_cursor', 'veh_swait', 'veh_rwait', 'veh_depart',
         'veh_owner', 'veh_tloss', 'lane_agg', 'drq_norm', 'phase', 'mplight', 'wave', 'wait', 'wait_norm', 'pressure', 'queue_sum', 'queue_max',
         'arrivals', 'departures', 'mplight_full']

_variants = {}


def variants():
    """the three variants of the CPU test (base, resampled + jittered + thinned, hand-made), built once"""
    if not _variants:
        from resco_amd import demand
        from test_demand_cpu import handmade_variant
        sc = load_scenario('cologne1')
        _variants['v'] = (sc, [sc, demand.demand_variant(sc, 7, keep=(0.6, 0.8), jitter_s=30), handmade_variant(sc)])
    return _variants['v']


def actions(sc, k, n=N, base=BASE):
    return np.stack([preroll_actions(sc, SEED, base + e, k) for e in range(n)]).astype(np.int32)


def dep_next_of(o, sc):
    """RS_BUF_DEP_NEXT of an oracle environment: per departure lane the first trip of its variant that is not inserted yet.  The
    backlogs are FIFO per lane, so it is the lane's first trip that has neither arrived (a row in the trip log) nor is on the network."""
    A = sc.arrays
    lane_of_route = A['edge_lane0'][A['route_edge'][A['route_start'][:-1]]]
    lanes = np.unique(lane_of_route)
    lane_of_trip = lane_of_route[A['trip_route']]
    inserted = o.trip_log()[:, 1] > 0
    v = o.vehicles()
    inserted[v['trip'][v['lane'] != 0xFFFF].astype(np.int64) & 0xFFFF] = True
    out = []
    for lane in lanes:
        waiting = np.nonzero((lane_of_trip == lane) & ~inserted)[0]
        out.append(int(waiting[0]) if len(waiting) else 0xFFFF)
    return np.array(out, np.int64)


@pytest.mark.parametrize('generic,block', [(False, 0), (False, 128), (True, 0), (True, -256)])
def test_every_environment_equals_the_oracle_on_its_own_variant(generic, block):
    """shipped cologne1: the literal kernel of the map (80 VGPRs by default; 128 threads: the 64-VGPR generic build of its capacity);
    capacity 256: no literal kernel fits, the generic kernels (default shape: 80 VGPRs; -256: the 128-VGPR build)"""
    from oracle.pyoracle import OracleEnv
    from resco_amd import demand
    from resco_amd.sim import BatchedSim
    sc, vs = variants()
    if generic:
        sc = dataclasses.replace(sc, capacity=256)
        vs = [dataclasses.replace(v, capacity=256) for v in vs]
    sim = BatchedSim(sc, N, env_base=BASE, block_threads=block, trip_log=1, **KW)
    plain_kernel = sim.info()['step_kernel']
    sim.set_demand(vs)
    kernel = sim.info()['step_kernel']
    print(plain_kernel, '->', kernel)
    if not generic and block == 0:
        assert plain_kernel == 'rs_step_kernel_fix_v80<cologne1>' and kernel.startswith('rs_step_kernel_fix_v80<cologne1')
    elif generic:
        assert plain_kernel == ('rs_step_kernel_v128<256>' if block else 'rs_step_kernel_v80<256>')
    else:
        assert plain_kernel == 'rs_step_kernel_v64<128>'
    assert kernel != plain_kernel and 'demand' in kernel
    assert sim.demand_info()[0] == K and list(sim.demand_info()[1]) == [1, 2, 0, 1, 2]
    sim.reset()
    ev = demand.env_variants(N, BASE, K)
    orcs = [OracleEnv(vs[ev[e]], env_index=BASE + e, trip_log=1, **KW) for e in range(N)]
    for o in orcs:
        o.observe()
    assert_env_equal(sim, orcs, -1)
    for step in range(36):
        a = actions(sc, step)
        sim.step(a)
        for e, o in enumerate(orcs):
            o.step(a[e])
        assert_env_equal(sim, orcs, step)
    st, dn = sim.stats(), sim.read('dep_next').astype(np.int64)
    cnt, waited = sim.backlog()
    for e, o in enumerate(orcs):
        so = o.stats()
        for k in st:
            assert st[k][e] == so[k], (k, e)
        np.testing.assert_array_equal(dn[e], dep_next_of(o, vs[ev[e]]), err_msg='dep_next env %d' % e)
        w, c = o.backlog_delay()
        assert cnt[e] == c and waited[e] == w
    assert len(set(int(x) for x in st['inserted'])) > 1
    sim.close()


def test_literal_kernel_of_the_64_vgpr_build_ingolstadt21():
    """rs_step_kernel_fix_v64<ingolstadt21, demand>, the kernel behind the measured figures: 3 environments, K = 2 (the base trips and a
    resampled, jittered, thinned variant of the eight-type demand), 12 env-steps against the oracle; and the refusal of a variant whose
    most common vehicle type is not the scenario's, which leaves the handle as it was"""
    from oracle.pyoracle import OracleEnv
    from resco_amd import demand
    from resco_amd.sim import BatchedSim
    sc = load_scenario('ingolstadt21')
    assert sc.arrays['vtype_params'].shape[0] > 1
    vs = [sc, demand.demand_variant(sc, 3, keep=(0.6, 0.8), jitter_s=30)]
    n = 3
    sim = BatchedSim(sc, n, env_base=BASE, **KW)
    assert sim.info()['step_kernel'] == 'rs_step_kernel_fix_v64<ingolstadt21>'
    sim.set_demand(vs)
    assert sim.info()['step_kernel'] == 'rs_step_kernel_fix_v64<ingolstadt21, demand>'
    common = demand.common_vtype(sc.arrays['trip_vtype'])
    other = np.full(sc.n_trips, (common + 1) % sc.arrays['vtype_params'].shape[0], np.int32)
    with pytest.raises(RuntimeError, match='most common vehicle type'):
        sim.set_demand([demand.with_trips(sc, sc.arrays['trip_depart'], sc.arrays['trip_route'], other)])
    assert sim.demand_info()[0] == 2 and list(sim.demand_info()[1]) == [1, 0, 1]
    sim.reset()
    ev = demand.env_variants(n, BASE, 2)
    orcs = [OracleEnv(vs[ev[e]], env_index=BASE + e, **KW) for e in range(n)]
    for o in orcs:
        o.observe()
    assert_env_equal(sim, orcs, -1)
    for step in range(12):
        a = actions(sc, step, n)
        sim.step(a)
        for e, o in enumerate(orcs):
            o.step(a[e])
        assert_env_equal(sim, orcs, step)
    st = sim.stats()
    for e, o in enumerate(orcs):
        so = o.stats()
        for k in st:
            assert st[k][e] == so[k], (k, e)
    assert st['inserted'][0] != st['inserted'][1]
    sim.close()


def test_trip_log_and_trip_metrics_follow_the_variant():
    from oracle.pyoracle import OracleEnv
    from resco_amd import demand
    from resco_amd.sim import BatchedSim
    sc, vs = variants()
    sim = BatchedSim(sc, N, env_base=BASE, trip_log=1, **KW)
    sim.set_demand(vs)
    sim.reset()
    ev = demand.env_variants(N, BASE, K)
    orcs = [OracleEnv(vs[ev[e]], env_index=BASE + e, trip_log=1, **KW) for e in range(N)]
    for step in range(60):
        a = actions(sc, step)
        sim.step(a)
        for e, o in enumerate(orcs):
            o.step(a[e])
    log, m = sim.read('trip_log'), sim.trip_metrics()
    assert log.shape == (N, sc.n_trips, 4)
    tol = sc.capacity * 2.0 ** -24          # (trip_metrics sums the running vehicles' timeLoss in float32: tests/test_demand_cpu.py)
    for e, o in enumerate(orcs):
        rec = o.trip_log()                  # the oracle's trip records of THIS environment's variant: row k = trip k of the variant
        np.testing.assert_array_equal(log[e], rec, err_msg='env %d' % e)
        v, sched = o.vehicles(), vs[ev[e]].arrays['trip_depart'].astype(np.int64)
        live = v['lane'] != 0xFFFF
        done = rec[:, 1] > 0
        on = v['trip'][live].astype(np.int64) & 0xFFFF
        # (a vehicle inserted at the end of second t carries depart tick t + 1: multi_signal.tripinfo_records)
        depart_delay = int((rec[done, 0] - 1 - sched[done]).sum() + (v['depart'][live].astype(np.int64) - 1 - sched[on]).sum())
        entries = int(done.sum()) + int(live.sum())
        loss = rec[done, 2].sum() / 1024.0 + v['time_loss'][live].astype(np.float64).sum()
        assert depart_delay == o.stats()['sum_depart_delay'], 'the log row of a trip carries the depart tick of ITS variant'
        assert m['delay'][e] == pytest.approx((loss + depart_delay) / max(1, entries), rel=tol)
        assert m['waiting'][e] == pytest.approx(o.stats()['sum_waiting'] / max(1, entries), rel=1e-12)
    sim.close()


def test_group_step_with_variants_equals_single_steps():
    from resco_amd.sim import BatchedSim, SimGroup
    sc, vs = variants()
    a_sim, b_sim = (BatchedSim(sc, N, env_base=BASE, **KW) for _ in range(2))
    for s in (a_sim, b_sim):
        s.set_demand(vs)
        s.reset()
    SimGroup([a_sim]).step('random', step_key=40, n_steps=6)
    for k in range(6):
        b_sim.act_random(40 + k)
        b_sim.step(None)
    a_sim.sync()
    for name in STATE + ['actions']:
        np.testing.assert_array_equal(a_sim.read(name), b_sim.read(name), err_msg=name)
    assert len(set(int(x) for x in a_sim.stats()['inserted'])) > 1
    a_sim.close()
    b_sim.close()


def _train(library):
    """MPLight on cologne1 x 8 environments with K = 4 variants, batch 32, 24 env-steps: the Python-driven --device-update loop
    (tests/test_gpu_group_train.py: python_training) or the same steps in one rs_group_train call per chunk (DeviceTrainer)"""
    import torch
    import test_gpu_group_train as G
    from resco_amd import demand
    from resco_amd.agents.idqn_learn import linear_epsilon
    from resco_amd.agents.train_fused import DeviceTrainer
    steps, n = 24, 8
    X = G.setup('mplight', 'cologne1', n, False, 1)
    env, L, P, R = X.pe.envs[0], X.learner, X.policy, X.replay
    env.horizon_steps = steps
    env.set_demand(demand.demand_set(X.pe.scenario, 4, 5, jitter_s=60, keep=(0.6, 1.0)))
    X.pe.set_seed(1000)
    ret = torch.zeros(n, X.S, device='cuda')
    if library:
        X.pe.reset()
        trainer = DeviceTrainer(X.pe, L, P, R, 1.0, 0.0, X.decay)
        assert not trainer.run(10, ret)
        assert trainer.run(14, ret)
    else:
        obs = env.reset()[X.state]
        actions_t = env.tensor('actions')
        pair = torch.zeros(n, X.S, dtype=torch.int32, device='cuda')
        for k in range(steps):
            P.act(obs, epsilon=linear_epsilon(L.t, 1.0, 0.0, X.decay), step_key=L.t, out=actions_t, pair_out=pair)
            R.stage(obs)
            o, r, done, _ = env.step(None)
            rew = r[X.reward].float()
            R.commit(pair, rew, done)
            ret += rew
            L.observe_step(R)
            obs = o[X.state]
    torch.cuda.synchronize()
    out = dict(par=L.flat.detach().cpu().clone(), m=L._m.detach().cpu().clone(), ret=ret.cpu().clone(), updates=L.n_updates,
               inserted=env.sim.stats()['inserted'].copy(), kernel=env.sim.info()['step_kernel'])
    L.close()
    X.pe.close()
    return out


def test_training_loop_in_one_library_call_equals_the_python_loop():
    import torch
    want, got = _train(False), _train(True)
    assert want['updates'] > 0 and 'demand' in want['kernel'] and len(set(int(x) for x in want['inserted'])) > 1
    assert got['updates'] == want['updates'] and list(got['inserted']) == list(want['inserted'])
    for k in ('par', 'm', 'ret'):
        assert torch.equal(got[k], want[k]), k


def test_restore_refuses_a_snapshot_of_another_demand_set_and_clear_demand_is_the_plain_handle():
    import torch
    from resco_amd.sim import BatchedSim
    sc, vs = variants()
    sim, plain = BatchedSim(sc, N, env_base=BASE, **KW), BatchedSim(sc, N, env_base=BASE, **KW)
    for step in range(3):
        sim.step(actions(sc, step))
    snap = sim.snapshot()
    sim.clear_demand()                                  # no variants in force: nothing happens, in the wrapper ...
    assert sim._lib.rs_set_demand(sim._h, 0, None, None) == 0      # ... and in the library: the snapshot stays good
    sim.restore(snap)
    sim.set_demand(vs)
    with pytest.raises(RuntimeError, match='another demand set'):
        sim.restore(snap)
    sim.free_snapshot(snap)
    sim.reset()
    for step in range(8):
        sim.step(actions(sc, step))
    assert len(set(int(x) for x in sim.stats()['inserted'])) > 1
    # refusals change nothing, on the device either
    with pytest.raises(RuntimeError, match='env_variant'):
        sim.set_demand(vs, env_variant=[0, 1, 2, 3, 0])
    assert sim.demand_info()[0] == K
    sim.clear_demand()
    assert sim.demand_info() == (0, None) and sim.info()['step_kernel'] == plain.info()['step_kernel']
    sim.reset()
    for step in range(12):
        a = actions(sc, step)
        sim.step(a)
        plain.step(a)
    sim.sync()
    plain.sync()
    for name in STATE:
        assert torch.equal(sim.tensor(name), plain.tensor(name)), name
    sim.close()
    plain.close()
