"""CPU: per-environment demand (rs_set_demand, resco_amd/demand.py) through the host emulation of the step kernel.

tests/demand_host/rs_emu_demand.cpp is tests/hostemu/rs_emu.cpp, unchanged, plus rs_set_demand on its handle: the selection of an
environment's trip tables is the kernel source's own (resco_step.h: Demand, resco_host.h: rs_reset_env), the check and the packing
of a call are the library's (resco_host.h: DemandHost).  Environment e of a handle with variants must equal, bit for bit, the CPU
oracle run on the scenario that holds e's trips -- in ascending, descending and shuffled thread order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_scenario, preroll_actions
from oracle.pyoracle import OracleEnv
from demand_host.emu import DemandEmuSim
from hostemu.emu import EmuSim
from resco_amd import demand
from test_hostemu import assert_equal

SEED, N, K, BASE = 11, 5, 3, 1          # 5 environments, 3 variants, env_base 1: environment 0 reads variant 1, and 5 is no multiple of 3
KW = dict(seed=SEED, sigma=-1.0, speed_dev=1)


def dep_lane_of_route(sc):
    A = sc.arrays
    return A['edge_lane0'][A['route_edge'][A['route_start'][:-1]]]


def handmade_variant(sc):
    """the base trips with ONE departure lane left without any trip (its trips take a route of another lane) and the last two trips
    departing at the horizon itself"""
    A = sc.arrays
    lane_of_route = dep_lane_of_route(sc)
    lanes, counts = np.unique(lane_of_route[A['trip_route']], return_counts=True)
    assert len(lanes) >= 2
    empty = lanes[np.argmin(counts)]                                # the lane that loses its trips
    other = int(np.nonzero(lane_of_route != empty)[0][0])           # a route that departs elsewhere
    route = A['trip_route'].copy()
    route[lane_of_route[route] == empty] = other
    depart = A['trip_depart'].copy()
    depart[-2:] = sc.horizon
    v = demand.with_trips(sc, depart, route, A['trip_vtype'])
    assert not (lane_of_route[v.arrays['trip_route']] == empty).any() and (v.arrays['trip_depart'] == sc.horizon).sum() >= 2
    return v


def two_types(sc):
    """the scenario with a SECOND vehicle type (a copy of the first; no trip uses it): shipped cologne1 has one type only, and the refusal
    of a variant whose most common type differs needs a type to differ to"""
    import dataclasses
    vp = sc.arrays['vtype_params']
    assert vp.shape[0] == 1
    return dataclasses.replace(sc, arrays=dict(sc.arrays, vtype_params=np.ascontiguousarray(np.vstack([vp, vp]))), vtype_ids=list(sc.vtype_ids) * 2)


@pytest.fixture(scope='module')
def variants():
    sc = load_scenario('cologne1')
    return sc, [sc, demand.demand_variant(sc, 7, keep=(0.6, 0.8), jitter_s=30), handmade_variant(sc)]


def oracles(vs, n=N, base=BASE, **kw):
    ev = demand.env_variants(n, base, len(vs))
    orcs = [OracleEnv(vs[ev[e]], env_index=base + e, **dict(KW, **kw)) for e in range(n)]
    for o in orcs:
        o.observe()
    return orcs


def actions(sc, k, n=N, base=BASE):
    return np.stack([preroll_actions(sc, SEED, base + e, k) for e in range(n)]).astype(np.int32)


def assert_stats_and_backlog(sim, orcs):
    st = sim.stats()
    cnt, waited = sim.backlog()
    for e, o in enumerate(orcs):
        so = o.stats()
        for k in st:
            assert st[k][e] == so[k], (k, e)
        w, c = o.backlog_delay()
        assert cnt[e] == c and waited[e] == w, (e, cnt[e], c, waited[e], w)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_every_environment_equals_the_oracle_on_its_own_variant(variants, order):
    sc, vs = variants
    sim = DemandEmuSim(sc, N, order=order, env_base=BASE, **KW)
    sim.set_demand(vs)
    assert sim.demand_info()[0] == K and list(sim.demand_info()[1]) == [1, 2, 0, 1, 2]
    sim.reset()
    orcs = oracles(vs)
    assert_equal(sim, orcs, -1)
    for step in range(40):
        a = actions(sc, step)
        sim.step(a)
        for e, o in enumerate(orcs):
            o.step(a[e])
        assert_equal(sim, orcs, step)
        assert_stats_and_backlog(sim, orcs)
    ins = sim.stats()['inserted']
    assert len(set(int(x) for x in ins)) > 1, 'the variants should differ in what they insert: %s' % ins
    assert list(sim.scheduled()) == [demand.scheduled(v) for v in sim.env_scenarios()]
    sim.close()


def test_trip_log_rows_and_metrics_follow_the_variant(variants):
    """RS_BUF_TRIP_LOG row k of environment e is trip k of e's variant; trip_metrics() charges each environment's own schedule"""
    sc, vs = variants
    sim = DemandEmuSim(sc, N, env_base=BASE, trip_log=1, **KW)
    sim.set_demand(vs)
    sim.reset()
    orcs = oracles(vs, trip_log=1)
    for step in range(60):
        a = actions(sc, step)
        sim.step(a)
        for e, o in enumerate(orcs):
            o.step(a[e])
    log = sim.read('trip_log')
    m = sim.trip_metrics()
    for e, o in enumerate(orcs):
        np.testing.assert_array_equal(log[e], o.trip_log(), err_msg='env %d' % e)
        so, v = o.stats(), o.vehicles()
        live = v['lane'] != 0xFFFF
        entries = so['arrived'] + int(live.sum())
        # trip_metrics adds the running vehicles' timeLoss up in float32: at most `capacity` non-negative terms, each addition off by
        # 2^-24 relative at the most, so the sum -- and the figures, whose other terms are integers -- is within capacity * 2^-24
        tol = sc.capacity * 2.0 ** -24
        loss = so['sum_time_loss_q10'] / 1024.0 + v['time_loss'][live].astype(np.float64).sum()
        assert m['delay'][e] == pytest.approx((loss + so['sum_depart_delay']) / max(1, entries), rel=tol)
        w, c = o.backlog_delay()
        assert m['delay_all'][e] == pytest.approx((loss + so['sum_depart_delay'] + w) / max(1, entries + c), rel=tol)
    sim.close()


def test_clear_demand_returns_to_the_scenario_s_trips(variants):
    sc, vs = variants
    sim = DemandEmuSim(sc, 2, env_base=BASE, **KW)
    plain = EmuSim(sc, 2, env_base=BASE, **KW)         # the untouched emulation: no rs_set_demand at all
    snap = sim.snapshot()                               # "no variants" asked of a handle without variants changes nothing:
    sim.clear_demand()                                  # the wrapper does not call, the library starts no new demand generation
    assert sim._lib.rs_set_demand(sim._h, 0, None, None) == 0
    sim.restore(snap)
    sim.free_snapshot(snap)
    sim.set_demand(vs[1:])
    sim.reset()
    for step in range(6):
        sim.step(actions(sc, step, 2))
    sim.clear_demand()
    assert sim.demand_info() == (0, None)
    sim.reset()
    for step in range(30):
        a = actions(sc, step, 2)
        sim.step(a)
        plain.step(a)
    for name in ('env', 'stats', 'dep_next', 'veh_lane', 'veh_trip', 'veh_pos', 'veh_speed', 'lane_agg', 'wait', 'mplight', 'tls'):
        np.testing.assert_array_equal(sim.read(name), plain.read(name), err_msg=name)
    sim.close()
    plain.close()


def test_two_pipes_equal_the_single_handle(variants):
    """the default map is keyed by the global environment index: pipes of 2 + 3 environments read what the 5-environment handle reads"""
    sc, vs = variants
    whole = DemandEmuSim(sc, 5, env_base=0, **KW)
    pipes = [DemandEmuSim(sc, 2, env_base=0, **KW), DemandEmuSim(sc, 3, env_base=2, **KW)]
    for s in [whole] + pipes:
        s.set_demand(vs)
        s.reset()
    for step in range(25):
        a = actions(sc, step, 5, 0)
        whole.step(a)
        pipes[0].step(a[:2])
        pipes[1].step(a[2:])
    for name in ('env', 'stats', 'dep_next', 'veh_lane', 'veh_trip', 'veh_pos', 'veh_speed', 'lane_agg', 'wait', 'mplight', 'tls'):
        np.testing.assert_array_equal(whole.read(name), np.concatenate([p.read(name) for p in pipes]), err_msg=name)
    for s in [whole] + pipes:
        s.close()


def test_generator_properties():
    sc = load_scenario('cologne1')
    n, hz = sc.n_trips, sc.horizon
    for seed, (lo, hi), jit in [(1, (0.6, 0.8), 30), (2, (0.3, 0.5), 0), (3, (1.0, 1.0), 60), (4, (0.0, 1.0), 5)]:
        a = demand.demand_variant(sc, seed, keep=(lo, hi), jitter_s=jit)
        b = demand.demand_variant(sc, seed, keep=(lo, hi), jitter_s=jit)
        for key in ('trip_depart', 'trip_route', 'trip_vtype', 'trips_cum'):
            np.testing.assert_array_equal(a.arrays[key], b.arrays[key])         # a pure function of its arguments
        assert a.n_trips == n and a.arrays['route_edge'] is sc.arrays['route_edge']     # (everything but the trips is shared)
        dep = a.arrays['trip_depart']
        assert (np.diff(dep) >= 0).all() and dep.min() >= 0 and dep.max() <= hz + 1
        np.testing.assert_array_equal(a.arrays['trips_cum'], [(dep <= t).sum() for t in range(hz + 2)])
        kept = demand.scheduled(a)
        assert lo * n - 0.03 * n <= kept <= hi * n + 0.03 * n, (seed, kept, n)
        assert a.arrays['trip_route'].max() < sc.n_routes and len(a.trip_ids) == n
    other = demand.demand_variant(sc, 5, keep=(0.6, 0.8), jitter_s=30)
    assert not np.array_equal(other.arrays['trip_depart'], demand.demand_variant(sc, 1, keep=(0.6, 0.8), jitter_s=30).arrays['trip_depart'])
    same = demand.demand_variant(sc, 9, resample=False)
    for key in ('trip_depart', 'trip_route', 'trip_vtype', 'trips_cum'):
        np.testing.assert_array_equal(same.arrays[key], sc.arrays[key])         # nothing asked for: the base trips
    s1, s2 = demand.demand_set(sc, 3, 21, jitter_s=10), demand.demand_set(sc, 3, 21, jitter_s=10)
    assert all(np.array_equal(x.arrays['trip_depart'], y.arrays['trip_depart']) for x, y in zip(s1, s2))
    assert not np.array_equal(s1[0].arrays['trip_depart'], s1[1].arrays['trip_depart'])
    np.testing.assert_array_equal(demand.env_variants(5, 1, 3), [1, 2, 0, 1, 2])
    assert demand.parse_spec('16,60,0.6,1.0') == (16, dict(jitter_s=60, keep=(0.6, 1.0))) and demand.parse_spec(None) == (0, {})


def test_with_trips_refuses_what_the_library_refuses():
    sc = load_scenario('cologne1')
    A = sc.arrays
    d, r, v = A['trip_depart'].copy(), A['trip_route'].copy(), A['trip_vtype'].copy()
    bad = lambda **kw: dict(dict(depart=d, route=r, vtype=v), **kw)
    assert d[len(d) // 2 - 1] > 0
    cases = [bad(depart=d[:-1]), bad(depart=np.where(np.arange(len(d)) == len(d) // 2, 0, d)),
             bad(depart=np.concatenate([[-1], d[1:]])), bad(depart=np.concatenate([d[:-1], [65535]])),
             bad(route=np.where(np.arange(len(r)) == 5, sc.n_routes, r)), bad(vtype=np.where(np.arange(len(v)) == 5, A['vtype_params'].shape[0], v))]
    for kw in cases:
        with pytest.raises(ValueError):
            demand.with_trips(sc, kw['depart'], kw['route'], kw['vtype'])


def test_every_refusal_leaves_the_handle_stepping_as_before(variants):
    sc, vs = variants
    sc, vs = two_types(sc), [two_types(v) for v in vs]      # two vehicle types, every trip of type 0
    sim = DemandEmuSim(sc, 3, env_base=BASE, **KW)
    ref = DemandEmuSim(sc, 3, env_base=BASE, **KW)
    for s in (sim, ref):
        s.set_demand(vs)
        s.reset()
    L, h = sim._lib, sim._h
    from resco_amd._abi import DemandStruct
    A = sc.arrays
    n = sc.n_trips
    i32 = lambda a: np.ascontiguousarray(a, np.int32)

    def call(K_, tabs, ev):
        structs = (DemandStruct * max(1, len(tabs)))()
        keep = []
        for k, t in enumerate(tabs):
            for name, a in zip(('trip_depart', 'trip_route', 'trip_vtype'), t):
                if a is not None:
                    a = i32(a)
                    keep.append(a)
                    setattr(structs[k], name, a.ctypes.data_as(C.POINTER(C.c_int32)))
        ev = None if ev is None else i32(ev)
        return L.rs_set_demand(h, K_, structs if tabs else None, None if ev is None else ev.ctypes.data)

    good = (A['trip_depart'], A['trip_route'], A['trip_vtype'])
    at = lambda a, i, x: np.where(np.arange(n) == i, x, a)
    assert A['vtype_params'].shape[0] == 2 and not A['trip_vtype'].any()
    other_vt = (np.arange(n) % 3 != 0).astype(np.int32)         # two trips in three of type 1: every type is valid, the most common one is not the scenario's
    tie_vt = (np.arange(n) < n // 2).astype(np.int32)           # (n odd: type 0 keeps the majority by one; n even: a tie, which goes to the lower index) -- accepted
    refusals = [
        ('n_variants < 0', lambda: call(-1, [good], [0, 0, 0])),
        ('NULL variants', lambda: call(1, [], [0, 0, 0])),
        ('NULL env_variant', lambda: call(1, [good], None)),
        ('NULL table', lambda: call(1, [(A['trip_depart'], None, A['trip_vtype'])], [0, 0, 0])),
        ('env_variant too large', lambda: call(1, [good], [0, 1, 0])),
        ('env_variant negative', lambda: call(1, [good], [0, -1, 0])),
        ('departs decrease', lambda: call(1, [(at(A['trip_depart'], n // 2, 0), A['trip_route'], A['trip_vtype'])], [0, 0, 0])),
        ('negative depart', lambda: call(1, [(at(A['trip_depart'], 0, -1), A['trip_route'], A['trip_vtype'])], [0, 0, 0])),
        ('depart above 65534', lambda: call(1, [(at(A['trip_depart'], n - 1, 65535), A['trip_route'], A['trip_vtype'])], [0, 0, 0])),
        ('route too large', lambda: call(1, [(A['trip_depart'], at(A['trip_route'], 7, sc.n_routes), A['trip_vtype'])], [0, 0, 0])),
        ('route negative', lambda: call(1, [(A['trip_depart'], at(A['trip_route'], 7, -1), A['trip_vtype'])], [0, 0, 0])),
        ('vtype too large', lambda: call(1, [(A['trip_depart'], A['trip_route'], at(A['trip_vtype'], 7, A['vtype_params'].shape[0]))], [0, 0, 0])),
        ('vtype negative', lambda: call(1, [(A['trip_depart'], A['trip_route'], at(A['trip_vtype'], 7, -1))], [0, 0, 0])),
    ]
    refusals.append(('another most common vehicle type', lambda: call(1, [(A['trip_depart'], A['trip_route'], other_vt)], [0, 0, 0])))
    assert A['trip_depart'][n // 2] > 0
    assert L.rs_set_demand(None, 0, None, None) == -1
    for step, (what, f) in enumerate(refusals):
        assert f() == -1, what                          # RS_EINVAL ...
        assert L.rs_last_error(h), what                 # ... with a text ...
        if what == 'another most common vehicle type':
            assert b'most common vehicle type is 1, the scenario\'s is 0' in L.rs_last_error(h)
        assert sim.demand_info()[0] == K, what          # ... and nothing changed: the handle goes on as its twin
        a = actions(sc, step, 3)
        sim.step(a)
        ref.step(a)
        for name in ('env', 'stats', 'dep_next', 'veh_trip', 'veh_pos', 'lane_agg'):
            np.testing.assert_array_equal(sim.read(name), ref.read(name), err_msg='%s after: %s' % (name, what))
    with pytest.raises(ValueError):
        sim.set_demand([load_scenario('cologne3')])     # (the wrapper: not a variant of this scenario)
    # ... while a variant that uses the second type without changing the most common one is taken (and then put back)
    assert call(1, [(A['trip_depart'], A['trip_route'], tie_vt)], [0, 0, 0]) == 0 and sim.demand_info()[0] == 1
    sim.set_demand(vs)
    with pytest.raises(ValueError):
        sim.set_demand(vs, env_variant=[0, 1])
    snap = sim.snapshot()
    sim.restore(snap)                                   # the same demand set: fine
    sim.set_demand(vs)
    with pytest.raises(RuntimeError, match='another demand set'):
        sim.restore(snap)
    sim.free_snapshot(snap)
    sim.close()
    ref.close()


def test_the_plain_emulation_has_no_demand_entry_point():
    """the feature is a new entry point bound behind hasattr: the untouched emulation library does not export it, and says so"""
    sc = load_scenario('cologne1')
    sim = EmuSim(sc, 1)
    assert not hasattr(sim._lib, 'rs_set_demand')
    with pytest.raises(RuntimeError, match='rs_set_demand'):
        sim.set_demand([sc])
    assert sim.demand_info() == (0, None)
    sim.clear_demand()                                  # nothing in force: no call at all
    sim.close()


def test_emulation_with_demand_under_the_sanitizers(variants, tmp_path):
    """tests/demand_host/demand_main.cpp: a program of its own (handle, two variants, ten steps, the refusals, the snapshot rule)
    built with -fsanitize=address,undefined.  Nothing of it is loaded into Python."""
    from resco_amd._abi import ScenarioStruct, pack_scenario
    sc, vs = variants
    st, keep = pack_scenario(sc)
    dump = tmp_path / 'cologne1.dump'
    n_envs, two = 3, vs[1:]
    with open(dump, 'wb') as f:
        f.write(C.string_at(C.addressof(st), ScenarioStruct.lane_len.offset))
        for a in keep:
            f.write(np.int64(a.nbytes).tobytes())
            f.write(a.tobytes())
        f.write(np.array([n_envs, len(two)], np.int32).tobytes())
        for v in two:
            for name in ('trip_depart', 'trip_route', 'trip_vtype'):
                f.write(np.ascontiguousarray(v.arrays[name], np.int32).tobytes())
        f.write(demand.env_variants(n_envs, 1, len(two)).tobytes())
    exe = str(tmp_path / 'demand_main')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-fno-omit-frame-pointer', '-static-libasan', '-static-libubsan', '-Wno-unknown-pragmas',
                           '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'resco_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'demand_host', 'demand_main.cpp'), '-o', exe])
    r = subprocess.run([exe, str(dump), '10'], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'ERROR' not in r.stderr and 'runtime error' not in r.stderr
    # the same episode through Python: the program's handle inserted what the library inserts
    sim = DemandEmuSim(sc, n_envs, order=2, env_base=1, seed=5, sigma=-1.0, speed_dev=1, trip_log=1)
    sim.set_demand(two)
    sim.reset()
    rng = np.uint32(2463534242)
    for s in range(10):
        a = np.zeros((n_envs, sc.n_signals), np.int32)
        for e in range(n_envs):
            for i in range(sc.n_signals):
                rng = np.uint32((int(rng) * 1664525 + 1013904223) & 0xFFFFFFFF)
                a[e, i] = (int(rng) >> 8) % int(sc.tls_ngreen[i])
        sim.step(a)
    assert r.stdout.strip().splitlines()[-1] == 'demand_main: inserted ' + ' '.join(str(int(x)) for x in sim.stats()['inserted'])
    sim.close()
