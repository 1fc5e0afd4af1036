"""GPU: the wave-level helpers of the step kernel (resco_amd/csrc/resco_sim.hip) -- rs_wave_add / rs_wave_max reduce over the 64 lanes in
the VALU (DPP) and lane 63 issues the one atomic; DevExec::next_chunk hands wave w chunk w without a memory access and tickets after
that -- and the look-ahead distance classify() leaves in L.vnx for the next plan (resco_step.h), against the C oracle
(tests/oracle_batch.py), bit for bit.

Case 1: cologne1 (128 slots) x 4 environments, bench mode, the seeded random policy, 50 env-steps, with block_threads 64, 128 and the
default.  What the helpers build is compared after EVERY env-step: the counters (`ticks`, `active_ticks`, `sum_waiting`, `inserted`,
`arrived` and the rest of rs_stats) and the `env` row, whose third column is the high-water mark rs_wave_max builds; after the last step
every buffer of bench.py's state digest.  The window is chosen on the oracle alone (asserted below, so the test cannot pass vacuously):
in the last env-step every environment adds to `sum_waiting` and to `active_ticks`, and holds more than 64 vehicles -- at block_threads 64
one wave moves all of them, so a lane of rs_wave_add carries more than 1 (in each of the last twelve env-steps every environment holds more than 64).

Case 2: ingolstadt21 (896 slots) x 2 environments, default block (512 threads, eight waves), env-steps 0..40 from reset, the same
comparison: next_chunk with it > 0 and nwv = 8 (about 300 vehicles by the end: five slot chunks and the list chunks over eight waves, so
some tickets bring work and some end a wave's loop; at block_threads 64 and 128 of case 1 one and two waves take every chunk after
their first by ticket).

Case 3: the same handle shape for 150 env-steps, because case 2 cannot show from the oracle alone that a ticket at nwv = 8 brings work (its
lists' lengths are not an output): by then one environment holds more than 512 slots below its high-water mark and the other more than
448, so the plan of the last env-step's first tick has nine and eight slot chunks before any list chunk (asserted on the oracle) -- in one
workgroup a ticket beyond the eight first chunks is a chunk of work whatever the lists hold.

Once on the kernels a handle picks by itself (the per-map one where the shape fits it) and once on the generic ones
(RESCO_STEP_GENERIC=1, read by rs_create), each in a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_scenario

pytestmark = pytest.mark.gpu

CASES = (('cologne1', 4, 50, 64), ('cologne1', 4, 50, 128), ('cologne1', 4, 50, 0), ('ingolstadt21', 2, 41, 0), ('ingolstadt21', 2, 150, 0))      # map, environments, env-steps, block_threads
SEED, ENV_BASE = 5, 0
DIGEST_BUFFERS = ('veh_lane', 'veh_trip', 'veh_pos', 'veh_speed', 'veh_swait', 'veh_rwait', 'tls', 'stats', 'mplight', 'drq_norm')     # bench.py: state_digest
VEH = (('veh_trip', 'trip'), ('veh_pos', 'pos'), ('veh_speed', 'speed'), ('veh_swait', 'sumo_wait'), ('veh_rwait', 'resco_wait'))

CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from conftest import load_scenario
from resco_amd.sim import BatchedSim
kernels = {}
for name, n, steps, block in %(cases)r:
    sim = BatchedSim(load_scenario(name), n, seed=%(seed)d, sigma=-1.0, speed_dev=1, env_base=%(base)d, block_threads=block)
    key = '%%s_%%d_%%d' %% (name, block, steps)
    kernels[key] = [sim.info()['step_kernel'], int(sim.info()['block_threads'])]
    stats, env = [], []
    for k in range(steps):
        sim.act_random(k)
        sim.step(None)
        stats.append(sim.read('stats').copy()); env.append(sim.read('env').copy())
    sim.sync()
    np.savez(os.path.join(%(out)r, key + '.npz'), stats_steps=np.stack(stats), env_steps=np.stack(env),
             **{b: np.ascontiguousarray(sim.read(b)) for b in %(buffers)r})
    sim.close()
print('DONE ' + json.dumps(kernels))
"""


def run_child(generic, out):
    os.makedirs(out)
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), cases=CASES, out=out, buffers=DIGEST_BUFFERS, seed=SEED, base=ENV_BASE)
    env = dict(os.environ, RESCO_STEP_GENERIC='1' if generic else '0')
    env.pop('RESCO_SIM_LIB', None)
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=150)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ''
    assert r.returncode == 0 and last.startswith('DONE '), (r.returncode, r.stderr[-3000:])
    return json.loads(last[5:]), {'%s_%d_%d' % (c[0], c[3], c[2]): dict(np.load(os.path.join(out, '%s_%d_%d.npz' % (c[0], c[3], c[2])))) for c in CASES}


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from resco_amd.build import build_library
    build_library()
    d = tmp_path_factory.mktemp('wave_helpers')
    return {False: run_child(False, os.path.join(str(d), 'own')), True: run_child(True, os.path.join(str(d), 'generic'))}


@pytest.fixture(scope='module')
def oracle():
    """the expected values of both shapes, computed once (the block shape is no input of the model):
    {(map, environments, env-steps): (per env-step: [(stats, env row) per environment], after the last: [(outputs, vehicles)])}"""
    from oracle_batch import OracleBatch
    ref = {}
    for name, n, steps, _ in CASES:
        if (name, n, steps) in ref:
            continue
        ob = OracleBatch(load_scenario(name), n, seed=SEED, env_base=ENV_BASE, sigma=-1.0, speed_dev=1)
        per_step = []
        for k in range(steps):
            ob.act_random(k)
            ob.step(None)
            row = []
            for e in ob.envs:
                st, v = e.stats(), e.vehicles()
                row.append((st, (e.time, v['next_trip'], v['hw'], st['active'])))
            per_step.append(row)
        ref[(name, n, steps)] = (per_step, [(e.outputs(), e.vehicles()) for e in ob.envs])
    return ref


def same_bits(x, y):
    """floats: the same type and the same bytes; integers: the same values (the oracle keeps some in wider types)"""
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype.kind == 'f' or y.dtype.kind == 'f':
        return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    return x.shape == y.shape and np.array_equal(x.astype(np.int64), y.astype(np.int64))


def test_the_window_exercises_the_helpers(oracle):
    """on the oracle alone: in the last env-step of the cologne1 window every environment adds waiting seconds and active ticks, and holds
    more than 64 vehicles (more than the 64 lanes of the one wave that moves them at block_threads 64)"""
    per_step, _ = oracle[('cologne1', 4, 50)]
    for e in range(4):
        last, before = per_step[-1][e][0], per_step[-2][e][0]
        print('env', e, 'active', last['active'], 'waiting in the last step', last['sum_waiting'] - before['sum_waiting'],
              'active ticks in the last step', last['active_ticks'] - before['active_ticks'], 'high-water mark', per_step[-1][e][1][2])
        assert last['sum_waiting'] - before['sum_waiting'] != 0
        assert last['active_ticks'] - before['active_ticks'] != 0
        assert last['active'] > 64
        # more chunks than waves at block_threads 64 (one wave) and 128 (two): chunks are handed out by ticket (next_chunk with it > 0)
        assert (per_step[-1][e][1][2] + 63) // 64 >= 2
    per_step, _ = oracle[('ingolstadt21', 2, 41)]
    for e in range(2):
        print('ingolstadt21 env', e, 'high-water mark', per_step[-1][e][1][2], 'active', per_step[-1][e][0]['active'])
        assert per_step[-1][e][0]['active'] > 64
    # case 3: the first tick of the last env-step starts from the state the env-step before it left, so its plan phase has exactly
    # ceil(hw / 64) slot chunks (plus the list chunks): more than the eight waves in at least one workgroup -- there a ticket brings work
    per_step, _ = oracle[('ingolstadt21', 2, 150)]
    chunks = [(per_step[-2][e][1][2] + 63) // 64 for e in range(2)]
    print('ingolstadt21, 150 env-steps: slot chunks of the plan at the first tick of the last env-step', chunks)
    assert max(chunks) > 8 and min(chunks) >= 8


@pytest.mark.parametrize('generic', [False, True], ids=['own_kernel', 'generic'])
@pytest.mark.parametrize('name,n,steps,block', CASES, ids=['%s-%d-%d' % (c[0], c[3], c[2]) for c in CASES])
def test_wave_helpers_on_the_device_equal_the_oracle(runs, oracle, name, n, steps, block, generic):
    from resco_amd.sim import STAT_KEYS
    kernels, got = runs[generic]
    key = '%s_%d_%d' % (name, block, steps)
    kernel, threads = kernels[key]
    print(key, kernel, threads, 'threads')
    assert threads == block or block == 0
    if generic:
        assert 'fix' not in kernel, kernel
    elif name == 'ingolstadt21':
        assert kernel == 'rs_step_kernel_fix_v64<ingolstadt21>' and threads == 512, (kernel, threads)
    a = got[key]
    per_step, final = oracle[(name, n, steps)]
    assert a['stats_steps'].shape[:2] == (steps, n) and a['env_steps'].shape == (steps, n, 4)
    # what rs_wave_add / rs_wave_max build, after every env-step
    for k in range(steps):
        for e in range(n):
            so, env_row = per_step[k][e]
            for i, stat in enumerate(STAT_KEYS):
                assert int(a['stats_steps'][k, e, i]) == so[stat], (key, 'step', k, 'env', e, stat, int(a['stats_steps'][k, e, i]), so[stat])
            assert tuple(int(x) for x in a['env_steps'][k, e]) == tuple(int(x) for x in env_row), (key, 'step', k, 'env', e, a['env_steps'][k, e], env_row)
    # every buffer of the state digest after the last one
    assert len(np.unique(a['veh_pos'], axis=0)) > 1, 'the environments must differ (sigma, speed deviation)'
    for e, (out, v) in enumerate(final):
        assert same_bits(a['veh_lane'][e], v['lane']), '%s: veh_lane env %d differs from the oracle' % (key, e)
        live = v['lane'] != 0xFFFF
        assert live.any()
        for g, r in VEH:
            x, y = a[g][e][live], v[r][live]
            if r == 'trip':
                y = y.astype(np.int64) & 0xFFFF
            assert same_bits(x, y), '%s: %s env %d differs from the oracle' % (key, g, e)
        for b in ('mplight', 'drq_norm'):
            assert same_bits(a[b][e], out[b]), '%s: %s env %d differs from the oracle' % (key, b, e)
        assert same_bits(a['tls'][e][:, 0], out['phase']), '%s: tls (phase) env %d differs from the oracle' % (key, e)
    # RS_BUF_TLS beyond the phase, and every whole buffer: the same bits from both kernels and from every block shape
    other = runs[not generic][1][key]
    for b in DIGEST_BUFFERS:
        assert a[b].dtype == other[b].dtype and a[b].tobytes() == other[b].tobytes(), '%s: %s differs between a handle\'s own kernel and the generic one' % (key, b)
    if block:
        ref = got['%s_0_%d' % (name, steps)]
        live = ref['veh_lane'] != 0xFFFF        # (a free slot keeps what its last tenant left)
        for b in DIGEST_BUFFERS:
            x, y = (a[b][live], ref[b][live]) if b.startswith('veh_') and b != 'veh_lane' else (a[b], ref[b])
            assert x.tobytes() == y.tobytes(), '%s: %s differs between block %d and the default shape' % (key, b, block)
