"""GPU: the two long paths of the plan phase -- the hop loop of phase_plan<true> with foe_blocked, and phase_lc_decide (resco_amd/csrc/
resco_step.h) -- on the device, against the C oracle (tests/oracle_batch.py).  The maps, steps, seed and env_base are those of
tests/test_long_paths_cpu.py, where the host emulation of the same source COUNTS that every kind of exit, stop, foe verdict and
lane-change outcome of these paths occurs in them: ingolstadt21 for 70 env-steps and cologne3 for 50, bench mode, seed 3, env_base 17,
the same random actions.  16 environments: one workgroup per environment, and look-ahead and lane-change lists of more than one chunk on
ingolstadt21 -- the smallest shape at which the chunked and the per-thread copy of these paths both run on the device.

Once on the per-map kernel and once on the generic one (RESCO_STEP_GENERIC=1), each in a fresh child process.  Every buffer of bench.py's
state digest, plus wait, pressure, queue_sum, arrivals and departures, must be bit-equal to the oracle's: the vehicle fields on the slots
that hold a vehicle (a free slot keeps what its last tenant left), everything else whole.  Of RS_BUF_TLS the oracle shows the phase
(column 0) and the departures; its other columns must be bit-equal between the two kernels, as must every whole buffer."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_scenario

pytestmark = pytest.mark.gpu

CASES = (('ingolstadt21', 70), ('cologne3', 50))
N_ENVS, SEED, ENV_BASE = 16, 3, 17
DIGEST_BUFFERS = ('veh_lane', 'veh_trip', 'veh_pos', 'veh_speed', 'veh_swait', 'veh_rwait', 'tls', 'stats', 'mplight', 'drq_norm')     # bench.py: state_digest
BUFFERS = DIGEST_BUFFERS + ('wait', 'pressure', 'queue_sum', 'arrivals', 'departures')
VEH = (('veh_trip', 'trip'), ('veh_pos', 'pos'), ('veh_speed', 'speed'), ('veh_swait', 'sumo_wait'), ('veh_rwait', 'resco_wait'))
EXPECT = {False: {'ingolstadt21': 'rs_step_kernel_fix_v64<ingolstadt21>', 'cologne3': 'rs_step_kernel_fix_v80<cologne3>'},
          True: {'ingolstadt21': 'rs_step_kernel_v64<896>', 'cologne3': 'rs_step_kernel_v80<256>'}}

CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from conftest import load_scenario
from resco_amd.sim import BatchedSim
kernels = {}
for name, steps in %(cases)r:
    sc = load_scenario(name)
    sim = BatchedSim(sc, %(n)d, seed=%(seed)d, sigma=-1.0, speed_dev=1, env_base=%(base)d)
    kernels[name] = sim.info()['step_kernel']
    rng = np.random.default_rng(0)
    for k in range(steps):
        sim.step(np.stack([rng.integers(0, sc.tls_ngreen) for _ in range(%(n)d)]).astype(np.int32))
    sim.sync()
    np.savez(os.path.join(%(out)r, name + '.npz'), **{b: np.ascontiguousarray(sim.read(b)) for b in %(buffers)r})
    sim.close()
print('DONE ' + json.dumps(kernels))
"""


def run_child(generic, out):
    os.makedirs(out)
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), cases=CASES, out=out, buffers=BUFFERS, n=N_ENVS, seed=SEED, base=ENV_BASE)
    env = dict(os.environ, RESCO_STEP_GENERIC='1' if generic else '0')
    env.pop('RESCO_SIM_LIB', None)
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=150)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ''
    assert r.returncode == 0 and last.startswith('DONE '), (r.returncode, r.stderr[-3000:])
    return json.loads(last[5:]), {name: dict(np.load(os.path.join(out, name + '.npz'))) for name, _ in CASES}


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from resco_amd.build import build_library
    build_library()
    d = tmp_path_factory.mktemp('long_paths')
    return {False: run_child(False, os.path.join(str(d), 'fix')), True: run_child(True, os.path.join(str(d), 'generic'))}


@pytest.fixture(scope='module')
def oracle():
    """the expected state of both maps, computed once: {map: (outputs, vehicles, stats) per environment}"""
    from oracle_batch import OracleBatch
    ref = {}
    for name, steps in CASES:
        sc = load_scenario(name)
        ob = OracleBatch(sc, N_ENVS, seed=SEED, env_base=ENV_BASE, sigma=-1.0, speed_dev=1)
        rng = np.random.default_rng(0)
        for k in range(steps):
            ob.step(np.stack([rng.integers(0, sc.tls_ngreen) for _ in range(N_ENVS)]).astype(np.int32))
        ref[name] = [(e.outputs(), e.vehicles(), e.stats()) for e in ob.envs]
    return ref


def same_bits(x, y):
    """floats: the same type and the same bytes; integers: the same values (the oracle keeps some in wider types)"""
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype.kind == 'f' or y.dtype.kind == 'f':
        return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    return x.shape == y.shape and np.array_equal(x.astype(np.int64), y.astype(np.int64))


def check_against_oracle(name, a, ref):
    from resco_amd.sim import STAT_KEYS
    st = a['stats']
    assert (st[:, 0] > 0).all() and (a['veh_lane'] != 0xFFFF).any(axis=1).all(), 'an empty network compares nothing'
    assert len(np.unique(a['veh_pos'], axis=0)) > 1, 'the environments must differ (sigma, speed deviation)'
    assert len(ref) == len(st)
    for e, (out, v, so) in enumerate(ref):
        assert same_bits(a['veh_lane'][e], v['lane']), '%s: veh_lane env %d differs from the oracle' % (name, e)
        live = v['lane'] != 0xFFFF
        for g, r in VEH:
            x, y = a[g][e][live], v[r][live]
            if r == 'trip':
                y = y.astype(np.int64) & 0xFFFF
            assert same_bits(x, y), '%s: %s env %d differs from the oracle' % (name, g, e)
        for i, key in enumerate(STAT_KEYS):
            assert int(st[e, i]) == so[key], (name, key, e)
        for b in ('mplight', 'drq_norm', 'wait', 'pressure', 'queue_sum', 'arrivals', 'departures'):
            assert same_bits(a[b][e], out[b]), '%s: %s env %d differs from the oracle' % (name, b, e)
        assert same_bits(a['tls'][e][:, 0], out['phase']), '%s: tls (phase) env %d differs from the oracle' % (name, e)


@pytest.mark.parametrize('generic', [False, True], ids=['per_map', 'generic'])
@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_long_paths_on_the_device_equal_the_oracle(runs, oracle, name, generic):
    kernels, got = runs[generic]
    assert kernels[name] == EXPECT[generic][name], kernels
    a = got[name]
    print(name, kernels[name], 'inserted', a['stats'][:, 0].tolist(), 'arrived', a['stats'][:, 1].tolist())
    check_against_oracle(name, a, oracle[name])
    other = runs[not generic][1][name]
    for b in BUFFERS:
        assert a[b].dtype == other[b].dtype and a[b].tobytes() == other[b].tobytes(), '%s: %s differs between the per-map and the generic kernel' % (name, b)
