"""GPU: the step kernel of a shipped map (rs_step_kernel_fix_v64 / _v80<map>: every table scalar and every offset of the working memory a
literal, resco_amd/csrc/resco_step.h KTabFix / LdsScn) changes which expressions the compiler can fold, never what is computed.  The
specialised and the generic kernel of the same library run the same 16 environments of cologne8, ingolstadt7, cologne3 and ingolstadt21,
seed 11, sigma 0.5 and speed deviation on, random policy, each in a fresh child process (RESCO_STEP_GENERIC, read when a handle is
created, picks the kernel): 80 env-steps of ingolstadt7 and 60 of the others -- by then junction walks with foes, hand-overs, lane changes
and insertions have all occurred -- and every buffer bench.py's state digest reads, plus the per-signal rewards and counters, must be
bit-equal.  One further handle has a non-default block: 256 threads on cologne8 select the 64-VGPR build, not the map's 80-VGPR one, so
the handle must fall back to the generic kernel in both children, and still give the bits of the default shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = (('cologne8', 60, 0), ('ingolstadt7', 80, 0), ('cologne3', 60, 0), ('ingolstadt21', 60, 0), ('cologne8', 60, 256))
DIGEST_BUFFERS = ('veh_lane', 'veh_trip', 'veh_pos', 'veh_speed', 'veh_swait', 'veh_rwait', 'tls', 'stats', 'mplight', 'drq_norm')     # bench.py: state_digest
BUFFERS = DIGEST_BUFFERS + ('wait', 'pressure', 'queue_sum', 'arrivals', 'departures')
EXPECT = {'cologne8': 'rs_step_kernel_fix_v80<cologne8>', 'ingolstadt7': 'rs_step_kernel_fix_v80<ingolstadt7>',
          'cologne3': 'rs_step_kernel_fix_v80<cologne3>', 'ingolstadt21': 'rs_step_kernel_fix_v64<ingolstadt21>'}
GENERIC = {'cologne8': 'rs_step_kernel_v80<256>', 'ingolstadt7': 'rs_step_kernel_v80<256>', 'cologne3': 'rs_step_kernel_v80<256>',
           'ingolstadt21': 'rs_step_kernel_v64<896>'}

CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from conftest import load_scenario
from resco_amd.sim import BatchedSim
kernels = {}
for name, steps, block in %(cases)r:
    sim = BatchedSim(load_scenario(name), 16, seed=11, sigma=0.5, speed_dev=1, block_threads=block)
    kernels['%%s/%%d' %% (name, block)] = sim.info()['step_kernel']
    for k in range(steps):
        sim.act_random(k)
        sim.step(None)
    sim.sync()
    np.savez(os.path.join(%(out)r, '%%s_%%d.npz' %% (name, block)), **{b: np.ascontiguousarray(sim.read(b)) for b in %(buffers)r})
    sim.close()
print('DONE ' + json.dumps(kernels))
"""


def run_child(generic, out):
    os.makedirs(out)
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), cases=CASES, out=out, buffers=BUFFERS)
    env = dict(os.environ, RESCO_STEP_GENERIC='1' if generic else '0')
    env.pop('RESCO_SIM_LIB', None)
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=150)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ''
    assert r.returncode == 0 and last.startswith('DONE '), (r.returncode, r.stderr[-3000:])
    return json.loads(last[5:]), {(name, block): dict(np.load(os.path.join(out, '%s_%d.npz' % (name, block)))) for name, _, block in CASES}


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from resco_amd.build import build_library
    build_library()
    d = tmp_path_factory.mktemp('scn_fix')
    return run_child(False, os.path.join(str(d), 'fix')), run_child(True, os.path.join(str(d), 'generic'))


def test_rs_info_names_the_kernel_each_handle_launches(runs):
    (kf, _), (kg, _) = runs
    print(kf, kg)
    for name, _, block in CASES:
        key = '%s/%d' % (name, block)
        if block == 0:
            assert kf[key] == EXPECT[name] and kg[key] == GENERIC[name], (key, kf[key], kg[key])
        else:       # 256 threads: the 64-VGPR build -- not the budget the map's kernel was instantiated for
            assert kf[key] == kg[key] == 'rs_step_kernel_v64<256>', (key, kf[key], kg[key])


@pytest.mark.parametrize('name,block', [(c[0], c[2]) for c in CASES])
def test_the_specialised_and_the_generic_kernel_give_the_same_bits(runs, name, block):
    (_, fix), (_, generic) = runs
    a, b = fix[(name, block)], generic[(name, block)]
    st = a['stats']
    print(name, block, 'inserted', st[:, 0].tolist(), 'arrived', st[:, 1].tolist())
    assert (st[:, 0] > 0).all() and (a['veh_lane'] != 0xFFFF).any(axis=1).all(), 'an empty network compares nothing'
    assert len(np.unique(a['veh_pos'], axis=0)) > 1, 'the environments must differ (sigma, speed deviation)'
    for buf in BUFFERS:
        assert a[buf].dtype == b[buf].dtype and a[buf].shape == b[buf].shape, buf
        assert a[buf].tobytes() == b[buf].tobytes(), '%s: %s differs between the specialised and the generic kernel' % (name, buf)
    if block:       # the block shape changes who does the work, not the result: the default shape's bits, from the specialised kernel
        ref = fix[(name, 0)]
        live = ref['veh_lane'] != 0xFFFF        # (a free slot keeps what its last tenant left)
        assert np.array_equal(a['veh_lane'], ref['veh_lane'])
        for buf in BUFFERS:
            x, y = (a[buf][live], ref[buf][live]) if buf.startswith('veh_') else (a[buf], ref[buf])
            assert x.tobytes() == y.tobytes(), '%s: %s differs between block %d and the default shape' % (name, buf, block)
