"""GPU: the whole-record loads of the table records (resco_amd/csrc/resco_tables.h: rec_load16, link_load, rec_load8) change how the step
kernel FETCHES a record, never what it computes.  The FIELD-LOADS build (resco_amd/build.py: -DRS_FIELD_LOADS, the kernel with the
compiler's field-wise loads) and the default library run the same 16 environments of the three 256-slot maps, sigma 0.5 and speed
deviation on, random policy, each in a fresh child process (RESCO_SIM_LIB picks the library when resco_amd.sim is imported): 80 env-steps
of ingolstadt7 and 60 of the others -- by then junction walks with foes, hand-overs, lane changes and insertions have all occurred --
and every buffer bench.py's state digest reads, plus the per-signal rewards and counters, must be bit-equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = (('cologne8', 60), ('ingolstadt7', 80), ('cologne3', 60))
DIGEST_BUFFERS = ('veh_lane', 'veh_trip', 'veh_pos', 'veh_speed', 'veh_swait', 'veh_rwait', 'tls', 'stats', 'mplight', 'drq_norm')     # bench.py: state_digest
BUFFERS = DIGEST_BUFFERS + ('wait', 'pressure', 'queue_sum', 'arrivals', 'departures')

CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from conftest import load_scenario
from resco_amd import sim as rsim
from resco_amd.sim import BatchedSim
assert os.path.samefile(rsim.LIB_PATH, %(lib)r), rsim.LIB_PATH
for name, steps in %(cases)r:
    sim = BatchedSim(load_scenario(name), 16, seed=11, sigma=0.5, speed_dev=1)
    for k in range(steps):
        sim.act_random(k)
        sim.step(None)
    sim.sync()
    np.savez(os.path.join(%(out)r, name + '.npz'), **{b: np.ascontiguousarray(sim.read(b)) for b in %(buffers)r})
    sim.close()
print('DONE')
"""


def run_child(lib, out):
    os.makedirs(out)
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), lib=lib, cases=CASES, out=out, buffers=BUFFERS)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, RESCO_SIM_LIB=lib), capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and r.stdout.strip().endswith('DONE'), (r.returncode, r.stderr[-3000:])
    return {name: dict(np.load(os.path.join(out, name + '.npz'))) for name, _ in CASES}


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from resco_amd.build import FIELDLOADS_LIB, LIB, build_fieldloads_library, build_library
    if not os.path.exists(FIELDLOADS_LIB):
        build_fieldloads_library()
    build_library()
    d = tmp_path_factory.mktemp('record_loads')
    return run_child(FIELDLOADS_LIB, os.path.join(str(d), 'field')), run_child(LIB, os.path.join(str(d), 'whole'))


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_field_loads_and_whole_record_loads_give_the_same_bits(runs, name):
    field, whole = runs
    a, b = field[name], whole[name]
    st = a['stats']
    print(name, 'inserted', st[:, 0].tolist(), 'arrived', st[:, 1].tolist())
    assert (st[:, 0] > 0).all() and (a['veh_lane'] != 0xFFFF).any(axis=1).all(), 'an empty network compares nothing'
    assert len(np.unique(a['veh_pos'], axis=0)) > 1, 'the environments must differ (sigma, speed deviation)'
    for buf in BUFFERS:
        assert a[buf].dtype == b[buf].dtype and a[buf].shape == b[buf].shape, buf
        assert a[buf].tobytes() == b[buf].tobytes(), '%s: %s differs between the field-loads build and the default library' % (name, buf)
