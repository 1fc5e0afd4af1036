"""CPU: the per-map step kernels see the constants of a handle as LITERALS (resco_amd/csrc/resco_step.h: ScnConsts, KTabFix, LdsScn;
the literals: the header resco_amd/build.py generates from the shipped scenarios).

The generated literals of each of the six shipped maps equal rs_scn_consts of the loaded scenario, member by member, and a scenario
perturbed in one constant gives other constants than the literals (what makes rs_create fall back to the generic kernel).  Which kernel
a handle launches and what the kernels compute is the GPU tests' matter (tests/test_gpu_scn_fix.py; the parity tests and the smoke
run launch the per-map kernels by default and compare them with the oracle)."""
import copy
import re

import numpy as np
import pytest

from conftest import load_scenario

MAPS = ['cologne1', 'cologne3', 'cologne8', 'ingolstadt1', 'ingolstadt7', 'ingolstadt21']


def header_literals():
    """{map: {member: value}} parsed from the generated header, and the maps its X-macro lists"""
    from resco_amd.build import generate_scn_header
    with open(generate_scn_header()) as f:
        text = f.read()
    out = {}
    for name, body in re.findall(r'struct ScnFix_(\w+) \{(.*?)\n\};', text, flags=re.S):
        out[name] = {k: int(v.rstrip('u'), 0) for k, v in re.findall(r'static constexpr u?int32_t (\w+) = (-?\w+);', body)}
    listed = re.findall(r'X\((\w+)\)', text[text.index('#define RS_SCN_MAPS(X)'):].splitlines()[0])
    return out, listed


@pytest.fixture(scope='module')
def literals():
    return header_literals()


def test_the_header_lists_the_six_shipped_maps(literals):
    lit, listed = literals
    assert sorted(lit) == sorted(listed) == sorted(MAPS)


@pytest.mark.parametrize('name', MAPS)
def test_generated_literals_equal_the_constants_of_the_loaded_scenario(literals, name):
    from resco_amd.build import scn_consts
    sc = load_scenario(name)
    host = scn_consts(sc)
    lit = literals[0][name]
    assert sorted(lit) == sorted(host)
    # every member of ScnConsts the kernels read
    for k in ('kmax', 'tls_maxl', 'n_signals', 'n_obs', 'n_vtypes', 'n_dep', 'n_arr', 'n_trips', 'n_cells', 'gstride', 'capacity', 'lmax',
              'step_length', 'yellow_length', 'horizon', 'maxlen_bits', 'occ_unit_bits', 'cell_inv_bits', 'o_vtp', 'o_tstate', 'o_arr',
              'o_insm', 'o_agg_q', 'lcap', 'lds_bytes', 'budget'):
        assert k in host, k
    for k in host:
        assert lit[k] == host[k], (name, k, lit[k], host[k])
    assert host['capacity'] == sc.capacity and host['kmax'] == sc.kmax and host['n_signals'] == sc.n_signals
    assert np.array([host['cell_inv_bits']], np.uint32).view(np.float32)[0] == np.float32(1.0) / np.float32(30.0)
    # the register budget rs_create chooses at the default block: 64 VGPRs (0) only for the map that runs four workgroups per CU
    assert host['budget'] == (0 if name == 'ingolstadt21' else 2)


def test_a_perturbed_scenario_has_other_constants_than_the_literals(literals):
    """rs_create launches a map's kernel only if EVERY constant of the handle equals the literals (resco_step.h: scn_fix_matches):
    each of these perturbations changes at least one member"""
    from resco_amd.build import scn_consts
    sc = load_scenario('cologne1')
    lit = literals[0]['cologne1']
    differs = lambda c: sorted(k for k in c if c[k] != lit[k])
    assert differs(scn_consts(sc)) == []
    cap = copy.copy(sc)
    cap.capacity = 192
    assert 'capacity' in differs(scn_consts(cap))
    vt = copy.copy(sc)
    vt.arrays = dict(sc.arrays)
    vt.arrays['vtype_params'] = np.concatenate([sc.arrays['vtype_params'], sc.arrays['vtype_params'][:1]])      # one more vehicle type
    assert 'n_vtypes' in differs(scn_consts(vt))
    assert differs(scn_consts(sc, step_length=12)) == ['step_length']
