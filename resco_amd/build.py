"""Build the HIP shared library in-tree (resco_amd/csrc/libresco_sim.so) for gfx950."""
import ctypes
import glob
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'csrc', 'resco_sim.hip')
LIB = os.path.join(HERE, 'csrc', 'libresco_sim.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
# what the build generates before the HIP compile (kept out of git): the host-only library that computes a scenario's handle constants
# and the header that holds them as literals, one struct per shipped map (resco_step.h: ScnConsts, KTabFix, LdsScn)
GEN_DIR = os.path.join(HERE, 'csrc', '_gen')
SCN_SRC = os.path.join(HERE, 'csrc', 'resco_scn_consts.cpp')
SCN_LIB = os.path.join(GEN_DIR, 'libresco_scn_consts.so')
SCN_HEADER = os.path.join(GEN_DIR, 'resco_scn_fix.h')
SCENARIO_DIR = os.path.join(HERE, 'scenarios')
CXX = os.environ.get('CXX', 'g++')
# -ffp-contract=off: fp32 results must equal the CPU oracle bit-for-bit (no FMA fusion).  The fp32-pair sums of resco_train.h
#   (ppo_pair_add and the helpers after it: two-sum, fmaf product errors) are exact only with it and without fast-math: a contracted
#   or re-associated `(hi - (s - bb)) + (x - bb)` is zero.  Keep it (tests/test_ppo_train_cpu.py and test_gpu_ppo_train.py notice).
# -disable-machine-licm: the step kernel's tick loop is long and register-starved (80 VGPRs for three workgroups per CU); with
#   machine LICM every 32-bit literal of the loop body is hoisted into a VGPR of its own and five values end up in scratch,
#   written per thread and tick: 110 MB of HBM writes per launch at 4096 environments and 2.5 % of the time (profiles/r03_*)
# -fno-honor-nans: no NaN exists in the model; with the flag the `x < y ? x : y` selects become v_min_f32 / v_max_f32 instead of v_cmp +
#   v_cndmask pairs (and the s_nop the pair needs on gfx950): +0.6-0.9 % (profiles/r06_ab_linkrec_nnan.txt); results bit-identical
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fno-honor-nans', '-mllvm', '-disable-machine-licm', '-fPIC', '-shared',
         '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(HERE, 'csrc'), '-I' + GEN_DIR]
_HDRS = [os.path.join(HERE, 'csrc', f) for f in ('resco_host.h', 'resco_step.h', 'resco_tables.h')] + \
        [os.path.join(ROOT, 'include', f) for f in ('resco_sim.h', 'resco_model.h')]
_DEPS = [SRC] + _HDRS + [os.path.join(HERE, 'csrc', f) for f in ('resco_policy.h', 'resco_frap.h', 'resco_fma2c.h', 'resco_fma2c_train.h', 'resco_ppo.h', 'resco_train.h', 'resco_ppo_train.h', 'resco_dqn_train.h', 'resco_dqn_per.h', 'resco_frap_train.h', 'resco_frap_per.h', 'resco_frap_multi.h', 'resco_group_train.h', 'resco_ppo_loop.h', 'resco_fma2c_loop.h')]


def _newer(target, deps):
    return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps)


def _replace(path, write):
    """write a file under a temporary name and rename it into place: processes that build at the same time never read half a file"""
    tmp = '%s.%d.tmp' % (path, os.getpid())
    write(tmp)
    os.replace(tmp, path)


def build_scn_consts_library(force=False):
    """The host-only library (g++, no device code) that exports rs_scn_consts: the constants rs_create derives from a scenario."""
    if not force and _newer(SCN_LIB, [SCN_SRC] + _HDRS):
        return SCN_LIB
    os.makedirs(GEN_DIR, exist_ok=True)
    _replace(SCN_LIB, lambda tmp: subprocess.check_call(
        [CXX, '-O1', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(HERE, 'csrc'),
         SCN_SRC, '-o', tmp, '-lm']))
    return SCN_LIB


def scn_consts(scenario, lib=None, **pack):
    """rs_scn_consts of a loaded Scenario as an ordered dict {member of ScnConsts: 32-bit value}; `lib`: any library that exports
    rs_scn_consts and rs_scn_const_names (default: the host-only one); pack: step_length / yellow_length as BatchedSim takes them."""
    from ._abi import pack_scenario
    L = ctypes.CDLL(lib or build_scn_consts_library())
    L.rs_scn_const_names.restype = ctypes.c_char_p
    names = L.rs_scn_const_names().decode().split(',')
    st, keep = pack_scenario(scenario, **pack)
    out = (ctypes.c_uint32 * len(names))()
    L.rs_scn_consts.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    rc = L.rs_scn_consts(ctypes.byref(st), out)
    del keep
    if rc != 0:
        raise RuntimeError('rs_scn_consts failed (%d)' % rc)
    signed = lambda n, v: v - (1 << 32) if v >= (1 << 31) and not (n.startswith('o_') or n.endswith('_bits')) else v
    return {n: signed(n, int(v)) for n, v in zip(names, out)}


def shipped_maps():
    """(map name, path) of every shipped scenario whose name can be a C++ identifier"""
    out = []
    for path in sorted(glob.glob(os.path.join(SCENARIO_DIR, '*.npz'))):
        name = os.path.splitext(os.path.basename(path))[0]
        if re.fullmatch(r'[A-Za-z][A-Za-z0-9_]*', name):
            out.append((name, path))
    return out


def scn_fix_text(consts_by_map):
    """the generated header: one struct of literals per map (floats as bit patterns) and the X-macro that lists the maps"""
    lines = ['// GENERATED by resco_amd/build.py from resco_amd/scenarios/*.npz (rs_scn_consts of every shipped map) -- not in git, do not edit.',
             '// One struct per map: the members of ScnConsts (resco_step.h) as literals; RS_SCN_MAPS lists the maps.', '#pragma once', '#include <stdint.h>']
    for name, consts in consts_by_map.items():
        lines.append('struct ScnFix_%s {' % name)
        for k, v in consts.items():
            if k.startswith('o_') or k.endswith('_bits') or v < 0:
                lines.append('    static constexpr %s %s = %s;' % ('int32_t' if v < 0 else 'uint32_t', k, v if v < 0 else '0x%08xu' % v))
            else:
                lines.append('    static constexpr int32_t %s = %d;' % (k, v))
        lines.append('};')
    lines.append('#define RS_SCN_MAPS(X)' + ''.join(' X(%s)' % name for name in consts_by_map))
    return '\n'.join(lines) + '\n'


def generate_scn_header(verbose=False):
    """Write the generated header (only when its inputs are newer than it, and then only when its text changes: the library is rebuilt
    when the header is newer).  A map whose constants
    cannot be produced is left out with a message; handles of that map run the generic step kernel."""
    from .scenario import Scenario
    maps = shipped_maps()
    # nothing to do while the header is newer than everything its text follows from: the scenarios, the constants source and its headers,
    # and the Python that packs a scenario and writes the text (a process that only wants the library pays a few stat calls)
    inputs = [SCN_SRC] + _HDRS + [path for _, path in maps] + [os.path.join(HERE, f) for f in ('build.py', '_abi.py', 'scenario.py')]
    if _newer(SCN_HEADER, inputs) and _newer(SCN_LIB, [SCN_SRC] + _HDRS):
        return SCN_HEADER
    consts = {}
    try:
        lib = build_scn_consts_library()
    except (OSError, subprocess.CalledProcessError) as e:       # no constants at all: every handle runs the generic step kernel
        print('resco_amd.build: no specialised step kernels, the host-only constants library did not build: %s' % e)
        lib, maps = None, []
    for name, path in maps:
        try:
            consts[name] = scn_consts(Scenario.load(path), lib)
        except Exception as e:      # noqa: BLE001 -- any failure costs this map its specialised kernel, never the build
            print('resco_amd.build: no specialised step kernel for %s: %s' % (name, e))
    text = scn_fix_text(consts)
    old = None
    if os.path.exists(SCN_HEADER):
        with open(SCN_HEADER) as f:
            old = f.read()
    if text != old:
        def write(tmp):
            with open(tmp, 'w') as f:
                f.write(text)
        os.makedirs(GEN_DIR, exist_ok=True)
        _replace(SCN_HEADER, write)
    elif not _newer(LIB, [SCN_HEADER]):
        os.utime(SCN_HEADER)        # same text, and the library has to be rebuilt anyway: the next call takes the short way
    if verbose:
        print('%s: %s' % (SCN_HEADER, ' '.join(consts) or '(no map)'))
    return SCN_HEADER


def build_library(force=False, verbose=False):
    force = force or os.environ.get('GRAFT_FORCE_BUILD') == '1'
    header = generate_scn_header(verbose)
    if not force and _newer(LIB, _DEPS + [header]):
        return LIB
    cmd = [HIPCC] + FLAGS + [SRC, '-o', LIB]
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd)
    return LIB


CHECK_LIB = os.path.join(HERE, 'csrc', 'libresco_sim_check.so')


def build_check_library(force=False):
    """The CHECKING build: the step kernel's classification invariants (RS_ASSERT) counted on the device instead of compiled out
    (rs_stats()[11]); one capacity (256 slots: cologne8, ingolstadt7, cologne3) so that it compiles in seconds.  Test infrastructure
    of tests/test_gpu_parity.py::test_device_invariant_counter -- never loaded by the package."""
    force = force or os.environ.get('GRAFT_FORCE_BUILD') == '1'
    if not force and os.path.exists(CHECK_LIB) and all(os.path.getmtime(CHECK_LIB) >= os.path.getmtime(d) for d in _DEPS):
        return CHECK_LIB
    subprocess.check_call([HIPCC] + FLAGS + ['-DRS_DEVICE_ASSERT', '-DRS_ONE_CAP=256', SRC, '-o', CHECK_LIB])
    return CHECK_LIB


FIELDLOADS_LIB = os.path.join(HERE, 'csrc', 'libresco_sim_fieldloads.so')


def build_fieldloads_library(force=False):
    """The FIELD-LOADS build: -DRS_FIELD_LOADS turns the whole-record loads of the table records (resco_tables.h: rec_load16, link_load,
    rec_load8) back into plain struct copies, which the compiler reads field by field -- the step kernel as it was before the helpers,
    instruction for instruction.  One capacity (256 slots) so that it compiles in seconds.  The other side of
    tests/test_gpu_record_loads.py (both builds must give the same bits) -- never loaded by the package.  Rebuilt when a source is
    newer than it, or with force=True."""
    if not force and os.path.exists(FIELDLOADS_LIB) and all(os.path.getmtime(FIELDLOADS_LIB) >= os.path.getmtime(d) for d in _DEPS):
        return FIELDLOADS_LIB
    subprocess.check_call([HIPCC] + FLAGS + ['-DRS_FIELD_LOADS', '-DRS_ONE_CAP=256', SRC, '-o', FIELDLOADS_LIB])
    return FIELDLOADS_LIB


if __name__ == '__main__':
    print(build_library(force=True, verbose=True))
