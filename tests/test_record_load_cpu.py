"""CPU: the whole-record loads of the scenario tables (resco_amd/csrc/resco_tables.h: rec_load16, rec_load8, link_load) through
tests/record_load_host/record_load_host.cpp, a program of its own built with -fsanitize=address,undefined: for every record type
and exactly sized heap arrays of 1, 2 and 3 records the helper returns the bytes of the struct copy and reads nothing outside the
array.  The -DRS_FIELD_LOADS flavour (plain struct copies) goes through the same program, and a control build that reads 16 bytes
of an 8-byte record shows that the sanitizer would catch it."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'record_load_host', 'record_load_host.cpp')
RECORDS = 6          # LaneRec, FoeRec, RouteRec, LinkRec, RStep, DepInfo
CHECKED = RECORDS * (1 + 2 + 3)


def build(out_dir, name, *defines):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
                           '-static-libasan', '-static-libubsan',      # (the runtimes inside the program: it needs nothing of its environment)
                           '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'resco_amd', 'csrc')] + list(defines) + [SRC, '-o', exe])
    return exe


def run(exe, *args):
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


@pytest.fixture(scope='module')
def out_dir(tmp_path_factory):
    return tmp_path_factory.mktemp('record_load_host')


@pytest.mark.parametrize('mode,defines', [('whole', ()), ('field', ('-DRS_FIELD_LOADS',))])
def test_helpers_equal_the_struct_copy_and_stay_inside_the_array(out_dir, mode, defines):
    exe = build(out_dir, 'record_load_' + mode, *defines)
    for seed in ('1', '0xC0FFEE11', '2654435769'):
        r = run(exe, seed)
        print(r.stdout, r.stderr[-3000:])
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout.strip().splitlines()[-1] == 'record_load_host %s: %d records checked, 0 failed' % (mode, CHECKED)
        assert 'ERROR' not in r.stderr and 'runtime error' not in r.stderr


def test_control_the_sanitizer_sees_a_wide_read_of_the_last_record(out_dir):
    r = run(build(out_dir, 'record_load_overread', '-DRECORD_LOAD_OVERREAD'))
    # (whichever of the two sanitizers meets the read first reports it: the address check or the object-size check)
    assert r.returncode != 0 and ('heap-buffer-overflow' in r.stderr or 'insufficient space' in r.stderr), (r.returncode, r.stderr[-2000:])
