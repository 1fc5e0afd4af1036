"""The host emulation of the step kernel with the long paths' counters behind BatchedSim's API (TEST INFRASTRUCTURE).

tests/longpath_host/rs_emu_count.cpp is tests/hostemu/rs_emu.cpp, unchanged, compiled with resco_step.h's RS_COUNT hook defined, plus
rs_longpath_counts.  Never imported by resco_amd/."""
import ctypes as C
import os
import subprocess

from hostemu.emu import EmuSim
from resco_amd import sim as _sim

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBS = {False: os.path.join(_HERE, '_build', 'librs_emu_count.so'), True: os.path.join(_HERE, '_build', 'librs_emu_count_shortlists.so')}
_libs = {}

# the kinds, in the order of resco_step.h's enum RsCount
KINDS = ('walks entered', 'second hop', 'third hop', 'fourth hop and beyond', 'walks that used up RM_MAX_HOPS', 'end of route', 'dead end',
         'stop at red / yellow', 'red / yellow too close to stop', 'minor link beyond the visibility distance', 'foe check entered',
         'foe check blocked', 'foe record skipped as red', 'foe blocked by arrival gap', 'foe blocked by via-1 mover',
         'foe blocked by via-2 mover', 'leader on a next lane', 'look-ahead exhausted', 'strategic need', 'speed-gain candidate',
         'speed-gain candidate with a leader on its own lane', 'speed-gain candidate that wants the change', 'urgent',
         'follower found on the target lane', 'change decided', 'lead-request written', 'cooperation request written', 'swap decided')


def build():
    subprocess.check_call(['make', '-C', _HERE, '-s'], stdout=subprocess.DEVNULL)


def lib(short_lists=False):
    if short_lists not in _libs:
        build()
        L = _sim.bind(C.CDLL(_LIBS[short_lists]))
        L.rs_longpath_counts.restype = C.c_int
        L.rs_longpath_counts.argtypes = [C.POINTER(C.c_longlong), C.c_int]
        _libs[short_lists] = L
    return _libs[short_lists]


def take_counts(short_lists=False):
    """{kind: count} since the last call (the counters belong to the library, not to a handle), and clear them"""
    buf = (C.c_longlong * 64)()
    n = lib(short_lists).rs_longpath_counts(buf, 64)
    assert n == len(KINDS), (n, len(KINDS))
    return {k: int(buf[i]) for i, k in enumerate(KINDS)}


class CountEmuSim(EmuSim):
    """EmuSim on the counting library (short_lists=True: the build whose work lists hold 8 slots)"""

    def _load(self):
        return lib(self._short)
