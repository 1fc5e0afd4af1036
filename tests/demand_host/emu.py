"""The host emulation of the step kernel with per-environment demand behind BatchedSim's API (TEST INFRASTRUCTURE).

tests/demand_host/rs_emu_demand.cpp is tests/hostemu/rs_emu.cpp, unchanged, plus rs_set_demand / rs_demand_info; the product's ctypes
wrapper (BatchedSim.set_demand / clear_demand) drives it as it drives the HIP library.  Never imported by resco_amd/."""
import ctypes as C
import os
import subprocess

from hostemu.emu import EmuSim
from resco_amd import sim as _sim

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, '_build', 'librs_emu_demand.so')
SRC = os.path.join(_HERE, 'rs_emu_demand.cpp')
_lib = None


def build():
    subprocess.check_call(['make', '-C', _HERE, '-s'], stdout=subprocess.DEVNULL)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        _lib = _sim.bind(C.CDLL(build()))
    return _lib


class DemandEmuSim(EmuSim):
    """EmuSim on the library that also exports rs_set_demand"""

    def _load(self):
        return lib()
