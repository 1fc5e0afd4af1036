"""CPU: the two long paths of the plan phase -- the hop loop of phase_plan<true> with foe_blocked, and phase_lc_decide (resco_amd/csrc/
resco_step.h) -- against the oracle, bit for bit, WITH the condition that keeps the comparison from hiding a path: the host emulation is
built with the RS_COUNT hook of the kernel source defined (tests/longpath_host), and over the two runs together every kind of thing those
paths can do must have been counted at least once.

Shuffled thread order, bench mode (sigma -1, speed deviation on), seed 3, env_base 17, 2 environments; ingolstadt21 for 70 env-steps and
cologne3 for 50.  The counts of these runs (the same before and after the hop loop got its one exit and the target-lane leader searches of
phase_lc_decide were merged -- the kinds are the model's, not the code's):

    kind                                                    ingolstadt21 x 70   cologne3 x 50
    walks entered                                                      127172           21100
    second hop                                                          38978            1840
    third hop                                                            6967             284
    fourth hop and beyond                                                2942              14
    walks that used up RM_MAX_HOPS                                          5               0
    end of route                                                         1941            1841
    dead end                                                              344             185
    stop at red / yellow                                                37683            7328
    red / yellow too close to stop                                        256              19
    minor link beyond the visibility distance                            3135             807
    foe check entered                                                    3158             851
    foe check blocked                                                    1389             416
    foe record skipped as red                                            2094             497
    foe blocked by arrival gap                                            805             233
    foe blocked by via-1 mover                                            579             177
    foe blocked by via-2 mover                                              5               6
    leader on a next lane                                               37137            6284
    look-ahead exhausted                                                45538            4239
    strategic need                                                       4838             771
    speed-gain candidate                                                11499            3462
    ... with a leader on its own lane                                    4826            1951
    ... that wants the change                                             870             355
    urgent                                                               2255             444
    follower found on the target lane                                    2687             307
    change decided                                                       2237             680
    lead-request written                                                 2388             207
    cooperation request written                                          1746             114
    swap decided                                                            0               2

(The three verdicts of a foe record add up to "foe check blocked".  The swap is the thinnest kind: two in cologne3, none in ingolstadt21.)

The second case runs both maps on the build whose work lists hold 8 entries (what test_hostemu.py::test_work_lists_overflow does): the
lists overflow in most ticks and every thread runs the long paths on its own slots, the OTHER inlined copy of the same source.  Who runs a
vehicle's plan changes, what the plan does cannot: the counts must be those of the first case."""
import numpy as np
import pytest

from conftest import load_scenario
from oracle.pyoracle import OracleEnv
from longpath_host.emu import KINDS, CountEmuSim, take_counts
from test_hostemu import assert_equal

RUNS = (('ingolstadt21', 70), ('cologne3', 50))
_counts = {}


def run_against_oracle(name, steps, short_lists):
    sc = load_scenario(name)
    n, base = 2, 17
    take_counts(short_lists)
    sim = CountEmuSim(sc, n, order=2, short_lists=short_lists, seed=3, sigma=-1.0, speed_dev=1, env_base=base)
    orcs = [OracleEnv(sc, env_index=base + e, seed=3, sigma=-1.0, speed_dev=1) for e in range(n)]
    for o in orcs:
        o.observe()
    assert_equal(sim, orcs, -1)
    rng = np.random.default_rng(0)
    for step in range(steps):
        acts = np.stack([rng.integers(0, sc.tls_ngreen) for _ in range(n)]).astype(np.int32)
        sim.step(acts)
        for e, o in enumerate(orcs):
            o.step(acts[e])
        if step % 5 == 4 or step == steps - 1:
            assert_equal(sim, orcs, step)
    st = sim.stats()
    for e, o in enumerate(orcs):
        so = o.stats()
        for k in st:
            assert st[k][e] == so[k], (k, e)
    sim.close()
    return take_counts(short_lists)


def counts(short_lists):
    if short_lists not in _counts:
        _counts[short_lists] = {name: run_against_oracle(name, steps, short_lists) for name, steps in RUNS}
    return _counts[short_lists]


def check_every_kind(per_map):
    for kind in KINDS:
        print('%-56s' % kind, ''.join('%14d' % per_map[name][kind] for name, _ in RUNS))
    missing = [kind for kind in KINDS if sum(per_map[name][kind] for name, _ in RUNS) < 1]
    assert not missing, 'never taken, so never compared with the oracle: %s' % missing


def test_long_paths_equal_the_oracle_and_every_kind_is_taken():
    check_every_kind(counts(False))


def test_long_paths_on_the_overflow_path_of_the_work_lists():
    short = counts(True)
    check_every_kind(short)
    assert short == counts(False)
