"""CPU: bench.py's plain run (the headline figure only) against its --full run, and --dump-outputs, on the host emulation of the kernel
(tests/hostemu) standing in for the HIP library."""
import numpy as np

from conftest import load_scenario
from hostemu.emu import EmuSim

STEPS, WARMUP, SEED = 8, 2, 5
STATE = ('veh_pos', 'veh_speed', 'veh_lane', 'veh_trip', 'tls', 'stats', 'mplight', 'drq_norm', 'phase', 'wait', 'wait_norm', 'actions')


def _pipes(sc, n=2, per=2):
    sims = [EmuSim(sc, per, seed=SEED, env_base=i * per) for i in range(n)]
    for s in sims:
        s.set_outputs(('drq_norm', 'mplight'))
    return sims


def test_plain_run_times_exactly_k_steps_and_computes_what_full_computes():
    """run_timed(extras=False) -- what a plain `bench.py` run does -- times exactly K steps (the barriers that bracket the timed region
    see K x 10 ticks between them), skips the all-outputs steps, the issue probe and the per-launch events, and leaves every environment in
    the state a --full run (extras, 20 all-outputs steps) leaves it in"""
    import bench
    sc = load_scenario('cologne1')
    full, plain = _pipes(sc), _pipes(sc)
    bench.run_timed(full, STEPS, WARMUP, lambda: None, lambda: None, lambda x: x, all_outputs_steps=20)
    ticks_at_barrier = []
    r = bench.run_timed(plain, STEPS, WARMUP, lambda: ticks_at_barrier.append(plain[0].stats()['ticks'].copy()), lambda: None,
                        lambda x: x, all_outputs_steps=0, extras=False)
    elapsed, kernel_ms, launches, st0, st1, all_out_rate, n_all, elapsed_local, issue_s = r
    assert len(ticks_at_barrier) == 2 and (ticks_at_barrier[1] - ticks_at_barrier[0] == STEPS * 10).all()
    assert elapsed > 0 and (kernel_ms, launches, st0, st1, all_out_rate, n_all, issue_s) == (0.0, 0, None, None, None, 0, None)
    w0 = bench.window_start(STEPS, WARMUP)
    for s in plain:
        assert (s.stats()['ticks'] == (w0 + STEPS) * 10).all()
    for name in STATE:
        np.testing.assert_array_equal(np.concatenate([s.read(name) for s in plain]), np.concatenate([s.read(name) for s in full]),
                                      err_msg=name)


def test_dump_outputs_writes_what_the_last_step_computed(tmp_path):
    """--dump-outputs: one DIR/<name>.npy per output of the timed path, float32 as it is and integers as float64, the pipes'
    environments in global order; above the size limit a seeded sample of the environments (the same in every run) with its indices"""
    import bench
    sc = load_scenario('cologne1')
    sims = _pipes(sc)
    for k in range(3):
        for s in sims:
            s.act_random(k)
            s.step(None)
    names = bench.dump_outputs(sims, str(tmp_path / 'all'))
    assert names == sorted(bench.DUMP_BUFFERS)
    for name in bench.DUMP_BUFFERS:
        a = np.load(str(tmp_path / 'all' / (name + '.npy')))
        want = np.concatenate([s.read(name) for s in sims])
        assert a.dtype == (np.float32 if want.dtype == np.float32 else np.float64), name
        assert a.shape == want.shape and a.shape[0] == 4
        np.testing.assert_array_equal(a, want.astype(a.dtype), err_msg=name)
    assert np.load(str(tmp_path / 'all' / 'drq_norm.npy')).any() and np.load(str(tmp_path / 'all' / 'actions.npy')).any()

    limit = sum(np.load(str(tmp_path / 'all' / (n + '.npy'))).nbytes for n in names) // 2
    for d in ('s1', 's2'):
        names = bench.dump_outputs(sims, str(tmp_path / d), limit=limit)
        assert 'env_index' in names
        assert sum(np.load(str(tmp_path / d / (n + '.npy'))).nbytes for n in names) <= limit
    idx = np.load(str(tmp_path / 's1' / 'env_index.npy'))
    assert idx.dtype == np.float64 and 0 < len(idx) < 4 and (np.diff(idx) > 0).all()
    for name in names:
        a, b = np.load(str(tmp_path / 's1' / (name + '.npy'))), np.load(str(tmp_path / 's2' / (name + '.npy')))
        np.testing.assert_array_equal(a, b, err_msg=name)
        if name != 'env_index':
            np.testing.assert_array_equal(a, np.load(str(tmp_path / 'all' / (name + '.npy')))[idx.astype(np.int64)], err_msg=name)
