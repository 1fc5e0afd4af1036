"""CPU: prioritised replay of the fused DQN update without a GPU -- the scalar pieces of resco_amd/csrc/resco_dqn_per.h through a host
build (tests/dqn_per_host) against numpy in float64 (the uniform from the counter hash, the beta schedule, the weight and the
priority of a row, the sequential restatement of the two-stage pick: zeros, a slot whose sum is 0, a value past the end); the Python
refusals, the signature rule, the tool's flag; the C ABI's new calls and struct."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from dqn_nstep_ref import valid_slots
from dqn_per_ref import PER_SEED, beta_at, pick_sequential, priorities, uniforms
from oracle_batch import murmur_hash
from resco_amd import sim as rsim
from resco_amd.agents.idqn_learn import PER_DEFAULTS, BatchedDQNLearner, per_options, per_options_signature
from resco_amd.agents.idqn_rollout import BatchedIDQN
from train_ref import _ulp, build_host

#         T  N    head count
RINGS = [(6, 5, 4, 4),          # not full: slots 4 and 5 were never written
         (6, 5, 2, 6),          # full and wrapped
         (8, 130, 3, 8),
         (8, 130, 0, 8),        # full, head at 0: the newest slot is the last
         (6, 130, 3, 3)]


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    vp, i32, u32, f32, f64, i64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_float, C.c_double, C.c_int64
    return build_host('dqn_per', tmp_path_factory.mktemp('dqn_per_host'), dict(
        dqn_per_host_seed_constant=([], u32), dqn_per_host_uniform=([u32] * 5, f32), dqn_per_host_beta=([f64, i64, i64], f32),
        dqn_per_host_priority=([f32] * 3, f32), dqn_per_host_row_weight=([f32] * 4, f32),
        dqn_per_host_pick=[vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, vp]))


def test_uniform_bit_for_bit(host):
    assert host.dqn_per_host_seed_constant() == PER_SEED
    seed = 0x5EED
    for u in (0, 1, 77, 2 ** 32 - 1):
        r0, r1 = uniforms(seed, u, 3, 40)
        for i in range(40):
            for s in range(3):
                for j, want in ((0, r0[i, s]), (1, r1[i, s])):
                    got = host.dqn_per_host_uniform(seed, u, s, i, j)
                    assert 0.0 <= got < 1.0 and float(got) == want, (u, i, s, j)
    # not the uniform draw's stream
    assert murmur_hash(seed ^ PER_SEED, 0, 0, 0, 0) != murmur_hash(seed, 0, 0, 0, 0)


def test_beta_schedule_bit_for_bit(host):
    for beta0 in (0.0, 0.4, 0.123456789, 1.0):
        for steps in (0, 1, 7, 1000, 10 ** 9):
            for u in (0, 1, 3, 6, 7, 8, 999, 1000, 10 ** 10):
                got = host.dqn_per_host_beta(beta0, steps, u)
                assert np.float32(got).tobytes() == beta_at(beta0, steps, u).tobytes(), (beta0, steps, u)
                assert beta0 - 1e-7 <= got <= 1.0
    assert host.dqn_per_host_beta(0.4, 0, 10 ** 6) == np.float32(0.4) and host.dqn_per_host_beta(0.4, 10, 10) == 1.0


def test_weight_and_priority_to_one_rounding(host):
    rng = np.random.default_rng(5)
    f = np.float32
    for _ in range(2000):
        q, Z, M, beta = f(np.exp(rng.uniform(-7, 5))), f(np.exp(rng.uniform(0, 12))), f(rng.integers(1, 2 ** 23)), f(rng.uniform(0, 1))
        x = f(f(M * q) / Z)                                 # the header's two float32 roundings before the power
        want = np.power(np.float64(x), -np.float64(beta))
        got = host.dqn_per_host_row_weight(q, Z, M, beta)
        assert abs(got - want) <= _ulp(want), (q, Z, M, beta, got, want)
        ad, eps, alpha = f(abs(rng.standard_normal()) * 3), f(1e-6), f(rng.uniform(0, 1))
        want = np.power(np.float64(f(ad + eps)), np.float64(alpha))
        got = host.dqn_per_host_priority(ad, eps, alpha)
        assert abs(got - want) <= _ulp(want), (ad, alpha, got, want)
    assert host.dqn_per_host_row_weight(0.0, 5.0, 10.0, 0.4) == 0.0 and host.dqn_per_host_row_weight(1.0, 0.0, 10.0, 0.4) == 0.0
    assert host.dqn_per_host_priority(2.0, 1e-6, 0.0) == 1.0 and host.dqn_per_host_priority(float('inf'), 1e-6, 0.5) == 0.0
    assert host.dqn_per_host_row_weight(3.0, 7.0, 11.0, 0.0) == 1.0


def _pick(host, prio, ssum, s, head, count, r0, r1):
    out = np.zeros(2, np.int32)
    T, N, S = prio.shape
    assert host.dqn_per_host_pick(prio.ctypes.data, ssum.ctypes.data, T, N, S, s, head, count, r0, r1, out.ctypes.data) == 0
    return int(out[0]), int(out[1])


@pytest.mark.parametrize('T,N,head,count', RINGS)
def test_sequential_pick_against_float64(host, T, N, head, count):
    """every pick lies where float64 puts it, up to 2 n 2^-24 Z (the worst case of ANY order of float32 summation of n non-negative
    terms, doubled); away from a boundary it IS float64's pick; no entry of weight 0, no slot of sum 0, neither the newest nor an
    unwritten slot is drawn"""
    prio = np.ascontiguousarray(priorities(T, N, head, count))
    ssum = prio.sum(1, dtype=np.float64).astype(np.float32)
    ok = valid_slots(T, head, count)
    if len(ok) > 1:
        assert (ssum[ok[len(ok) // 2]] == 0).all(), 'the case holds a slot whose sum is 0'
    rng = np.random.default_rng(T + N)
    clear = 0
    for _ in range(400):
        s = int(rng.integers(0, 3))
        r0, r1 = (np.float32(int(x) * 2.0 ** -24) for x in rng.integers(0, 2 ** 24, 2))
        t, e = _pick(host, prio, ssum, s, head, count, r0, r1)
        assert t in ok and ssum[t, s] > 0 and prio[t, e, s] > 0
        for w, k, r in ((ssum[ok, s].astype(np.float64), ok.index(t), r0), (prio[t, :, s].astype(np.float64), e, r1)):
            Cm = np.concatenate([[0.0], np.cumsum(w)])
            Z, tol = Cm[-1], 2 * len(w) * 2.0 ** -24 * Cm[-1]
            assert Cm[k] - tol <= r * Z <= Cm[k + 1] + tol, (t, e, s, r)
            if np.abs(Cm - r * Z).min() > tol:
                assert k == pick_sequential(w, r * Z)
                clear += 1
    assert clear > 400


def test_pick_past_the_end_takes_the_last_positive_entry(host):
    """a threshold no cumulative value exceeds (here: a sum that is larger than its leaves' total) gives the last entry of positive weight"""
    prio = np.zeros((3, 6, 1), np.float32)
    prio[0, :, 0] = [0, 1, 0, 2, 0, 0]
    prio[1, :, 0] = [0, 0, 0, 0, 0, 5]
    ssum = np.array([[4.0], [5.0], [0.0]], np.float32)         # slot 0: 4 > 3 = its leaves
    top = np.float32(1 - 2.0 ** -24)
    assert _pick(host, prio, ssum, 0, 2, 2, 0.0, top) == (0, 3)   # count 2: slot 0 alone is valid; 0.99.. x 4 > 3: past the end
    assert _pick(host, prio, ssum, 0, 2, 2, 0.0, 0.0) == (0, 1)   # threshold 0: the first POSITIVE entry, not entry 0
    assert _pick(host, prio, ssum, 0, 2, 2, 0.0, 0.5) == (0, 3)   # 2 < 0.5 x 4: not entry 1
    assert _pick(host, prio, ssum, 0, 0, 3, top, 0.0) == (1, 5)   # full ring at head 0: slots 0, 1 valid, 2 the newest
    assert _pick(host, prio, ssum, 0, 0, 3, 0.0, 0.0) == (0, 1)


def test_python_refusals_and_signature():
    net = BatchedIDQN((5, 3), (4, 2))
    net.init_like_reference(1)
    with pytest.raises(ValueError, match='no prioritised replay'):
        BatchedDQNLearner(net, per={})
    assert per_options(None, 'x') is None and per_options({}, 'x') == PER_DEFAULTS
    assert per_options(dict(alpha=1, beta_steps=7.0), 'x') == dict(PER_DEFAULTS, alpha=1.0, beta_steps=7)
    for bad, word in ((dict(alpha=1.5), 'alpha'), (dict(alpha=-0.1), 'alpha'), (dict(beta0=2), 'beta0'), (dict(eps=0), 'eps'), (dict(beta_steps=-1), 'beta_steps'),
                      (dict(gamma=1), 'unknown')):
        with pytest.raises(ValueError, match=word):
            per_options(bad, 'x')
    plain = {'batch': 4}
    assert per_options_signature(dict(plain), None) == plain, 'the keys are absent while off'
    assert per_options_signature(dict(plain), per_options({}, 'x')) == dict(plain, per_alpha=0.6, per_beta0=0.4, per_beta_steps=0, per_eps=1e-6)
    import inspect
    from resco_amd.agents.idqn_learn_fused import FusedDQNLearner
    assert 'per_options_signature' in inspect.getsource(FusedDQNLearner.signature)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        FusedDQNLearner(net, per={})


def test_training_tool_flag():
    from tools import idqn_train
    f = idqn_train.target_flags
    assert f(['--per', '--device-loop', 'cologne1']) == (dict(per=True), ['--device-loop', 'cologne1'])
    assert f(['--device-update', '--per', '0.5,0.3,100', '--n-step', '3', '64']) == (dict(per=(0.5, 0.3, 100), n_step=3), ['--device-update', '64'])
    assert f(['--per', '0.5,0.3']) == (dict(per=(0.5, 0.3)), [])
    assert f(['--per', '256']) == (dict(per=True), ['256']), 'a plain number is the next positional argument'
    assert f(['cologne1']) == ({}, ['cologne1'])
    for bad in (['--per', '1.5,0.3'], ['--per', '0.5,-1'], ['--per', '0.5,0.3,-2']):
        with pytest.raises(SystemExit):
            f(bad)
    with pytest.raises(SystemExit, match='--device-update'):
        idqn_train.main('cologne1', 2, 1, per=True)


def test_abi_declares_and_exports_prioritised_replay():
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for decl in (r'int rs_dqn_set_priorities\(rs_dqn_handle p, const rs_dqn_per \*per\);',
                 r'int rs_dqn_get_priorities\(rs_dqn_handle p, rs_dqn_per \*out, int32_t \*on\);',
                 r'int rs_dqn_per_rebuild\(rs_dqn_handle p, void \*stream\);',
                 r'int rs_dqn_per_fill\(rs_dqn_handle p, int32_t slot, void \*stream\);',
                 r'int rs_dqn_per_commit\(rs_dqn_handle p, const rs_dqn_ring \*ring, const int32_t \*idx, int32_t batch, void \*stream\);'):
        assert re.search(decl, text), decl
    body = text[text.index('typedef struct rs_dqn_per {') + len('typedef struct rs_dqn_per {'):text.index('} rs_dqn_per;')]
    names = [n.strip().lstrip('*') for d in body.split(';') if d.strip() for n in re.sub(r'^\s*(float|int32_t|double|int64_t)\s*', '', d.strip()).split(',')]
    assert [f[0] for f in rsim.DQNPer._fields_] == names and C.sizeof(rsim.DQNPer) == 3 * 8 + 2 * 4 + 3 * 8 + 8
    # rs_dqn_ring and rs_train keep their size
    from resco_amd._abi import TrainStruct
    assert C.sizeof(rsim.DQNRing) == 4 * 8 + 4 * 4 and C.sizeof(TrainStruct) == 136
    from resco_amd.build import build_library
    build_library()
    L = rsim.load_library()
    for name in ('rs_dqn_set_priorities', 'rs_dqn_get_priorities', 'rs_dqn_per_rebuild', 'rs_dqn_per_fill', 'rs_dqn_per_commit'):
        assert name in rsim.ABI_SYMBOLS and hasattr(L, name), name
    # a NULL handle is refused with a text before anything touches a device
    per, on = rsim.DQNPer(), C.c_int32(7)
    assert L.rs_dqn_set_priorities(None, C.byref(per)) == -1 and b'rs_dqn_set_priorities' in L.rs_last_error(None)
    assert L.rs_dqn_get_priorities(None, C.byref(per), C.byref(on)) == -1 and on.value == 7
    assert L.rs_dqn_per_rebuild(None, None) == -1 and b'rs_dqn_per_rebuild' in L.rs_last_error(None)
    assert L.rs_dqn_per_fill(None, 0, None) == -1 and b'rs_dqn_per_fill' in L.rs_last_error(None)
    assert L.rs_dqn_per_commit(None, None, None, 1, None) == -1 and b'rs_dqn_per_commit' in L.rs_last_error(None)
