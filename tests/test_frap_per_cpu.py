"""CPU: prioritised replay of the fused MPLight update without a GPU -- the draw's uniforms against the oracle's counter hash; the
three-stage pick (dqn_per_pick_seq applied three times, tests/frap_per_host) against float64; THE order of the sums restated in numpy
against the sequential pick; the Python refusals, the signature rule and the tools' flags; the C ABI's five calls and the struct's
layout against a compiled sizeof / offsetof; the weighted row loss inside whole minibatches on the host against float64 autograd of
the weighted loss (tests/frap_per_ref.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import frap_nstep_ref as fn
import frap_per_ref as fp
import frap_train_ref as ft
from conftest import ROOT
from resco_amd import sim as rsim
from resco_amd.agents.idqn_learn import PER_DEFAULTS
from resco_amd.agents.mplight import MPLightLearner

CALLS = ['rs_mplight_dqn_set_priorities', 'rs_mplight_dqn_get_priorities', 'rs_mplight_dqn_per_rebuild', 'rs_mplight_dqn_per_fill',
         'rs_mplight_dqn_per_commit']
IDS = ['P%d-D%d-T%d-B%d-n%d-dq%d' % (s[0], s[1], s[2], s[5], s[8], s[9]) for s in fn.SHAPES]
#         T  N    S   head count
RINGS = [(4, 4, 2, 0, 4),           # the smallest
         (6, 5, 3, 4, 4),           # not full: slots 4 and 5 were never written
         (6, 5, 3, 2, 6),           # full and wrapped
         (8, 130, 3, 0, 8),         # the environment level crosses two chunk boundaries with a ragged end; head at 0
         (6, 3, 70, 3, 6),          # the signal level crosses a chunk
         (70, 2, 2, 5, 70)]         # the slot level crosses a chunk


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return fp.build_frap_per_host(tmp_path_factory.mktemp('frap_per_host'))


# ------------------------------------------------------------------------------------------------------------ 1. the uniforms
def test_uniforms_bit_for_bit(host):
    seed = 0x5EED
    for u in (0, 1, 77, 2 ** 32 - 1):
        want, other = fp.uniforms(seed, u, 40), fp.uniform_draw_values(seed, u, 40)
        for i in range(40):
            for j in range(3):
                got = host.frap_per_host_uniform(seed, u, i, j)
                assert 0.0 <= got < 1.0 and float(got) == want[i, j], (u, i, j)
        assert (want != other).all(), 'the uniform draw\'s stream'


# --------------------------------------------------------------------------------------------------------------- 2. the pick
def _pick(host, prio, esum, ssum, head, count, r):
    out = np.zeros(3, np.int32)
    T, N, S = prio.shape
    assert host.frap_per_host_pick(prio.ctypes.data, esum.ctypes.data, ssum.ctypes.data, T, N, S, head, count, r[0], r[1], r[2], out.ctypes.data) == 0
    return tuple(int(x) for x in out)


def _zero_patterns(prio, T, head, count):
    """the patterns the case must hold: one valid slot all zero, one environment of another valid slot all zero, positive values in
    the newest and the unwritten slots"""
    ok = fn.valid_slots(T, head, count)
    if len(ok) > 1:
        assert any((prio[t] == 0).all() for t in ok)
        assert any((prio[t, e] == 0).all() and (prio[t] > 0).any() for t in ok for e in range(prio.shape[1]))
    assert all((prio[t] > 0).all() for t in range(T) if t not in ok)
    assert abs((prio[ok] == 0).mean() - 1 / 3) < 0.3


@pytest.mark.parametrize('T,N,S,head,count', RINGS)
def test_three_stage_sequential_pick_against_float64(host, T, N, S, head, count):
    """every pick lies where float64 puts it up to 2 n 2^-24 times the level's total (the worst case of ANY float32 summation order of
    n non-negative terms, doubled); away from a boundary it IS float64's pick; never drawn: an entry of weight 0, the newest slot, an
    unwritten slot"""
    prio = np.ascontiguousarray(fp.priorities(T, N, S, head, count))
    _zero_patterns(prio, T, head, count)
    esum = prio.sum(2, dtype=np.float64).astype(np.float32)
    ssum = esum.sum(1, dtype=np.float64).astype(np.float32)
    ok = fn.valid_slots(T, head, count)
    rng = np.random.default_rng(T + N + S)
    clear = 0
    for _ in range(300):
        r = [np.float32(int(x) * 2.0 ** -24) for x in rng.integers(0, 2 ** 24, 3)]
        t, e, s = _pick(host, prio, esum, ssum, head, count, r)
        assert t in ok and ssum[t] > 0 and esum[t, e] > 0 and prio[t, e, s] > 0
        for w, k, rr in ((ssum[ok].astype(np.float64), ok.index(t), r[0]), (esum[t].astype(np.float64), e, r[1]), (prio[t, e].astype(np.float64), s, r[2])):
            Cm = np.concatenate([[0.0], np.cumsum(w)])
            Z, tol = Cm[-1], 2 * len(w) * 2.0 ** -24 * Cm[-1]
            assert Cm[k] - tol <= rr * Z <= Cm[k + 1] + tol, (t, e, s, rr)
            if np.abs(Cm - rr * Z).min() > tol:
                assert k == fp.pick_sequential(w, rr * Z)
                clear += 1
    assert clear > 600


@pytest.mark.parametrize('T,N,S,head,count', RINGS)
def test_the_scan_order_agrees_with_the_sequential_pick_away_from_boundaries(host, T, N, S, head, count):
    """the numpy restatement of THE order (chunked Hillis-Steele) that the device test compares bit for bit: its sums are within
    n 2^-24 of float64, and its draw is the sequential one's wherever no level sits at a boundary"""
    prio = np.ascontiguousarray(fp.priorities(T, N, S, head, count))
    esum, ssum = fp.sums(prio)
    e64 = prio.sum(2, dtype=np.float64)
    assert (np.abs(esum - e64) <= S * 2.0 ** -24 * e64).all() and ((esum == 0) == (e64 == 0)).all()
    s64 = esum.sum(1, dtype=np.float64)
    assert (np.abs(ssum - s64) <= N * 2.0 ** -24 * s64).all() and ((ssum == 0) == (s64 == 0)).all()
    idx = fp.draw(prio, esum, ssum, head, count, 0x5EED, 3, 33)
    ft.check_sample(idx, T, N, S, head, count)
    r = fp.uniforms(0x5EED, 3, 33).astype(np.float32)
    same = sum(tuple(idx[i]) == _pick(host, prio, esum, ssum, head, count, r[i]) for i in range(33))
    assert same >= 30, same
    assert (prio[idx[:, 0], idx[:, 1], idx[:, 2]] > 0).all()


def test_pick_past_the_end_takes_the_last_positive_entry(host):
    prio = np.zeros((3, 2, 6), np.float32)
    prio[0, 1] = [0, 1, 0, 2, 0, 0]
    esum = np.array([[0, 4], [0, 0], [0, 0]], np.float32)       # (0, 1): 4 > 3 = its leaves
    ssum = np.array([4, 0, 0], np.float32)
    top = np.float32(1 - 2.0 ** -24)
    assert _pick(host, prio, esum, ssum, 2, 2, (0.0, 0.0, top)) == (0, 1, 3)    # 0.99.. x 4 > 3: past the end
    assert _pick(host, prio, esum, ssum, 2, 2, (0.0, 0.0, 0.0)) == (0, 1, 1)    # threshold 0: the first POSITIVE entry
    assert _pick(host, prio, esum, ssum, 0, 3, (top, top, 0.5)) == (0, 1, 3)    # slot 1 is valid but has sum 0; 2 < 0.5 x 4
    assert fp.pick(prio[0, 1], np.float32(top * 4)) == 3 and fp.pick(prio[0, 0], 0.0) == 0


# ----------------------------------------------------------------------------------------------------------- 3. the Python side
def test_python_refusals_and_signature():
    from resco_amd.agents.mplight_learn_fused import FusedMPLightLearner
    c = fn.ring_case(*(fn.SHAPES[0][:5] + fn.SHAPES[0][6:]))
    with pytest.raises(ValueError, match='prioritised replay'):
        MPLightLearner(c['net'], per={})
    for bad, word in ((dict(alpha=1.5), 'alpha'), (dict(beta0=2), 'beta0'), (dict(eps=0), 'eps'), (dict(beta_steps=-1), 'beta_steps'), (dict(gamma=1), 'unknown')):
        with pytest.raises(ValueError, match=word):
            FusedMPLightLearner(c['net'], per=bad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        FusedMPLightLearner(c['net'], per={})
    assert 'per_options_signature' in inspect.getsource(FusedMPLightLearner.signature)
    assert FusedMPLightLearner.STATE_FOLLOWS_REPLAY is True
    assert 'per' in inspect.signature(FusedMPLightLearner.__init__).parameters
    assert PER_DEFAULTS == dict(alpha=0.6, beta0=0.4, beta_steps=0, eps=1e-6)


def test_tools_flags():
    from tools import mplight_multimap_train, mplight_train
    f = mplight_train.target_flags
    assert f(['--per', '--device-loop', 'cologne1']) == (dict(per=True), ['--device-loop', 'cologne1'])
    assert f(['--device-update', '--per', '0.5,0.3,100', '64']) == (dict(per=(0.5, 0.3, 100)), ['--device-update', '64'])
    with pytest.raises(SystemExit, match='--per needs --device-update or --device-loop'):
        mplight_train.main('cologne1', 2, 1, per=True)
    with pytest.raises(SystemExit, match='--per'):
        mplight_multimap_train.main(('cologne1',), (2,), 1, per=True)


# --------------------------------------------------------------------------------------------------------------------- 4. the ABI
def test_abi_declares_and_exports_prioritised_replay(host):
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for decl in (r'int rs_mplight_dqn_set_priorities\(rs_mplight_dqn_handle p, const rs_mplight_per \*per\);',
                 r'int rs_mplight_dqn_get_priorities\(rs_mplight_dqn_handle p, rs_mplight_per \*out, int32_t \*on\);',
                 r'int rs_mplight_dqn_per_rebuild\(rs_mplight_dqn_handle p, void \*stream\);',
                 r'int rs_mplight_dqn_per_fill\(rs_mplight_dqn_handle p, int32_t slot, void \*stream\);',
                 r'int rs_mplight_dqn_per_commit\(rs_mplight_dqn_handle p, const rs_mplight_ring \*ring, const int32_t \*idx, int32_t batch, void \*stream\);'):
        assert re.search(decl, text), decl
    names = ['prio', 'esum', 'ssum', 'pmax', 'capacity', 'n_envs', 'n_signals', 'alpha', 'beta0', 'eps', 'beta_steps']
    assert [f[0] for f in rsim.MPLightPer._fields_] == names
    layout = np.zeros(12, np.int64)
    host.frap_per_host_layout(layout.ctypes.data)
    assert C.sizeof(rsim.MPLightPer) == layout[0]
    assert [getattr(rsim.MPLightPer, k).offset for k in names] == layout[1:].tolist()
    assert C.sizeof(rsim.MPLightRing) == 4 * 8 + 6 * 4, 'rs_mplight_ring keeps its size'
    from resco_amd.build import build_library
    build_library()
    L = rsim.load_library()
    for name in CALLS:
        assert name in rsim.ABI_SYMBOLS and hasattr(L, name), name
    # a NULL handle is refused with a text before anything touches a device
    per, on = rsim.MPLightPer(), C.c_int32(7)
    assert L.rs_mplight_dqn_set_priorities(None, C.byref(per)) == -1 and b'rs_mplight_dqn_set_priorities' in L.rs_last_error(None)
    assert L.rs_mplight_dqn_get_priorities(None, C.byref(per), C.byref(on)) == -1 and on.value == 7
    assert L.rs_mplight_dqn_per_rebuild(None, None) == -1 and b'rs_mplight_dqn_per_rebuild' in L.rs_last_error(None)
    assert L.rs_mplight_dqn_per_fill(None, 0, None) == -1 and b'rs_mplight_dqn_per_fill' in L.rs_last_error(None)
    assert L.rs_mplight_dqn_per_commit(None, None, None, 1, None) == -1 and b'rs_mplight_dqn_per_commit' in L.rs_last_error(None)


# --------------------------------------------------------------------------------------------- 5. the weighted gradient on the host
@pytest.mark.parametrize('shape', fn.SHAPES, ids=IDS)
def test_host_weighted_gradient(host, shape):
    """the PER phases over a whole minibatch on the host, on a ring whose forbidden places hold NaN: gradient and loss within 4 e_ref of
    the weighted float64 truth, |delta| the truth's rounded to fp32 within 1 ulp32"""
    P, D, T, N, S, B, head, count, n_step, dq, done_slots = shape
    c = fn.ring_case(P, D, T, N, S, head, count, n_step, dq, tuple(done_slots))
    idx, prio, w64, g64, e_ref, l64, e_loss, d64 = fp.reference(shape)      # (asserts the conditions on the references alone)
    w32 = fp.weights(prio, idx, head, count, 0.4, np.float32)
    assert np.abs(w32 - w64).max() <= 8 * 2.0 ** -24
    got, loss, ad = fp.host_grads(host, c, idx, w32)
    print(shape)
    worst = ft.compare(ft.names_of(c['net']), got, loss, g64, e_ref, l64, e_loss, who='host')
    assert not worst, worst
    want = np.abs(d64).astype(np.float32)
    assert (np.abs(ad.astype(np.float64) - want) <= ft.ulp32(want)).all(), np.abs(ad - want).max()
    assert all(np.abs(got[k]).max() > 0 for k in got if np.abs(g64[k]).max() > 0)
