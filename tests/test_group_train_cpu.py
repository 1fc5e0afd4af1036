"""CPU: the launch-free pieces of the in-library DQN training loop (resco_amd/csrc/resco_group_train.h) through a host build of the
same header (tests/group_train_host): the pack's analytic fragment index against idqn_fused.repack_index and its values against
pack_idqn_weights, the recorder's and the target sync's bodies against numpy, the per-step bookkeeping against a Python restatement
of the tools' --device-update loop, and the C ABI of the loop (header, ABI_SYMBOLS, exports, the rs_train mirror)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from resco_amd import sim as rsim
from resco_amd._abi import TrainStruct
from resco_amd.agents.idqn_fused import pack_idqn_weights, repack_index
from resco_amd.agents.idqn_learn import linear_epsilon
from resco_amd.agents.idqn_rollout import BatchedIDQN
from train_ref import build_host

TRAIN_CALLS = ['rs_dqn_sync_target', 'rs_group_train', 'rs_idqn_pack_weights', 'rs_mplight_dqn_sync_target']


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    return build_host('group_train', tmp_path_factory.mktemp('group_train_host'), dict(
        gt_host_pack_index=[i32, i32, i32, vp], gt_host_pack=[i32, i32, i32] + [vp] * 8 + [i32], gt_host_f2h=([C.c_float], C.c_uint16),
        gt_host_record=[vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, i32, i32], gt_host_sync=[vp, vp, i64, i32],
        gt_host_plan=[i32, i64, i32, i32, i32, i64, i32, i32, i32, f64, f64, i32, i32, vp]))


def ptr(a):
    return a.ctypes.data if a is not None else None


# ---------------------------------------------------------------------------------------------------------------- the pack
@pytest.mark.parametrize('lmax', range(2, 18))
def test_pack_index_equals_repack_index(host, lmax):
    for amax in range(1, 9):
        want = repack_index(lmax, amax)
        for which, key in enumerate(('w1', 'w2', 'w3')):
            got = np.full(len(want[key]) + 1, -7, np.int32)
            assert host.gt_host_pack_index(which, lmax, amax, ptr(got)) == len(want[key]), (key, amax)
            assert np.array_equal(got[:-1], want[key]) and got[-1] == -7, (key, lmax, amax)


def test_half_conversion_rounds_to_nearest_even(host):
    """the host's restatement of the conversion (the device uses its convert instruction) against numpy's astype: ties, the
    denormal range, overflow, both signs"""
    rng = np.random.default_rng(3)
    bits = np.concatenate([rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32),
                           np.arange(0x38000000, 0x38000000 + 0x6000, 0x800, dtype=np.uint32),      # around the first normal half
                           np.arange(0x33000000 - 4, 0x33000000 + 4, dtype=np.uint32),                # around 2^-25
                           np.arange(0x477FE000 - 0x2000, 0x477FE000 + 0x3000, 0x800, dtype=np.uint32),
                           (np.float16(np.arange(1, 2048)).astype(np.float32) * np.float32(2.0 ** -24)).view(np.uint32)])
    x = bits.view(np.float32)
    x = x[~np.isnan(x)]
    x = np.concatenate([x, -x, (x.view(np.uint32) + 0x1000).view(np.float32), (x.view(np.uint32) | 0x1000).view(np.float32)])
    x = x[~np.isnan(x)]
    with np.errstate(over='ignore'):
        want = x.astype(np.float16).view(np.uint16)
    got = np.array([host.gt_host_f2h(float(v)) for v in x], np.uint16)
    assert np.array_equal(got, want)


@pytest.mark.parametrize('lanes,actions', [([2], [1]), ([5, 3], [4, 2]), ([17, 8, 4], [8, 3, 5]), ([9, 9], [2, 2])])
def test_pack_values_equal_pack_idqn_weights(host, lanes, actions):
    torch.manual_seed(len(lanes) * 100 + lanes[0])
    net = BatchedIDQN(lanes, actions, dtype=torch.float32)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn_like(p) * 0.37)
    want = pack_idqn_weights(net)
    S, lmax, amax = len(lanes), net.lmax, net.amax
    f = lambda t: np.ascontiguousarray(t.detach().numpy(), np.float32)
    src = [f(net.fc1_w), f(net.fc2_w), f(net.fc3_w), f(net.fc3_b)]
    guard = 64
    out = [np.full(want[k].size + guard, 0x7B7B, np.uint16) for k in ('w1', 'w2', 'w3')] + [np.full(S * 32 + guard, 7.5, np.float32)]
    for threads in (1, 7, 256):
        assert host.gt_host_pack(S, lmax, amax, *[ptr(a) for a in src], *[ptr(a) for a in out], threads) > 0
        for k, o in zip(('w1', 'w2', 'w3'), out):
            assert np.array_equal(o[:-guard].view(np.float16), want[k].reshape(-1)), k
            assert (o[-guard:] == 0x7B7B).all(), 'written behind ' + k
        assert np.array_equal(out[3][:-guard].reshape(S, 32), want['b3']) and (out[3][-guard:] == 7.5).all()


# ---------------------------------------------------------------------------------------------------------------- the recorder
def _aligned(n_bytes, offset):
    """a uint8 view of n_bytes whose address is `offset` past a 16-byte boundary, inside a buffer with 32 guard bytes either side"""
    raw = np.full(n_bytes + 96, 0xA5, np.uint8)
    start = (-raw.ctypes.data) % 16 + 32 + offset
    return raw, raw[start:start + n_bytes]


@pytest.mark.parametrize('kind,n', [(0, 85), (0, 5 * 85), (0, 8), (0, 7), (0, 1003), (1, 13), (1, 5 * 13), (1, 64), (2, 49), (2, 3 * 49), (2, 4)])
@pytest.mark.parametrize('so,do', [(0, 0), (0, 6), (10, 0), (2, 2), (4, 12)])
def test_recorder_observation_copies(host, kind, n, so, do):
    """f16 copy, int32 -> f32, f32 copy: aligned bases (the 16-byte path with its tail) and unaligned ones, sizes that are not
    multiples of 8 halfs / 4 words; nothing is written outside the destination"""
    esz = 2 if kind == 0 else 4
    so, do = so // esz * esz, do // esz * esz
    rng = np.random.default_rng(n * 31 + kind)
    raw_s, src = _aligned(n * esz, so)
    raw_d, dst = _aligned(n * esz, do)
    if kind == 0:
        val = rng.standard_normal(n).astype(np.float16)
        want = val.view(np.uint8)
    elif kind == 1:
        val = rng.integers(-3000, 3000, n).astype(np.int32)
        want = val.astype(np.float32).view(np.uint8)
    else:
        val = rng.standard_normal(n).astype(np.float32)
        want = val.view(np.uint8)
    src[:] = val.view(np.uint8)
    vec = int(src.ctypes.data % 16 == 0 and dst.ctypes.data % 16 == 0)
    for threads in (1, 3, 64):
        raw_d[:] = 0xA5
        assert host.gt_host_record(src.ctypes.data, dst.ctypes.data, n, kind, vec, None, None, None, None, None, 0, 0, None, 0, threads) == 0
        assert np.array_equal(dst, want)
        outside = np.ones(len(raw_d), bool)
        off = dst.ctypes.data - raw_d.ctypes.data
        outside[off:off + n * esz] = False
        assert (raw_d[outside] == 0xA5).all()
    if vec:     # the element path gives the same
        raw_d[:] = 0xA5
        assert host.gt_host_record(src.ctypes.data, dst.ctypes.data, n, kind, 0, None, None, None, None, None, 0, 0, None, 0, 5) == 0
        assert np.array_equal(dst, want)


@pytest.mark.parametrize('rew_i32', [0, 1])
@pytest.mark.parametrize('n_sig', [1, 5, 21 * 3, 257])
def test_recorder_transition(host, rew_i32, n_sig):
    rng = np.random.default_rng(n_sig + rew_i32)
    act = rng.integers(0, 16, n_sig).astype(np.int32)
    rew = rng.integers(-500, 1, n_sig).astype(np.int32) if rew_i32 else rng.standard_normal(n_sig).astype(np.float32)
    ret0 = rng.standard_normal(n_sig).astype(np.float32)
    for with_ret in (False, True):
        for done in (0, 1):
            a_out, r_out, ret, d_out = np.full(n_sig + 1, -9, np.int16), np.full(n_sig + 1, -9, np.float32), ret0.copy(), np.full(3, 9, np.uint8)
            assert host.gt_host_record(None, None, 0, 0, 0, ptr(act), ptr(a_out), ptr(rew), ptr(r_out), ptr(ret) if with_ret else None, n_sig, rew_i32,
                                       d_out[1:].ctypes.data, done, 4) == 0
            assert np.array_equal(a_out[:-1], act.astype(np.int16)) and a_out[-1] == -9
            assert np.array_equal(r_out[:-1], rew.astype(np.float32)) and r_out[-1] == -9
            assert np.array_equal(ret, ret0 + rew.astype(np.float32) if with_ret else ret0)
            assert list(d_out) == [9, done, 9]
    # the first pipe alone writes done: a NULL destination leaves it
    assert host.gt_host_record(None, None, 0, 0, 0, ptr(act), ptr(a_out), ptr(rew), ptr(r_out), None, n_sig, rew_i32, None, 1, 2) == 0


@pytest.mark.parametrize('n,so,do', [(1, 0, 0), (1365, 0, 0), (1365, 4, 0), (1413, 8, 8), (4096, 0, 0), (3, 12, 4)])
def test_target_sync_copy(host, n, so, do):
    rng = np.random.default_rng(n)
    raw_s, src = _aligned(n * 4, so)
    raw_d, dst = _aligned(n * 4, do)
    val = rng.standard_normal(n).astype(np.float32)
    src[:] = val.view(np.uint8)
    for threads in (1, 5, 256):
        raw_d[:] = 0xA5
        assert host.gt_host_sync(src.ctypes.data, dst.ctypes.data, n, threads) == 0
        assert np.array_equal(dst.view(np.float32), val)
        assert (raw_d == 0xA5).sum() >= len(raw_d) - n * 4 - 8 and (raw_d[:32] == 0xA5).all() and (raw_d[-32:] == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------------- the bookkeeping
def python_loop(capacity, pool, batch, target_update, updates, t, head, count, n_steps, horizon_left, eps, decay):
    """what the tools' --device-update loops decide per step: DeviceReplay / MPLightReplay.commit's position, len(replay), the
    learners' observe_step, linear_epsilon.  horizon_left: steps until the episode's last one (done is set there)"""
    out = []
    for k in range(n_steps):
        e = np.float32(linear_epsilon(t, eps[0], eps[1], decay))       # c_float(python float): one rounding
        slot = head
        done = int(k == horizon_left)
        head = (slot + 1) % capacity
        count = min(count + 1, capacity)
        key = t & 0xFFFFFFFF
        t += 1
        sync = int(t % target_update == 0)
        update = int(max(0, count - 1) * pool >= batch and updates >= 1)
        out.append((slot, head, count, sync, update, done, key, int(e.view(np.uint32))))
    return out, t, head, count


def plans(host, capacity, pool, batch, target_update, updates, t0, head, count, done_step, eps, decay, n_steps):
    out = np.zeros((n_steps, 8), np.uint32)
    assert host.gt_host_plan(capacity, pool, batch, target_update, updates, t0, head, count, done_step, eps[0], eps[1], decay, n_steps, ptr(out)) == 0
    return [tuple(int(v) for v in row) for row in out]


def test_step_plan_equals_the_python_loop_for_any_split(host):
    rng = np.random.default_rng(11)
    cases = [(2, 1, 1, 1, 1, 0, 0, 0, 9), (8, 16, 32, 7, 1, 0, 0, 0, 20), (8, 8 * 21, 32, 7, 1, 13, 5, 8, 20), (3, 4, 100, 2, 2, 5, 2, 3, 11)]
    for _ in range(60):
        capacity = int(rng.integers(2, 40))
        count = int(rng.integers(0, capacity + 1))
        cases.append((capacity, int(rng.integers(1, 400)), int(rng.integers(1, 300)), int(rng.integers(1, 30)), int(rng.integers(0, 3)),
                      int(rng.integers(0, 5000)), int(rng.integers(0, capacity)), count, int(rng.integers(1, 80))))
    seen = dict(wrap=0, saturate=0, sync=0, update=0, idle=0)
    for capacity, pool, batch, target_update, updates, t0, head, count, n_steps in cases:
        eps, decay = (1.0, float(rng.choice([0.0, 0.05]))), int(rng.choice([0, 1, 37, 1000, 7001]))
        want, _, head_end, count_end = python_loop(capacity, pool, batch, target_update, updates, t0, head, count, n_steps, n_steps - 1, eps, decay)
        got = plans(host, capacity, pool, batch, target_update, updates, t0, head, count, n_steps - 1, eps, decay, n_steps)
        assert got == want, (capacity, pool, batch, target_update, updates, t0, head, count, n_steps)
        assert (got[-1][1], got[-1][2]) == (head_end, count_end)
        seen['wrap'] += any(g[1] == 0 for g in got)
        seen['saturate'] += count < capacity and got[-1][2] == capacity
        seen['sync'] += any(g[3] for g in got)
        seen['update'] += any(g[4] for g in got)
        seen['idle'] += any(not g[4] for g in got)
        # any split of the same steps into calls: each call starts where the caller's advance left the position
        for _ in range(3):
            cuts = sorted(set(rng.integers(1, n_steps, min(n_steps - 1, int(rng.integers(0, 5)))).tolist())) if n_steps > 1 else []
            pieces, t, h, c, start = [], t0, head, count, 0
            for end in cuts + [n_steps]:
                n = end - start
                done_step = n_steps - 1 - start if start <= n_steps - 1 < end else -1
                pieces += plans(host, capacity, pool, batch, target_update, updates, t, h, c, done_step, eps, decay, n)
                t, h, c, start = t + n, (h + n) % capacity, min(c + n, capacity), end
            assert pieces == want, (cuts, capacity, n_steps)
    assert all(v > 3 for v in seen.values()), seen


def test_epsilon_bits(host):
    """float32 bits of the schedule at and around its corners, for the decays the tools use"""
    for decay in (0, 1, 16, 288, 1152, 8640, 10 ** 6):
        for end in (0.0, 0.05, 0.01):
            ts = sorted(set([0, 1, 2, 3, 5, 7, max(decay - 1, 0), decay, decay + 1, decay // 2, decay // 3, 2 * decay + 1]))
            for t in ts:
                got = plans(host, 4, 1, 1, 1, 1, t, 0, 0, -1, (1.0, end), decay, 1)[0][7]
                assert got == int(np.float32(linear_epsilon(t, 1.0, end, decay)).view(np.uint32)), (decay, end, t)


# ---------------------------------------------------------------------------------------------------------------- the ABI
def _header():
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        return f.read()


def test_train_calls_are_declared_bound_and_exported():
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(rs_[a-z_]+)\s*\(', text)))
    for s in TRAIN_CALLS:
        assert s in declared and s in rsim.ABI_SYMBOLS, s
    from resco_amd.build import build_library
    build_library()
    L = rsim.load_library()
    for s in TRAIN_CALLS:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert len(L.rs_group_train.argtypes) == 4 and len(L.rs_idqn_pack_weights.argtypes) == 3


def test_train_struct_matches_header():
    """rs_train: the mirror lists the header's fields in header order with the header's types, and has no padding"""
    text = _header()
    body = text[text.index('typedef struct rs_train {') + len('typedef struct rs_train {'):text.index('} rs_train;')]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    ctype = {'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'int64_t': C.c_int64, 'double': C.c_double}
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r'^(const\s+)?(\w+)\s+(.*)$', decl)
        base, names = m.group(2), [n.strip() for n in m.group(3).split(',')]
        for n in names:
            pointer = n.startswith('*') or base == 'rs_policy_handle'
            fields.append((n.lstrip('*'), C.c_void_p if pointer else ctype[base]))
    assert TrainStruct._fields_ == fields
    assert C.sizeof(TrainStruct) == sum(C.sizeof(t) for _, t in fields) == 136
    for s in TRAIN_CALLS:
        assert s in re.sub(r'/\*.*?\*/', '', text, flags=re.S)
