"""CPU: the launch-free pieces of the in-library PPO training loop (resco_amd/csrc/resco_ppo_loop.h and the actor-critic pack of
resco_group_train.h) through a host build of the same headers (tests/ppo_loop_host): the shuffle is a bijection, deterministic and
marginally uniform; the pack's analytic index against ippo_fused.ippo_repack_index and its values against pack_ippo_weights; the
per-step bookkeeping against a Python restatement of tools/ippo_train.py's loop; and the C ABI of the loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from resco_amd import sim as rsim
from resco_amd._abi import PPOTrainStruct, RolloutStruct
from resco_amd.agents.idqn_fused import repack_index
from resco_amd.agents.ippo import BatchedIPPO
from resco_amd.agents.ippo_fused import ippo_repack_index, pack_ippo_weights
from train_ref import build_host

LOOP_CALLS = ['rs_group_ppo_train', 'rs_ippo_pack_weights', 'rs_ppo_perm']
SEEDS = (0, 0xC0FFEE11)


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    vp, i32, u32, i64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_int64
    return build_host('ppo_loop', tmp_path_factory.mktemp('ppo_loop_host'), dict(
        gp_host_hash=([u32] * 5, u32), gp_host_half_bits=[i32], gp_host_perm=[i32, i32, u32, u32, vp, i32], gp_host_done=[vp, i32, i32, i32],
        gp_host_plan=[i32, i32, i32, i64, i64, i32, vp], gp_host_pack_index=[i32, i32, i32, i32, vp], gp_host_pack_value=[i32, i32, i32] + [vp] * 10 + [i32]))


def ptr(a):
    return a.ctypes.data if a is not None else None


def perm(host, n, epochs, seed, key, threads=1):
    out = np.full(epochs * n + 1, -7, np.int32)
    assert host.gp_host_perm(n, epochs, seed, key, ptr(out), threads) == 0
    assert out[-1] == -7, 'written behind the rows'
    return out[:-1].reshape(epochs, n)


# ---------------------------------------------------------------------------------------------------------------- the shuffle
def test_host_hash_is_the_projects_counter_hash(host):
    rng = np.random.default_rng(5)
    for w in rng.integers(0, 2 ** 32, (50, 5), dtype=np.uint64).tolist() + [[0] * 5, [0xFFFFFFFF] * 5]:
        assert host.gp_host_hash(*w) == rsim._murmur(w[0], w[1:])


def test_domain_is_below_four_n(host):
    for n in list(range(1, 301)) + [1000, 7680, 30720, 2 ** 20, 2 ** 20 + 1, 2 ** 31 - 1]:
        h = host.gp_host_half_bits(n)
        assert 1 <= h <= 16 and n <= 4 ** h and (4 ** h < 4 * n or n == 1)


@pytest.mark.parametrize('seed', SEEDS)
def test_permutation_is_a_bijection(host, seed):
    for n in list(range(1, 301)) + [1000, 7680, 30720]:
        p = perm(host, n, 3, seed, 9)
        assert np.array_equal(np.sort(p, axis=1), np.broadcast_to(np.arange(n, dtype=np.int32), (3, n))), n
    assert perm(host, 1, 3, seed, 0).tolist() == [[0]] * 3


def test_permutation_is_deterministic_and_keyed(host):
    for n in (8, 9, 65, 96, 1000):
        a = perm(host, n, 3, SEEDS[1], 4)
        assert np.array_equal(a, perm(host, n, 3, SEEDS[1], 4, threads=7))                # a pure function: any grid, any order
        assert np.array_equal(a[:2], perm(host, n, 2, SEEDS[1], 4))                         # row e does not depend on the number of epochs
        assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2]) and not np.array_equal(a[0], a[2])
        assert not np.array_equal(a, perm(host, n, 3, SEEDS[1], 5)) and not np.array_equal(a, perm(host, n, 3, SEEDS[0], 4))
        assert not any(np.array_equal(r, np.arange(n)) for r in a)


def test_marginal_uniformity(host):
    """n = 8, epoch 0, one seed, update keys 0 .. 4095: every (position, value) count is a binomial(4096, 1/8) under a uniform
    shuffle, mean 512, standard deviation sqrt(4096 / 8 * 7 / 8) = 21.2; 512 +- 128 is six of them.  Fixed keys: deterministic."""
    counts = np.zeros((8, 8), np.int64)
    for key in range(4096):
        counts[np.arange(8), perm(host, 8, 1, SEEDS[1], key)[0]] += 1
    print(counts)
    assert counts.sum() == 8 * 4096 and (np.abs(counts - 512) <= 128).all(), counts


def test_done_bytes(host):
    for m, hit in [(1, 0), (6, -1), (6, 5), (6, 6), (300, 257), (5, -3)]:
        d = np.full(m + 2, 9, np.uint8)
        for threads in (1, 4, 256):
            assert host.gp_host_done(d[1:].ctypes.data, m, hit, threads) == 0
            assert d[0] == 9 and d[-1] == 9 and d[1:-1].tolist() == [int(j == hit) for j in range(m)]


# ---------------------------------------------------------------------------------------------------------------- the pack
@pytest.mark.parametrize('lmax', range(2, 18))
def test_pack_index_equals_ippo_repack_index(host, lmax):
    for amax in range(1, 9):
        for value, want in ((1, ippo_repack_index(lmax, amax)), (0, repack_index(lmax, amax))):
            for which, key in enumerate(('w1', 'w2', 'w3')):
                got = np.full(len(want[key]) + 1, -7, np.int32)
                assert host.gp_host_pack_index(value, which, lmax, amax, ptr(got)) == len(want[key]), (key, amax)
                assert np.array_equal(got[:-1], want[key]) and got[-1] == -7, (value, key, lmax, amax)


@pytest.mark.parametrize('lanes,actions', [([2], [1]), ([5, 3], [4, 2]), ([17, 8, 4], [8, 3, 5]), ([9, 9], [2, 2])])
def test_pack_values_equal_pack_ippo_weights(host, lanes, actions):
    torch.manual_seed(len(lanes) * 100 + lanes[0])
    net = BatchedIPPO(lanes, actions, dtype=torch.float32)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn_like(p) * 0.37)
        net.v_w[0, 3, 0], net.v_w[0, 4, 0], net.v_b[0, 0] = 2.0 ** -25 * 1.5, 70000.0, -3.25      # half a denormal's step; infinity in f16
    with np.errstate(over='ignore'):
        want = pack_ippo_weights(net)
    S, lmax, amax = len(lanes), net.lmax, net.amax
    f = lambda t: np.ascontiguousarray(t.detach().numpy(), np.float32)
    src = [f(net.fc1_w), f(net.fc2_w), f(net.fc3_w), f(net.fc3_b), f(net.v_w), f(net.v_b)]
    guard = 64
    out = [np.full(want[k].size + guard, 0x7B7B, np.uint16) for k in ('w1', 'w2', 'w3')] + [np.full(S * 32 + guard, 7.5, np.float32)]
    for threads in (1, 7, 256):
        assert host.gp_host_pack_value(S, lmax, amax, *[ptr(a) for a in src], *[ptr(a) for a in out], threads) > 0
        for k, o in zip(('w1', 'w2', 'w3'), out):
            assert np.array_equal(o[:-guard], want[k].reshape(-1).view(np.uint16)), k
            assert (o[-guard:] == 0x7B7B).all(), 'written behind ' + k
        assert np.array_equal(out[3][:-guard].reshape(S, 32), want['b3']) and (out[3][-guard:] == 7.5).all()
    w3 = out[2][:-guard].view(np.float16).reshape(S, 8, 64, 4)
    assert np.isinf(w3).sum() == 1 and want['b3'][0, 8] == -3.25 and (want['b3'][:, amax:8] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- the bookkeeping
def python_loop(T, steps, episodes):
    """what the loop of tools/ippo_train.py main_device_rollout decides per env-step: the slot, done at the episode's last step, the
    update after the step that fills the segment, its shuffle's key (updates so far), the step's key"""
    out, i, t_global, updates = [], 0, 0, 0
    for _ in range(episodes):
        for k in range(steps):
            slot, key, done = i, t_global & 0xFFFFFFFF, int(k == steps - 1)
            i, t_global = i + 1, t_global + 1
            update = int(i == T)
            out.append((slot, done, update, updates & 0xFFFFFFFF, key))
            if update:
                updates, i = updates + 1, 0
    return out


def plans(host, T, slot0, done_step, t0, update0, n_steps):
    out = np.zeros((n_steps, 5), np.uint32)
    assert host.gp_host_plan(T, slot0, done_step, t0, update0, n_steps, ptr(out)) == 0
    return [tuple(int(v) for v in row) for row in out]


@pytest.mark.parametrize('split', [(20,), (7, 13), (1,) * 20])
@pytest.mark.parametrize('T', [6, 1, 7, 20, 30])
def test_step_plan_equals_the_python_loop_for_any_split(host, split, T):
    """two episodes of 20 steps; T = 6: the fourth segment spans the reset; 1: an update every step; 30: a segment longer than an episode"""
    steps = 20
    want = python_loop(T, steps, 2)
    got, slot, t, updates = [], 0, 0, 0
    for _ in range(2):
        left = steps
        for c in split:
            got += plans(host, T, slot, c - 1 if c == left else -1, t, updates, c)
            updates, slot, t, left = updates + (slot + c) // T, (slot + c) % T, t + c, left - c
        assert left == 0
    assert got == want
    if T == 6:
        assert sum(g[2] for g in got) == 6 and got[19][0] == 1 and got[19][1] == 1       # the fourth segment spans the reset


def test_keys_wrap_to_32_bits(host):
    p = plans(host, 4, 3, -1, 2 ** 32 - 1, 2 ** 33 + 5, 2)
    assert p == [(3, 0, 1, 5, 0xFFFFFFFF), (0, 0, 0, 6, 0)]


# ---------------------------------------------------------------------------------------------------------------- the ABI
def _header():
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        return f.read()


def test_loop_calls_are_declared_bound_and_exported():
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(rs_[a-z_]+)\s*\(', text)))
    for s in LOOP_CALLS:
        assert s in declared and s in rsim.ABI_SYMBOLS, s
    from resco_amd.build import build_library
    build_library()
    L = rsim.load_library()
    for s in LOOP_CALLS:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert len(L.rs_group_ppo_train.argtypes) == 4 and len(L.rs_ippo_pack_weights.argtypes) == 3 and len(L.rs_ppo_perm.argtypes) == 6


def test_ppo_train_struct_matches_header():
    """rs_ppo_train: the mirror lists the header's fields in header order with the header's types, and has no padding of its own"""
    text = _header()
    body = text[text.index('typedef struct rs_ppo_train {') + len('typedef struct rs_ppo_train {'):text.index('} rs_ppo_train;')]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    ctype = {'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'int64_t': C.c_int64, 'float': C.c_float, 'rs_rollout': RolloutStruct}
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r'^(const\s+)?(\w+)\s+(.*)$', decl)
        base, names = m.group(2), [n.strip() for n in m.group(3).split(',')]
        for n in names:
            pointer = n.startswith('*') or base in ('rs_policy_handle', 'rs_ppo_handle')
            fields.append((n.lstrip('*'), C.c_void_p if pointer else ctype[base]))
    assert PPOTrainStruct._fields_ == fields
    assert C.sizeof(PPOTrainStruct) == sum(C.sizeof(t) for _, t in fields) == 168
    assert rsim.Rollout is RolloutStruct


def test_python_side_is_there():
    from resco_amd.agents.ippo_learn_fused import FusedPPOLearner
    from resco_amd.agents.train_fused import DevicePPOTrainer
    import inspect
    assert 'perm' in inspect.signature(FusedPPOLearner.update_from_rollout).parameters and hasattr(FusedPPOLearner, 'device_perm')
    assert inspect.signature(FusedPPOLearner.update_from_rollout).parameters['perm'].default is None
    assert callable(DevicePPOTrainer.run) and hasattr(rsim.SimGroup, 'ppo_train')
