"""CPU: the multi-map MPLight update (resco_amd/csrc/resco_frap_multi.h) before it meets a GPU -- the host build of its draw and of its
grouped gradient (tests/frap_multi_host) against the Python restatement of the draw and the yardstick of tests/frap_multi_ref.py, the
restated hash against the project's, the C ABI (header, ABI_SYMBOLS, exports, struct mirror), and the checkpoint loader that takes
FRAP weights across maps."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import frap_multi_ref as fm
import frap_train_ref as ft
from conftest import ROOT
from resco_amd import checkpoint
from resco_amd import sim as rsim
from resco_amd.agents.mplight import FRAP

CALLS = ['rs_mplight_multi_create', 'rs_mplight_multi_destroy', 'rs_mplight_multi_grad', 'rs_mplight_multi_sample', 'rs_mplight_multi_set_steps',
         'rs_mplight_multi_step', 'rs_mplight_multi_steps', 'rs_mplight_multi_sync_target', 'rs_mplight_multi_update']


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return fm.build_frap_multi_host(tmp_path_factory.mktemp('frap_multi_host'))


def test_restated_hash_is_the_counter_hash(host):
    """frap_multi_hash (host and device) against d_hash as the host builds restate it and against resco_amd/sim.py's"""
    rng = np.random.default_rng(3)
    assert host.frap_multi_max_maps() == fm.MAX_MAPS
    for _ in range(200):
        seed, a, b, c, d = (int(x) for x in rng.integers(0, 2 ** 32, 5))
        h = host.frap_multi_hash_of(seed, a, b, c, d)
        assert h == host.frap_multi_d_hash_of(seed, a, b, c, d) == rsim._murmur(seed, (a, b, c, d))


@pytest.mark.parametrize('rings', fm.RING_SETS)
def test_host_sample_is_the_rule(host, rings):
    """B = 33 (one chunk) and 700 (three chunks of the sampler, the last ragged): idx and counts equal the restatement; grouped,
    stable, every group a valid draw of its ring; a ring with count < 2 never drawn"""
    for B in (33, 700):
        for u in (0, 1, 77):
            rc, idx, counts = fm.host_sample(host, 0x5EED, u, rings, B)
            want, want_counts = fm.predict_sample(0x5EED, u, rings, B)
            assert rc == 0 and counts == want_counts and np.array_equal(idx, want)
            fm.check_grouped(idx, counts, rings)
    assert [c > 0 for c in counts] == [r[4] >= 2 for r in rings], 'at B = 700 every ring with a transition is drawn from, no other'


def test_draw_is_uniform_over_the_pooled_transitions(host):
    """the share of a map is its pool's share of the total (the property the rule exists for), within 5 sigma of a binomial"""
    rings = fm.RING_SETS[0]
    cum = fm.pools_of(rings)
    B = 20000
    _, _, counts = fm.host_sample(host, 11, 5, rings, B)
    for m, c in enumerate(counts):
        p = (cum[m + 1] - cum[m]) / cum[-1]
        assert abs(c - B * p) <= 5 * np.sqrt(B * p * (1 - p)), (m, c, B * p)


def test_host_sample_refuses(host):
    assert fm.host_sample(host, 1, 0, [(6, 3, 1, 1, 1), (5, 2, 2, 0, 0)], 8)[0] == -1          # total == 0
    assert fm.host_sample(host, 1, 0, [(6, 3, 1, 6, 5)], 8)[0] == -1                            # head outside the ring
    assert fm.host_sample(host, 1, 0, [(3, 2 ** 15, 2 ** 15, 0, 3)], 8)[0] == -1                # a pool of 2^31
    assert fm.host_sample(host, 1, 0, [(6, 3, 1, 2, 5)] * 9, 8)[0] == -1                        # nine maps


@pytest.mark.parametrize('D,maps,counts', fm.CASES)
def test_host_multi_gradient(host, D, maps, counts):
    cases = fm.map_cases(D, maps)
    idx, g64, e_ref, l64, e_loss = fm.reference(D, maps, counts)
    got, loss = fm.host_grads(host, cases, idx, counts)
    print('D %d maps %s counts %s' % (D, maps, counts))
    worst = ft.compare(ft.names_of(cases[0]['net']), got, loss, g64, e_ref, l64, e_loss, who='host')
    assert not worst, worst
    wrong = idx.copy()
    wrong[:, 0] = (wrong[:, 0] + 1) % len(maps)             # the tag is not read: the group decides
    again, loss2 = fm.host_grads(host, cases, wrong, counts)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got) and loss == loss2


def test_one_map_is_the_single_map_gradient(host, tmp_path):
    """n_maps = 1: frap_multi_grad equals frap_train_grad on the same rows bit for bit"""
    single = ft.build_frap_train_host(tmp_path)
    P, D, T, N, S, B = 5, 4, 5, 6, 3, 11
    c = ft.case(P, D, T, N, S)
    idx = ft.draw_idx(c, B)
    want, wloss = ft.host_grads(single, c, idx)
    got, loss = fm.host_grads(host, [c], np.concatenate((np.zeros((B, 1), np.int32), idx), -1), [B])
    assert all(want[k].tobytes() == got[k].tobytes() for k in want) and np.float32(wloss).tobytes() == np.float32(loss).tobytes()


def test_abi_of_the_multi_map_update():
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        text = f.read()
    declared = set(re.findall(r'\b(rs_[a-z_]+)\s*\(', re.sub(r'/\*.*?\*/', '', text, flags=re.S)))
    from resco_amd.build import build_library
    build_library()
    L = rsim.load_library()
    assert sorted(s for s in declared if s.startswith('rs_mplight_multi_')) == CALLS
    for name in CALLS:
        assert name in rsim.ABI_SYMBOLS and hasattr(L, name), name
    body = text[text.index('typedef struct rs_mplight_map {') + len('typedef struct rs_mplight_map {'):text.index('} rs_mplight_map;')]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [re.sub(r'^(const\s+)?int32_t\s*\*?', '', d.strip()) for d in body.split(';') if d.strip()]
    assert [f[0] for f in rsim.MPLightMap._fields_] == names and C.sizeof(rsim.MPLightMap) == 24


def _frap(P, D, seed):
    rng = np.random.default_rng(P)
    import frap_ref as fr
    return fr.make_net(fr.synthetic_signal_set(P, 2, rng)[0], D, seed=seed)


def test_checkpoint_loader_accepts_across_pairs_and_refuses_across_demand_shape(tmp_path):
    src = _frap(9, 1, seed=5)
    path = str(tmp_path / 'single.pt')
    checkpoint.save(path, agent='MPLight', map_name='cologne8', objects=dict(net=src), progress=dict(episode=3, rows=[{'episode': 2}]))
    dst = _frap(4, 1, seed=6)
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    with pytest.raises(ValueError, match='oshape'):         # the existing loader refuses across P, and stays as it is
        checkpoint.load(path, agent='MPLight', map_name='cologne8', objects=dict(net=dst), strict=False)
    assert all(torch.equal(before[k], v) for k, v in dst.state_dict().items())
    progress = checkpoint.load_frap_weights(path, dst)
    assert progress['episode'] == 3
    assert all(torch.equal(src.state_dict()[k], v) for k, v in dst.state_dict().items())
    assert isinstance(dst, FRAP) and dst.oshape == 4
    # a multi-map checkpoint names its networks net0, net1, ..
    multi = str(tmp_path / 'multi.pt')
    checkpoint.save(multi, agent='MPLightMulti', map_name='a+b', objects=dict(net0=src, net1=_frap(3, 1, seed=5)), progress=dict(episode=1, rows=[]))
    dst13 = _frap(13, 1, seed=7)
    checkpoint.load_frap_weights(multi, dst13)
    assert all(torch.equal(src.state_dict()[k], v) for k, v in dst13.state_dict().items())
    # across demand_shape, another agent's file, a file without a network: refused, nothing written
    full = _frap(4, 4, seed=8)
    before = {k: v.clone() for k, v in full.state_dict().items()}
    with pytest.raises(ValueError, match='demand_shape'):
        checkpoint.load_frap_weights(path, full)
    other = str(tmp_path / 'idqn.pt')
    checkpoint.save(other, agent='IDQN', map_name='cologne8', objects=dict(net=src), progress={})
    with pytest.raises(ValueError, match='agent'):
        checkpoint.load_frap_weights(other, dst)
    bare = str(tmp_path / 'bare.pt')
    checkpoint.save(bare, agent='MPLight', map_name='cologne8', objects=dict(q=src), progress={})
    with pytest.raises(ValueError, match='objects'):
        checkpoint.load_frap_weights(bare, dst)
    assert all(torch.equal(before[k], v) for k, v in full.state_dict().items())
