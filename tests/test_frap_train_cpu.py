"""CPU: the fused MPLight update (resco_amd/csrc/resco_frap_train.h) before it meets a GPU -- the float64 reference and its yardstick
(tests/frap_train_ref.py), the header's host-compilable pieces run over whole minibatches (tests/frap_train_host) against that
reference, the minibatch draw against the counter hash, the C ABI of the update (header, ABI_SYMBOLS, exports, struct mirror); no CPU
fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import frap_ref as fr
import frap_train_ref as ft
from conftest import ROOT
from dqn_train_ref import RING_STATES
from resco_amd import sim as rsim

CALLS = ['rs_mplight_dqn_create', 'rs_mplight_dqn_destroy', 'rs_mplight_dqn_grad', 'rs_mplight_dqn_sample', 'rs_mplight_dqn_step',
         'rs_mplight_dqn_steps', 'rs_mplight_dqn_update']
# (P, D, T, N, S, B): both ends and the three lane-group widths of the forward, both demand shapes
CASES = [(2, 1, 4, 5, 3, 33), (5, 4, 5, 6, 3, 70), (13, 1, 6, 7, 2, 45), (16, 4, 4, 9, 3, 50)]


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return ft.build_frap_train_host(tmp_path_factory.mktemp('frap_train_host'))


@pytest.mark.parametrize('P,D', [(2, 1), (5, 4), (13, 1), (16, 4)])
def test_float64_restatement_is_the_reference_forward(P, D):
    """frap_forward in float64 against frap_ref.frap_ref (numpy, the reference's own formulation) on every class of rows"""
    rng = np.random.default_rng(P)
    pairs = fr.synthetic_signal_set(P, 4, rng)[0]
    net = fr.make_net(pairs, D, scale=2.0)
    w64 = {k: v.detach() for k, v in ft.weights_as(net, torch.float64).items()}
    for name, rows in fr.obs_classes(P, D, 6, 4, rng).items():
        rows = rows.reshape(-1, rows.shape[-1])
        q = ft.frap_forward(w64, pairs, D, torch.from_numpy(rows.astype(np.float64))).numpy()
        ref = fr.frap_ref(net.state_dict(), pairs, D, rows)
        assert np.abs(q - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), name


@pytest.mark.parametrize('P,D,T,N,S,B', CASES)
def test_yardstick_is_satisfiable_by_float32(P, D, T, N, S, B):
    """every member of the float32 family is itself within 4 e_ref of the truth, on every tensor and the loss; the fixture's
    conditions hold on the truth"""
    idx, g64, e_ref, l64, e_loss, family, d64 = ft.reference(P, D, T, N, S, B)
    assert 0.2 <= ft.huber_fraction(d64) <= 0.8
    for label, g, l in family:
        for k in g64:
            assert np.abs(g[k] - g64[k]).max() <= 4 * e_ref[k], (label, k)
            assert (g[k][g64[k] == 0] == 0).all(), (label, k)
        assert abs(l - l64) <= 4 * e_loss, label
    assert all(e_ref[k] >= ft.ulp32(np.abs(g64[k]).max()) for k in g64)
    if P > 2:
        assert all(np.abs(g64[k]).max() > 0 for k in g64), [k for k in g64 if np.abs(g64[k]).max() == 0]
    assert (g64['lane_conv.weight'] == 0).any(), 'dead channels: exact zeros the candidates must reproduce'


def test_every_tensor_has_gradient_and_relation_units_are_alive():
    c = ft.case(5, 4, 5, 6, 3)
    re = c['net'].state_dict()['relation_embedding.weight']
    assert int((re > 0).sum()) >= 2, 'more than one unit of relation_embedding is alive'
    g64 = ft.reference(5, 4, 5, 6, 3, 70)[1]
    assert np.count_nonzero(g64['relation_embedding.weight']) >= 2


def test_done_rows_never_read_their_successor():
    c = dict(ft.case(5, 4, 5, 6, 3))
    assert c['done'][1]
    idx = ft.draw_idx(c, 20, slots=(1,))
    clean = ft.torch_grads(c, idx, torch.float64)[0]
    c['obs'] = c['obs'].copy()
    c['obs'][2] = np.nan
    dirty = ft.torch_grads(c, idx, torch.float64)[0]
    assert all(np.isfinite(v).all() and np.array_equal(v, clean[k]) for k, v in dirty.items())


@pytest.mark.parametrize('P,D,T,N,S,B', CASES + ft.GPU_CASES)
def test_host_minibatch_gradient(host, P, D, T, N, S, B):
    """the header's pieces accumulated over a whole minibatch on the host against the float64 truth, under the yardstick (the cases of
    this file and those the device is given)"""
    assert host.frap_train_tile_rows() == ft.TILE_ROWS
    c = ft.case(P, D, T, N, S)
    idx, g64, e_ref, l64, e_loss, _, _ = ft.reference(P, D, T, N, S, B)
    got, loss = ft.host_grads(host, c, idx)
    print('P %d D %d ring %d x %d x %d, B %d (tile %d rows)' % (P, D, T, N, S, B, host.frap_train_tile_rows()))
    worst = ft.compare(ft.names_of(c['net']), got, loss, g64, e_ref, l64, e_loss, who='host')
    assert not worst, worst


def test_host_ring_semantics(host):
    """rows of the last slot (successor: slot 0), rows of a done slot whose successor holds NaN, an action outside 0 .. P - 1"""
    P, D, T, N, S, B = 5, 4, 5, 6, 3, 40
    c = dict(ft.case(P, D, T, N, S))
    idx, g64, e_ref, l64, e_loss, _, _ = ft.reference(P, D, T, N, S, B, slots=(0, 1, 3, T - 1))
    assert (idx[:, 0] == T - 1).sum() > 3 and (idx[:, 0] == 1).sum() > 3
    c['obs'], c['act'], c['rew'] = c['obs'].copy(), c['act'].copy(), c['rew'].copy()
    c['obs'][2], c['rew'][2] = np.nan, np.nan
    hi = idx[c['act'][idx[:, 0], idx[:, 1], idx[:, 2]] == P - 1]
    lo = idx[c['act'][idx[:, 0], idx[:, 1], idx[:, 2]] == 0]
    assert len(hi) and len(lo)
    c['act'][hi[0][0], hi[0][1], hi[0][2]] = P + 3
    c['act'][lo[0][0], lo[0][1], lo[0][2]] = -2
    got, loss = ft.host_grads(host, c, idx)
    worst = ft.compare(ft.names_of(c['net']), got, loss, g64, e_ref, l64, e_loss, who='host')
    assert not worst, worst


@pytest.mark.parametrize('T,N,head,count', RING_STATES)
def test_sampling_against_the_counter_hash(host, T, N, head, count):
    """frap_dqn_sample_index of the header through the host build (whose d_hash is a restatement) against sim._murmur"""
    B, S, seed = 33, 3, 0x5EED
    draws = []
    for u in (0, 1, 77):
        idx = np.full((B, 3), -1, np.int32)
        assert host.frap_train_sample(seed, u, T, N, S, head, count, B, idx.ctypes.data) == 0
        assert np.array_equal(idx, ft.predict_sample(seed, u, T, N, S, head, count, B))
        ft.check_sample(idx, T, N, S, head, count)
        draws.append(idx)
    assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[1], draws[2])
    assert len(np.unique(draws[0][:, 0])) == count - 1 and len(np.unique(draws[0][:, 2])) == S
    assert host.frap_train_sample(seed, 0, T, N, S, head, 1, B, draws[0].ctypes.data) == -1


def _header():
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        return f.read()


def test_abi_declares_and_exports_the_update():
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = set(re.findall(r'\b(rs_[a-z_]+)\s*\(', text))
    from resco_amd.build import build_library
    build_library()
    L = rsim.load_library()
    for name in CALLS:
        assert name in declared and name in rsim.ABI_SYMBOLS and hasattr(L, name), name


def test_ring_mirror_lists_the_headers_fields():
    text = _header()
    body = text[text.index('typedef struct rs_mplight_ring {') + len('typedef struct rs_mplight_ring {'):text.index('} rs_mplight_ring;')]
    names = []
    for decl in body.split(';'):
        decl = re.sub(r'^(const\s+)?(float|int16_t|int32_t|uint8_t)\s*', '', decl.strip())
        names += [n.strip().lstrip('*') for n in decl.split(',') if n.strip()]
    assert [f[0] for f in rsim.MPLightRing._fields_] == names == ['obs', 'act', 'rew', 'done', 'capacity', 'n_envs', 'n_signals', 'width', 'head', 'count']
    assert C.sizeof(rsim.MPLightRing) == 4 * 8 + 6 * 4


def test_learner_refuses_a_cpu_net():
    from resco_amd.agents.mplight_learn_fused import FusedMPLightLearner
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        FusedMPLightLearner(fr.make_net(ft.case(2, 1, 4, 5, 3)['pairs'], 1))
