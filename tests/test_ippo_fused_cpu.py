"""IPPO's device path without a GPU: the weight pack with the value column (pack_ippo_weights, the device re-pack's gather index),
the fused GAE + standardisation of resco_amd/csrc/resco_ppo.h compiled for the host (tests/ppo_host) against gae() and the
standardisation of resco_amd/agents/ippo.py, and the new declarations of the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from idqn_kernel_ref import dense_fc23, make_net
from ppo_ref import build_ppo_host, gae_case, gae_errors, host_gae
from resco_amd import sim as rsim
from resco_amd.agents.idqn_fused import pack_idqn_weights
from resco_amd.agents.ippo import BatchedIPPO, BatchedPPOLearner
from resco_amd.agents.ippo_fused import VALUE_COL, fc3_with_value, ippo_repack_index, pack_ippo_weights


def _net(lmax, seed):
    net, _ = make_net(lmax, seed=seed, cls=BatchedIPPO)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                       # the reference initialises the biases with zeros: give the value bias something to carry
        net.v_b.add_(torch.randn(net.v_b.shape, generator=g))
        net.fc3_b.add_(0.2 * torch.randn(net.fc3_b.shape, generator=g) * net.action_mask)
    return net


@pytest.mark.parametrize('lmax', [2, 9, 17])
def test_pack_adds_only_the_value_column(lmax):
    net = _net(lmax, seed=lmax)
    S = len(net.lanes)
    a, b = pack_idqn_weights(net), pack_ippo_weights(net)
    assert sorted(a) == sorted(b)
    for k in a:
        if k not in ('w3', 'b3'):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    assert a['w3'].dtype == b['w3'].dtype == np.float16 and a['w3'].shape == b['w3'].shape
    da, db = dense_fc23(a['w3'], S, 1), dense_fc23(b['w3'], S, 1)          # [S, 64 inputs, 32 columns] as the kernel multiplies them
    keep = np.arange(32) != VALUE_COL
    assert np.array_equal(da[:, :, keep], db[:, :, keep]) and not da[:, :, VALUE_COL].any()
    assert np.array_equal(a['b3'][:, keep], b['b3'][:, keep]) and not a['b3'][:, VALUE_COL].any()
    # the two new entries, read back the way the kernel reads them: the value head rounded to fp16 / kept in fp32
    v_w = net.v_w.detach().numpy()[:, :, 0]
    assert np.array_equal(db[:, :, VALUE_COL], v_w.astype(np.float16).astype(np.float64)) and v_w.any()
    assert np.array_equal(b['b3'][:, VALUE_COL], net.v_b.detach().numpy()[:, 0].astype(np.float32)) and b['b3'][:, VALUE_COL].all()
    # the bytes of columns 0..7 in the packed fragments themselves: only the lanes of column 8 differ
    col = np.arange(64) & 31
    assert np.array_equal(a['w3'][:, :, col != VALUE_COL], b['w3'][:, :, col != VALUE_COL])


@pytest.mark.parametrize('lmax', [2, 9, 17])
def test_device_repack_index_reproduces_the_host_pack(lmax):
    """refresh_on_device gathers w1 / w2 / w3 with these indices (index_select, mask, cast to fp16): the same on the CPU"""
    net = _net(lmax, seed=100 + lmax)
    S = len(net.lanes)
    pk = pack_ippo_weights(net)
    src = dict(w1=net.fc1_w.detach(), w2=net.fc2_w.detach(), w3=fc3_with_value(net))
    for k, idx in ippo_repack_index(lmax, net.amax).items():
        flat = src[k].reshape(S, -1).float()
        got = torch.index_select(flat, 1, torch.as_tensor(np.maximum(idx, 0))) * torch.as_tensor((idx >= 0).astype(np.float32))
        # (values, not bytes: a masked-out fragment is x * 0, which is -0 for a negative x)
        assert np.array_equal(got.to(torch.float16).numpy().reshape(-1), pk[k].reshape(-1)), k


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return build_ppo_host(tmp_path_factory.mktemp('ppo'))


def test_gae_host_build_against_the_learners_own_functions(host):
    """T = 32, N = 48, S = 5; truth = gae() + standardisation in float64; e_ref = what the same functions lose in float32.  The host
    build sums in another (fixed) order: 4 e_ref is allowed for that and nothing else.  A second call gives the same bits."""
    rew, val, last, done = gae_case()
    adv, ret = host_gae(host, rew, val, last, done)
    ea, er, ref_a, ref_r = gae_errors(adv, ret, rew, val, last, done)
    print('adv: |host - truth| %.3e, e_ref %.3e;  ret: |host - truth| %.3e, e_ref %.3e' % (ea, ref_a, er, ref_r))
    assert ref_a > 0 and ref_r > 0
    assert ea <= 4 * ref_a and er <= 4 * ref_r
    adv2, ret2 = host_gae(host, rew, val, last, done)
    assert adv.tobytes() == adv2.tobytes() and ret.tobytes() == ret2.tobytes()
    # what standardised means: per signal zero mean and unit (biased) deviation over the T * N samples
    flat = adv.reshape(-1, adv.shape[-1]).astype(np.float64)
    assert np.abs(flat.mean(0)).max() < 1e-6 and np.abs(flat.std(0) - 1.0).max() < 1e-5


def test_gae_does_not_bootstrap_across_done(host):
    """the steps up to a `done` do not see what comes after it: changing rewards and values behind it leaves their returns alone"""
    rew, val, last, done = gae_case(seed=3)
    _, ret = host_gae(host, rew, val, last, done)
    cut = int(np.nonzero(done)[0][0])
    rew2, val2 = rew.copy(), val.copy()
    rew2[cut + 1:] += 1.0
    val2[cut + 1:] -= 2.0
    _, ret2 = host_gae(host, rew2, val2, last + 5.0, done)
    assert ret[:cut + 1].tobytes() == ret2[:cut + 1].tobytes() and not np.array_equal(ret[cut + 1:], ret2[cut + 1:])


def test_update_from_rollout_refuses_cpu_tensors():
    net = BatchedIPPO([3, 4], [2, 3])
    net.init_like_reference(seed=0)
    T, N, S = 4, 6, 2

    class CpuRollout:
        def cat(self, name):
            shape = (T, N, S, net.lmax, 5) if name == 'obs' else (T, N, S)
            return torch.zeros(shape, dtype=torch.float16 if name == 'obs' else (torch.int32 if name == 'act' else torch.float32))

    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BatchedPPOLearner(net).update_from_rollout(CpuRollout(), torch.zeros(N, S), torch.zeros(T, dtype=torch.bool))


def test_abi_declares_the_new_calls():
    with open(os.path.join(ROOT, 'include', 'resco_sim.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    declared = set(re.findall(r'\b(rs_[a-z_]+)\s*\(', text))
    for sym in ('rs_ippo_act', 'rs_group_rollout', 'rs_ppo_gae'):
        assert sym in declared and sym in rsim.ABI_SYMBOLS, sym
    assert re.search(r'RS_AGENT_IPPO\s*=\s*6\b', text) and rsim.AGENT['ippo'] == 6
    body = text[text.index('typedef struct rs_rollout {') + len('typedef struct rs_rollout {'):text.index('} rs_rollout;')]
    names = []
    for decl in body.split(';'):
        decl = re.sub(r'^(void|int32_t|float)\s*', '', decl.strip())
        names += [n.strip().lstrip('*') for n in decl.split(',') if n.strip()]
    assert [f[0] for f in rsim.Rollout._fields_] == names
    import ctypes as C
    assert C.sizeof(rsim.Rollout) == 5 * 8 + 8          # five pointers, T, padding
    from resco_amd.build import build_library
    build_library()
    L = rsim.load_library()
    for sym in ('rs_ippo_act', 'rs_group_rollout', 'rs_ppo_gae'):
        assert hasattr(L, sym), sym
