"""GPU: the fused FMA2C acting kernel (rs_fma2c_*; resco_amd/csrc/resco_fma2c.h) against the float64 restatement of the reference
(tests/fma2c_ref.py) by the yardstick of tests/fma2c_check.py, its split / value-only / reset contracts bit for bit, rs_group_step with
RS_AGENT_FMA2C, the refusals, and a training smoke run.  Inputs are synthetic lane aggregates unless said otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_scenario
from fma2c_check import A_MAX, Case, compare, reference

pytestmark = pytest.mark.gpu

SALT = 0x5A2C9D47           # resco_fma2c.h: FM_SALT
TILE = 32                   # resco_fma2c.h: FM_TM
SEED = 11
_cases = {}


def case(map_name, full=False):
    from resco_amd.config.mdp_config import activate
    key = (map_name, full)
    if key not in _cases:
        _cases[key] = Case(map_name, full)
        _cases[key].net.cuda()
    activate('FMA2CFull' if full else 'FMA2C', map_name)
    return _cases[key]


def policy_for(c, max_envs, seed=SEED):
    from resco_amd.agents.fma2c import FusedFMA2C
    return FusedFMA2C(c.net, max_envs, seed=seed)


def uniforms(T, N, K, seed=SEED, env_base=0, key0=0):
    """what the kernel draws with: d_u01 of the counter hash over (seed ^ FM_SALT; env_base + env, agent, step_key, 0)"""
    from resco_amd.sim import _murmur
    u = np.zeros((T, N, K))
    for t in range(T):
        for n in range(N):
            for k in range(K):
                u[t, n, k] = (_murmur((seed ^ SALT) & 0xFFFFFFFF, (env_base + n, k, key0 + t, 0)) >> 8) / 16777216.0
    return u


def kernel_steps(pol, agg, env_base=0, key0=0, want=('pi', 'value', 'rows')):
    T, N = agg.shape[:2]
    steps = []
    for t in range(T):
        out = pol.act(torch.as_tensor(agg[t]).cuda().contiguous(), step_key=key0 + t, env_base=env_base, want=want)
        torch.cuda.synchronize()
        step = {k: v.cpu().numpy() for k, v in out.items()}
        step['state'] = pol.buffer('state')[env_base:env_base + N].cpu().numpy()
        step['actions'] = np.concatenate([pol.buffer('mgr_actions')[env_base:env_base + N].cpu().numpy(), step['actions']], axis=1)
        steps.append(step)
    return steps


def library_state(pol):
    torch.cuda.synchronize()
    return [pol.buffer(b).cpu().numpy().copy() for b in ('state', 'mgr_actions')] + [pol.fingerprints().cpu().numpy()]


# ------------------------------------------------------------------------------------------------ kernel against float64
@pytest.mark.parametrize('map_name,full,N', [(m, False, n) for m in ('cologne1', 'cologne3', 'ingolstadt21') for n in (1, 3, TILE + 1)] +
                         [('ingolstadt7', True, 3)])
def test_kernel_against_float64(map_name, full, N):
    """four chained act calls (state and both fingerprint buffers in use): pi, value, state, rows_out within 4 e_ref + 2 ulp32 of
    float64; the drawn action is the inverse-CDF choice on every row farther than 8 e_ref from a CDF boundary (at most 1 % nearer)"""
    c = case(map_name, full)
    T = 4
    agg = c.lane_agg(np.random.default_rng(5), T, N)
    u = uniforms(T, N, c.layout.K)
    truth, e_ref = reference(c, agg, u)
    pol = policy_for(c, N)
    steps = kernel_steps(pol, agg)
    compare(c, truth, e_ref, u, steps, label='kernel %s N=%d' % (map_name, N))
    fp = pol.fingerprints().cpu().numpy()
    np.testing.assert_array_equal(fp, steps[-1]['pi'])          # the fingerprint the next act reads is the last pi
    pol.close()


# ------------------------------------------------------------------------------------------------ split over env_base
def test_split_batch_is_bit_equal():
    """N = 6 in one call against two calls of 3 with env_base 0 and 3 on one policy: every output and the library's state"""
    c = case('cologne3')
    T, N = 3, 6
    agg = c.lane_agg(np.random.default_rng(6), T, N)
    one, two = policy_for(c, N), policy_for(c, N)
    for t in range(T):
        a = kernel_steps(one, agg[t:t + 1], key0=t)[0]
        b0 = kernel_steps(two, agg[t:t + 1, :3], env_base=0, key0=t)[0]
        b1 = kernel_steps(two, agg[t:t + 1, 3:], env_base=3, key0=t)[0]
        for k in ('pi', 'value', 'rows', 'actions', 'state'):
            np.testing.assert_array_equal(a[k], np.concatenate([b0[k], b1[k]]), err_msg='%s step %d' % (k, t))
        for x, y in zip(library_state(one), library_state(two)):
            np.testing.assert_array_equal(x, y)
    one.close(); two.close()


# ------------------------------------------------------------------------------------------------ value-only
def test_value_only_call():
    """the bootstrap call gives the bits of the full call's value on the same input and leaves state, fingerprints, manager actions
    and the next act's outputs alone"""
    c = case('cologne3')
    L, N = c.layout, 5
    agg = c.lane_agg(np.random.default_rng(7), 3, N)
    pol, twin = policy_for(c, N), policy_for(c, N)
    kernel_steps(pol, agg[:2]); kernel_steps(twin, agg[:2])
    full = kernel_steps(twin, agg[2:3], key0=2)[0]              # the full call on the same history and input
    before = library_state(pol)
    nxt = torch.as_tensor(agg[2]).cuda().contiguous()
    v_last = pol.value(nxt).cpu().numpy()                       # with the managers' LAST actions: the reference's bootstrap (fma2c.py:146-151)
    # a manager's row does not depend on anybody's draw: the full call saw the same input
    np.testing.assert_array_equal(v_last[:, :L.M], full['value'][:, :L.M])
    # a worker's row leads with the managers' actions: lend the value call the ones the full call drew (the buffer is the library's,
    # lent by rs_fma2c_buffer), and every agent's value has the full call's bits
    macts = pol.buffer('mgr_actions')
    saved = macts.clone()
    macts.copy_(torch.as_tensor(full['actions'][:, :L.M].astype(np.int32)).cuda())
    v = pol.value(nxt).cpu().numpy()
    macts.copy_(saved)
    np.testing.assert_array_equal(v, full['value'])
    for x, y in zip(before, library_state(pol)):
        np.testing.assert_array_equal(x, y)
    a = kernel_steps(pol, agg[2:3], key0=2)[0]
    for k in ('pi', 'value', 'rows', 'actions', 'state'):
        np.testing.assert_array_equal(a[k], full[k])
    pol.close(); twin.close()


# ------------------------------------------------------------------------------------------------ reset
def test_reset():
    c = case('cologne3')
    N = 4
    agg = c.lane_agg(np.random.default_rng(8), 3, N)
    pol, fresh = policy_for(c, N), policy_for(c, N)
    kernel_steps(pol, agg[:2])
    fp = pol.fingerprints().cpu().numpy()
    assert np.abs(pol.buffer('state').cpu().numpy()).max() > 0 and fp.max() > 0
    pol.reset(0, 2)                                                     # the first two environments only
    torch.cuda.synchronize()
    st = pol.buffer('state').cpu().numpy()
    assert np.abs(st[:2]).max() == 0 and np.abs(st[2:]).max() > 0
    np.testing.assert_array_equal(pol.fingerprints().cpu().numpy(), fp)     # kept, as the reference keeps them
    pol.reset(clear_fingerprints=True)
    torch.cuda.synchronize()
    assert np.abs(pol.buffer('state').cpu().numpy()).max() == 0 and np.abs(pol.buffer('fingerprints').cpu().numpy()).max() == 0
    a, b = kernel_steps(pol, agg[2:3], key0=9)[0], kernel_steps(fresh, agg[2:3], key0=9)[0]
    for k in ('pi', 'value', 'rows', 'actions', 'state'):
        np.testing.assert_array_equal(a[k], b[k])
    pol.close(); fresh.close()


# ------------------------------------------------------------------------------------------------ rs_group_step
def _sims(sc, n, k, seed=2):
    from resco_amd.sim import BatchedSim, SimGroup
    per = n // k
    sims = [BatchedSim(sc, per, seed=seed, env_base=i * per, device_envs=n) for i in range(k)]
    for s in sims:
        s.reset()
        SimGroup([s]).step('random', step_key=0, n_steps=5)
        s.sync()
    return sims


def test_group_step_equals_python_loop_and_pipes():
    """cologne3 x 4 environments, 6 steps: rs_group_step(RS_AGENT_FMA2C) against the Python loop of rs_fma2c_act + rs_step (actions,
    lane_agg, phases bit-equal), and two pipes of 2 against one handle of 4"""
    from resco_amd.sim import SimGroup
    c = case('cologne3')
    n, steps = 4, 6
    pa, pb, pc = policy_for(c, n), policy_for(c, n), policy_for(c, n)
    a, b, one = _sims(c.sc, n, 2), _sims(c.sc, n, 2), _sims(c.sc, n, 1)
    SimGroup(a).step('fma2c', step_key=30, n_steps=steps, policy=pa.handle, seed=SEED)
    SimGroup(one).step('fma2c', step_key=30, n_steps=steps, policy=pc.handle, seed=SEED)
    for k in range(steps):
        for s in b:
            pb.act(s.tensor('lane_agg'), step_key=30 + k, env_base=s.env_base, actions=s.tensor('actions'), want=())
            s.step(None, stream=1)
    torch.cuda.synchronize()
    for s in a + one:
        s.sync()
    read = lambda sims: [np.concatenate([s.read(x) for s in sims]) for x in ('actions', 'lane_agg', 'phase')]
    for x, y, z in zip(read(a), read(b), read(one)):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z)
    for x, y, z in zip(library_state(pa), library_state(pb), library_state(pc)):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z)
    assert read(a)[1].sum() > 0
    for s in a + b + one:
        s.close()
    for p in (pa, pb, pc):
        p.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from resco_amd.agents.mplight import FusedMPLight, frap_from_scenario
    from resco_amd.sim import BatchedSim, Fma2cDesc, SimGroup
    c = case('cologne3')
    L, N = c.layout, 4
    pol = policy_for(c, N)
    lib = pol._lib
    err = lambda: (lib.rs_last_error(None) or b'').decode()
    agg = torch.as_tensor(c.lane_agg(np.random.default_rng(9), 1, N)[0]).cuda().contiguous()
    acts = torch.full((N, L.S), -7, dtype=torch.int32, device='cuda')
    val = torch.full((N, L.K), -7.0, device='cuda')
    mnet = frap_from_scenario(c.sc, 1).cuda()
    mnet.init_like_reference(0)
    mpl = FusedMPLight(mnet, c.sc)

    def untouched():
        torch.cuda.synchronize()
        assert int((acts != -7).sum()) == 0 and int((val != -7.0).sum()) == 0

    # a handle of another kind, both ways
    assert lib.rs_fma2c_act(mpl.handle, agg.data_ptr(), N, 0, 0, 0, None, acts.data_ptr(), None, val.data_ptr(), None, 1) == -1
    assert 'not an rs_fma2c_create policy' in err()
    assert lib.rs_fma2c_value(mpl.handle, agg.data_ptr(), N, 0, val.data_ptr(), 1) == -1 and 'not an rs_fma2c_create policy' in err()
    assert lib.rs_fma2c_reset(mpl.handle, 0, N, 0, 1) == -1 and 'not an rs_fma2c_create policy' in err()
    assert lib.rs_fma2c_set_device_weights(mpl.handle, agg.data_ptr()) == -1 and 'not an rs_fma2c_create policy' in err()
    mobs = torch.zeros(N, L.S, 13, dtype=torch.int32, device='cuda')
    assert lib.rs_mplight_act(pol.handle, mobs.data_ptr(), N, 0, 0.0, 0, 0, None, acts.data_ptr(), None, None, 1) == -1
    assert 'not an rs_mplight_create policy' in err()
    assert lib.rs_idqn_act(pol.handle, mobs.data_ptr(), N, 0, 0, 0.0, 0, 0, None, acts.data_ptr(), None, 1) == -1
    assert 'not an rs_idqn_create policy' in err()
    untouched()
    # rows outside the library's state
    for n, base in ((N, 1), (N + 1, 0), (0, 0), (1, -1)):
        assert lib.rs_fma2c_act(pol.handle, agg.data_ptr(), n, base, 0, 0, None, acts.data_ptr(), None, val.data_ptr(), None, 1) == -1
        assert 'env_base + n_envs <= max_envs' in err()
        assert lib.rs_fma2c_value(pol.handle, agg.data_ptr(), n, base, val.data_ptr(), 1) == -1 and 'env_base + n_envs <= max_envs' in err()
        assert lib.rs_fma2c_reset(pol.handle, base, n, 0, 1) == -1 and 'env_base + n_envs <= max_envs' in err()
    # a NULL where one is required
    assert lib.rs_fma2c_act(pol.handle, None, N, 0, 0, 0, None, acts.data_ptr(), None, val.data_ptr(), None, 1) == -1 and 'lane_agg is NULL' in err()
    assert lib.rs_fma2c_value(pol.handle, agg.data_ptr(), N, 0, None, 1) == -1 and 'NULL' in err()
    assert lib.rs_fma2c_act(None, agg.data_ptr(), N, 0, 0, 0, None, acts.data_ptr(), None, val.data_ptr(), None, 1) == -1 and 'NULL' in err()
    untouched()
    # widths outside the documented limits, tables that do not add up, NULL descriptor / weights
    keep = L.desc_arrays()
    w = np.ascontiguousarray(c.net.packed().cpu().numpy(), np.float32)

    def create(**over):
        arrays = dict(keep, **{k: v for k, v in over.items() if k in keep})
        d = Fma2cDesc(L.K, L.M, L.S, L.O, 0, 5.0, 4.0, 100.0, 4.0, *[arrays[n].ctypes.data for n in Fma2cDesc.ARRAYS])
        h = C.c_void_p()
        rc = lib.rs_fma2c_create(0, C.byref(d), over.get('weights', w.ctypes.data), over.get('max_envs', N), C.byref(h))
        assert h.value is None
        return rc
    bad = keep['n_a'].copy(); bad[0] = 9
    assert create(n_a=bad) == -1 and 'widths outside the limits' in err()
    bad = keep['n_w'].copy(); bad[L.M] = 33
    assert create(n_w=bad) == -1 and 'widths outside the limits' in err()
    bad = keep['n_s'].copy(); bad[0] += 1
    assert create(n_s=bad) == -1 and 'do not add up' in err()
    assert create(weights=None) == -1 and 'NULL' in err()
    assert create(max_envs=0) == -1
    assert lib.rs_fma2c_create(0, None, w.ctypes.data, N, C.byref(C.c_void_p())) == -1 and 'NULL' in err()
    # rs_group_step: a policy of another kind, scenario or size, and a switched-off lane_agg
    sim = BatchedSim(c.sc, N, seed=1)
    sim.reset()
    grp = SimGroup([sim])
    before = sim.read('actions')
    herr = lambda: (lib.rs_last_error(sim._h) or b'').decode()
    with pytest.raises(RuntimeError, match='not an rs_fma2c_create policy'):
        grp.step('fma2c', policy=mpl.handle)
    with pytest.raises(RuntimeError, match='rs_mplight_create policy'):
        grp.step('mplight', policy=pol.handle)
    other = case('cologne1')
    pol1 = policy_for(other, N)
    with pytest.raises(RuntimeError, match='built for this scenario'):
        grp.step('fma2c', policy=pol1.handle)
    case('cologne3')
    small = policy_for(c, N - 1)
    with pytest.raises(RuntimeError, match='exceeds the policy'):
        grp.step('fma2c', policy=small.handle)
    sim.set_outputs(('drq_norm',))
    with pytest.raises(RuntimeError, match='RS_BUF_LANE_AGG, which rs_set_outputs has switched off'):
        grp.step('fma2c', policy=pol.handle)
    assert 'RS_BUF_LANE_AGG' in herr()
    sim.sync()
    np.testing.assert_array_equal(sim.read('actions'), before)
    assert np.abs(pol.buffer('state').cpu().numpy()).max() == 0         # nothing was ever launched on this policy
    for p in (pol, pol1, small, mpl):
        p.close()
    sim.close()


# ------------------------------------------------------------------------------------------------ training smoke
def test_training_smoke():
    """tools/fma2c_train.py --steps-per-episode 120 cologne1 16 2: the loss is finite, every agent's weights moved, and the fused
    policy's next pi equals BatchedFMA2C's on the updated weights within the bound.  No claim about learning."""
    import fma2c_ref as R
    from resco_amd.agents.fma2c import BatchedFMA2C
    from tools.fma2c_train import main
    c0 = Case('cologne1', seed=0)
    start = BatchedFMA2C(c0.layout).init_like_reference(0).packed()
    keep = {}
    rows, final = main('cologne1', 16, 2, seed=0, steps_per_episode=120, quiet=True, keep=keep)
    net, pol, L = keep['net'], keep['policy'], keep['layout']
    assert len(rows) == 2 and all(np.isfinite(r['loss']) for r in rows) and keep['learner'].updates == 2
    moved = (net.packed().cpu() != start).float()
    from resco_amd.agents.fma2c import PARAMS
    off = 0
    per_agent = torch.zeros(L.K)
    for name in PARAMS:
        p = getattr(net, name)
        per_agent += moved[off:off + p.numel()].reshape(L.K, -1).sum(dim=1)
        off += p.numel()
    assert (per_agent > 0).all()
    # one more act of the fused policy on the updated weights against the float64 reference of those weights
    N = 16
    c0.net = net
    agg = c0.lane_agg(np.random.default_rng(10), 1, N)
    torch.cuda.synchronize()
    state0 = pol.buffer('state').cpu().numpy().astype(np.float64)
    fp0 = pol.fingerprints().cpu().numpy().astype(np.float64)
    u = uniforms(1, N, L.K, seed=7, key0=777)
    truth, e_ref = reference(c0, agg, u, state0, fp0)
    step = kernel_steps(pol, agg, key0=777)[0]
    compare(c0, truth, e_ref, u, [step], label='after training')
    with torch.no_grad():
        out = net.act(L.obs_rows(torch.as_tensor(agg[0]).cuda()), torch.as_tensor(state0, dtype=torch.float32).cuda(),
                      torch.as_tensor(fp0, dtype=torch.float32).cuda(), torch.as_tensor(u[0], dtype=torch.float32).cuda())
    assert (np.abs(out['pi'].cpu().numpy().astype(np.float64) - truth[0]['pi']) <= R.bound(e_ref['pi'], truth[0]['pi'])).all()
    pol.close()
    keep['env'].close()
