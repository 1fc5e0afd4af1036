"""Shared by tests/test_fma2c_cpu.py and tests/test_gpu_fma2c.py (TEST INFRASTRUCTURE): the case set-up, the float64 / float32 chains
of tests/fma2c_ref.py over several act steps, and the comparison of a candidate (BatchedFMA2C, the host build of the kernel's pieces,
the kernel) against them by the yardstick of fma2c_ref: 4 e_ref + 2 ulp32(|truth|) per element, e_ref per tensor class."""
import numpy as np

import fma2c_ref as R
from conftest import load_scenario

A_MAX = 8


class Case:
    """one map with its layout, a network initialised like the reference's, and the reference's view of both"""

    def __init__(self, map_name, full=False, seed=3):
        import torch
        from resco_amd.agents.fma2c import BatchedFMA2C, FMA2CLayout
        from resco_amd.config.mdp_config import activate
        from resco_amd.config.signal_config import signal_configs
        from resco_amd.multi_signal import fma2c_state_tables
        self.map, self.full = map_name, full
        self.mdp = activate('FMA2CFull' if full else 'FMA2C', map_name)
        self.sc = load_scenario(map_name)
        self.layout = L = FMA2CLayout(self.sc, full)
        torch.manual_seed(seed)
        self.net = BatchedFMA2C(L).init_like_reference(seed)
        with torch.no_grad():       # biases are zero in the reference's init: give them values so that every term is exercised
            g = torch.Generator().manual_seed(seed + 1)
            for n in ('fcw_b', 'fcf_b', 'fct_b', 'lb', 'head_b'):
                getattr(self.net, n).copy_(0.1 * torch.randn(getattr(self.net, n).shape, generator=g))
            self.net.fct_b.mul_(self.net.has_w[:, None, None])
            self.net.head_b[:, 0].mul_(self.net.act_mask.float())
            self.net.head_b[:, 1, 1:] = 0
        keys, self.s_idx, self.s_scale = fma2c_state_tables(self.sc, self.mdp, full)[:3]
        n_actions = {sid: int(g) for sid, g in zip(self.sc.signal_ids, self.sc.tls_ngreen)}
        self.table = R.agent_table(signal_configs[map_name], self.mdp, {k: len(self.s_idx[k]) for k in keys}, n_actions)
        self.names = list(self.table.keys())
        self.managers = list(self.mdp['management'].keys())

    def ref_params(self, net=None):
        """the candidate network's weights as the reference's per-agent dicts (float64), padding stripped"""
        net, out = net or self.net, {}
        for k, name in enumerate(self.names):
            a = self.table[name]
            out[name] = {}
            for ni, nn_ in enumerate(('pi', 'v')):
                g = lambda t: getattr(net, t).detach().cpu().double().numpy()[k, ni]
                n_in, n_out = (224 if a['n_w'] else 192), (a['n_a'] if ni == 0 else 1)
                p = dict(fcw_w=g('fcw_w')[:a['n_s']], fcw_b=g('fcw_b'), fcf_w=g('fcf_w')[:a['n_f']], fcf_b=g('fcf_b'), wx=g('wx')[:n_in], wh=g('wh'),
                         lb=g('lb'), head_w=g('head_w')[:, :n_out], head_b=g('head_b')[:n_out])
                if a['n_w']:
                    p.update(fct_w=g('fct_w')[:a['n_w']], fct_b=g('fct_b'))
                out[name][nn_] = p
        return out

    def lane_agg(self, rng, T, N):
        """synthetic lane aggregates on both sides of every clip: wave / norm_wave around clip_wave (4 * 5 = 20 vehicles), max_wait
        around clip_wait * norm_wait (400 s), total_wait and speed sums likewise for the full state"""
        O = self.sc.n_obs
        agg = np.zeros((T, N, O, 5), np.float32)
        agg[..., 0] = rng.integers(0, 18, (T, N, O)); agg[..., 1] = rng.integers(0, 18, (T, N, O))
        agg[..., 2] = rng.uniform(0, 5000, (T, N, O)); agg[..., 3] = rng.uniform(0, 800, (T, N, O))
        agg[..., 4] = rng.uniform(0, 20000, (T, N, O))
        return agg


def chain(case, params, agg, u, dt, forced_actions=None, state0=None, fp0=None):
    """T act steps of fma2c.py:103-132 for N environments in dtype dt.  agg [T, N, O, 5], u [T, N, K].  forced_actions [T, N, K]: the
    actions to continue with (the float32 evaluation follows the truth's draws).  Returns per step dicts of [N, K, ..] arrays."""
    T, N = agg.shape[0], agg.shape[1]
    names, tab = case.names, case.table
    state = {n: (np.zeros((N, 4, 64), dt) if state0 is None else state0[:, k].astype(dt)) for k, n in enumerate(names)}
    fp = {n: (np.zeros((N, tab[n]['n_a']), dt) if fp0 is None else fp0[:, k, :tab[n]['n_a']].astype(dt)) for k, n in enumerate(names)}
    W = max(tab[n]['n_s'] + tab[n]['n_w'] + tab[n]['n_f'] for n in names)
    steps = []
    for t in range(T):
        rows_env = [R.states_rows(case.mdp, case.full, agg[t, n], case.s_idx, case.s_scale) for n in range(N)]
        fp_read = {n: v.copy() for n, v in fp.items()}          # read once, before anybody acts (fma2c.py:106)
        acts, out = {}, dict(pi=np.zeros((N, len(names), A_MAX)), value=np.zeros((N, len(names))), state=np.zeros((N, len(names), 4, 64)),
                             rows=np.zeros((N, len(names), W)), actions=np.zeros((N, len(names)), np.int64))
        for k, name in enumerate(names):                          # managers come first in `names`
            a = tab[name]
            x = np.stack([R.assemble(tab, name, rows_env[n][name], {m: acts[m][n] for m in a['mgr_src']}, {s: fp_read[s][n] for s in a['fp_src']})
                          for n in range(N)])
            pi, v, st = R.agent_forward(params[name], a, x, state[name], False, dt)
            act = R.draw(pi.astype(np.float64), u[t, :, k]) if forced_actions is None else forced_actions[t, :, k]
            acts[name], state[name], fp[name] = act, st, pi
            out['pi'][:, k, :a['n_a']], out['value'][:, k], out['state'][:, k], out['actions'][:, k] = pi, v, st, act
            out['rows'][:, k, :x.shape[1]] = x
        steps.append(out)
    return steps


CLASSES = ('pi', 'value', 'state', 'rows')


def reference(case, agg, u, state0=None, fp0=None):
    """truth (float64), and e_ref per tensor class from the plain float32 evaluation that follows the truth's actions"""
    params = case.ref_params()
    truth = chain(case, params, agg, u, np.float64, None, state0, fp0)
    forced = np.stack([s['actions'] for s in truth])
    plain = chain(case, params, agg, u, np.float32, forced, state0, fp0)
    e_ref = {c: max(float(np.abs(np.asarray(p[c], np.float64) - t[c]).max()) for p, t in zip(plain, truth)) for c in CLASSES}
    return truth, e_ref


def compare(case, truth, e_ref, u, candidate_steps, classes=CLASSES, cap=0.01, label=''):
    """candidate_steps: per step a dict of numpy arrays in the layout of chain().  Every class within 4 e_ref + 2 ulp32 of the truth on
    the environments whose draws so far agree with the truth's; the drawn action equals the truth's on every row whose uniform is
    farther than 8 e_ref(pi) from every CDF boundary; the excluded rows (nearer than that, or of an environment that has left the
    truth's trajectory at such a row) stay below `cap` of all rows."""
    T, N, K = u.shape
    tainted = np.zeros(N, bool)
    excluded = 0
    for t, (tr, cand) in enumerate(zip(truth, candidate_steps)):
        ok = ~tainted
        for c in classes:
            err = np.abs(np.asarray(cand[c], np.float64) - tr[c])
            lim = R.bound(e_ref[c], tr[c])
            bad = (err > lim)[ok]
            print('%s step %d %-5s max err %.3e  e_ref %.3e' % (label, t, c, float(err[ok].max()) if ok.any() else 0.0, e_ref[c]))
            assert not bad.any(), '%s step %d: %s exceeds 4 e_ref + 2 ulp32 (max err %.3e, e_ref %.3e)' % (label, t, c, float(err[ok].max()), e_ref[c])
        for k, name in enumerate(case.names):
            n_a = case.table[name]['n_a']
            margin = R.cdf_margin(tr['pi'][:, k, :n_a], u[t, :, k])
            safe = margin > 8.0 * e_ref['pi']
            same = np.asarray(cand['actions'])[:, k] == tr['actions'][:, k]
            assert same[ok & safe].all(), '%s step %d agent %s: the drawn action differs from the inverse-CDF choice on a safe row' % (label, t, name)
            excluded += int((~safe | tainted).sum())
            tainted |= ~same
    share = excluded / float(T * N * K)
    print('%s excluded rows: %.5f of all (cap %.2f)' % (label, share, cap))
    assert share <= cap
