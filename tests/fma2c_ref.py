"""FMA2C restated from the reference's TF1 code in numpy, one agent at a time, in dicts (TEST INFRASTRUCTURE; shares no code with
resco_amd/agents/fma2c.py, which it judges).  Every function takes a dtype: float64 is the truth, float32 the plain evaluation whose
distance from the truth sizes the bound (the convention of tests/train_ref.py and tests/frap_ref.py):
    e_ref = max |float32 evaluation - truth| over a tensor class;  a candidate gets 4 e_ref + 2 ulp32(|truth|) per element.

Reference lines (resco_benchmark/agents/): fma2c.py:41-70 sizes, :75-132 fingerprints and act; ma2c.py:124-147 MA2CAgent,
:286-306 loss / clip / RMSProp, :383-398 backward, :411-456 FPLstmACPolicy, :482-532 fc / lstm, :566-612 OnPolicyBuffer."""
import numpy as np

N_FW, N_FP, N_FT, N_LSTM, MGR_ACTS = 128, 64, 32, 64, 4         # agent_config.py:39-63


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def bound(e_ref, truth):
    return 4.0 * e_ref + 2.0 * ulp32(truth)


# ---------------------------------------------------------------------------------------------- sizes (fma2c.py:41-70)
def agent_table(signal_config, mdp, obs_len, n_actions):
    """name -> dict(n_a, n_s, n_w, n_f, fp_src, mgr_src), managers in `management` order then -- as the repository orders them --
    the workers in the order of `n_actions` (all_ts_ids).  n_s is the model's (ma2c.py:163: n_s - n_f - n_w of MA2CAgent's)."""
    sup = {w: m for m, ws in mdp['management'].items() for w in ws}         # main.py:62-66
    mn = mdp['management_neighbors']
    out = {}
    for manager in mdp['management']:
        fp = MGR_ACTS * len(mn[manager])
        out[manager] = dict(n_a=MGR_ACTS, n_s=obs_len[manager], n_w=0, n_f=fp, fp_src=list(mn[manager]), mgr_src=[])
    for worker in n_actions:
        downstream = signal_config[worker]['downstream']
        nbs = [downstream[d] for d in downstream]
        src = [nb for nb in nbs if nb is not None and sup[nb] == sup[worker]]
        fp = sum(n_actions[nb] for nb in src)
        lanes = []
        for d in signal_config[worker]['lane_sets']:
            for lane in signal_config[worker]['lane_sets'][d]:
                if lane not in lanes:
                    lanes.append(lane)
        mgmt = len(mn[sup[worker]]) + 1
        n_s_agent = obs_len[worker] + mgmt + fp                              # MA2CAgent: observation_shape[0] + fingerprint_size
        out[worker] = dict(n_a=n_actions[worker], n_s=n_s_agent - fp - len(lanes), n_w=len(lanes), n_f=fp, fp_src=src,
                           mgr_src=[sup[worker]] + list(mn[sup[worker]]))
    return out


# ---------------------------------------------------------------------------------------------- input rows (fma2c.py:75-132)
def assemble(table, name, obs, acts, fingerprint):
    """[manager actions] ++ states row ++ fingerprints of the sources, raw integers cast to float"""
    a = table[name]
    fps = [np.asarray(fingerprint[s], np.float64) for s in a['fp_src']]
    fp = np.concatenate(fps) if fps else np.zeros(0)
    row = np.concatenate([np.asarray(obs, np.float64), fp])
    if a['mgr_src']:
        row = np.concatenate([np.asarray([acts[m] for m in a['mgr_src']], np.float64), row])
    return row


def states_rows(mdp, full, lane_agg, s_idx, s_scale):
    """states.fma2c / fma2c_full rows (states.py:162-305) of one environment from its lane aggregates [O, 5] in float64, through the
    repository's index tables (multi_signal.fma2c_state_tables, which the simulator's own tests pin)"""
    agg = np.asarray(lane_agg, np.float64)
    blocks = [np.clip((agg[:, 0] + agg[:, 1]) / mdp['norm_wave'], 0, mdp['clip_wave'])]
    if full:
        blocks += [np.clip(agg[:, 2] / 28 / mdp['norm_wave'], 0, mdp['clip_wave']), np.clip(agg[:, 4] / 20 / 28 / mdp['norm_wave'], 0, mdp['clip_wave'])]
    blocks.append(np.clip(agg[:, 3] / mdp['norm_wait'], 0, mdp['clip_wait']))
    F = np.concatenate(blocks)
    return {k: F[np.asarray(s_idx[k], np.int64)] * np.asarray(s_scale[k], np.float64) for k in s_idx}


# ---------------------------------------------------------------------------------------------- net (ma2c.py:411-456, 482-532)
def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def net_forward(p, a, x, c, h, done, dt, keep=None):
    """one _build_net step for a batch: x [N, n_s + n_w + n_f], c / h [N, 64], done [N] or scalar -> out [N, n_out], c, h"""
    x = np.asarray(x, dt)
    n_s, n_w = a['n_s'], a['n_w']
    W = lambda k: np.asarray(p[k], dt)
    a0 = x[:, :n_s] @ W('fcw_w') + W('fcw_b')
    a1 = x[:, n_s + n_w:] @ W('fcf_w') + W('fcf_b')
    parts, pre = [np.maximum(a0, 0), np.maximum(a1, 0)], [a0, a1]
    if n_w > 0:
        a2 = x[:, n_s:n_s + n_w] @ W('fct_w') + W('fct_b')
        parts.append(np.maximum(a2, 0)); pre.append(a2)
    hc = np.concatenate(parts, axis=1)
    keepd = np.asarray(1.0 - np.asarray(done, np.float64), dt).reshape(-1, 1)
    c_in, h_in = np.asarray(c, dt) * keepd, np.asarray(h, dt) * keepd
    z = hc @ W('wx') + h_in @ W('wh') + W('lb')
    i, f, o, u = sigmoid(z[:, :64]), sigmoid(z[:, 64:128]), sigmoid(z[:, 128:192]), np.tanh(z[:, 192:])
    c2 = f * c_in + i * u
    tc = np.tanh(c2)
    h2 = o * tc
    out = h2 @ W('head_w') + W('head_b')
    if keep is not None:
        keep.append(dict(x=x, pre=pre, hc=hc, c_in=c_in, h_in=h_in, i=i, f=f, o=o, u=u, tc=tc, h2=h2, keepd=keepd))
    return out, c2, h2


def softmax(l):
    e = np.exp(l - l.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def agent_forward(params, a, x, state, done=False, dt=np.float64):
    """params = {'pi': {...}, 'v': {...}}; state [N, 4, 64] (pi c, pi h, v c, v h) -> pi [N, n_a], v [N], new state"""
    lp, c0, h0 = net_forward(params['pi'], a, x, state[:, 0], state[:, 1], done, dt)
    v, c1, h1 = net_forward(params['v'], a, x, state[:, 2], state[:, 3], done, dt)
    return softmax(lp), v[:, 0], np.stack([c0, h0, c1, h1], axis=1)


def draw(pi, u):
    """inverse CDF: the first action whose running sum exceeds u"""
    cdf = np.cumsum(pi, axis=-1)
    return np.minimum((u[..., None] >= cdf).sum(axis=-1), pi.shape[-1] - 1)


def cdf_margin(pi, u):
    """distance of u from the nearest inner CDF boundary of pi (rows are safe to compare when it exceeds the error of the CDF)"""
    cdf = np.cumsum(pi, axis=-1)[..., :-1]
    return np.abs(cdf - u[..., None]).min(axis=-1) if cdf.shape[-1] else np.full(u.shape, np.inf)


# ---------------------------------------------------------------------------------------------- OnPolicyBuffer (ma2c.py:566-612)
def buffer_returns(rs, vs, dones, R, gamma):
    """rs, vs: lists over the steps; dones: [pre-step done of step 0, then the post-step done of every step]; -> Rs, Advs"""
    Rs, Advs = [], []
    for r, v, done in zip(rs[::-1], vs[::-1], dones[:0:-1]):
        R = r + gamma * R * (1.0 - done)
        Rs.append(R); Advs.append(R - v)
    Rs.reverse(); Advs.reverse()
    return Rs, Advs


def clip_reward(r, norm=2000.0, clip=2.0):
    return np.clip(np.asarray(r, np.float64) / norm, -clip, clip)            # ma2c.py:220-225


# ---------------------------------------------------------------------------------------------- loss and gradients (ma2c.py:286-306)
def agent_loss_grads(params, a, xs, acts, dones, Rs, Advs, state0, dt=np.float64, v_coef=0.5, beta=0.001):
    """xs [T, N, W], acts [T, N], dones [T] pre-step, Rs / Advs [T, N], state0 [N, 4, 64].  Returns loss, grads {'pi': {...}, 'v': {...}}
    of loss = -mean(log(clip(pi))[a] Adv) + 0.5 v_coef mean((R - v)^2) - beta mean(entropy), means over T x N, by hand-written BPTT"""
    T, N = xs.shape[0], xs.shape[1]
    NT = dt(T * N)
    Rs, Advs = np.asarray(Rs, dt), np.asarray(Advs, dt)
    grads, loss = {}, dt(0)
    for ni, net in enumerate(('pi', 'v')):
        p = params[net]
        keep, outs = [], []
        c, h = state0[:, 2 * ni], state0[:, 2 * ni + 1]
        for t in range(T):
            out, c, h = net_forward(p, a, xs[t], c, h, float(dones[t]), dt, keep)
            outs.append(out)
        g = {k: np.zeros_like(np.asarray(v, dt)) for k, v in p.items()}
        douts = []
        for t in range(T):
            if net == 'pi':
                pi = softmax(outs[t])
                lp = np.log(np.clip(pi, 1e-10, 1.0))
                ent = -(pi * lp).sum(axis=1)
                onehot = np.eye(a['n_a'], dtype=dt)[acts[t]]
                loss = loss - ((lp * onehot).sum(axis=1) * Advs[t]).sum() / NT - dt(beta) * ent.sum() / NT
                douts.append(-(Advs[t][:, None] / NT) * (onehot - pi) + dt(beta) / NT * pi * (lp + ent[:, None]))
            else:
                v = outs[t][:, 0]
                loss = loss + dt(0.5 * v_coef) * ((Rs[t] - v) ** 2).sum() / NT
                douts.append((dt(v_coef) * (v - Rs[t]) / NT)[:, None])
        dc_next, dh_next = np.zeros((N, 64), dt), np.zeros((N, 64), dt)
        W = lambda k: np.asarray(p[k], dt)
        for t in range(T - 1, -1, -1):
            k = keep[t]
            g['head_w'] += k['h2'].T @ douts[t]; g['head_b'] += douts[t].sum(axis=0)
            dh = douts[t] @ W('head_w').T + dh_next
            do = dh * k['tc']
            dc = dc_next + dh * k['o'] * (1 - k['tc'] ** 2)
            df, di, du = dc * k['c_in'], dc * k['u'], dc * k['i']
            dz = np.concatenate([di * k['i'] * (1 - k['i']), df * k['f'] * (1 - k['f']), do * k['o'] * (1 - k['o']), du * (1 - k['u'] ** 2)], axis=1)
            g['wx'] += k['hc'].T @ dz; g['wh'] += k['h_in'].T @ dz; g['lb'] += dz.sum(axis=0)
            dhc = dz @ W('wx').T
            dc_next, dh_next = dc * k['f'] * k['keepd'], (dz @ W('wh').T) * k['keepd']
            n_s, n_w = a['n_s'], a['n_w']
            segs = [('fcw', k['x'][:, :n_s], 0, N_FW), ('fcf', k['x'][:, n_s + n_w:], N_FW, N_FP)] + ([('fct', k['x'][:, n_s:n_s + n_w], N_FW + N_FP, N_FT)] if n_w else [])
            for j, (nm, xin, off, wd) in enumerate(segs):
                da = dhc[:, off:off + wd] * (k['pre'][j] > 0)
                g[nm + '_w'] += xin.T @ da; g[nm + '_b'] += da.sum(axis=0)
        grads[net] = g
    return loss, grads


def global_norm_scale(grads, clip=40.0):
    """tf.clip_by_global_norm over both nets of ONE agent (ma2c.py:299-302): every gradient times clip / max(norm, clip)"""
    norm = np.sqrt(sum((np.asarray(v, np.float64) ** 2).sum() for net in grads.values() for v in net.values()))
    return clip / max(norm, clip), norm


def tf_rmsprop(w, g, ms, lr=2.5e-4, decay=0.99, eps=1e-5):
    """TF1 RMSPropOptimizer without momentum: ms (initialised to ONES by TF) <- decay ms + (1 - decay) g^2; w <- w - lr g / sqrt(ms + eps)"""
    ms = decay * ms + (1.0 - decay) * g * g
    return w - lr * g / np.sqrt(ms + eps), ms
