"""Tests-only reference of the fused IDQN forward (rs_idqn_forward_kernel, resco_amd/csrc/resco_policy.h) that rounds where the
kernel rounds.

Plain numpy in float64.  It takes the arrays `pack_idqn_weights` produces -- what rs_idqn_create receives -- and reads the packed
MFMA fragments with the kernel's own index arithmetic, so the host runs the kernel's layout for every lmax and head size HP.

With `rounding=True`:
  * conv weights and bias go to fp16 (round to nearest even), each conv feature is the kernel's fp16 FMA chain
    fma(w00, x[h][w], b) -> + w01 x[h][w+1] -> + w10 x[h+1][w] -> + w11 x[h+1][w+1], every step rounded to fp16, then ReLU;
  * fc1 / fc2 / fc3 have fp16 operands and exact (float64) sums; after fc1 and fc2: + fp32 bias, ReLU, round to fp16;
  * Q = sum + b3.
With `rounding=False` nothing is rounded beyond the fp16 operands the packed arrays already hold: the float64 forward of the same
network.

Alongside Q comes an element-wise bound on |Q_kernel - Q_ref| derived from the arithmetic: fp32 accumulation along the kernel's own
MFMA chains (accumulation_error), the fp16 neighbour a rounded activation may reach when the device's fp32 sum lies on the other side
of a rounding boundary, both propagated through the next layers with |W|.  The accumulation model assumes that one MFMA adds its
8 exact fp16 products with at most 8 fp32 roundings; the textbook n_products * 2^-24 * sum|a b| per dot product needs no such
assumption, but with n = 4096 products in fc1 it exceeds the whole effect of the fp16 rounding.

`select_actions` restates the kernel's epilogue (greedy first maximum, epsilon-greedy draw, mode-1 categorical draw) on any Q array.
"""
import numpy as np

from resco_amd.sim import _murmur

QMAX = 8                    # POL_QMAX
U32 = 2.0 ** -24            # unit roundoff of fp32
SALT = 0x1D0A17             # seed ^ SALT keys the policy's draws (resco_policy.h:248, 253-254)


def make_net(lmax, seed=0, cls=None):
    """A BatchedIDQN (or `cls`, e.g. BatchedIPPO) of max(lmax - 1, 8) signals that covers every lane count 2..lmax and every action
    count 1..8, paired differently, initialised like the reference.  Returns (net, the per-signal modules)."""
    if cls is None:
        from resco_amd.agents.idqn_rollout import BatchedIDQN as cls
    S = max(lmax - 1, 8)
    lanes = [2 + s % (lmax - 1) for s in range(S)]
    lanes[-1] = lmax
    actions = [1 + (3 * s) % 8 for s in range(S)]
    net = cls(lanes, actions)
    mods = net.init_like_reference(seed=seed)
    return net, mods


def random_obs(lanes, lmax, n, rng):
    """fp16 observations in [0, 1), zero past each signal's lanes"""
    obs = np.zeros((n, len(lanes), lmax, 5), np.float16)
    for s, L in enumerate(lanes):
        obs[:, s, :L] = rng.random((n, L, 5)).astype(np.float16)
    return obs


def _r16(x):
    return x.astype(np.float16).astype(np.float64)


def fc1_fragment_index(S, lmax):
    """[S, 64 channels, hp k-steps, 2 n-tiles, 64 lanes] -> index of the h4 fragment in the flat w1 buffer, exactly as the kernel
    forms it: wg = w1 + ((s * 64 * hp * 2 + nh) * 64 + lane), fragment (c, kk) at wg + (c * hp + kk) * 128 (resco_policy.h:149-150,
    157, 179), hp = lmax // 2 (rs_idqn_create)."""
    hp = lmax // 2
    s, c, kk, nh, lane = np.ix_(np.arange(S), np.arange(64), np.arange(hp), np.arange(2), np.arange(64))
    return ((s * 64 * hp * 2 + nh) * 64 + lane) + (c * hp + kk) * 128


def dense_fc1(w1, S, lmax):
    """fc1 weights as the kernel multiplies them: [S, 64 channels, hp, 2 (g), 4 (j), 64 outputs].  The A fragment of lane l holds
    row h = 2 kk + g, column w = j (g = l >> 5, resco_policy.h:121, 171); B column i = l & 31 of n-tile nh is output nh * 32 + i."""
    hp = lmax // 2
    flat = np.asarray(w1).reshape(-1, 4).astype(np.float64)
    idx = fc1_fragment_index(S, lmax)                                   # [S, 64, hp, 2 nh, 64 lane]
    frag = flat[idx]                                                    # [S, 64, hp, nh, lane, j]
    frag = frag.reshape(S, 64, hp, 2, 2, 32, 4)                         # lane -> (g, i)
    return frag.transpose(0, 1, 2, 4, 6, 3, 5).reshape(S, 64, hp, 2, 4, 64)     # [S, c, kk, g, j, nh * 32 + i]


def dense_fc23(w, S, n_tiles):
    """fc2 (n_tiles 2) / fc3 (1): the A fragment of k-step kk reads y[i][kk * 8 + g * 4 + j], the B fragment is
    w[(kk * n_tiles + nh) * 64 + lane] of the signal's block (resco_policy.h:201-205, 222-226) -> [S, 64 inputs, 32 * n_tiles]."""
    flat = np.asarray(w).reshape(S, -1, 4).astype(np.float64)
    kk, nh, lane = np.ix_(np.arange(8), np.arange(n_tiles), np.arange(64))
    frag = flat[:, (kk * n_tiles + nh) * 64 + lane]                    # [S, kk, nh, lane, j]
    frag = frag.reshape(S, 8, n_tiles, 2, 32, 4)                        # lane -> (g, i)
    return frag.transpose(0, 1, 3, 5, 2, 4).reshape(S, 64, 32 * n_tiles)


def conv_features(w, s, obs, hp_s, rounding=True):
    """The conv features one signal's k-steps feed into fc1: [n, 64, hp_s, 2, 4] (channel, kk, g, j) for row h = 2 kk + g, column j.
    obs: [n, lmax, 5] of signal s.  Rows h >= lmax - 1 see zero inputs (resco_policy.h:124-125): relu(bias), multiplied by the
    zero fc1 rows the packing puts there."""
    n, lmax = obs.shape[0], obs.shape[1]
    H = lmax - 1
    r = _r16 if rounding else (lambda a: a)
    x = np.zeros((n, 2 * hp_s + 1, 5))
    rows = min(lmax, 2 * hp_s + 1)                                     # the staged rows (resco_policy.h:99-111)
    x[:, :rows] = obs[:, :rows]
    h = np.arange(2 * hp_s)
    valid = (h < H)[None, :, None]
    x0 = np.where(valid, x[:, h], 0.0)                                  # [n, h, 5]: rows h, h + 1 as the lane holds them
    x1 = np.where(valid, x[:, h + 1], 0.0)
    cw = r(w['conv_w'][s].astype(np.float64))                           # (_Float16) casts of resco_policy.h:143-145
    cb = r(w['conv_b'][s].astype(np.float64))
    w00, w01, w10, w11 = (cw[:, k][None, :, None, None] for k in range(4))
    b = cb[None, :, None, None]
    a00, a01 = x0[:, None, :, 0:4], x0[:, None, :, 1:5]                # [n, 1, h, w]
    a10, a11 = x1[:, None, :, 0:4], x1[:, None, :, 1:5]
    f = r(w00 * a00 + b)                                                # the packed FMA chain of resco_policy.h:166-170
    f = r(w01 * a01 + f)
    f = r(w10 * a10 + f)
    f = r(w11 * a11 + f)
    f = np.maximum(f, 0.0)                                              # [n, 64, 2 hp_s, 4]
    return f.reshape(n, 64, hp_s, 2, 4)


def fc1_accumulators(hp_s):
    """the accumulator (0 / 1) each fc1 MFMA (c, kk) adds into: (kk + d * HP) & 1 with d = c mod D, the register ring's depth
    (resco_policy.h:151, 173-174; POL_RING = 16)"""
    D = 2 if hp_s >= 5 else (4 if hp_s >= 3 else (8 if hp_s == 2 else 16))
    c, kk = np.meshgrid(np.arange(64), np.arange(hp_s), indexing='ij')
    return ((kk + (c % D) * hp_s) & 1).reshape(-1)


def accumulation_error(y, my, Wt, acc_of_step, e_in, chunk=128):
    """Bound on the fp32 accumulation error of the kernel's MFMA chains u = sum over k-steps of (8 exact fp16 products).

    One v_mfma_f32_32x32x8_f16 adds 8 products to an accumulator: at most 8 fp32 additions, each off by at most 2 u (u = 2^-24,
    2 u even if the unit truncates) of a magnitude <= |acc before| + sum|products of the step|.  |acc before| is the exact partial
    sum of that accumulator in the kernel's order (k-step by k-step, acc_of_step: which of the accumulators) plus e_in, what the
    device's own operands may change; the merge of two accumulators adds one more rounding.  y: [n, K] operands, my >= |y_dev|,
    Wt [K, O], K = 8 * k-steps."""
    n, K = y.shape
    steps, O = K // 8, Wt.shape[1]
    Wk, Wa = Wt.reshape(steps, 8, O), np.abs(Wt).reshape(steps, 8, O)
    out = np.zeros((n, O))
    n_acc = int(acc_of_step.max()) + 1
    for m0 in range(0, n, chunk):
        sl = slice(m0, m0 + chunk)
        P = np.matmul(y[sl].reshape(-1, steps, 8).transpose(1, 0, 2), Wk)          # [steps, n, O]: each MFMA's contribution
        Pa = np.matmul(my[sl].reshape(-1, steps, 8).transpose(1, 0, 2), Wa)
        err = 16 * U32 * Pa.sum(0)
        finals = 0.0
        for a in range(n_acc):
            Pk = P[acc_of_step == a]
            prev = np.cumsum(Pk, axis=0) - Pk                                       # the accumulator before each of its MFMAs
            err += 16 * U32 * (np.abs(prev).sum(0) + len(Pk) * e_in[sl])
            finals = finals + np.abs(Pk.sum(0))
        if n_acc > 1:
            err += 2 * U32 * (finals + e_in[sl])
        out[sl] = err
    return out


def idqn_kernel_ref(w, lanes, obs, n_envs, rounding=True):
    """Q-values [n_envs, S, 8] (-inf beyond a signal's actions) and their error bound [n_envs, S, 8] (0 where -inf).

    w: the dict of pack_idqn_weights (the arrays rs_idqn_create takes); lanes: the per-signal lane counts the kernel was told
    (rs_idqn_set_lanes: hp_sig = lanes // 2 k-steps per channel run); obs: fp16 observations [>= n_envs, S, lmax, 5]."""
    obs = np.asarray(obs)
    assert obs.dtype == np.float16
    S, lmax = obs.shape[1], obs.shape[2]
    n = n_envs
    x = obs[:n].astype(np.float64)
    W1 = dense_fc1(w['w1'], S, lmax)
    W2, W3 = dense_fc23(w['w2'], S, 2), dense_fc23(w['w3'], S, 1)[:, :, :QMAX]
    b1, b2 = w['b1'].astype(np.float64), w['b2'].astype(np.float64)
    b3 = w['b3'].astype(np.float64)[:, :QMAX]
    r = _r16 if rounding else (lambda a: a)
    q = np.full((n, S, QMAX), -np.inf)
    bound = np.zeros((n, S, QMAX))

    def layer(y, ey, Wt, bias, acc_of_step, last=False):
        """fp32-accumulated dot products of fp16 operands: u = y W + bias, and the bound on |u_dev - u_ref| given |y_dev - y| <= ey"""
        u = y @ Wt + bias
        e_in = ey @ np.abs(Wt)                                          # what the device's own activations change
        eu = e_in + accumulation_error(y, np.abs(y) + ey, Wt, acc_of_step, e_in)
        eu = 1.01 * (eu + 2 * U32 * (np.abs(u) + eu))                   # + the fp32 bias add (1 %: second-order terms)
        if last:
            return u, eu
        # ReLU and the fp16 cast are monotone: the device's activation lies between those of u - eu and u + eu, so it can be
        # off by at most the distance to the fp16 neighbour those reach (one ulp where the device's fp32 sum may round the other
        # way, nothing where no rounding boundary is within eu, nothing for a unit that is dead either way)
        relu_r = lambda v: r(np.maximum(v, 0.0))
        y = relu_r(u)
        return y, np.maximum(y - relu_r(u - eu), relu_r(u + eu) - y)

    for s in range(S):
        hs = int(lanes[s]) // 2                                         # hp_sig (rs_idqn_set_lanes)
        na = int(w['n_actions'][s])
        f = conv_features(w, s, x[:, s], hs, rounding).reshape(n, -1)      # [n, 64 * hs * 8] in (c, kk, g, j) order
        Wf = W1[s, :, :hs].reshape(-1, 64)
        y1, e1 = layer(f, np.zeros_like(f), Wf, b1[s], fc1_accumulators(hs))
        y2, e2 = layer(y1, e1, W2[s], b2[s], np.zeros(8, np.int64))
        qs, eq = layer(y2, e2, W3[s], b3[s], np.zeros(8, np.int64), last=True)
        q[:, s, :na] = qs[:, :na]
        bound[:, s, :na] = eq[:, :na]
    return q, bound


def first_max(q, n_actions):
    """greedy action: the first maximum over a < na, strict > (resco_policy.h:240-242)"""
    n_actions = np.asarray(n_actions)
    best = np.zeros(q.shape[:-1], np.int64)
    bq = q[..., 0].copy()
    for a in range(1, QMAX):
        take = (a < n_actions) & (q[..., a] > bq)
        best = np.where(take, a, best)
        bq = np.where(take, q[..., a], bq)
    return best


def u01(h):
    return np.float32(h >> 8) * np.float32(1.0 / 16777216.0)       # d_u01


def select_actions(q, n_actions, mode=0, eps=0.0, seed=0, env_base=0, step_key=0):
    """The kernel's epilogue on Q-values q [n, S, 8] (resco_policy.h:235-255).  Returns (actions [n, S], margin [n, S]): in mode 1
    margin = the distance of u z from the nearest cumulative boundary over z (the host's exp is not the device's __expf: rows with
    a small margin may fall either way), +inf elsewhere."""
    n, S = q.shape[0], q.shape[1]
    n_actions = np.asarray(n_actions)
    greedy = first_max(q, n_actions)
    act = greedy.copy()
    margin = np.full((n, S), np.inf)
    key, hs = (seed ^ SALT) & 0xFFFFFFFF, step_key & 0xFFFFFFFF
    if mode == 1:
        for m in range(n):
            for s in range(S):
                na = int(n_actions[s])
                e = np.exp(q[m, s, :na].astype(np.float64) - q[m, s, greedy[m, s]])
                z = e.sum()
                t = float(u01(_murmur(key, ((env_base + m) & 0xFFFFFFFF, s, hs, 2)))) * z
                cum = np.cumsum(e)
                hit = np.nonzero(t < cum)[0]
                act[m, s] = hit[0] if len(hit) else na - 1
                margin[m, s] = np.abs(t - cum[:-1]).min() / z if na > 1 else np.inf
    elif eps > 0.0:
        e32 = np.float32(eps)
        for m in range(n):
            for s in range(S):
                words = ((env_base + m) & 0xFFFFFFFF, s, hs)
                if u01(_murmur(key, words + (0,))) < e32:
                    act[m, s] = _murmur(key, words + (1,)) % int(n_actions[s])
    return act, margin
