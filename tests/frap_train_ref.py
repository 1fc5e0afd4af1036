"""Tests-only helpers of the fused MPLight update (resco_amd/csrc/resco_frap_train.h): a dtype-generic torch restatement of FRAP's
forward (FRAP.forward itself casts its input to float32, so a float64 module fails on it), kink-free replay rings, the truth --
MPLightLearner.loss and torch.optim.Adam evaluated by torch in float64 -- the yardstick, the Python twin of the minibatch draw, an
Adam adapter over FRAP's parameters, and the host build of the header's pieces (tests/frap_train_host).

The yardstick.  truth = float64; the device (and the host build) get 4 e_ref per tensor.  e_ref from ONE float32 evaluation is not
a usable bound for the tensors of 1 - 8 elements: with fresh weights the single-run e_ref of before_merge.bias and
relation_embedding.weight falls to a tenth of an ulp32 of the tensor's largest element, and a second, equally legitimate float32
evaluation lands many times that away.  So e_ref of a tensor is the MAXIMUM distance from the truth over a family of float32
evaluations -- the batch as drawn, the same on 7 row permutations, and the batch in chunks of 16 rows with the chunk gradients
accumulated in float32 -- floored at 1 ulp32 of the tensor's largest |truth|.  tests/test_frap_train_cpu.py asserts that every member
of the family is itself within 4 e_ref.  Everything asserted in here is asserted on the references alone."""
import ctypes as C
import functools

import numpy as np
import torch

import frap_ref as fr
from resco_amd.sim import _murmur
from train_ref import TAU, build_host

GAMMA, LR = 0.99, 1e-3
FRAP_TRAIN_SALT = 0x7B1D5C33        # resco_frap_train.h
N_PERMS, CHUNK = 7, 16
TILE_ROWS = 4                       # FPT_TM of resco_frap_train.h (tests/test_frap_train_cpu.py holds it to the header's)
# (P, D, T, N, S, B) of the device's minibatch test: P over both ends and the forward's three lane-group widths; B = 1, below one
# tile, across a tile boundary, two tiles and a ragged third, and two sizes of many tiles with a ragged last one
GPU_CASES = [(2, 1, 3, 4, 2, 1), (4, 4, 4, 5, 3, TILE_ROWS - 1), (5, 1, 5, 6, 3, TILE_ROWS + 1), (8, 4, 6, 7, 2, 2 * TILE_ROWS + 3),
             (13, 1, 8, 11, 4, 70), (16, 4, 4, 9, 3, 45)]


def names_of(net):
    return tuple(net.state_dict().keys())


def weights_as(net, dtype):
    """name -> leaf tensor of net's parameters in dtype (CPU), requiring grad"""
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_() for k, v in net.state_dict().items()}


def frap_forward(w, pairs, D, obs, want_pre=False):
    """FRAP.forward restated in the dtype of w (name -> tensor) on rows obs [B, 1 + 12 D] of the same dtype -> Q [B, P]; with
    want_pre also the pre-activations of the three ReLU layers that see the observation: movement [B, 12, 16], lane_conv and
    hidden_layer [B, P, P - 1, 20] (item (i, j): row i, the j-th other pair in ascending order)."""
    pairs_t = torch.tensor([[int(a), int(b)] for a, b in pairs], dtype=torch.long)
    P = pairs_t.shape[0]
    ph = obs[:, 0].to(torch.int64).clamp(0, P - 1)
    x = obs[:, 1:]
    pp = pairs_t[ph]
    mv = torch.arange(12)
    bits = ((mv[None, :] == pp[:, :1]) | (mv[None, :] == pp[:, 1:])).long()
    phase = torch.sigmoid(w['p.weight'][bits])
    win = torch.arange(12)[:, None] + torch.arange(D)[None, :]
    demand = torch.sigmoid(x[:, win] @ w['d.weight'].T + w['d.bias'])
    pre_e = torch.cat((phase, demand), -1) @ w['lane_embedding.weight'].T + w['lane_embedding.bias']
    e = torch.relu(pre_e)
    pair = e[:, pairs_t[:, 0]] + e[:, pairs_t[:, 1]]
    ii, jj = zip(*[(i, j) for i in range(P) for j in range(P) if i != j])
    comp = torch.tensor([int(len(set(pairs_t[i].tolist() + pairs_t[j].tolist())) == 3) for i, j in zip(ii, jj)])
    pre_lc = torch.cat((pair[:, list(ii)], pair[:, list(jj)]), -1) @ w['lane_conv.weight'].reshape(20, 32).T + w['lane_conv.bias']
    rel = torch.relu(torch.relu(w['relation_embedding.weight'][comp]) @ w['relation_conv.weight'].reshape(20, 4).T + w['relation_conv.bias'])
    pre_h = (torch.relu(pre_lc) * rel) @ w['hidden_layer.weight'].reshape(20, 20).T + w['hidden_layer.bias']
    y = torch.relu(pre_h) @ w['before_merge.weight'].reshape(20) + w['before_merge.bias'].reshape(())
    q = y.reshape(-1, P, P - 1).sum(-1)
    if want_pre:
        return q, pre_e, pre_lc.reshape(-1, P, P - 1, 20), pre_h.reshape(-1, P, P - 1, 20)
    return q


def relation_pre(w):
    """the pre-activations of the relation branch (they depend on the weights alone): relation_embedding [2, 4], relation_conv [2, 20]"""
    re = w['relation_embedding.weight']
    return re, torch.relu(re) @ w['relation_conv.weight'].reshape(20, 4).T + w['relation_conv.bias']


def _near_kinks(w64, pairs, D, obs, act):
    """bool [n]: a pre-activation of row (obs, action act) that carries gradient lies within TAU of zero"""
    with torch.no_grad():
        _, pre_e, pre_lc, pre_h = frap_forward(w64, pairs, D, torch.from_numpy(obs).double(), want_pre=True)
    n = obs.shape[0]
    g = torch.from_numpy(act).long()
    rows = torch.arange(n)
    near = (pre_e.abs() < TAU).flatten(1).any(-1) | (pre_lc[rows, g].abs() < TAU).flatten(1).any(-1) | (pre_h[rows, g].abs() < TAU).flatten(1).any(-1)
    return near.numpy()


def _draw_obs(P, D, n, rng):
    """rows [n, 1 + 12 D] float32: the phase column over -1 .. P (both clamps occur), demands as the simulator's (small counts; D = 4:
    fractions of them)"""
    ph = rng.integers(-1, P + 1, (n, 1)).astype(np.float64)
    dem = rng.integers(0, 9, (n, 12)).astype(np.float64) if D == 1 else np.abs(rng.normal(0.0, 2.0, (n, 12 * D)))
    return np.concatenate((ph, dem), -1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(P, D, T, N, S, seed=1, scale=2.0, done_slots=(1,)):
    """A kink-free ring of T slots x N environments x S signals for a FRAP of P synthetic phase pairs: dict(net, target, pairs, obs f32
    [T, N, S, W], act int16, rew f32 [T, N, S], done bool [T], sc: the scenario stand-in of frap_ref.synthetic_signal_set, valid bool [S, P]).  Every parameter is `scale` times its fresh draw (so that more than one
    unit of relation_embedding is alive); the rewards put the temporal-difference error of a row at 1.5 x a standard normal draw, so
    that about half of the rows fall on either branch of the Huber loss.  Shared and never changed."""
    rng = np.random.default_rng(1000 * P + 10 * D + seed)
    pairs, _, order, sc = fr.synthetic_signal_set(P, S, rng)
    net, target = fr.make_net(pairs, D, scale=scale, seed=seed), fr.make_net(pairs, D, scale=scale, seed=seed + 1000)
    w64, t64 = weights_as(net, torch.float64), weights_as(target, torch.float64)
    n = T * N * S
    obs = _draw_obs(P, D, n, rng)
    act = rng.integers(0, P, n).astype(np.int16)
    for _ in range(200):
        hit = _near_kinks(w64, pairs, D, obs, act)
        if not hit.any():
            break
        obs[hit] = _draw_obs(P, D, int(hit.sum()), rng)
    assert not _near_kinks(w64, pairs, D, obs, act).any(), 'the case generator left a kink'
    for pre in relation_pre(w64):
        assert (pre.abs() > TAU).all(), 'a relation unit sits on its kink: choose another seed'
    with torch.no_grad():
        o = torch.from_numpy(obs)
        for a, b in zip(frap_forward(w64, pairs, D, o.double(), True)[1:], frap_forward(weights_as(net, torch.float32), pairs, D, o, True)[1:]):
            rows = torch.arange(n)
            sel = (lambda t: t) if a.dim() == 3 else (lambda t: t[rows, torch.from_numpy(act).long()])
            assert torch.equal(sel(a) > 0, sel(b) > 0), 'float32 and float64 disagree on a ReLU mask'
        y = frap_forward(w64, pairs, D, o.double()).gather(-1, torch.from_numpy(act).long().unsqueeze(-1)).squeeze(-1).reshape(T, N, S)
        nxt = frap_forward(t64, pairs, D, o.double()).max(-1).values.reshape(T, N, S)
    done = np.zeros(T, bool)
    done[[t for t in done_slots if t < T]] = True
    boot = GAMMA * torch.roll(nxt, -1, 0) * torch.from_numpy(~done).double().reshape(T, 1, 1)
    rew = (y - boot).numpy() + 1.5 * rng.standard_normal((T, N, S))
    W = 1 + 12 * D
    valid = np.zeros((S, P), bool)
    for s in range(S):
        valid[s, order[s][order[s] >= 0]] = True
    return dict(net=net, target=target, pairs=pairs, P=P, D=D, obs=obs.reshape(T, N, S, W), act=act.reshape(T, N, S),
                rew=rew.astype(np.float32), done=done, sc=sc, valid=valid)


def draw_idx(c, B, seed=0, slots=None):
    """B rows (t, e, s) of the case's ring, int32 [B, 3]"""
    T, N, S = c['obs'].shape[:3]
    rng = np.random.default_rng(B + 7919 * seed)
    t = rng.integers(0, T, B) if slots is None else rng.choice(np.asarray(slots), B)
    return np.stack([t, rng.integers(0, N, B), rng.integers(0, S, B)], -1).astype(np.int32)


def batch_of(c, idx, dtype):
    """(o, g, r, o2, d) of MPLightReplay.sample's shapes for idx [B, 3]; the successor of a row whose slot ended an episode is all
    zeros (whatever the ring holds there: the bootstrap is cut, so it must never matter); actions clamped as the kernel clamps them"""
    idx = np.asarray(idx)
    T = c['obs'].shape[0]
    t, e, s = idx[:, 0], idx[:, 1], idx[:, 2]
    d = c['done'][t]
    o2 = c['obs'][(t + 1) % T, e, s].copy()
    o2[d] = 0
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    g = np.clip(c['act'][t, e, s].astype(np.int64), 0, c['P'] - 1)
    return f(c['obs'][t, e, s]).to(dtype), f(g), f(c['rew'][t, e, s]).to(dtype), f(o2).to(dtype), f(d).to(dtype)


def _per_row_loss(w, wt, c, batch, mask=None):
    """MPLightLearner.loss restated on frap_forward -> (Huber terms [B], delta [B]); the target's max runs over ALL P outputs (mask: bool
    [B, P], the outputs a WRONG learner would restrict it to)"""
    o, g, r, o2, d = batch
    y = frap_forward(w, c['pairs'], c['D'], o).gather(-1, g.unsqueeze(-1)).squeeze(-1)
    with torch.no_grad():
        q2 = frap_forward(wt, c['pairs'], c['D'], o2)
        if mask is not None:
            q2 = q2.masked_fill(~torch.from_numpy(mask), float('-inf'))
        tgt = r + GAMMA * (1.0 - d) * q2.max(dim=-1).values
    return torch.nn.functional.smooth_l1_loss(y, tgt, reduction='none'), (y - tgt).detach()


def torch_grads(c, idx, dtype, chunk=None, target=None, masked=False):
    """The mean Huber loss on rows idx [B, 3] in dtype and its backward -> (dict name -> float64 numpy gradient, float64 loss, float64
    numpy delta [B]).  chunk: the rows in chunks of that many, the chunk gradients accumulated in dtype (autograd's .grad).  masked: the target's max over the signal's valid pairs only -- what the update must NOT compute."""
    w = weights_as(c['net'], dtype)
    wt = {k: v.detach() for k, v in weights_as(c['target'] if target is None else target, dtype).items()}
    B = len(idx)
    step = B if chunk is None else int(chunk)
    total, deltas = torch.zeros((), dtype=dtype), []
    for i in range(0, B, step):
        per, delta = _per_row_loss(w, wt, c, batch_of(c, idx[i:i + step], dtype), c['valid'][idx[i:i + step, 2]] if masked else None)
        part = per.sum() / B
        part.backward()
        total = total + part.detach()
        deltas.append(delta)
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().double().numpy() for k, v in w.items()}
    return grads, float(total.double()), torch.cat(deltas).double().numpy()


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(P, D, T, N, S, B, slots=None, seed=1):
    """(idx, truth gradients, e_ref per tensor, truth loss, e_ref of the loss, the float32 family, delta64): computed once, shared,
    never changed.  family: list of (label, gradients, loss)."""
    c = case(P, D, T, N, S, seed=seed)
    idx = draw_idx(c, B, slots=slots)
    g64, l64, d64 = torch_grads(c, idx, torch.float64)
    rng = np.random.default_rng(B)
    family = [('as drawn',) + torch_grads(c, idx, torch.float32)[:2]]
    for k in range(N_PERMS):
        family.append(('permutation %d' % k,) + torch_grads(c, idx[rng.permutation(B)], torch.float32)[:2])
    family.append(('chunks of %d' % CHUNK,) + torch_grads(c, idx, torch.float32, chunk=CHUNK)[:2])
    e_ref = {k: max(max(np.abs(g[k] - g64[k]).max() for _, g, _ in family), float(ulp32(np.abs(g64[k]).max()))) for k in g64}
    e_loss = max(max(abs(l - l64) for _, _, l in family), float(ulp32(l64)))
    return idx, g64, e_ref, l64, e_loss, family, d64


def huber_fraction(d64):
    return float((np.abs(d64) > 1).mean())


def compare(names, got, loss, g64, e_ref, l64, e_loss, who='dev'):
    """every tensor finite and within 4 e_ref of the truth, entries that are exactly zero in the truth exactly zero -> the list of
    tensors that are not, for the caller to assert empty; prints every figure"""
    worst = []
    for k in names:
        g = np.asarray(got[k], np.float64).reshape(g64[k].shape)
        assert np.isfinite(g).all(), k
        err = np.abs(g - g64[k]).max()
        print('  %-28s max |truth| %.3e  |%s - truth| %.3e  e_ref %.3e  ratio %.2f' % (k, np.abs(g64[k]).max(), who, err, e_ref[k], err / e_ref[k]))
        if err > 4 * e_ref[k]:
            worst.append((k, err, e_ref[k]))
        if (g[g64[k] == 0] != 0).any():
            worst.append((k, 'non-zero where the truth is exactly zero'))
    if loss is not None:
        err = abs(float(loss) - l64)
        print('  %-28s truth %.6e  |%s - truth| %.3e  e_ref %.3e  ratio %.2f' % ('loss', l64, who, err, e_loss, err / e_loss))
        if err > 4 * e_loss:
            worst.append(('loss', err, e_loss))
    return worst


def unpack(flat, net):
    """packed vector (numpy) -> dict name -> array of the parameter's shape"""
    out, off = {}, 0
    for k, v in net.state_dict().items():
        out[k] = np.asarray(flat[off:off + v.numel()]).reshape(tuple(v.shape))
        off += v.numel()
    assert off == len(flat)
    return out


# ---- Adam from given gradients over FRAP's parameters (train_ref.adam_step asks for a network of the stacked trunk's class)
def adam_name(k):
    return k.replace('.', '__')


class _Params(torch.nn.Module):
    def __init__(self, state_dict, dtype):
        super().__init__()
        for k, v in state_dict.items():
            self.register_parameter(adam_name(k), torch.nn.Parameter(v.detach().cpu().to(dtype).clone()))


def adam_step(net, grads, state, dtype, lr=LR):
    """torch.optim.Adam(lr).step from GIVEN gradients (name -> array) in dtype; net: a FRAP (read when state is None); state: what the
    previous call returned, or None -> dict(net, opt) as train_ref.state_arrays / assert_adam_state read it, the parameters named
    adam_name(k)"""
    if state is None:
        holder = _Params(net.state_dict(), dtype)
        state = dict(net=holder, opt=torch.optim.Adam(holder.parameters(), lr=lr))
    for k, p in state['net'].named_parameters():
        p.grad = torch.as_tensor(np.asarray(grads[k.replace('__', '.')])).to(dtype).reshape(p.shape).clone()
    state['opt'].step()
    return state


# ---- the draw
def predict_sample(seed, u, T, N, S, head, count, B):
    """the minibatch rs_mplight_dqn_sample draws for update u: int32 [B, 3] of (slot, environment, signal)"""
    idx = np.zeros((B, 3), np.int32)
    sd = (seed ^ FRAP_TRAIN_SALT) & 0xFFFFFFFF
    for i in range(B):
        k = _murmur(sd, (u, i, 0, 0)) % (count - 1)
        idx[i] = ((head - count + k) % T, _murmur(sd, (u, i, 0, 1)) % N, _murmur(sd, (u, i, 0, 2)) % S)
    return idx


def check_sample(idx, T, N, S, head, count):
    """what every minibatch must satisfy, whoever drew it"""
    t, e, s = idx[:, 0], idx[:, 1], idx[:, 2]
    assert ((t >= 0) & (t < T) & (e >= 0) & (e < N) & (s >= 0) & (s < S)).all()
    assert (t != (head - 1) % T).all(), 'the newest slot has no successor yet'
    if count < T:
        assert (t < count).all(), 'an unwritten slot was drawn'


def build_frap_train_host(out_dir):
    vp, i32, u32, f32 = C.c_void_p, C.c_int32, C.c_uint32, C.c_float
    return build_host('frap_train', out_dir, dict(frap_train_grad=[vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, C.c_double, vp, vp, vp],
                                                  frap_train_sample=[u32, u32, i32, i32, i32, i32, i32, i32, vp],
                                                  frap_train_tile_rows=[]))


def host_grads(host, c, idx, dy_out=None):
    """frap_train_grad on the case's ring -> (dict name -> float32 gradient, float32 loss); dy_out: float32 [B] for the rows' dy"""
    from resco_amd.agents.mplight import pack_mplight_weights
    w, wt = (np.ascontiguousarray(pack_mplight_weights(n).numpy(), np.float32) for n in (c['net'], c['target']))
    T, N, S = c['obs'].shape[:3]
    arrs = [np.ascontiguousarray(c['obs'], np.float32), np.ascontiguousarray(c['act'], np.int16), np.ascontiguousarray(c['rew'], np.float32),
            np.ascontiguousarray(c['done'], np.uint8), np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(c['pairs'], np.int32)]
    grad, loss = np.full(len(w), np.nan, np.float32), np.full(1, np.nan, np.float32)
    p = lambda a: a.ctypes.data
    rc = host.frap_train_grad(p(w), p(wt), c['D'], c['P'], p(arrs[5]), p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), T, N, S, p(arrs[4]), len(idx),
                              GAMMA, p(grad), p(loss), p(dy_out) if dy_out is not None else None)
    assert rc == 0
    return unpack(grad, c['net']), float(loss[0])
