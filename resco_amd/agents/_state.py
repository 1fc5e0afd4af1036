"""What the state_dict() / load_state_dict() of the learners, policies, rings and trainers share (resco_amd/checkpoint.py writes
and reads what they return).

The one rule: loading copies INTO the existing storages (`copy_`) and never rebinds a tensor or `.data` -- the library has
borrowed the device pointers of the parameters, targets, gradients and moments (learn_fused.FusedLearnerBase._create), of the flat
vectors of FusedMPLightLearner and of the policies' packed buffers, and a rebind would leave the kernels reading the old memory
without any error.  A state dict holds only tensors (references to the live ones: the writer moves them to the CPU) and plain
Python scalars, lists and dicts; an object's weights sit under 'weights' (all a strict=False load reads), the rest under 'state'.
"""
import torch


@torch.no_grad()
def copy_into(dst, src, name):
    """dst <- src in place; shape and dtype must be dst's (the device may differ)"""
    if not torch.is_tensor(src) or tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
        got = '%s %s' % (tuple(src.shape), src.dtype) if torch.is_tensor(src) else type(src).__name__
        raise ValueError('%s: the checkpoint holds %s, the object %s %s' % (name, got, tuple(dst.shape), dst.dtype))
    dst.copy_(src)


def copy_dict_into(dst, src, name):
    """every tensor of the dict dst <- the tensor of that name in src, in place"""
    if sorted(dst) != sorted(src):
        raise ValueError('%s: the checkpoint holds the tensors %s, the object %s' % (name, sorted(src), sorted(dst)))
    for k, t in dst.items():
        copy_into(t, src[k], '%s.%s' % (name, k))


def module_tensors(module):
    """name -> the module's own parameter and buffer tensors (nn.Module.state_dict: references, detached)"""
    return dict(module.state_dict())


def load_module(module, tensors, name):
    """nn.Module.load_state_dict without its rebinding corner cases: a plain copy_ into every parameter and persistent buffer"""
    copy_dict_into(module_tensors(module), tensors, name)


# ---- torch.optim.Adam, in a layout of our own (the optimizer's own state_dict carries tuples and None)
def adam_state(opt):
    """{'step': [float per parameter], 'exp_avg': [...], 'exp_avg_sq': [...]} in parameter order.  Before the first step torch has
    created nothing: step 0 and zero moments stand for it (what the first step starts from), so the shapes never depend on it."""
    params = [p for g in opt.param_groups for p in g['params']]
    have = [p for p in params if len(opt.state.get(p, {}))]
    if not have:
        return {'step': [0.0] * len(params), 'exp_avg': [torch.zeros_like(p) for p in params], 'exp_avg_sq': [torch.zeros_like(p) for p in params]}
    assert len(have) == len(params), 'an Adam state that covers only some of the parameters'
    return {'step': [float(opt.state[p]['step']) for p in params], 'exp_avg': [opt.state[p]['exp_avg'] for p in params],
            'exp_avg_sq': [opt.state[p]['exp_avg_sq'] for p in params]}


@torch.no_grad()
def load_adam_state(opt, sd, name):
    """into the optimizer's EXISTING state tensors (a graph-captured update keeps reading them); a parameter without state yet gets
    what torch.optim.Adam's own first step would create"""
    params = [p for g in opt.param_groups for p in g['params']]
    if not (len(sd['step']) == len(sd['exp_avg']) == len(sd['exp_avg_sq']) == len(params)):
        raise ValueError('%s: the checkpoint holds Adam state of %d parameters, the optimizer has %d' % (name, len(sd['step']), len(params)))
    for i, (p, group) in enumerate((p, g) for g in opt.param_groups for p in g['params']):
        st = opt.state[p]
        if not len(st):
            on_dev = bool(group.get('capturable')) or bool(group.get('fused'))
            st['step'] = torch.zeros((), dtype=torch.float32, device=p.device) if on_dev else torch.tensor(0.0, dtype=torch.float32)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        for k in ('exp_avg', 'exp_avg_sq'):
            copy_into(st[k], sd[k][i], '%s.%s[%d]' % (name, k, i))
        st['step'].fill_(float(sd['step'][i]))


# ---- the replay rings (idqn_learn.DeviceReplay, mplight.MPLightReplay)
def ring_signature(rp):
    return {'capacity': rp.T, 'n_envs': rp.N, 'n_signals': rp.S}


def ring_state(rp, replay=True):
    """the ring and its position; replay=False: an EMPTY ring (head = count = 0, no arrays)"""
    if not replay:
        return {'state': {'head': 0, 'count': 0}}
    return {'state': {'obs': rp.obs, 'act': rp.act, 'rew': rp.rew, 'done': rp.done, 'head': int(rp.head), 'count': int(rp.count)}}


def load_ring_state(rp, sd, name):
    st = sd['state']
    head, count = int(st['head']), int(st['count'])
    if not (0 <= head < rp.T and 0 <= count <= rp.T):
        raise ValueError('%s: head %d / count %d lie outside a ring of %d slots' % (name, head, count, rp.T))
    if 'obs' in st:
        for k in ('obs', 'act', 'rew', 'done'):
            copy_into(getattr(rp, k), st[k], '%s.%s' % (name, k))
    elif head or count:
        raise ValueError('%s: a ring position (%d, %d) without the ring' % (name, head, count))
    rp.head, rp.count = head, count
    if hasattr(rp, '_pos'):         # DeviceReplay mirrors its position on the device for the graph-captured PyTorch learner
        rp._pos[0] = head
        rp._pos[1] = count


def fused_counter_state(learner):
    """the library's Adam step count of a fused learner (0 before the handle exists)"""
    return int(learner.n_updates)


def set_fused_counter(learner, t, name):
    """rs_*_set_steps: the handle's counter <- t (the bias-correction step and, for the DQN learners, the key of the next draw)"""
    t = int(t)
    if learner._h is None:
        if t:
            raise ValueError('%s: the learner has no library handle yet, its step count (%d) cannot be restored' % (name, t))
        return
    fn = getattr(learner._lib, learner.PREFIX + '_set_steps', None)
    if fn is None:
        raise RuntimeError('the loaded library has no %s_set_steps: rebuild it (there is no CPU fallback)' % learner.PREFIX)
    if fn(learner._h, t) != 0:
        learner._fail(learner.PREFIX + '_set_steps', -1)
