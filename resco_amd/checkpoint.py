"""Checkpoints of device training: one file format, loud refusals.

    save(path, agent=..., map_name=..., objects={...}, progress={...}, replay=True)
    progress = load(path, agent=..., map_name=..., objects={...}, strict=True)

`objects` is name -> whatever holds training state: the networks (nn.Module: BatchedIDQN, FRAP, BatchedIPPO, BatchedFMA2C), the
learners, the fused policies, the rings and segments, the trainers, `torch.Generator`s, and the environments (VecMultiSignal), which
contribute only their shape to the signature.  List a network before the learner and the policy that read it: objects are loaded in
the order given, and a policy re-packs what its network holds when its turn comes.  Everything except a module, a generator and an
environment has `state_dict()` -> {'weights': {...}, 'state': {...}} and `load_state_dict(sd, weights_only=False)`, and may have
`signature()` -> the hyper-parameters that shape the trajectory (agents/_state.py has the rule they all follow: load IN PLACE).

The file is ONE torch.save of tensors (moved to the CPU) and plain Python scalars, lists and dicts -- no class is pickled, so
`torch.load(path, weights_only=True)` reads it:

    {'format': 1, 'signature': {'agent', 'map', 'replay', 'objects': [names], 'fields': {'name.field': value},
                                'tensors': {'name/path': [shape, dtype]}}, 'objects': {name: state dict}, 'progress': {...}}

`load` builds the same signature from the live objects and compares it BEFORE it touches anything; a mismatch raises a ValueError
that names the field and both values.  strict=False (evaluation, fine-tuning): every object given must be in the file, only the
networks' shapes must match and only weights are loaded.  Checkpoints are taken at an episode boundary: `save` refuses an
environment inside an episode.  replay=False leaves the DQN ring out (ingolstadt21 x 1024 at 2048 slots is 7.5 GB); the loaded ring
is then empty and the resumed run is a valid continuation, not the same one.

    progress = load_frap_weights(path, net)

takes FRAP weights ACROSS maps: a FRAP's tensors do not depend on its map, so the network of any MPLight, MPLightFULL or multi-map
MPLight checkpoint loads into a FRAP of any number of phase pairs (only demand_shape and the tensor shapes are compared).
"""
import os

import torch
import torch.nn as nn

FORMAT = 1


# ---------------------------------------------------------------------------------------------- what an object contributes
def _is_env(obj):
    return hasattr(obj, 'horizon_steps') and hasattr(obj, 'steps') and hasattr(obj, 'n_envs')


def _module_fields(m):
    """the shape of a network, from the attributes the four network classes carry"""
    out = {}
    for k in ('lanes', 'actions', 'lmax', 'amax', 'oshape', 'demand_shape'):
        if hasattr(m, k):
            v = getattr(m, k)
            out[k] = [int(x) for x in v] if isinstance(v, (list, tuple)) else int(v)
    if hasattr(m, 'layout'):
        out.update(K=int(m.layout.K), M=int(m.layout.M), W=int(m.layout.W))
    return out


def _state_of(obj, replay):
    """(fields, state dict) of one object; the state dict holds references to the live tensors"""
    if _is_env(obj):
        return {'n_envs': int(obj.n_envs), 'n_signals': int(obj.n_signals), 'horizon_steps': int(obj.horizon_steps)}, {}
    if isinstance(obj, torch.Generator):
        return {}, {'state': {'rng': obj.get_state()}}
    if isinstance(obj, nn.Module):
        return _module_fields(obj), {'weights': dict(obj.state_dict())}
    if not hasattr(obj, 'state_dict') and hasattr(obj, 'signature'):
        return dict(obj.signature()), {}                # e.g. DeviceTrainer: no counters of its own
    if not hasattr(obj, 'state_dict'):
        raise TypeError('%s has no state_dict(): it cannot be part of a checkpoint' % type(obj).__name__)
    fields = dict(obj.signature()) if hasattr(obj, 'signature') else {}
    # a ring, or a learner whose state beside the ring is saved with it only (the priorities of FusedDQNLearner and FusedMPLightLearner)
    with_replay = (hasattr(obj, 'head') and hasattr(obj, 'count')) or getattr(obj, 'STATE_FOLLOWS_REPLAY', False)
    return fields, (obj.state_dict(replay=replay) if with_replay else obj.state_dict())


def _walk(x, path, out):
    """path -> [shape, dtype] of every tensor below x"""
    if torch.is_tensor(x):
        out[path] = [[int(d) for d in x.shape], str(x.dtype)]
    elif isinstance(x, dict):
        for k, v in x.items():
            _walk(v, '%s/%s' % (path, k), out)
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _walk(v, '%s/%d' % (path, i), out)


def _to_cpu(x):
    if torch.is_tensor(x):
        return x.detach().to('cpu', copy=True)          # (a copy also of a CPU view: torch.save would write the view's whole storage)
    if isinstance(x, dict):
        return {str(k): _to_cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_to_cpu(v) for v in x]
    if isinstance(x, (bool, int, float, str)) or x is None:
        return x
    raise TypeError('a checkpoint holds tensors and plain scalars, lists and dicts, not %s' % type(x).__name__)


def _describe(agent, map_name, objects, replay, hyper=None):
    fields, tensors, states = {}, {}, {}
    for name, obj in objects.items():
        f, sd = _state_of(obj, replay)
        for k, v in f.items():
            fields['%s.%s' % (name, k)] = v
        _walk(sd, name, tensors)
        states[name] = sd
    for k, v in (hyper or {}).items():
        fields['hyper.%s' % k] = v
    sig = {'format': FORMAT, 'agent': str(agent), 'map': str(map_name), 'replay': bool(replay), 'objects': list(objects), 'fields': fields,
           'tensors': tensors}
    return sig, states


# ---------------------------------------------------------------------------------------------- save / load
def save(path, *, agent, map_name, objects, progress, replay=True, hyper=None):
    """Write the checkpoint (under a temporary name, renamed into place).  hyper: further name -> scalar entries of the signature
    that no object carries (the planned episodes; the decay steps of a loop that runs in Python).  Returns the path."""
    for name, obj in objects.items():
        if _is_env(obj) and 0 < int(obj.steps) < int(obj.horizon_steps):
            raise ValueError('%s is inside an episode (step %d of %d): checkpoints are taken at an episode boundary' %
                             (name, int(obj.steps), int(obj.horizon_steps)))
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()                        # the loops are asynchronous
    sig, states = _describe(agent, map_name, objects, replay, hyper)
    ck = {'format': FORMAT, 'signature': _to_cpu(sig), 'objects': _to_cpu(states), 'progress': _to_cpu(dict(progress))}
    tmp = '%s.%d.tmp' % (path, os.getpid())
    torch.save(ck, tmp)
    os.replace(tmp, path)
    return path


def _mismatch(field, theirs, ours):
    return ValueError('checkpoint mismatch in %s: the file has %r, this run has %r' % (field, theirs, ours))


def load(path, *, agent, map_name, objects, strict=True, hyper=None):
    """Load the checkpoint into `objects`, in place, and return its progress dict.  Nothing is modified unless the whole signature
    matches.  strict=False: weights only; every object given must be in the file, and only the networks' shapes are compared."""
    ck = torch.load(path, weights_only=True, map_location='cpu')
    if not isinstance(ck, dict) or ck.get('format') != FORMAT:
        raise _mismatch('format', ck.get('format') if isinstance(ck, dict) else type(ck).__name__, FORMAT)
    theirs = ck['signature']
    ours, _ = _describe(agent, map_name, objects, bool(theirs['replay']), hyper)
    if strict:
        for k in ('agent', 'map', 'objects'):
            if theirs[k] != ours[k]:
                raise _mismatch(k, theirs[k], ours[k])
        for kind in ('fields', 'tensors'):
            differ = lambda k: _plain(theirs[kind].get(k, '(absent)')) != _plain(ours[kind].get(k, '(absent)'))
            bad = [k for k in sorted(set(theirs[kind]) | set(ours[kind])) if differ(k)]
            if bad:         # the first in full, the others by name
                e = _mismatch(bad[0], theirs[kind].get(bad[0], '(absent)'), ours[kind].get(bad[0], '(absent)'))
                raise e if len(bad) == 1 else ValueError('%s (and in %s)' % (e, ', '.join(bad[1:])))
    else:
        for name, obj in objects.items():
            if name not in theirs['objects']:
                raise _mismatch('objects', theirs['objects'], list(objects))
            if isinstance(obj, nn.Module):
                for k, b in ours['fields'].items():
                    if k.startswith(name + '.') and _plain(theirs['fields'].get(k, '(absent)')) != _plain(b):
                        raise _mismatch(k, theirs['fields'].get(k, '(absent)'), b)
        for k, b in ours['tensors'].items():
            if k.partition('/')[2].startswith('weights/') and _plain(theirs['tensors'].get(k, '(absent)')) != _plain(b):
                raise _mismatch(k, theirs['tensors'].get(k, '(absent)'), b)
    # ---- from here on the objects are written
    for name, obj in objects.items():
        sd = ck['objects'][name]
        if _is_env(obj) or (not hasattr(obj, 'load_state_dict') and not isinstance(obj, torch.Generator)):
            continue
        if isinstance(obj, torch.Generator):
            if strict:
                obj.set_state(sd['state']['rng'])
        elif isinstance(obj, nn.Module):
            from .agents import _state
            _state.load_module(obj, sd['weights'], name)
        else:
            obj.load_state_dict(sd, weights_only=not strict)
    return ck['progress']


FRAP_AGENTS = ('MPLight', 'MPLightFULL', 'MPLightMulti', 'MPLightFULLMulti')


def load_frap_weights(path, net):
    """FRAP weights across maps: the network of any MPLight, MPLightFULL or multi-map MPLight checkpoint into `net`, a FRAP of ANY
    number of phase pairs, in place (a net whose parameters are views of a learner's vector writes through to it).  FRAP's tensors
    do not depend on the map, so only demand_shape and the tensor shapes are compared -- not oshape, which `load` refuses on.
    Nothing is modified unless all of it matches.  Returns the file's progress dict."""
    from .agents import _state
    ck = torch.load(path, weights_only=True, map_location='cpu')
    if not isinstance(ck, dict) or ck.get('format') != FORMAT:
        raise _mismatch('format', ck.get('format') if isinstance(ck, dict) else type(ck).__name__, FORMAT)
    theirs = ck['signature']
    if theirs['agent'] not in FRAP_AGENTS:
        raise _mismatch('agent', theirs['agent'], 'one of %s' % (FRAP_AGENTS,))
    name = next((n for n in ('net', 'net0') if n in theirs['objects'] and 'weights' in ck['objects'].get(n, {})), None)
    if name is None:
        raise _mismatch('objects', theirs['objects'], "a FRAP network named 'net' or 'net0'")
    d = theirs['fields'].get('%s.demand_shape' % name, '(absent)')
    if _plain(d) != int(net.demand_shape):
        raise _mismatch('%s.demand_shape' % name, d, int(net.demand_shape))
    ours = {}
    _walk({'weights': dict(net.state_dict())}, name, ours)
    for k in sorted(set(ours) | {t for t in theirs['tensors'] if t.startswith(name + '/weights/')}):
        a, b = theirs['tensors'].get(k, '(absent)'), ours.get(k, '(absent)')
        if _plain(a) != _plain(b):
            raise _mismatch(k, a, b)
    _state.load_module(net, ck['objects'][name]['weights'], name)
    return ck['progress']


def _plain(x):
    """tuples and lists compare alike (torch.load gives back lists)"""
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, float):
        return float(x)
    return x


# ---------------------------------------------------------------------------------------------- what the training tools share
def tool_flags(argv):
    """--save PATH [--save-freq K] [--save-replay] --load PATH [--eval] [--stop-after K] taken out of an argument list ->
    (keyword arguments for the tool's main(), the remaining arguments)"""
    kw, rest, i = {}, [], 0
    valued = {'--save': ('save', str), '--load': ('load', str), '--save-freq': ('save_freq', int), '--stop-after': ('stop_after', int)}
    while i < len(argv):
        a = argv[i]
        if a in valued:
            if i + 1 >= len(argv):
                raise SystemExit('%s needs a value' % a)
            kw[valued[a][0]] = valued[a][1](argv[i + 1])
            i += 2
            continue
        if a == '--save-replay':
            kw['save_replay'] = True
        elif a == '--eval':
            kw['eval_only'] = True
        else:
            rest.append(a)
        i += 1
    if kw.get('eval_only') and not kw.get('load'):
        raise SystemExit('--eval needs --load PATH')
    return kw, rest


class Counters:
    """The state a loop written in Python keeps in local variables (step and slot counters, flags, its own buffers), as an object a
    checkpoint can hold: Counters(t=0, slot=0, done=[False] * T, buf=tensor); tensors are loaded in place."""

    def __init__(self, **values):
        self.__dict__.update(values)

    def state_dict(self):
        return {'state': dict(vars(self))}

    def load_state_dict(self, sd, weights_only=False):
        from .agents import _state
        if weights_only:
            return
        if sorted(sd['state']) != sorted(vars(self)):
            raise ValueError('Counters: the checkpoint holds %s, the loop %s' % (sorted(sd['state']), sorted(vars(self))))
        for k, v in sd['state'].items():
            if torch.is_tensor(getattr(self, k)):
                _state.copy_into(getattr(self, k), v, 'Counters.%s' % k)
            else:
                setattr(self, k, v)


def due(ep_done, episodes, save, save_freq, stop_after):
    """(write the checkpoint now, leave now) after `ep_done` of `episodes` planned episodes: written after every save_freq-th episode,
    after the last, and before leaving at --stop-after"""
    stop = bool(stop_after) and ep_done >= int(stop_after) and ep_done < episodes
    write = bool(save) and (stop or ep_done == episodes or (int(save_freq) > 0 and ep_done % int(save_freq) == 0))
    return write, stop


# ---------------------------------------------------------------------------------------------- the reference's IDQN layout
def _adam_of(learner):
    """(step, m-net, v-net): the learner's Adam moments as two BatchedIDQN-shaped CPU modules, and its step count"""
    from .agents import _state
    from .agents.idqn_rollout import BatchedIDQN
    net = learner.net if hasattr(learner, 'net') else learner.q
    hold = [BatchedIDQN(net.lanes, net.actions) for _ in range(2)]
    names = [k for k, _ in net.named_parameters()]
    if hasattr(learner, 'opt'):
        st = _state.adam_state(learner.opt)
        step = int(st['step'][0])
        sets = [dict(zip(names, st[k])) for k in ('exp_avg', 'exp_avg_sq')]
    else:
        step, sets = int(learner.n_updates), [learner.m, learner.v]
    with torch.no_grad():
        for h, src in zip(hold, sets):
            for k in names:
                getattr(h, k).copy_(src[k])
    return step, hold[0], hold[1]


def _file_of(directory, sid):
    return os.path.join(directory, 'agent_%s.pt' % sid)


@torch.no_grad()
def save_reference_idqn(directory, net, learner, signal_ids):
    """One file per signal, agent_<signal id>.pt = {'model_state_dict', 'optimizer_state_dict'}, as the reference's DQN agents
    write them: the model is the state_dict of reference_q_network(L_s, A_s) (keys 0.*, 3.*, 5.*, 7.*), un-padded; the optimizer
    dict is produced by a real torch.optim.Adam over that module whose step / exp_avg / exp_avg_sq were filled from the learner
    (BatchedDQNLearner or FusedDQNLearner), so its layout is whatever this torch writes.  Returns the paths."""
    signal_ids = list(signal_ids)
    if len(signal_ids) != len(net.lanes):
        raise ValueError('%d signal ids for a network of %d signals' % (len(signal_ids), len(net.lanes)))
    step, m_net, v_net = _adam_of(learner)
    lr = learner.opt.param_groups[0]['lr'] if hasattr(learner, 'opt') else learner.lr
    mods, m_mods, v_mods = net.to_reference_modules(), m_net.to_reference_modules(), v_net.to_reference_modules()
    os.makedirs(directory, exist_ok=True)
    paths = []
    for sid, mod, mm, vm in zip(signal_ids, mods, m_mods, v_mods):
        opt = torch.optim.Adam(mod.parameters(), lr=lr)
        if step > 0:
            for p in mod.parameters():
                p.grad = torch.zeros_like(p)
            opt.step()                                  # a zero gradient moves nothing: it only makes torch create its state
            for p, pm, pv in zip(mod.parameters(), mm.parameters(), vm.parameters()):
                st = opt.state[p]
                st['step'].fill_(float(step))
                st['exp_avg'].copy_(pm)
                st['exp_avg_sq'].copy_(pv)
                p.grad = None
        paths.append(_file_of(directory, sid))
        torch.save({'model_state_dict': mod.state_dict(), 'optimizer_state_dict': opt.state_dict()}, paths[-1])
    return paths


@torch.no_grad()
def load_reference_idqn(directory, net, learner=None, signal_ids=()):
    """The way back: agent_<signal id>.pt of every signal into `net` (in place) and, when a learner is given and the files hold
    optimizer state, its Adam moments and step count (in place; the target network is synchronised to the loaded weights, as a
    reference agent that loads does).  Returns the per-signal modules."""
    from .agents import _state
    from .agents.idqn_rollout import BatchedIDQN, reference_q_network
    signal_ids = list(signal_ids)
    if len(signal_ids) != len(net.lanes):
        raise ValueError('%d signal ids for a network of %d signals' % (len(signal_ids), len(net.lanes)))
    mods, m_mods, v_mods, steps = [], [], [], []
    for sid, L, A in zip(signal_ids, net.lanes, net.actions):
        ck = torch.load(_file_of(directory, sid), weights_only=True, map_location='cpu')
        trio = [reference_q_network(L, A) for _ in range(3)]
        trio[0].load_state_dict(ck['model_state_dict'])
        opt = torch.optim.Adam(trio[0].parameters())
        opt.load_state_dict(ck['optimizer_state_dict'])
        st = [opt.state.get(p, {}) for p in trio[0].parameters()]
        steps.append(int(st[0]['step']) if len(st[0]) else 0)
        for mod, key in ((trio[1], 'exp_avg'), (trio[2], 'exp_avg_sq')):
            for p, s in zip(mod.parameters(), st):
                p.copy_(s[key]) if len(s) else p.zero_()
        mods.append(trio[0]); m_mods.append(trio[1]); v_mods.append(trio[2])
    if len(set(steps)) > 1:
        raise ValueError('the signals\' optimizers stand at different steps (%s): one stacked Adam cannot continue them' % steps)
    net.load_reference_modules(mods)
    if learner is not None:
        hold_m = BatchedIDQN(net.lanes, net.actions).load_reference_modules(m_mods)
        hold_v = BatchedIDQN(net.lanes, net.actions).load_reference_modules(v_mods)
        names = [k for k, _ in net.named_parameters()]
        if hasattr(learner, 'opt'):
            sd = {'step': [float(steps[0])] * len(names), 'exp_avg': [getattr(hold_m, k).detach() for k in names],
                  'exp_avg_sq': [getattr(hold_v, k).detach() for k in names]}
            _state.load_adam_state(learner.opt, sd, 'load_reference_idqn')
            learner.n_updates = steps[0]
        else:
            _state.copy_dict_into(learner.m, {k: getattr(hold_m, k).detach() for k in learner.m}, 'load_reference_idqn.m')
            _state.copy_dict_into(learner.v, {k: getattr(hold_v, k).detach() for k in learner.v}, 'load_reference_idqn.v')
            _state.set_fused_counter(learner, steps[0], 'load_reference_idqn')
        learner.sync_target()
    return mods
