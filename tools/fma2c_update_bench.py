#!/usr/bin/env python3
"""Device-event time of one A2C update of FMA2C at a full segment: the fused learner (rs_fma2c_learn_*; FusedA2CLearner) and the
PyTorch learner (A2CLearner) in the same process, on the same recorded segment.

    python tools/fma2c_update_bench.py [--fused-only] [--split] [map] [n_envs] [T] [windows]

The segment comes from T acts of the fused policy on synthetic lane aggregates with random rewards; no simulator runs.  After one
warm-up update every learner is timed over `windows` updates of the same segment (device events around the update; the weights
move, the work does not change).  Prints one JSON line with min / median / max in ms per learner; --split adds the fused update's
parts from events around rs_fma2c_learn_grad and rs_fma2c_learn_step (the kernels inside grad: a kernel trace of this script)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resco_amd.agents.fma2c import A2CLearner, BatchedFMA2C, FMA2CLayout, FusedFMA2C      # noqa: E402
from resco_amd.agents.fma2c_learn_fused import FusedA2CLearner                           # noqa: E402
from resco_amd.config.map_config import map_configs                                     # noqa: E402
from resco_amd.config.mdp_config import activate                                        # noqa: E402
from resco_amd.multi_signal import load_scenario                                        # noqa: E402


def timed(fn, windows):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(min_ms=round(min(ms), 3), median_ms=round(float(np.median(ms)), 3), max_ms=round(max(ms), 3))


def main(map_name='cologne1', n=256, T=120, windows=5, fused_only=False, split=False):
    activate('FMA2C', map_name)
    sc = load_scenario(map_name, None, map_configs.get(map_name, {}).get('lights', ()), 3)
    layout = FMA2CLayout(sc, False)
    net = BatchedFMA2C(layout).init_like_reference(0).cuda()
    policy = FusedFMA2C(net, n, seed=7)
    fused = FusedA2CLearner(net, policy, n, batch_size=T)
    gen = torch.Generator(device='cuda').manual_seed(0)
    macts = policy.buffer('mgr_actions')
    for t in range(T):
        agg = torch.rand(n, layout.O, 5, device='cuda', generator=gen) * torch.tensor([18.0, 18.0, 5000.0, 800.0, 20000.0], device='cuda')
        out = policy.act(agg.contiguous(), step_key=t, want=('value', 'rows'), out=fused.slot())
        fused.add(out['rows'], torch.cat([macts, out['actions']], dim=1), torch.randn(n, layout.K, device='cuda', generator=gen) * 1000.0, out['value'], False)
    boot, state = torch.randn(n, layout.K, device='cuda', generator=gen), policy.buffer('state').clone()
    res = dict(map=map_name, envs=n, T=T, agents=layout.K, windows=windows)

    def fused_update():
        fused.n = T
        fused.update(boot, state)
    res['fused'] = timed(fused_update, windows)
    if split:
        fused.n = T
        res['fused_grad'] = timed(lambda: fused.grad(boot), windows)
        res['fused_step'] = timed(fused.step, windows)
    if not fused_only:
        ref = A2CLearner(net, n, batch_size=T)
        ref.rows.copy_(fused.rows); ref.acts.copy_(fused.acts); ref.vals.copy_(fused.vals)
        ref.rews.copy_(torch.clamp(fused.rews / 2000.0, -2.0, 2.0))

        def torch_update():
            ref.n, ref.dones = T, [False] * (T + 1)
            ref.update(boot, state)
        res['pytorch'] = timed(torch_update, windows)
        res['ratio_of_medians'] = round(res['pytorch']['median_ms'] / res['fused']['median_ms'], 2)
    print(json.dumps(res), flush=True)
    fused.close()
    policy.close()
    return res


if __name__ == '__main__':
    a = sys.argv[1:]
    fo, sp = '--fused-only' in a, '--split' in a
    a = [x for x in a if x not in ('--fused-only', '--split')]
    main(a[0] if len(a) > 0 else 'cologne1', int(a[1]) if len(a) > 1 else 256, int(a[2]) if len(a) > 2 else 120, int(a[3]) if len(a) > 3 else 5,
         fused_only=fo, split=sp)
