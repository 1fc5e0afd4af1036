#!/usr/bin/env python3
"""A/B in ONE process: the FMA2C training loop in the library (tools/fma2c_train.py --device-loop: one rs_group_fma2c_train per episode)
against the Python-driven --device-update loop, and, as a third column, the Python loop with the reward kernel (--device-update
--device-rewards), alternating, `rounds` times each.

    python tools/fma2c_loop_ab.py [--full] [map] [n_envs] [episodes] [rounds]

Every round of a variant is a fresh run of the tool's own function (new environment, network, policy, learner); its first episode
warms up and is dropped.  Prints per round and variant the env-steps/s with learning of the remaining episodes, and at the end one
JSON line with the medians, ms per env-step (all environments), the ratios to the --device-update loop and the spread between the
rounds of a variant.  The third column separates what the reward kernel buys from what the loop buys: 'rewards' and 'loop' compute
the same bits (tests/test_gpu_fma2c_loop.py); 'python' sums the rewards in the dense product's order, so its training is not the
same numbers."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import fma2c_train                                         # noqa: E402

VARIANTS = {'python': dict(device_update=True), 'rewards': dict(device_update=True, device_rewards=True), 'loop': dict(device_loop=True)}


def main(map_name='cologne1', n=256, episodes=5, rounds=3, full=False):
    rates, steps = {k: [] for k in VARIANTS}, 0
    for r in range(rounds):
        for k, flags in VARIANTS.items():
            rows, final = fma2c_train.main(map_name, n, episodes, 0, full=full, quiet=True, **flags)
            steps = final['steps_per_episode']
            rates[k].append([row['env_steps_per_s'] for row in rows[1:]])
            print('fma2c %s x %d %s round %d: %s env-steps/s, updates %d, last delay %.2f s' % (
                map_name, n, k, r, rates[k][-1], rows[-1]['updates'], rows[-1]['avg_delay_s']), flush=True)
    med = {k: statistics.median(x for rnd in v for x in rnd) for k, v in rates.items()}
    spread = {k: round(max(statistics.median(rnd) for rnd in v) / min(statistics.median(rnd) for rnd in v) - 1.0, 4) for k, v in rates.items()}
    print(json.dumps(dict(agent='FMA2CFULL' if full else 'FMA2C', map=map_name, envs=n, steps_per_episode=steps, episodes=episodes, rounds=rounds,
                          env_steps_per_s=rates, median=med, ms_per_env_step={k: round(n / v * 1e3, 4) for k, v in med.items()},
                          ratio_to_python={k: round(v / med['python'], 3) for k, v in med.items()}, spread_between_rounds=spread)), flush=True)


if __name__ == '__main__':
    a = sys.argv[1:]
    full = '--full' in a
    a = [x for x in a if x != '--full']
    main(a[0] if len(a) > 0 else 'cologne1', *[int(x) for x in a[1:4]], full=full)
