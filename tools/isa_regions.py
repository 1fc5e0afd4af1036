#!/usr/bin/env python3
"""The tick loop of ONE step kernel by instruction class: regions P, C and M (between two workgroup barriers) of one or more builds.

    python tools/isa_regions.py <kernel> <label>=<file.s> [<label>=<file.s> ...]

<file.s> is the gfx950 assembly hipcc keeps with -save-temps (tools/isa_map.sh, tools/isa.sh); <kernel> is a substring of the kernel's
mangled name, e.g. rs_step_kernel_fix_v64I19ScnFix_ingolstadt21Lb0 or rs_step_kernel_v64ILi896ELb0.  Regions as in tools/isa_loads.py; the
tick loop is taken to be the largest region (P) and the two that follow it (C, M), as in tools/isa_sloads.py.  Columns: instructions,
SALU (s_* that are neither loads, waits, barriers, branches nor nops), s_waitcnt with lgkmcnt(0), LDS instructions (ds_*), of those
ds_bpermute_b32, DPP instructions (*_dpp), VALU (v_*), VMEM (global_ / buffer_ / flat_ / scratch_).
"""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.isa_loads import kernel_text  # noqa: E402
from tools.isa_sloads import NOT_SALU  # noqa: E402

COLS = ('insts', 'salu', 'lgkm0', 'lds', 'bpermute', 'dpp', 'valu', 'vmem')


def regions(body):
    out = [collections.Counter()]
    for code in body:
        op, r = code.split()[0], out[-1]
        r['insts'] += 1
        if op == 's_barrier':
            out.append(collections.Counter())
        elif op == 's_waitcnt':
            r['lgkm0'] += 'lgkmcnt(0)' in code
        elif op.startswith('s_'):
            r['salu'] += not op.startswith(NOT_SALU)
        elif op.startswith('ds_'):
            r['lds'] += 1
            r['bpermute'] += op == 'ds_bpermute_b32'
        elif op.startswith('v_'):
            r['valu'] += 1
            r['dpp'] += op.endswith('_dpp')
        elif op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
            r['vmem'] += 1
    return out


def main(argv):
    if len(argv) < 3:
        raise SystemExit(__doc__)
    print('  %-32s %-6s' % ('build', 'region') + ''.join('%9s' % c for c in COLS) + '   kernel')
    for spec in argv[2:]:
        label, _, path = spec.partition('=')
        body = kernel_text(path, argv[1])
        regs = regions(body)
        big = max(range(len(regs)), key=lambda i: regs[i]['insts'])
        for name, i in zip('PCM', (big, big + 1, big + 2)):
            print('  %-32s %-6s' % (label if name == 'P' else '', name) + ''.join('%9d' % regs[i][c] for c in COLS) +
                  ('   %d instructions' % len(body) if name == 'P' else ''))


if __name__ == '__main__':
    main(sys.argv)
